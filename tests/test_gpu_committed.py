"""The committed sum-check on the GPU through the C ABI: the
linear-combination kernel and the eq table against the Python model on all
fields, the batched KZG opening against zk_dev_kzg_get_proof (one table) and
against the model's G1 points (three tables), and whole proofs — the zero-check
at n = 3 equal to the model's bytes, larger ones accepted by the host verifier
with every public evaluation checked, every kind of damage rejected."""
from __future__ import annotations

import ctypes as C
import functools
import random

import numpy as np
import pytest

import committed_cases as cc
import committed_oracle as mo
import composed_oracle as cm
import extreme_tables as xt
import pyoracle as po

import zk_amd
from zk_amd._lib import ZK_EINVAL, ZK_EUNSUPPORTED, ZK_OK, lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import KZG

pytestmark = pytest.mark.gpu
R = mo.R
SENTINEL = cc.SENTINEL
COUNTS = (1, 2, 255, 256, 257, 4097)  # the block edge (256 threads) and the grid-stride tail


@functools.lru_cache(maxsize=None)
def _kzg(nvars: int) -> KZG:
    return KZG(cc.taus(nvars), zk_amd.default_context(0))


# ---- zk_dev_mle_lincomb ---------------------------------------------------------
def _lincomb(ctx, field, tables, coeffs, constant, count, out, repr_=0, ntables=None, null=()):
    arr = (C.c_void_p * max(len(tables), 1))(*[t.ptr.value for t in tables])
    args = {"tables": arr, "coeffs": ptr(as_limbs(list(coeffs))), "out": out.ptr,
            "constant": None if constant is None else ptr(as_limbs([constant]))}
    for name in null:
        args[name] = None
    return lib().zk_dev_mle_lincomb(ctx.h, field, repr_, args["tables"], len(tables) if ntables is None else ntables,
                                    args["coeffs"], args["constant"], count, args["out"])


@functools.lru_cache(maxsize=None)
def _lincomb_inputs(field: int):
    """16 tables of 4097 values and 16 coefficients, with boundary values among them"""
    p = po.MODULI[field]
    rng = random.Random(700 + field)
    tabs = [[rng.randrange(p) for _ in range(4097)] for _ in range(16)]
    for i, v in enumerate((0, 1, p - 1)):
        tabs[i][i] = tabs[15][4096 - i] = v
    coeffs = [rng.randrange(p) for _ in range(16)]
    coeffs[1], coeffs[2] = p - 1, 0
    return tabs, coeffs


@pytest.mark.parametrize("ntables", [1, 2, 3, 16])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_lincomb_matches_the_model(ctx, field, ntables):
    p = po.MODULI[field]
    tabs, coeffs = _lincomb_inputs(field)
    tabs, coeffs = tabs[:ntables], coeffs[:ntables]
    dev = [ctx.upload(field, tb) for tb in tabs]
    fill = [7] * 4098
    for constant in (None, p - 1, 12345):
        want = mo.lincomb(p, tabs, coeffs, constant or 0)
        for count in COUNTS:
            out = ctx.upload(field, fill)
            assert _lincomb(ctx, field, dev, coeffs, constant, count, out) == ZK_OK
            got = out.to_ints()
            assert got[:count] == want[:count], (constant, count)
            assert got[count:] == fill[count:], "wrote past count"
    assert zk_amd.DeviceTable.lincomb(dev, coeffs, 5).to_ints() == mo.lincomb(p, tabs, coeffs, 5)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_lincomb_with_a_repeated_table(ctx, field):
    p = po.MODULI[field]
    tabs, coeffs = _lincomb_inputs(field)
    a, b = ctx.upload(field, tabs[0][:300]), ctx.upload(field, tabs[1][:300])
    out = ctx.alloc(field, 300)
    assert _lincomb(ctx, field, [a, b, a, a], coeffs[:4], 9, 300, out) == ZK_OK
    assert out.to_ints() == mo.lincomb(p, [tabs[0][:300], tabs[1][:300], tabs[0][:300], tabs[0][:300]], coeffs[:4], 9)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_lincomb_largest_accumulator(ctx, field):
    """16 tables whose words in memory are all p - 1, every coefficient word p - 1:
    the unreduced sum is 16 (p - 1)^2, the most the kernel's accumulator sees"""
    p = po.MODULI[field]
    count = 257
    t = xt.Table(field, [p - 1], np.zeros(count, np.intp))
    assert t.word_ints() == [p - 1] * count
    a, b = ctx.upload(field, t.words, repr=1), ctx.upload(field, t.words, repr=1)
    out = ctx.alloc(field, count)
    words = [p - 1] * 16
    assert _lincomb(ctx, field, [a, b] * 8, words, p - 1, count, out, repr_=1) == ZK_OK
    rinv = pow(xt.R, -1, p)
    want_word = (16 * (p - 1) * (p - 1) * rinv + (p - 1)) % p
    assert xt.ints(out.download(repr=1)) == [want_word] * count
    c = xt.canonical(field, p - 1)  # the same in field values
    assert out.to_ints() == [(16 * c * c + c) % p] * count


def test_lincomb_error_paths_write_nothing(ctx):
    field, p = 0, po.MODULI[0]
    vals = list(range(1, 301))
    tabs = [ctx.upload(field, vals) for _ in range(17)]
    out = ctx.upload(field, [3] * 300)

    def code(tables, coeffs, count=300, o=out, **kw):
        rc = _lincomb(ctx, kw.pop("field", field), tables, coeffs, kw.pop("constant", None), count, o, **kw)
        return rc, out.to_ints() == [3] * 300 and tabs[1].to_ints() == vals

    assert code(tabs[:2], [1, 2], o=tabs[1]) == (ZK_EINVAL, True)        # d_out aliases an input: unchanged
    assert code(tabs[:3], [1, 2, 3], o=tabs[0])[0] == ZK_EINVAL
    assert code(tabs[:2], [1, 2], ntables=0) == (ZK_EINVAL, True)
    assert code(tabs[:2], [1, 2], count=0) == (ZK_EINVAL, True)
    assert code(tabs, [1] * 17) == (ZK_EUNSUPPORTED, True)               # ntables > 16
    assert code(tabs[:2], [1, p]) == (ZK_EINVAL, True)                   # a coefficient >= p
    assert code(tabs[:2], [1, 2], constant=p) == (ZK_EINVAL, True)
    assert code(tabs[:2], [1, 2], field=3) == (ZK_EINVAL, True)
    assert code(tabs[:2], [1, 2], repr_=2) == (ZK_EINVAL, True)
    for null in ("tables", "coeffs", "out"):
        assert code(tabs[:2], [1, 2], null=(null,)) == (ZK_EINVAL, True), null
    assert code(tabs[:16], [1] * 16) == (ZK_OK, False)                   # the cap itself is fine
    assert out.to_ints() == [16 * v % p for v in vals]


# ---- zk_dev_mle_eq_table / zk_mle_eq_table ---------------------------------------
@pytest.mark.parametrize("field", [0, 1, 2])
def test_eq_table_matches_the_model(ctx, field):
    p = po.MODULI[field]
    rng = random.Random(80 + field)
    for n in list(range(0, 8)) + [10]:
        pt = [rng.randrange(p) for _ in range(n)]
        if n >= 3:
            pt[0], pt[1], pt[2] = 0, 1, p - 1
        want = mo.eq_table(p, pt)
        assert zk_amd.DeviceTable.eq(ctx, field, pt).to_ints() == want, n
        assert zk_amd.MultilinearPoly.eq(pt, field, ctx).evaluation == want, n


def test_eq_table_error_paths(ctx):
    out = ctx.upload(0, [3] * 4)
    L = lib()
    pt = as_limbs([1, 2])
    assert L.zk_dev_mle_eq_table(ctx.h, 0, 0, None, 2, out.ptr) == ZK_EINVAL
    assert L.zk_dev_mle_eq_table(ctx.h, 0, 0, ptr(pt), 2, None) == ZK_EINVAL
    assert L.zk_dev_mle_eq_table(ctx.h, 3, 0, ptr(pt), 2, out.ptr) == ZK_EINVAL
    assert L.zk_dev_mle_eq_table(ctx.h, 0, 2, ptr(pt), 2, out.ptr) == ZK_EINVAL
    assert L.zk_dev_mle_eq_table(ctx.h, 0, 0, ptr(as_limbs([1, po.MODULI[0]])), 2, out.ptr) == ZK_EINVAL
    assert L.zk_dev_mle_eq_table(ctx.h, 0, 0, ptr(pt), 27, out.ptr) == ZK_EUNSUPPORTED
    assert out.to_ints() == [3] * 4
    host = np.full((4, 4), SENTINEL, np.uint64)
    assert L.zk_mle_eq_table(ctx.h, 0, 0, ptr(pt), 27, ptr(host)) == ZK_EUNSUPPORTED
    assert L.zk_mle_eq_table(ctx.h, 0, 0, None, 2, ptr(host)) == ZK_EINVAL
    assert (host == SENTINEL).all()


# ---- batched KZG ----------------------------------------------------------------
@pytest.mark.parametrize("nvars", [1, 2, 3, 4, 5, 6, 10])
def test_batch_open_of_one_table_is_get_proof_byte_for_byte(ctx, nvars):
    k = _kzg(nvars)
    evals = cm.random_tables(2, 1, nvars, 300 + nvars)[0]
    evals[0], evals[-1] = R - 1, 0
    rng = random.Random(nvars)
    point = [rng.randrange(R) for _ in range(nvars)]
    value = po.evaluate(R, evals, point)
    table = ctx.upload(2, evals)
    want = k.get_proof_device(value, point, table)
    for rho in (0, rng.randrange(R)):
        assert k.batch_open_device(rho, [value], point, [table]) == want, rho
    assert k.batch_open(R - 1, [value], point, [evals]) == want
    assert table.to_ints() == evals  # the input is only read


def test_commit_batch_equals_single_commits(ctx):
    nvars, ntab = 5, 3
    k = _kzg(nvars)
    tabs = cm.random_tables(2, ntab, nvars, 55)
    tabs[1] = [0] * (1 << nvars)
    single = [k.commit(tb) for tb in tabs]
    assert single[1] is None
    assert k.commit_batch(tabs) == single
    assert k.commit_batch([ctx.upload(2, tb) for tb in tabs]) == single
    out = np.full((3, 12), SENTINEL, np.uint64)
    assert lib().zk_dev_kzg_commit_batch(ctx.h, k.h, None, 3, ptr(out)) == ZK_EINVAL
    assert lib().zk_dev_kzg_commit_batch(ctx.h, k.h, (C.c_void_p * 3)(), 0, ptr(out)) == ZK_EINVAL
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("nvars", [1, 2, 3])
def test_batch_open_equals_the_models_points(ctx, nvars):
    k = _kzg(nvars)
    basis, g2 = cc.setup(nvars)
    assert k.g2_taus == g2
    a, b = cm.random_tables(2, 2, nvars, 400 + nvars)
    tabs = [a, [0] * (1 << nvars), b]
    rng = random.Random(40 + nvars)
    point, rho = [rng.randrange(R) for _ in range(nvars)], rng.randrange(R)
    vals = [po.evaluate(R, tb, point) for tb in tabs]
    want = mo.batch_open(tabs, rho, vals, point, basis)
    assert k.batch_open(rho, vals, point, tabs) == want
    assert k.batch_open_device(rho, vals, point, [ctx.upload(2, tb) for tb in tabs]) == want
    cms = k.commit_batch(tabs)
    assert cms == [mo.ko.commit(tb, basis) for tb in tabs]
    assert KZG.batch_verify(cms, rho, vals, want, point, g2)
    assert not KZG.batch_verify(cms, rho, [vals[0], vals[1], (vals[2] + 1) % R], want, point, g2)


def test_batch_open_error_paths_write_nothing(ctx):
    k = _kzg(3)
    tabs = [ctx.upload(2, list(range(8))) for _ in range(17)]
    out = np.full((3, 12), SENTINEL, np.uint64)

    def code(ntables, rho=5, null=False):
        arr = (C.c_void_p * 17)(*[t.ptr.value for t in tabs])
        rc = lib().zk_dev_kzg_batch_open(ctx.h, k.h, 0, None if null else arr, ntables, ptr(as_limbs([rho])),
                                         ptr(as_limbs([1] * 17)), ptr(as_limbs([1, 2, 3])), ptr(out))
        return rc, bool((out == SENTINEL).all())

    assert code(0) == (ZK_EINVAL, True)
    assert code(17) == (ZK_EUNSUPPORTED, True)
    assert code(2, rho=R) == (ZK_EINVAL, True)
    assert code(2, null=True) == (ZK_EINVAL, True)
    assert code(16) == (ZK_OK, False)


# ---- whole proofs ------------------------------------------------------------------
def _as_dict(proof: zk_amd.CommittedProof) -> dict:
    return {"polys": [list(q.coefficient) for q in proof.proof_polynomials], "claimed_sum": proof.claimed_sum,
            "challenges": list(proof.random_challenges), "table_evals": list(proof.table_evals),
            "mask": proof.committed_mask, "commitments": list(proof.commitments), "opening": list(proof.opening)}


def _sum_poly(tables, factors, ctx):
    mles = [zk_amd.MultilinearPoly(as_limbs(tb), 2, ctx) for tb in tables]
    # every table in a first product of its own order, so that composed_tables() keeps the indices
    return zk_amd.SumPoly([zk_amd.ProductPoly.from_polys([mles[i] for i in term]) for term in factors]), mles


def test_zero_check_equals_the_models_bytes(ctx):
    nvars = 3
    tables, factors, mask = cc.shape("zero_check", nvars)
    want, _, claim = cc.model_proof("zero_check", nvars)
    sp, _ = _sum_poly(tables, factors, ctx)
    assert [to_ints(t) for t in sp.composed_tables()[0]] == tables
    t = zk_amd.Transcript(2)
    got = _as_dict(zk_amd.committed_prove(claim, sp, t, _kzg(nvars), mask, ctx=ctx))
    for key in ("commitments", "polys", "challenges", "table_evals", "opening", "claimed_sum", "mask"):
        assert got[key] == want[key], key
    mt = mo.Transcript(2)
    mo.prove(tables, factors, mask, claim, cc.setup(nvars)[0], mt)
    assert t.get_random_challenge() == mt.get_random_challenge()  # the transcripts end in one state


@pytest.mark.parametrize("name,nvars", [(s, n) for s in cc.SHAPES for n in (1, 2, 3)])
def test_every_shape_equals_the_model(ctx, name, nvars):
    """the device-resident entry; `same_pointer` passes one device table under two mask bits"""
    tables, factors, mask = cc.shape(name, nvars)
    want, _, claim = cc.model_proof(name, nvars)
    dev = [ctx.upload(2, tb) for tb in tables]
    if name == "same_pointer":
        dev[1] = dev[0]
    got = _prove_raw(ctx, _kzg(nvars), dev, factors, mask, claim, dev=True)
    assert got.rc == ZK_OK
    d = got.as_dict(mask)
    for key in ("commitments", "polys", "challenges", "table_evals", "opening"):
        assert d[key] == want[key], key


class RawProof:
    def __init__(self, nvars, ntables, degree, ncommitted):
        n = max(nvars, 1)
        self.coeffs = np.full((n, degree + 1, 4), SENTINEL, np.uint64)
        self.nco = np.full(n, 0xEE, np.uint8)
        self.ch = np.full((n, 4), SENTINEL, np.uint64)
        self.ev = np.full((max(ntables, 1), 4), SENTINEL, np.uint64)
        self.cs = np.full((1, 4), SENTINEL, np.uint64)
        self.cm = np.full((max(ncommitted, 1), 12), SENTINEL, np.uint64)
        self.op = np.full((n, 12), SENTINEL, np.uint64)
        self.rc, self.state = None, b""

    def arrays(self):
        return (self.coeffs, self.ch, self.ev, self.cs, self.cm, self.op)

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.arrays()) and bool((self.nco == 0xEE).all())

    def same(self, other):
        return all(np.array_equal(a, b) for a, b in zip(self.arrays(), other.arrays())) and \
            np.array_equal(self.nco, other.nco) and self.state == other.state

    def as_dict(self, mask):
        return {"polys": [to_ints(self.coeffs[k, : self.nco[k]]) for k in range(len(self.nco))],
                "challenges": to_ints(self.ch), "table_evals": to_ints(self.ev), "mask": mask,
                "commitments": cc.points_from(self.cm), "opening": cc.points_from(self.op)}


def _prove_raw(ctx, k, tables, factors, mask, claim, dev=False, commitments_in=None, nvars=None, ntables=None,
               null=(), pre=b""):
    """zk_committed_sumcheck_prove (tables: lists of integers) or, dev=True, the device entry (DeviceTables)"""
    nt = len(tables) if ntables is None else ntables
    n = k.nvars if nvars is None else nvars
    degree = len(factors[0])
    out = RawProof(max(n, k.nvars), len(tables), degree, bin(mask & 0xFFFF).count("1"))
    limbs = None if dev else [as_limbs(list(tb)) for tb in tables]
    arr = (C.c_void_p * len(tables))(*[(t.ptr.value if dev else a.ctypes.data) for t, a in zip(tables, limbs or tables)])
    fac = np.array(factors, np.uint8).reshape(-1)
    t = zk_amd.Transcript(2)
    if pre:
        t.append(pre)
    args = {"tables": arr, "factors": ptr(fac), "claim": ptr(as_limbs([claim])), "t": t.h, "coeffs": ptr(out.coeffs),
            "nco": ptr(out.nco), "ch": ptr(out.ch), "ev": ptr(out.ev), "cs": ptr(out.cs), "cm": ptr(out.cm),
            "op": ptr(out.op), "kzg": k.h}
    for name in null:
        args[name] = None
    cin = None if commitments_in is None else ptr(commitments_in)
    fn = lib().zk_dev_committed_sumcheck_prove if dev else lib().zk_committed_sumcheck_prove
    out.rc = fn(ctx.h, args["kzg"], 0, args["tables"], nt, n, args["factors"], len(factors), degree, mask, cin,
                args["claim"], args["t"], args["coeffs"], args["nco"], args["ch"], args["ev"], args["cs"], args["cm"],
                args["op"])
    out.state = t.to_bytes()
    return out


def _big_zero_check(nvars: int, ntables: int):
    """A true identity of 5 or 16 tables: sum_g eq a_g b_g + eq negc_g one = 0 with
    negc_g = -a_g b_g. Tables: 0 eq, 1 one (public), then a_g, b_g, negc_g per
    group (committed), then committed tables no term names up to `ntables`."""
    groups = (ntables - 2) // 3
    N = 1 << nvars
    rng = random.Random(1000 * nvars + ntables)
    pt = [rng.randrange(R) for _ in range(nvars)]
    tables = [mo.eq_table(R, pt), [1] * N]
    factors = []
    for g in range(groups):
        a = [rng.randrange(R) for _ in range(N)]
        b = [rng.randrange(R) for _ in range(N)]
        base = len(tables)
        tables += [a, b, [(-x * y) % R for x, y in zip(a, b)]]
        factors += [[0, base, base + 1], [0, base + 2, 1]]
    while len(tables) < ntables:
        tables.append([rng.randrange(R) for _ in range(N)])
    mask = ((1 << ntables) - 1) & ~0b11
    return tables, factors, mask, pt


@functools.lru_cache(maxsize=None)
def _big_case(nvars: int, ntables: int):
    tables, factors, mask, pt = _big_zero_check(nvars, ntables)
    ctx = zk_amd.default_context(0)
    dev = [ctx.upload(2, tb) for tb in tables]
    proof = _prove_raw(ctx, _kzg(nvars), dev, factors, mask, 0, dev=True)
    return tables, factors, mask, pt, dev, proof


@pytest.mark.parametrize("nvars,ntables", [(10, 5), (10, 16), (14, 5), (14, 16)])
def test_large_proofs_are_accepted_and_public_evaluations_hold(ctx, nvars, ntables):
    tables, factors, mask, pt, dev, proof = _big_case(nvars, ntables)
    assert proof.rc == ZK_OK
    d = proof.as_dict(mask)
    k = _kzg(nvars)
    rc, ok, chal, _ = cc.verify_raw(d, factors, 0, k.g2_taus)
    assert (rc, ok) == (ZK_OK, 1) and chal == d["challenges"]
    # what the verifier leaves to the caller: the public tables at the challenges
    assert d["table_evals"][0] == zk_amd.MultilinearPoly.eq_eval(pt, chal, 2)
    assert d["table_evals"][0] == zk_amd.MultilinearPoly(as_limbs(tables[0]), 2, ctx).evaluate(chal)
    assert d["table_evals"][1] == 1 == zk_amd.MultilinearPoly(as_limbs(tables[1]), 2, ctx).evaluate(chal)
    cp = zk_amd.CommittedProof([zk_amd.UnivariatePoly(q, 2) for q in d["polys"]], 0, chal, d["table_evals"], mask,
                               d["commitments"], d["opening"])
    res = zk_amd.committed_verify(cp, 0, zk_amd.Transcript(2), factors, k.g2_taus,
                                  public_tables={0: tables[0], 1: tables[1]}, ctx=ctx)
    assert res.verified and res.random_challenges == chal
    wrong = zk_amd.committed_verify(cp, 0, zk_amd.Transcript(2), factors, k.g2_taus,
                                    public_tables={0: tables[1], 1: tables[1]}, ctx=ctx)
    assert not wrong.verified  # a public table that is not the one proved about
    for i, t in enumerate(dev[:3]):
        assert t.to_ints() == tables[i]  # the inputs are only read


@pytest.mark.parametrize("damage", sorted(cc.TAMPERINGS) + ["transcript"])
def test_damaged_gpu_proofs_are_rejected(ctx, damage):
    tables, factors, mask, pt, dev, proof = _big_case(10, 5)
    d = proof.as_dict(mask)
    g2 = _kzg(10).g2_taus
    if damage == "transcript":
        assert cc.verify_raw(d, factors, 0, g2, pre=cc.PRE_BYTES)[:2] == (ZK_OK, 0)
    else:
        cc.TAMPERINGS[damage](d)
        assert cc.verify_raw(d, factors, 0, g2)[:2] == (ZK_OK, 0)


def test_device_entry_equals_host_entry_and_commitments_in(ctx):
    tables, factors, mask, pt, dev, proof = _big_case(10, 5)
    k = _kzg(10)
    host = _prove_raw(ctx, k, tables, factors, mask, 0)
    assert host.rc == ZK_OK and host.same(proof)
    given = _prove_raw(ctx, k, dev, factors, mask, 0, dev=True, commitments_in=proof.cm)
    assert given.rc == ZK_OK and given.same(proof)
    # commitments handed in are absorbed and returned as given, not recomputed
    other = proof.cm.copy()
    other[[0, 1]] = other[[1, 0]]
    swapped = _prove_raw(ctx, k, dev, factors, mask, 0, dev=True, commitments_in=other)
    assert swapped.rc == ZK_OK and np.array_equal(swapped.cm, other) and not np.array_equal(swapped.ch, proof.ch)
    assert cc.verify_raw(swapped.as_dict(mask), factors, 0, k.g2_taus)[:2] == (ZK_OK, 0)
    # a transcript with history gives another proof, which verifies against the same history only
    pre = _prove_raw(ctx, k, dev, factors, mask, 0, dev=True, pre=cc.PRE_BYTES)
    assert not np.array_equal(pre.ch, proof.ch)
    assert cc.verify_raw(pre.as_dict(mask), factors, 0, k.g2_taus, pre=cc.PRE_BYTES)[:2] == (ZK_OK, 1)
    assert cc.verify_raw(pre.as_dict(mask), factors, 0, k.g2_taus)[:2] == (ZK_OK, 0)


def test_a_false_identity_is_rejected(ctx):
    tables, factors, mask, pt, dev, proof = _big_case(10, 5)
    k = _kzg(10)
    bad = [list(tb) for tb in tables]
    bad[4][137] = (bad[4][137] + 1) % R  # one entry of c
    got = _prove_raw(ctx, k, bad, factors, mask, 0)
    assert got.rc == ZK_OK
    assert cc.verify_raw(got.as_dict(mask), factors, 0, k.g2_taus)[:2] == (ZK_OK, 0)


def test_prove_error_paths_write_nothing(ctx):
    k = _kzg(3)
    tables, factors, mask = cc.shape("zero_check", 3)
    dev = [ctx.upload(2, tb) for tb in tables]
    fresh = zk_amd.Transcript(2).to_bytes()

    def code(**kw):
        use_dev = kw.pop("dev", True)
        r = _prove_raw(ctx, kw.pop("k", k), dev if use_dev else tables, kw.pop("factors", factors),
                       kw.pop("mask", mask), kw.pop("claim", 0), dev=use_dev, **kw)
        return r.rc, r.untouched() and r.state == fresh

    assert code()[0] == ZK_OK and code(dev=False)[0] == ZK_OK
    for dv in (True, False):
        assert code(dev=dv, mask=0) == (ZK_EINVAL, True)
        assert code(dev=dv, mask=mask | 1 << 6) == (ZK_EINVAL, True)      # a bit at ntables
        assert code(dev=dv, mask=1 << 20) == (ZK_EINVAL, True)
        assert code(dev=dv, k=_kzg(2), nvars=3) == (ZK_EINVAL, True)      # nvars is not the setup's
        assert code(dev=dv, nvars=0) == (ZK_EINVAL, True)
        assert code(dev=dv, claim=R) == (ZK_EINVAL, True)
        assert code(dev=dv, ntables=17) == (ZK_EUNSUPPORTED, True)        # the composed caps, unchanged
        assert code(dev=dv, factors=[[0, 1, 6]]) == (ZK_EINVAL, True)
        for null in ("tables", "factors", "claim", "t", "coeffs", "nco", "ch", "ev", "cs", "cm", "op", "kzg"):
            assert code(dev=dv, null=(null,)) == (ZK_EINVAL, True), null
    off = np.zeros((3, 12), np.uint64)
    off[0, 0] = off[0, 6] = 1                                             # (1, 1) is not on the curve
    assert code(commitments_in=off) == (ZK_EINVAL, True)
    big = [tables[0]] + [[R] + tb[1:] for tb in tables[1:2]] + tables[2:]
    r = _prove_raw(ctx, k, big, factors, mask, 0)                         # a table value >= p (host entry)
    assert r.rc == ZK_EINVAL and r.untouched() and r.state == fresh

"""The R1CS prover on the GPU through the C ABI: the row pass
(zk_r1cs_mul) and the column pass (zk_r1cs_matrix_evals, and a proof's second
sum-check) against the Python model on all fields over instances built to hit
every branch of the grouping; whole proofs equal to the model's byte for byte,
committed ones down to the G1 points; larger true instances accepted, false
ones and every kind of damage rejected; every error with nothing written.

Nothing written past 2^sx or 2^sy is checked with guard words behind the
outputs of zk_dev_r1cs_mul and zk_dev_r1cs_mul_t."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import random

import numpy as np
import pytest

import r1cs_cases as rc
import r1cs_oracle as ro
from pyoracle import MODULI

import zk_amd
from zk_amd import R1CS, MultilinearPoly, Transcript
from zk_amd._lib import ZK_EDEVICE, ZK_EINVAL, ZK_OK, lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import KZG, _g1_array

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL
SIZES = ("1_1", "1_2", "2_2", "3_2", "3_4")
EDGE_SIZES = (1, 255, 256, 257, 513)


def _r1cs(inst, ctx=None) -> R1CS:
    return R1CS(inst.field, inst.nrows, inst.sy, inst.npub, inst.A, inst.B, inst.C, ctx)


@functools.lru_cache(maxsize=None)
def _kzg(nvars: int) -> KZG:
    return KZG(rc.taus(nvars), zk_amd.default_context(0))


def _proof_dict(p) -> dict:
    return {"polys1": [q.coefficient for q in p.round_polys_1], "polys2": [q.coefficient for q in p.round_polys_2],
            "va": p.va, "vb": p.vb, "vc": p.vc, "vw": p.vw, "commitment": p.commitment, "opening": list(p.opening),
            "rx": p.rx, "ry": p.ry}


def _same(got: dict, want: dict) -> bool:
    return all(got[k] == want[k] for k in got)


# ---- the grouping's edges -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges(field: int, nrows: int = 1000, sy: int = 11):
    """One instance with: rows and columns of exactly 1, 255, 256, 257 and 513
    entries (single chunk, the cut, splits into 2 and 3 slots), a row and a
    column with none, one column read by every other row (nrows is no power of
    two), a (row, col) twice in one matrix and once in all three, values 0, 1,
    p - 1, and one row and one column that are each a whole chunk of 256
    entries p - 1 in one matrix: against x = p - 1 the largest accumulator.
    The counts are asserted below."""
    p = MODULI[field]
    rng = random.Random(900 + field)
    Y = 1 << sy
    ONE = Y // 2  # the constant column
    M = [[], [], []]
    val = lambda: rng.choice((0, 1, p - 1, rng.randrange(p), rng.randrange(p)))
    for k, n in enumerate(EDGE_SIZES):
        for j in range(n):  # row 10 + k has n entries in all: the constant column, then columns 101 ..
            M[rng.randrange(3)].append((10 + k, 100 + j if j else ONE, val()))
        for j in range(n):  # column 40 + k has n entries, rows 100 ..
            M[rng.randrange(3)].append((100 + j, 40 + k, val()))
    for r in range(nrows):  # the constant column, read by every row but the empty one (rows 10 .. 14 and 22 read it above / below)
        if r not in (7, 10, 11, 12, 13, 14, 22):
            M[r % 3].append((r, ONE, val()))
    M[0] += [(20, 700, 5), (20, 700, p - 3)]                      # twice in one matrix
    for m in M:
        m.append((21, 701, p - 1))                                # the same (row, col) in all three
    M[1] += [(22, 800 + j, p - 1) for j in range(256)]            # row 22: 256 products (p - 1)(p - 1) in one accumulator
    M[2] += [(300 + j, 45, p - 1) for j in range(256)]            # column 45: the same for the column pass
    for m in M:
        rng.shuffle(m)
    inst = ro.Instance(field, nrows, sy, 2, M[0], M[1], M[2])
    ent = [e for m in M for e in m]
    by_row, by_col = collections.Counter(e[0] for e in ent), collections.Counter(e[1] for e in ent)
    assert [by_row[10 + k] for k in range(5)] == list(EDGE_SIZES) == [by_col[40 + k] for k in range(5)]
    assert by_row[7] == 0 and by_col[39] == 0
    assert {e[0] for e in ent if e[1] == ONE} == set(range(nrows)) - {7}  # (800 + 224 is the constant column)
    assert by_col[ONE] > 3 * 256 and nrows & (nrows - 1)
    for key, which, t in ((22, 0, 1), (45, 1, 2)):  # a whole chunk of 256 entries p - 1, all in one matrix
        mine = [e for e in ent if e[which] == key]
        assert len(mine) == 256 and all(e[2] == p - 1 for e in mine)
        assert sum(1 for e in M[t] if e[which] == key) == 256
    return inst


@pytest.mark.parametrize("field", [0, 1, 2])
def test_row_pass_matches_the_model_on_the_grouping_edges(ctx, field):
    p = MODULI[field]
    inst = edges(field)
    r = _r1cs(inst, ctx)
    rng = random.Random(5)
    for z in ([p - 1] * (1 << inst.sy), [rng.randrange(p) for _ in range(1 << inst.sy)]):
        assert list(r.mul(z)) == ro.mul(inst, z)
    # the device entry, with guard words behind every output
    X = 1 << inst.sx
    z = [p - 1] * (1 << inst.sy)
    dz = ctx.upload(field, z)
    outs = [ctx.upload(field, [7] * (X + 8)) for _ in range(3)]
    assert lib().zk_dev_r1cs_mul(r.h, dz.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr) == ZK_OK
    for got, want in zip(outs, ro.mul(inst, z)):
        got = got.to_ints()
        assert got[:X] == want and got[X:] == [7] * 8, "wrote past 2^sx"
    r.close()


@pytest.mark.parametrize("field", [0, 1, 2])
def test_column_pass_matches_the_model_on_the_grouping_edges(ctx, field):
    p = MODULI[field]
    inst = edges(field)
    r, host = _r1cs(inst, ctx), _r1cs(inst)
    rng = random.Random(6)
    for _ in range(2):
        rx = [rng.randrange(p) for _ in range(inst.sx)]
        ry = [rng.randrange(p) for _ in range(inst.sy)]
        want = ro.matrix_evals(inst, rx, ry)
        assert r.matrix_evals(rx, ry) == want
        assert host.matrix_evals(rx, ry) == want
    rx, ry = [p - 1] * inst.sx, [0, 1, p - 1] + [p - 1] * (inst.sy - 3)
    assert r.matrix_evals(rx, ry) == ro.matrix_evals(inst, rx, ry)
    r.close()
    host.close()


@pytest.mark.parametrize("field", [0, 1, 2])
def test_column_pass_tables_and_guard_words(ctx, field):
    """the transposes themselves, entry by entry, with guard words behind every output"""
    p = MODULI[field]
    inst = edges(field)
    r = _r1cs(inst, ctx)
    X, Y = 1 << inst.sx, 1 << inst.sy
    rng = random.Random(8)
    for x in ([p - 1] * X, [rng.randrange(p) for _ in range(X)]):
        outs = [ctx.upload(field, [7] * (Y + 8)) for _ in range(3)]
        assert lib().zk_dev_r1cs_mul_t(r.h, ctx.upload(field, x).ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr) == ZK_OK
        for got, want in zip(outs, ro.mul_t(inst, x)):
            got = got.to_ints()
            assert got[:Y] == want and got[Y:] == [7] * 8, "wrote past 2^sy"
    assert ro.mul_t(inst, [1] * X)[0][39] == 0  # (the empty column is zeroed, not skipped)
    r.close()
    host = _r1cs(inst)
    assert lib().zk_dev_r1cs_mul_t(host.h, ctx.upload(field, [1] * X).ptr, ctx.upload(field, [7] * Y).ptr,
                                   ctx.upload(field, [7] * Y).ptr, ctx.upload(field, [7] * Y).ptr) == ZK_EDEVICE
    host.close()


@functools.lru_cache(maxsize=None)
def _edge_proof(field: int):
    """the edges instance is not satisfied; the model proves it all the same, and so must the device"""
    inst = edges(field)
    rng = random.Random(7 + field)
    p = MODULI[field]
    w = [rng.randrange(p) for _ in range(1 << (inst.sy - 1))]
    io = [p - 1, 1]
    return w, io, ro.prove(inst, w, io, ro.Transcript(field))


@pytest.mark.parametrize("field", [0, 1, 2])
def test_proof_over_the_grouping_edges_equals_the_model(ctx, field):
    """both passes inside a proof: M of the second sum-check comes from the column pass"""
    inst = edges(field)
    w, io, want = _edge_proof(field)
    r = _r1cs(inst, ctx)
    got = _proof_dict(r.prove(w, io, Transcript(field)))
    assert _same({k: got[k] for k in ("polys1", "va", "vb", "vc", "rx")}, want)
    assert _same({k: got[k] for k in ("polys2", "vw", "ry")}, want)
    assert not r.verify(r.prove(w, io, Transcript(field)), io, Transcript(field)).verified  # (not satisfied)
    r.close()


@pytest.mark.parametrize("field", [0, 2])
def test_wide_and_tall_and_empty_matrices(ctx, field):
    """sx > sy, sx < sy, and an empty C"""
    p = MODULI[field]
    rng = random.Random(11)
    for nrows, sy, per_row in ((300, 3, 2), (3, 9, 40)):
        inst, w, io = rc.random_instance(field, nrows, sy, 1, per_row, 200 + nrows)
        r = _r1cs(inst, ctx)
        z = ro.z_of(inst, w, io)
        assert list(r.mul(z)) == ro.mul(inst, z)
        rx = [rng.randrange(p) for _ in range(inst.sx)]
        ry = [rng.randrange(p) for _ in range(inst.sy)]
        assert r.matrix_evals(rx, ry) == ro.matrix_evals(inst, rx, ry)
        pr = r.prove(w, io, Transcript(field))
        assert _same(_proof_dict(pr), {**ro.prove(inst, w, io, ro.Transcript(field)), "commitment": None})
        assert r.verify(pr, io, Transcript(field)).verified
        r.close()
    inst, w, io = rc.random_instance(field, 6, 3, 1, 2, 300)
    inst = ro.Instance(field, 6, 3, 1, inst.A, inst.B, [])
    r = _r1cs(inst, ctx)
    z = ro.z_of(inst, w, io)
    assert list(r.mul(z)) == ro.mul(inst, z) and r.mul(z)[2] == [0] * 8
    rx, ry = [3, 4, 5], [6, 7, 8]
    assert r.matrix_evals(rx, ry) == ro.matrix_evals(inst, rx, ry) and r.matrix_evals(rx, ry)[2] == 0
    assert _same(_proof_dict(r.prove(w, io, Transcript(field))),
                 {**ro.prove(inst, w, io, ro.Transcript(field)), "commitment": None})
    r.close()


# ---- whole proofs against the model ---------------------------------------------
@pytest.mark.parametrize("name", SIZES + ("cubic", "chain5"))
@pytest.mark.parametrize("field", [0, 1, 2])
def test_uncommitted_proofs_equal_the_model(ctx, field, name):
    inst, w, io = rc.case(name, field)
    want = rc.model_proof(name, field)
    r = _r1cs(inst, ctx)
    tp, tm = Transcript(field), ro.Transcript(field)
    got = r.prove(w, io, tp)
    ro.prove(inst, w, io, tm)
    assert _same(_proof_dict(got), {**want, "commitment": None})
    dev = r.prove(ctx.upload(field, w), io, Transcript(field))  # the device entry
    assert _proof_dict(dev) == _proof_dict(got)
    tv = Transcript(field)
    res = r.verify(got, io, tv)
    assert res.verified and res.rx == want["rx"] and res.ry == want["ry"]
    assert tp.get_random_challenge() == tv.get_random_challenge() == tm.get_random_challenge()  # one state
    host = _r1cs(inst)
    assert host.verify(got, io, Transcript(field)).verified
    assert r.is_satisfied(w, io) and host.is_satisfied(w, io)
    host.close()
    r.close()


@pytest.mark.parametrize("name", ["1_2", "2_2", "3_2", "3_4", "cubic"])
def test_committed_proofs_equal_the_model(ctx, name):
    field = 2
    inst, w, io = rc.case(name, field)
    want = rc.model_proof(name, field, committed=True)
    kzg, g2 = _kzg(inst.sy - 1), rc.setup(inst.sy - 1)[1]
    r = _r1cs(inst, ctx)
    tp, tm = Transcript(field), ro.Transcript(field)
    got = r.prove(w, io, tp, kzg)
    ro.prove(inst, w, io, tm, rc.setup(inst.sy - 1)[0])
    assert got.committed and _same(_proof_dict(got), want)  # (the G1 points of the commitment and the opening too)
    dev = r.prove(ctx.upload(field, w), io, Transcript(field), kzg)
    assert _proof_dict(dev) == _proof_dict(got)
    again = r.prove(w, io, Transcript(field), kzg, commitment=got.commitment)  # commitment_in
    assert _proof_dict(again) == _proof_dict(got)
    tv = Transcript(field)
    assert r.verify(got, io, tv, g2).verified
    assert tp.get_random_challenge() == tv.get_random_challenge() == tm.get_random_challenge()
    host = _r1cs(inst)
    assert host.verify(got, io, Transcript(field), g2).verified
    assert not host.verify(got, io, Transcript(field), rc.other_g2(inst.sy - 1)).verified  # a wrong setup
    host.close()
    r.close()


# ---- larger true instances ------------------------------------------------------
def _damage(proof, field: int, how: str):
    import copy

    p = MODULI[field]
    q = copy.deepcopy(proof)
    if how in ("coefficient1", "coefficient2"):
        polys = q.round_polys_1 if how == "coefficient1" else q.round_polys_2
        c = polys[-1].coefficient
        if c:
            c[0] = (c[0] + 1) % p
        else:
            c.append(1)
    elif how in ("va", "vb", "vc", "vw"):
        setattr(q, how, (getattr(q, how) + 1) % p)
    elif how == "commitment":
        q.commitment = rc.another_point(q.commitment)
    elif how == "quotient":
        q.opening[0] = rc.another_point(q.opening[0])
    return q


@pytest.mark.parametrize("field,lg,committed", [(0, 10, False), (1, 10, False), (2, 10, False), (2, 14, True)])
def test_squaring_chains_are_accepted_and_false_ones_rejected(ctx, field, lg, committed):
    p = MODULI[field]
    inst, w, io = rc.chain(field, 1 << lg)
    assert (inst.sx, inst.sy) == (lg, lg + 1)
    r = _r1cs(inst, ctx)
    kzg = _kzg(inst.sy - 1) if committed else None
    g2 = kzg.g2_taus if committed else None
    assert r.is_satisfied(w, io)
    proof = r.prove(w, io, Transcript(field), kzg)
    res = r.verify(proof, io, Transcript(field), g2)
    assert res.verified and res.rx == proof.rx and res.ry == proof.ry
    z = r.z(w, io)
    az, bz, cz = r.mul(z)
    assert all(a * b % p == c for a, b, c in zip(az, bz, cz))
    for tab, v in zip((az, bz, cz), (proof.va, proof.vb, proof.vc)):  # va vb - vc from the tables themselves
        assert MultilinearPoly(tab, field, ctx).evaluate(res.rx) == v
    assert MultilinearPoly(w, field, ctx).evaluate(res.ry[1:]) == proof.vw
    # a false witness, and a true proof against other public values
    bad_w = list(w)
    bad_w[len(w) // 3] = (bad_w[len(w) // 3] + 1) % p
    assert not r.is_satisfied(bad_w, io)
    assert not r.verify(r.prove(bad_w, io, Transcript(field), kzg), io, Transcript(field), g2).verified
    assert not r.verify(proof, [(io[0] + 1) % p], Transcript(field), g2).verified
    hows = list(rc.TAMPERINGS) + (list(rc.TAMPERINGS_COMMITTED) if committed else [])
    for how in hows:
        assert not r.verify(_damage(proof, field, how), io, Transcript(field), g2).verified, how
    t = Transcript(field)
    t.append(rc.PRE_BYTES)
    assert not r.verify(proof, io, t, g2).verified
    r.close()


# ---- error paths: the code, and nothing written ---------------------------------
def _prove_raw(r, inst, w, io, kzg=None, repr_=0, null=(), device_w=None):
    L = lib()
    sx, sy = inst.sx, inst.sy
    bufs = {"c1": np.full((sx, 4, 4), SENTINEL, np.uint64), "n1": np.full(sx, 0xA5, np.uint8),
            "c2": np.full((sy, 3, 4), SENTINEL, np.uint64), "n2": np.full(sy, 0xA5, np.uint8),
            "ev": np.full((4, 4), SENTINEL, np.uint64), "rx": np.full((sx, 4), SENTINEL, np.uint64),
            "ry": np.full((sy, 4), SENTINEL, np.uint64), "cm": np.full((1, 12), SENTINEL, np.uint64),
            "op": np.full((max(sy - 1, 1), 12), SENTINEL, np.uint64)}
    t = L.zk_transcript_new()
    before = rc.transcript_bytes(t)
    args = {k: ptr(v) for k, v in bufs.items()}
    args.update(w=ptr(as_limbs(list(w))) if device_w is None else device_w.ptr, io=ptr(as_limbs(list(io))), t=t)
    for k in null:
        args[k] = None
    fn = L.zk_r1cs_prove if device_w is None else L.zk_dev_r1cs_prove
    code = fn(r.h, repr_, args["w"], args["io"], kzg.h if kzg is not None else None, None, args["t"], args["c1"],
              args["n1"], args["c2"], args["n2"], args["ev"], args["rx"], args["ry"], args["cm"], args["op"])
    untouched = all(bool((v == (0xA5 if v.dtype == np.uint8 else SENTINEL)).all()) for v in bufs.values())
    untouched = untouched and rc.transcript_bytes(t) == before
    L.zk_transcript_free(t)
    return code, untouched


def test_error_paths_write_nothing(ctx):
    field = 2
    p = MODULI[field]
    inst, w, io = rc.case("3_4", field)
    r, host = _r1cs(inst, ctx), _r1cs(inst)
    assert _prove_raw(r, inst, w, io) == (ZK_OK, False)
    for null in ("w", "io", "t", "c1", "n1", "c2", "n2", "ev", "rx", "ry"):
        assert _prove_raw(r, inst, w, io, null=(null,)) == (ZK_EINVAL, True), null
        assert _prove_raw(r, inst, w, io, null=(null,), device_w=ctx.upload(field, w)) == (ZK_EINVAL, True), null
    assert _prove_raw(r, inst, w, io, repr_=2) == (ZK_EINVAL, True)
    assert _prove_raw(r, inst, w, [p] + io[1:]) == (ZK_EINVAL, True)              # io >= p
    assert _prove_raw(r, inst, w, io, kzg=_kzg(2)) == (ZK_EINVAL, True)            # a setup of other than sy - 1 variables
    for null in ("cm", "op"):
        assert _prove_raw(r, inst, w, io, kzg=_kzg(3), null=(null,)) == (ZK_EINVAL, True), null
    assert _prove_raw(host, inst, w, io) == (ZK_EDEVICE, True)                     # a host-only handle cannot prove
    inst0, w0, io0 = rc.case("3_4", 0)
    r0 = _r1cs(inst0, ctx)
    assert _prove_raw(r0, inst0, w0, io0, kzg=_kzg(3)) == (ZK_EINVAL, True)        # KZG is BLS12-381 Fr only
    r0.close()
    # verify: every error with nothing written, a rejection with nothing but the verdict
    proof = rc.model_proof("3_4", field, committed=True)
    g2 = rc.setup(3)[1]
    assert rc.verify_raw(r.h, inst, proof, io, g2)[:2] == (ZK_OK, 1)
    for null in ("c1", "n1", "c2", "n2", "ev", "t", "ok", "rx", "ry", "io", "cm", "op", "g2"):
        res = rc.verify_raw(r.h, inst, proof, io, g2, null=(null,))
        assert (res[0], res[4]) == (ZK_EINVAL, True), null
    bad = dict(proof, commitment=(proof["commitment"][0], 1))
    res = rc.verify_raw(r.h, inst, bad, io, g2)
    assert (res[0], res[4]) == (ZK_EINVAL, True)                                   # a commitment off the curve
    res = rc.verify_raw(r.h, inst, dict(proof, va=p), io, g2)
    assert (res[0], res[4]) == (ZK_EINVAL, True)
    res = rc.verify_raw(r.h, inst, rc.damaged(proof, field, "vw"), io, g2)
    assert res[:2] == (ZK_OK, 0) and res[4]
    # mul and matrix_evals
    X, Y = 1 << inst.sx, 1 << inst.sy
    outs = [np.full((X, 4), SENTINEL, np.uint64) for _ in range(3)]
    z = as_limbs([p] + [1] * (Y - 1))
    assert lib().zk_r1cs_mul(r.h, 0, ptr(z), ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert all(bool((o == SENTINEL).all()) for o in outs)
    assert lib().zk_r1cs_mul(r.h, 0, None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert lib().zk_dev_r1cs_mul(host.h, ctx.upload(field, [1] * Y).ptr, ctx.upload(field, [7] * X).ptr,
                                 ctx.upload(field, [7] * X).ptr, ctx.upload(field, [7] * X).ptr) == ZK_EDEVICE
    out = np.full((3, 4), SENTINEL, np.uint64)
    pt = as_limbs([p] * 4)
    assert lib().zk_r1cs_matrix_evals(r.h, 0, ptr(pt), ptr(pt), ptr(out)) == ZK_EINVAL
    assert bool((out == SENTINEL).all())
    r.close()
    host.close()

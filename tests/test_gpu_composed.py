"""The composed sum-check on the GPU through the C ABI. The
four-table shape must give zk_gkr_sumcheck_prove's bytes; small proofs of every
degree must equal the dense model (tests/composed_oracle.py) exactly; the
device path must equal the host path (csrc/composed_plan.hpp, which the CPU
tests compare with the model); the device-resident call must equal the
host-memory one and leave its inputs alone; a 2^18-entry proof, too large for
the model, is checked by soundness. Each case makes its own Context so that the
knobs it sets are the ones read."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import composed_oracle as cm
import pyoracle as po

import zk_amd
from zk_amd._lib import ZK_EINVAL, ZK_EUNSUPPORTED, ZK_OK, lib
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5A5A5A5A5A5A5A5
KNOBS = ("ZK_COMPOSED_HOST_LG", "ZK_ATOMIC_FANIN", "ZK_GRID_CAP")


def _context(monkeypatch, **knobs):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, str(value))
    return zk_amd.Context(0)


def _tables(field, ntables, nvars, seed):
    return [as_limbs(tb) for tb in cm.random_tables(field, ntables, nvars, seed)]


class Raw:
    """One call's raw outputs, pre-filled with a sentinel."""

    def __init__(self, nvars, ntables, width):
        n = max(nvars, 1)
        self.coeffs = np.full((n, width, 4), SENTINEL, np.uint64)
        self.nco = np.full(n, 0xEE, np.uint8)
        self.ch = np.full((n, 4), SENTINEL, np.uint64)
        self.ev = np.full((max(ntables, 1), 4), SENTINEL, np.uint64)
        self.cs = np.full((1, 4), SENTINEL, np.uint64)
        self.state = b""
        self.rc = None

    def untouched(self):
        return all((a == SENTINEL).all() for a in (self.coeffs, self.ch, self.ev, self.cs)) and (self.nco == 0xEE).all()

    def same_proof(self, other):
        return (np.array_equal(self.coeffs, other.coeffs) and np.array_equal(self.nco, other.nco)
                and np.array_equal(self.ch, other.ch) and self.state == other.state)

    def polys(self):
        return [to_ints(self.coeffs[k, : self.nco[k]]) for k in range(len(self.nco))]


def _composed(ctx, field, tables, factors, claim, dev=False, nvars=None, ntables=None, nterms=None, degree=None,
              claim_limbs=None, repr_=0):
    """zk_composed_sumcheck_prove (tables: uint64[n, 4] arrays) or, dev=True, zk_dev_composed_sumcheck_prove
    (tables: DeviceTable); the keyword overrides feed the error-path cases."""
    n = nvars if nvars is not None else (tables[0].shape[0] if not dev else tables[0].count).bit_length() - 1
    nt = ntables if ntables is not None else len(tables)
    fac = np.array([f for term in factors for f in term], np.uint8)
    nterms = nterms if nterms is not None else len(factors)
    degree = degree if degree is not None else len(factors[0])
    arr = (C.c_void_p * max(len(tables), 1))(*[(t.ptr.value if dev else t.ctypes.data) for t in tables])
    out = Raw(min(n, 26), nt, min(degree, 8) + 1)
    t = zk_amd.Transcript(field if field in (0, 1, 2) else 0)
    fn = lib().zk_dev_composed_sumcheck_prove if dev else lib().zk_composed_sumcheck_prove
    cl = claim_limbs if claim_limbs is not None else as_limbs([claim])
    out.rc = fn(ctx.h, field, repr_, arr, nt, n, ptr(fac), nterms, degree, ptr(cl), t.h, ptr(out.coeffs), ptr(out.nco),
                ptr(out.ch), ptr(out.ev), ptr(out.cs))
    out.state = t.to_bytes()
    return out


def _gkr(ctx, field, tables, claim):
    n = tables[0].shape[0].bit_length() - 1
    out = Raw(n, 4, 3)
    arr = (C.c_void_p * 4)(*[t.ctypes.data for t in tables])
    t = zk_amd.Transcript(field)
    out.rc = lib().zk_gkr_sumcheck_prove(ctx.h, field, 0, arr, n, ptr(as_limbs([claim])), t.h, ptr(out.coeffs),
                                         ptr(out.nco), ptr(out.ch), ptr(out.cs))
    out.state = t.to_bytes()
    return out


# ---- the four-table shape against the existing prover --------------------------
@pytest.mark.parametrize("host_lg", ["0", None])
def test_four_table_shape_gives_gkr_proves_bytes(monkeypatch, host_lg):
    ctx = _context(monkeypatch, **({} if host_lg is None else {"ZK_COMPOSED_HOST_LG": host_lg}))
    try:
        for field, nvars in [(0, n) for n in range(1, 15)] + [(1, 10), (2, 10)]:
            tabs = _tables(field, 4, nvars, 4000 + 20 * field + nvars)
            got = _composed(ctx, field, tabs, cm.SHAPES["gkr4"][1], 99)
            want = _gkr(ctx, field, tabs, 99)
            assert got.rc == want.rc == ZK_OK
            assert got.same_proof(want) and np.array_equal(got.cs, want.cs), (field, nvars)
    finally:
        ctx.close()


# ---- against the dense model, every round on the device ------------------------
# nvars 1: the first-round kernel only, one pair; 2, 3: the fused kernel at h = 1, 2; 9: one block; 10: two
# blocks, atomic fan-in; 12 with ZK_ATOMIC_FANIN=4: eight blocks through the two-level fan-in; 12 with
# ZK_GRID_CAP=2: every thread loops four times; 14: the largest model-checked size
MODEL_CASES = [(1, {}), (2, {}), (3, {}), (9, {}), (10, {}), (12, {"ZK_ATOMIC_FANIN": 4}), (12, {"ZK_GRID_CAP": 2}),
               (14, {})]
_model_cache: dict = {}


def _model(shape, field, nvars):
    key = (shape, field, nvars)
    if key not in _model_cache:
        ntables, factors = cm.SHAPES[shape]
        ints = cm.random_tables(field, ntables, nvars, 5000 + nvars)
        _model_cache[key] = (ints, cm.prove(field, 7, ints, factors, po.Transcript(field)))
    return _model_cache[key]


@pytest.mark.parametrize("nvars,knobs", MODEL_CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("shape", ["deg1", "deg2", "deg3", "deg4", "deg3_shared"])
def test_device_rounds_equal_the_dense_model(monkeypatch, shape, nvars, knobs):
    field = {"deg1": 1, "deg2": 2}.get(shape, 0)
    factors = cm.SHAPES[shape][1]
    ints, (polys, _, chal, evals) = _model(shape, field, nvars)
    ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=0, **knobs)
    try:
        got = _composed(ctx, field, [as_limbs(tb) for tb in ints], factors, 7)
        assert got.rc == ZK_OK
        assert got.polys() == polys
        assert to_ints(got.ch) == chal and to_ints(got.ev) == evals and to_ints(got.cs) == [7]
        st = ctx.stats()["kernels"]
        assert st["gkr_round0"]["launches"] == 1 and st["gkr_round"]["launches"] == nvars - 1
    finally:
        ctx.close()


# ---- the device path against the host path -------------------------------------
@pytest.mark.parametrize("field", [0, 1, 2])
def test_device_path_equals_host_path(monkeypatch, field):
    tabs = _tables(field, 4, 12, 6000 + field)
    factors = cm.SHAPES["deg3_shared"][1]
    res = []
    for lg in (0, 12):
        ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=lg)
        try:
            res.append(_composed(ctx, field, tabs, factors, 1))
            launches = sum(ctx.stats()["kernels"][k]["launches"] for k in ("gkr_round0", "gkr_round"))
            assert launches == (12 if lg == 0 else 0)
        finally:
            ctx.close()
    assert res[0].rc == res[1].rc == ZK_OK
    assert res[0].same_proof(res[1]) and np.array_equal(res[0].ev, res[1].ev)


# ---- device-resident tables ---------------------------------------------------
@pytest.mark.parametrize("host_lg", ["0", None])
def test_device_resident_call_equals_host_memory_call(monkeypatch, host_lg):
    ctx = _context(monkeypatch, **({} if host_lg is None else {"ZK_COMPOSED_HOST_LG": host_lg}))
    try:
        for field, shape, nvars in ((0, "deg3_shared", 11), (2, "deg4", 8), (1, "deg1", 3), (0, "deg3", 0)):
            ntables, factors = cm.SHAPES[shape]
            tabs = _tables(field, ntables, nvars, 6100 + nvars)
            dts = [ctx.upload(field, t) for t in tabs]
            before = [d.download(1) for d in dts]
            got = _composed(ctx, field, dts, factors, 3, dev=True)
            want = _composed(ctx, field, tabs, factors, 3)
            assert got.rc == want.rc == ZK_OK
            assert got.same_proof(want) and np.array_equal(got.ev, want.ev) and np.array_equal(got.cs, want.cs)
            for d, b, t in zip(dts, before, tabs):  # inputs read-only
                assert np.array_equal(d.download(1), b) and np.array_equal(d.download(0), t)
            if nvars == 0:
                assert to_ints(got.ev) == [to_ints(t)[0] for t in tabs]
            for d in dts:
                d.free()
    finally:
        ctx.close()


# ---- a size the model cannot reach: soundness -----------------------------------
def test_2_18_entries_degree_3_verifies(monkeypatch):
    field, nvars = 0, 18
    p = po.MODULI[field]
    rng = np.random.default_rng(18)
    limbs = [rng.integers(0, 1 << 64, size=(1 << nvars, 4), dtype=np.uint64) for _ in range(3)]
    for a in limbs:
        a[:, 3] &= np.uint64((1 << 60) - 1)  # below p
    ints = [to_ints(a) for a in limbs]
    true = sum(e * a * b for e, a, b in zip(*ints)) % p
    factors = cm.SHAPES["deg3"][1]
    ctx = _context(monkeypatch)
    try:
        mles = [zk_amd.MultilinearPoly(a, field, ctx) for a in limbs]
        sp = zk_amd.SumPoly([zk_amd.ProductPoly.from_polys(mles)])
        assert sp.composed_tables()[1] == factors
        proof = zk_amd.composed_prove(true, sp, zk_amd.Transcript(field), ctx)
        v = zk_amd.composed_verify(proof.proof_polynomials, true, zk_amd.Transcript(field), 3)
        assert v.verified and v.random_challenges == proof.random_challenges and proof.claimed_sum == true
        assert v.final_claimed_sum == zk_amd.composed_combine(proof.table_evals, factors, field)
        for m, e in zip(mles, proof.table_evals):
            assert m.evaluate(proof.random_challenges) == e
        bad = zk_amd.composed_verify(proof.proof_polynomials, (true + 1) % p, zk_amd.Transcript(field), 3)
        assert not bad.verified
    finally:
        ctx.close()


# ---- claimed_sum is carried, never used -----------------------------------------
def test_a_wrong_claimed_sum_gives_the_same_round_polynomials(monkeypatch):
    ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=3)
    try:
        ntables, factors = cm.SHAPES["deg3_shared"]
        tabs = _tables(0, ntables, 10, 6200)
        true = cm.true_sum(po.MODULI[0], [to_ints(t) for t in tabs], factors)
        a, b = _composed(ctx, 0, tabs, factors, true), _composed(ctx, 0, tabs, factors, (true + 5) % po.MODULI[0])
        assert a.rc == b.rc == ZK_OK and a.same_proof(b) and np.array_equal(a.ev, b.ev)
        assert to_ints(a.cs) == [true] and to_ints(b.cs) == [(true + 5) % po.MODULI[0]]
    finally:
        ctx.close()


# ---- error paths: the code, and nothing written -----------------------------------
def test_error_paths_write_nothing(monkeypatch):
    ctx = _context(monkeypatch)
    try:
        p = po.MODULI[0]
        tabs = _tables(0, 3, 4, 6300)
        dts = [ctx.upload(0, t) for t in tabs]
        f3 = [[0, 1, 2]]
        for dev, tt in ((False, tabs), (True, dts)):
            def call(**kw):
                r = _composed(ctx, kw.pop("field", 0), kw.pop("tables", tt), kw.pop("factors", f3), 1, dev=dev, nvars=4, **kw)
                assert r.untouched(), kw
                return r.rc
            assert _composed(ctx, 0, tt, f3, 1, dev=dev).rc == ZK_OK
            assert call(ntables=0) == ZK_EINVAL
            assert call(nterms=0) == ZK_EINVAL
            assert call(degree=0) == ZK_EINVAL
            assert call(factors=[[0, 1, 3]]) == ZK_EINVAL           # a factor index >= ntables
            assert call(field=3) == ZK_EINVAL                        # unknown field
            assert call(repr_=2) == ZK_EINVAL                        # unknown repr
            assert call(claim_limbs=as_limbs([p])) == ZK_EINVAL      # claimed sum >= p
            assert call(ntables=17) == ZK_EUNSUPPORTED
            assert call(nterms=17, factors=[[0, 1, 2]] * 17) == ZK_EUNSUPPORTED
            assert call(degree=5, factors=[[0, 1, 2, 0, 1]]) == ZK_EUNSUPPORTED
            r = _composed(ctx, 0, tt, f3, 1, dev=dev, nvars=27)
            assert r.rc == ZK_EUNSUPPORTED and r.untouched()
            nulls = (C.c_void_p * 3)(tt[0].ptr.value if dev else tt[0].ctypes.data, None, None)
            out = Raw(4, 3, 4)
            t = zk_amd.Transcript(0)
            fn = lib().zk_dev_composed_sumcheck_prove if dev else lib().zk_composed_sumcheck_prove
            fac = np.array([0, 1, 2], np.uint8)
            args = [ctx.h, 0, 0, nulls, 3, 4, ptr(fac), 1, 3, ptr(as_limbs([1])), t.h, ptr(out.coeffs), ptr(out.nco),
                    ptr(out.ch), ptr(out.ev), ptr(out.cs)]
            assert fn(*args) == ZK_EINVAL and out.untouched()       # a null table
            for i in (0, 3, 6, 9, 10, 11, 12, 13, 14, 15):          # every pointer argument null in turn
                a = list(args)
                a[3] = (C.c_void_p * 3)(*[(x.ptr.value if dev else x.ctypes.data) for x in tt])
                a[i] = None
                assert fn(*a) == ZK_EINVAL and out.untouched(), i
        bad = [t.copy() for t in tabs]
        bad[1][5] = as_limbs([p])[0]
        r = _composed(ctx, 0, bad, f3, 1)                            # a table value >= p
        assert r.rc == ZK_EINVAL and r.untouched()
        for d in dts:
            d.free()
    finally:
        ctx.close()

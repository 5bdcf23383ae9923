"""The lookup argument on the GPU: the batched inversion at the
edges of its plan, the multiplicity count on the hash's hard cases, and proofs
equal to tests/lookup_oracle.py byte for byte, accepted, and rejected when
damaged. Nothing written past an output's end is checked with guard words
behind it."""
from __future__ import annotations

import ctypes as C
import functools
import random

import numpy as np
import pytest

import lookup_cases as lc
import lookup_oracle as lo
from pyoracle import MODULI
from r1cs_cases import taus

import zk_amd
from zk_amd import Lookup, _lib
from zk_amd.elems import as_limbs, ptr
from zk_amd.kzg import KZG, _g1_array

pytestmark = pytest.mark.gpu

EINVAL, EDEVICE, EUNSUPPORTED = 1, 2, 5
RUN, WAVE, BLOCK = lc.RUN, lc.WAVE, lc.BLOCK
# one below, at and above every size at which the kernel's shape changes: a
# lane's second element, a full wave tile, a full block tile, two block tiles
EDGES = [RUN * WAVE, RUN * BLOCK, 2 * RUN * BLOCK]
COUNTS = [1, 63, 64, 65] + [e + d for e in EDGES for d in (-1, 0, 1)]
assert (RUN, WAVE, BLOCK) == (64, 64, 256) and COUNTS[4:] == [4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769]
GUARD = 8


@functools.lru_cache(maxsize=None)
def _values(field: int, count: int):
    """random values with 1 and p - 1 among them and a zero at both ends, and their inverses"""
    p = MODULI[field]
    rng = random.Random(count * 3 + field)
    v = [rng.randrange(1, p) for _ in range(count)]
    for i, x in ((count // 3, 1), (count // 2, p - 1), (0, 0), (count - 1, 0)):
        v[i] = x
    return v, [pow(x, p - 2, p) for x in v]


def _inverse_checked(ctx, field: int, v, want):
    """out of place behind guard words, in place, and the host entry: all equal `want`"""
    L = _lib.lib()
    n = len(v)
    src = ctx.upload(field, v)
    dst = ctx.upload(field, [7] * (n + GUARD))
    assert L.zk_dev_fe_batch_inverse(ctx.h, field, src.ptr, n, dst.ptr) == 0, L.zk_last_error()
    got = dst.to_ints()
    assert got[:n] == want and got[n:] == [7] * GUARD, "wrote past count"
    assert src.to_ints() == v, "the input was changed"
    inp = ctx.upload(field, v + [7] * GUARD)
    assert L.zk_dev_fe_batch_inverse(ctx.h, field, inp.ptr, n, inp.ptr) == 0, L.zk_last_error()
    got = inp.to_ints()
    assert got[:n] == want and got[n:] == [7] * GUARD, "in place: wrong, or wrote past count"
    for t in (src, dst, inp):
        t.free()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("field", [0, 1, 2])
def test_batch_inverse_at_the_plan_edges(ctx, field, count):
    v, want = _values(field, count)
    _inverse_checked(ctx, field, v, want)
    if count <= 4097:  # device entry equals host entry
        assert zk_amd.batch_inverse(v, field) == want == zk_amd.batch_inverse(v, field, ctx)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_batch_inverse_zero_patterns(ctx, field):
    count = 2 * RUN * WAVE + 1
    base, inv = _values(field, count)
    lane_run = [1 * RUN * WAVE + 5 + WAVE * k for k in range(RUN)]  # wave 1, lane 5: its whole run
    wave_tile = list(range(0, RUN * WAVE))                          # wave 0: everything it owns
    for zeros in (lane_run, wave_tile, lane_run[:-1], range(count)):
        v, want = list(base), list(inv)
        for i in zeros:
            v[i] = want[i] = 0
        _inverse_checked(ctx, field, v, want)


def test_batch_inverse_errors(ctx):
    L = _lib.lib()
    t = ctx.upload(2, [3, 4, 5, 6, 7, 8])
    before = t.to_ints()
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, t.ptr, 4, C.c_void_p(t.ptr.value + 32)) == EINVAL  # partial overlap
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, C.c_void_p(t.ptr.value + 64), 4, t.ptr) == EINVAL
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, t.ptr, 0, t.ptr) == EINVAL
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, None, 4, t.ptr) == EINVAL
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, t.ptr, 4, None) == EINVAL
    assert L.zk_dev_fe_batch_inverse(None, 2, t.ptr, 4, t.ptr) == EINVAL
    assert L.zk_dev_fe_batch_inverse(ctx.h, 3, t.ptr, 4, t.ptr) == EINVAL
    assert t.to_ints() == before
    # disjoint halves of one buffer are fine
    assert L.zk_dev_fe_batch_inverse(ctx.h, 2, t.ptr, 3, C.c_void_p(t.ptr.value + 96)) == 0
    assert t.to_ints() == before[:3] + [pow(x, lo.R - 2, lo.R) for x in before[:3]]


# ---- multiplicities -------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.COUNT_CASES)
@pytest.mark.parametrize("field", [0, 1, 2])
def test_multiplicities_match_the_model(ctx, field, name):
    table, f, n = lc.case(name, field)
    want_m, want_missing = lo.multiplicities(table, f, n)
    N = 1 << n
    lk = Lookup(table, ctx, field)
    assert lk.slots() == lo.hash_slots(table)
    df = ctx.upload(field, f)
    dm = ctx.upload(field, [7] * (N + GUARD))
    missing = C.c_uint64(1 << 40)
    L = _lib.lib()
    for _ in range(2):  # the counters are zeroed on every call
        assert L.zk_dev_lookup_multiplicities(lk.h, df.ptr, len(f), dm.ptr, n, C.byref(missing)) == 0, L.zk_last_error()
        got = dm.to_ints()
        assert got[:N] == want_m and got[N:] == [7] * GUARD, "wrong, or wrote past 2^n"
        assert missing.value == want_missing
    assert df.to_ints() == f
    assert lk.multiplicities(f, n) == (want_m, want_missing)  # the host entry, through the device
    if name == "one_value":
        assert want_m[0] == 1 << 12
    if name == "odd_T":  # fewer entries than slots, and more slots than the column needs
        assert L.zk_dev_lookup_multiplicities(lk.h, df.ptr, 3, dm.ptr, n, C.byref(missing)) == 0
        assert dm.to_ints()[:N] == lo.multiplicities(table, f[:3], n)[0] and missing.value == 0
    lk.close()


def test_multiplicities_errors(ctx):
    L = _lib.lib()
    lk = Lookup([3, 4, 5, 6, 7], ctx)
    df = ctx.upload(2, [3, 4, 5, 6] + [7] * 8)
    dm = ctx.upload(2, [7] * 8)
    miss = C.c_uint64(99)
    for args in [(None, 4, dm.ptr, 3, C.byref(miss)), (df.ptr, 4, None, 3, C.byref(miss)), (df.ptr, 4, dm.ptr, 3, None),
                 (df.ptr, 0, dm.ptr, 3, C.byref(miss)), (df.ptr, 4, dm.ptr, 0, C.byref(miss)),
                 (df.ptr, 4, dm.ptr, 2, C.byref(miss)), (df.ptr, 4, C.c_void_p(df.ptr.value + 32), 3, C.byref(miss))]:
        assert L.zk_dev_lookup_multiplicities(lk.h, *args) == EINVAL
    assert L.zk_dev_lookup_multiplicities(lk.h, df.ptr, 4, dm.ptr, 25, C.byref(miss)) == EUNSUPPORTED
    assert L.zk_dev_lookup_multiplicities(lk.h, df.ptr, (1 << 24) + 1, dm.ptr, 3, C.byref(miss)) == EUNSUPPORTED
    assert dm.to_ints() == [7] * 8 and miss.value == 99
    host = Lookup([3, 4, 5, 6, 7])
    assert L.zk_dev_lookup_multiplicities(host.h, df.ptr, 4, dm.ptr, 3, C.byref(miss)) == EDEVICE
    lk.close()
    host.close()


# ---- proofs -----------------------------------------------------------------------------
def _kzg(nvars: int) -> KZG:
    return KZG(taus(nvars), zk_amd.default_context(0))


def _as_dict(p) -> dict:
    return {"n": p.n, "polys": [list(q.coefficient) for q in p.round_polys], "table_evals": list(p.table_evals),
            "commitments": list(p.commitments), "opening": list(p.opening), "missing": p.missing, "point": list(p.point)}


KEYS = ("polys", "table_evals", "commitments", "opening", "missing", "point")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_proofs_equal_the_model(ctx, n):
    table, f = lc.small(n)
    want = lc.model_proof(n)
    lk = Lookup(table, ctx)
    kzg = _kzg(n)
    t = zk_amd.Transcript(2)
    got = _as_dict(lk.prove(f, t, kzg))
    for k in KEYS:
        assert got[k] == want[k], k
    assert t.get_random_challenge() == want["end_state"]
    # the device entry, with f's commitment handed in
    t2 = zk_amd.Transcript(2)
    dev = _as_dict(lk.prove(ctx.upload(2, f), t2, kzg, commitment=want["commitments"][lo.F]))
    assert dev == got and t2.get_random_challenge() == want["end_state"]
    # verified by the device handle and by a host-only one, the transcripts ending where the prover's did
    for verifier in (lk, Lookup(table)):
        tv = zk_amd.Transcript(2)
        res = verifier.verify(zk_amd.LookupProof(n, got["polys"], got["table_evals"], got["commitments"], got["opening"]),
                              tv, kzg.g2_taus)
        assert res.verified and res.point == want["point"]
        assert tv.get_random_challenge() == want["end_state"]
    # a column with a non-member: proved all the same, reported, rejected
    table_m, f_m = lc.small(n, missing=True)
    want_m = lc.model_proof(n, missing=True)
    lkm = Lookup(table_m, ctx)
    got_m = lkm.prove(f_m, zk_amd.Transcript(2), kzg)
    assert got_m.missing == 1
    for k in KEYS:
        assert _as_dict(got_m)[k] == want_m[k], k
    assert not lkm.verify(got_m, zk_amd.Transcript(2), kzg.g2_taus).verified
    lk.close()
    lkm.close()


@functools.lru_cache(maxsize=None)
def _range_check(bad: bool):
    """4096 random bytes against t = 0 .. 255 (bad: one entry is 256) -> (column, proof, end state)"""
    n = 12
    rng = random.Random(12)
    f = [rng.randrange(256) for _ in range(1 << n)]
    if bad:
        f[1234] = 256
    lk = Lookup(list(range(256)), zk_amd.default_context(0))
    t = zk_amd.Transcript(2)
    proof = lk.prove(f, t, _kzg(n))
    lk.close()
    return f, proof, t.get_random_challenge()


def test_range_check_accepted(ctx):
    f, proof, end = _range_check(False)
    assert proof.missing == 0 and len(proof.round_polys) == 12
    t = zk_amd.Transcript(2)
    res = Lookup(list(range(256))).verify(proof, t, _kzg(12).g2_taus)
    assert res.verified and res.point == proof.point and t.get_random_challenge() == end
    assert proof.table_evals[lo.F] == zk_amd.MultilinearPoly(f, 2, ctx).evaluate(proof.point)
    m, _ = lo.multiplicities(list(range(256)), f, 12)
    assert proof.table_evals[lo.M] == zk_amd.MultilinearPoly(m, 2, ctx).evaluate(proof.point)
    assert proof.table_evals[lo.ONE] == 1 and proof.table_evals[lo.NEG] == lo.R - 1


def test_range_check_with_a_non_member_rejected(ctx):
    _, proof, _ = _range_check(True)
    assert proof.missing == 1
    assert not Lookup(list(range(256))).verify(proof, zk_amd.Transcript(2), _kzg(12).g2_taus).verified


@pytest.mark.parametrize("how", sorted(lc.TAMPERINGS))
def test_damaged_device_proof_rejected(ctx, how):
    _, proof, _ = _range_check(False)
    q = lc.damaged(_as_dict(proof), how)
    h = lc.handle(list(range(256)))
    rc, ok, _, _, untouched = lc.verify_raw(h, q, _kzg(12).g2_taus)
    assert (rc, ok) == (0, 0) and untouched
    _lib.lib().zk_lookup_free(h)


def test_other_statements_rejected(ctx):
    _, proof, _ = _range_check(False)
    q = _as_dict(proof)
    g2 = _kzg(12).g2_taus
    h = lc.handle(list(range(256)))
    assert lc.verify_raw(h, q, g2)[:2] == (0, 1)
    assert lc.verify_raw(h, q, g2, pre=lc.PRE_BYTES)[1::3] == (0, True)           # other bytes absorbed first
    assert lc.verify_raw(h, q, KZG([x + 1 for x in taus(12)], ctx).g2_taus)[1::3] == (0, True)  # a wrong setup
    _lib.lib().zk_lookup_free(h)
    h2 = lc.handle([0, 1, 3] + list(range(3, 256)))  # a changed table entry
    assert lc.verify_raw(h2, q, g2)[1::3] == (0, True)
    _lib.lib().zk_lookup_free(h2)


def _prove_raw(lk, f, n, kzg, null=(), repr_=0, device=None, n_arg=None, cin=None):
    """-> (rc, nothing written and the transcript unchanged)"""
    L = _lib.lib()
    t = L.zk_transcript_new()
    before = lc.transcript_bytes(t)
    outs = {"cf": np.full((n, 4, 4), lc.SENTINEL, np.uint64), "ev": np.full((11, 4), lc.SENTINEL, np.uint64),
            "pt": np.full((n, 4), lc.SENTINEL, np.uint64), "cm": np.full((4, 12), lc.SENTINEL, np.uint64),
            "op": np.full((n, 12), lc.SENTINEL, np.uint64)}
    nco = np.full(n, 0xA5, np.uint8)
    miss = C.c_uint64(99)
    a = {"f": device.ptr if device is not None else ptr(as_limbs(f)), "kzg": kzg.h if kzg is not None else None,
         "cin": cin, "t": t, "nco": ptr(nco), "miss": C.byref(miss), **{k: ptr(v) for k, v in outs.items()}}
    for k in null:
        a[k] = None
    fn = L.zk_dev_lookup_prove if device is not None else L.zk_lookup_prove
    rc = fn(lk.h, repr_, a["f"], n if n_arg is None else n_arg, a["kzg"], a["cin"], a["t"], a["cf"], a["nco"], a["ev"],
            a["pt"], a["cm"], a["op"], a["miss"])
    clean = (all((v == lc.SENTINEL).all() for v in outs.values()) and (nco == 0xA5).all() and miss.value == 99
             and lc.transcript_bytes(t) == before)
    L.zk_transcript_free(t)
    return rc, clean


def test_prove_errors_write_nothing(ctx):
    n = 3
    table, f = lc.small(n)
    lk, kzg = Lookup(table, ctx), _kzg(n)
    df = ctx.upload(2, f)
    assert _prove_raw(lk, f, n, kzg)[0] == 0
    for dev in (None, df):
        for null in ("f", "kzg", "t", "cf", "nco", "ev", "pt", "cm", "op", "miss"):
            rc, clean = _prove_raw(lk, f, n, kzg, null=(null,), device=dev)
            assert rc == EINVAL and (clean or null == "t"), null
        assert _prove_raw(lk, f, n, kzg, repr_=2, device=dev) == (EINVAL, True)
        assert _prove_raw(lk, f, n, kzg, n_arg=0, device=dev) == (EINVAL, True)
        assert _prove_raw(lk, f, n, kzg, n_arg=2, device=dev) == (EINVAL, True)   # T = 7 > 2^2
        assert _prove_raw(lk, f, n, kzg, n_arg=25, device=dev) == (EUNSUPPORTED, True)
        assert _prove_raw(lk, f, n, _kzg(4), device=dev) == (EINVAL, True)        # a setup of another variable count
        off = _g1_array([lc.model_proof(n)["commitments"][lo.F]])
        off[0, 0] ^= 1
        assert _prove_raw(lk, f, n, kzg, device=dev, cin=ptr(off)) == (EINVAL, True)  # a commitment off the curve
    arr = as_limbs(f)  # a column entry >= p, host entry
    arr[2] = as_limbs([lo.R - 1])[0]
    arr[2, 0] += 1
    L = _lib.lib()
    t = L.zk_transcript_new()
    outs = [np.full(s, lc.SENTINEL, np.uint64) for s in ((n, 4, 4), (11, 4), (n, 4), (4, 12), (n, 12))]
    nco = np.full(n, 0xA5, np.uint8)
    miss = C.c_uint64(99)
    assert L.zk_lookup_prove(lk.h, 0, ptr(arr), n, kzg.h, None, t, ptr(outs[0]), ptr(nco), ptr(outs[1]), ptr(outs[2]),
                             ptr(outs[3]), ptr(outs[4]), C.byref(miss)) == EINVAL
    assert all((o == lc.SENTINEL).all() for o in outs) and miss.value == 99
    L.zk_transcript_free(t)
    # a handle of another field, and a host-only one
    lk0 = Lookup([1, 2, 3], ctx, field=0)
    assert _prove_raw(lk0, f, n, kzg) == (EINVAL, True)
    assert _prove_raw(Lookup(table), f, n, kzg) == (EDEVICE, True)
    lk0.close()
    lk.close()

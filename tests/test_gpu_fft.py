"""GPU parity of the NTT (zk_amd.fft, csrc/fft.hpp) with fft/src/fft.rs as
restated in tests/fft_oracle.py. The result is an exact field element, so every
check is equality: the reference's own three tests, every power of two through
the single-pass path and the smallest two-pass shapes, multi-pass plans forced
at small sizes by ZK_FFT_STAGES, the grid-stride path, the default plan at its
three-pass depth against tests/golden/fft.json and against closed forms, at
its four-pass depth (2^25) against the Horner kernel, the device-table API, and
the polynomial product against the schoolbook."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import coracle as co
import fft_oracle as fo
import pyoracle as po
from conftest import ROOT

import zk_amd
from zk_amd import _lib, fft, poly
from zk_amd.api import UnivariatePoly
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu

FR_FIELDS = [0, 2]
FQ = 1
CANON, MONT = 0, 1
SEED = 11

with open(os.path.join(ROOT, "tests", "golden", "fft.json")) as _fh:
    GOLD = json.load(_fh)
T = GOLD["tile_log"]  # kFftTileLog (test_fft_cpu.py checks it against the build)


@functools.lru_cache(maxsize=None)
def _inputs(field: int, n: int) -> tuple:
    """synth(field, 11, 0, 0, n) on the host: the prefix of one table (shared, never modified)."""
    return tuple(co.from_limbs(co.synth(field, SEED, 0, 0, n)))


@functools.lru_cache(maxsize=None)
def _want(field: int, n: int, inverse: bool = False) -> tuple:
    x = _inputs(field, n)
    return tuple(fo.fft_interpolate(field, x) if inverse else fo.fft_evaluate(field, x))


def _mont(field: int, values) -> np.ndarray:
    p = po.MODULI[field]
    return as_limbs([v * (1 << 256) % p for v in values])


def _dev(ctx, field: int, n: int):
    return ctx.synth(field, n, SEED, 0)


# --- the reference's tests (:88-138) ---------------------------------------------------
def test_splits_poly_correctly():  # :88-101
    p = po.MODULI[0]
    assert fft.split_poly([2, p - 14, 2, 1]) == ([2, 2], [p - 14, 1])


@pytest.mark.parametrize("field", FR_FIELDS)
def test_evaluates_poly(ctx, field):  # :103-125
    p = po.MODULI[field]
    ev = fft.fft_evaluate(UnivariatePoly([1, 2, 3, 4], field), ctx)
    w = fft.get_root_of_unity(4, field)
    assert ev == [(1 + 2 * x + 3 * x * x + 4 * x * x * x) % p for x in (pow(w, i, p) for i in range(4))]
    assert ev == fft.fft_evaluate([1, 2, 3, 4], ctx, field)


@pytest.mark.parametrize("field", FR_FIELDS)
def test_interpolates_poly(ctx, field):  # :127-138
    ev = fft.fft_evaluate(UnivariatePoly([1, 2, 3, 4], field), ctx)
    back = fft.fft_interpolate(ev, field, ctx)
    assert back.coefficient == [1, 2, 3, 4] and back.field == field
    # untrimmed (UnivariatePoly::new :59)
    assert fft.fft_interpolate(fft.fft_evaluate([7, 0, 0, 0], ctx, field), field, ctx).coefficient == [7, 0, 0, 0]


def test_fq_has_only_two_domains(ctx):
    p = po.MODULI[FQ]
    assert fft.fft_evaluate([5], ctx, FQ) == [5] and fft.fft_interpolate([5], FQ, ctx).coefficient == [5]
    assert fft.fft_evaluate([3, p - 1], ctx, FQ) == [2, 4] == fo.fft_evaluate(FQ, [3, p - 1])
    assert fft.fft_interpolate([2, 4], FQ, ctx).coefficient == [3, p - 1]


# --- every power of two up to the smallest two-pass shapes --------------------------------
@pytest.mark.parametrize("k", range(0, T + 3))
@pytest.mark.parametrize("field", FR_FIELDS)
def test_every_small_power_of_two(ctx, field, k):
    L = _lib.lib()
    n = 1 << k
    x = list(_inputs(field, n))
    fwd, inv = list(_want(field, n)), list(_want(field, n, True))
    assert fft.fft_evaluate(x, ctx, field) == fwd
    assert fft.fft_interpolate(x, field, ctx).coefficient == inv
    assert fft.fft_interpolate(fwd, field, ctx).coefficient == x
    # Montgomery in, Montgomery out
    out = np.zeros((n, 4), np.uint64)
    assert L.zk_fft_evaluate(ctx.h, field, MONT, ptr(_mont(field, x)), n, ptr(out)) == 0
    assert np.array_equal(out, _mont(field, fwd))
    assert L.zk_fft_interpolate(ctx.h, field, MONT, ptr(_mont(field, x)), n, ptr(out)) == 0
    assert np.array_equal(out, _mont(field, inv))
    # the device table the other tests start from is this table
    assert fft.dev_fft(_dev(ctx, field, n)).to_ints() == fwd


# --- multi-pass plans at oracle-checkable sizes -----------------------------------------
@pytest.mark.parametrize("stages", [1, 2, 3, 5])
@pytest.mark.parametrize("field", FR_FIELDS)
def test_plans_under_a_stage_cap(monkeypatch, field, stages):
    """A context created under ZK_FFT_STAGES=s does at most s stages per pass: up
    to 13 passes, uneven widths (13 = 5 + 4 + 4), passes of a single stage."""
    monkeypatch.setenv("ZK_FFT_STAGES", str(stages))
    capped = zk_amd.Context(0)
    monkeypatch.delenv("ZK_FFT_STAGES")
    try:
        for k in (11, 12, 13):
            n = 1 << k
            t = _dev(capped, field, n)
            y = fft.dev_fft(t)
            assert y.to_ints() == list(_want(field, n)), k
            assert fft.dev_fft(y, inverse=True, out=y) is y  # in place
            assert y.to_ints() == list(_inputs(field, n)), k
            assert fft.dev_fft(t, inverse=True).to_ints() == list(_want(field, n, True)), k
    finally:
        capped.close()


@pytest.mark.parametrize("field", FR_FIELDS)
def test_grid_stride_path(monkeypatch, field):
    """Under ZK_GRID_CAP=3 at most 3 blocks run a kernel. A tile is 2^(T+2) elements,
    so 2^(T+3) is two tiles (one per block, the cap only shrinks the grid) and
    2^(T+5) is eight: the blocks take 3, 3 and 2 tiles, the tile loop runs again
    and the LDS tile is reused. The product's pad and pointwise kernels stride too
    (2 048 elements = 8 blocks of work over 3)."""
    monkeypatch.setenv("ZK_GRID_CAP", "3")
    capped = zk_amd.Context(0)
    monkeypatch.delenv("ZK_GRID_CAP")
    try:
        for k in (T + 3, T + 5):
            n = 1 << k
            x = _dev(capped, field, n)
            assert fft.dev_fft(x).to_ints() == list(_want(field, n)), k
            assert fft.dev_fft(x, inverse=True).to_ints() == list(_want(field, n, True)), k
            assert fft.dev_fft(x, out=x) is x and x.to_ints() == list(_want(field, n)), k  # in place
            assert fft.dev_fft(x, inverse=True, out=x).to_ints() == list(_inputs(field, n)), k
        # three passes in place (both scratch tables), 128 tiles over 3 blocks: the fixture's digest
        n = 1 << (2 * T + 1)
        x = _dev(capped, field, n)
        before = x.download(MONT)
        fft.dev_fft(x, out=x)
        assert _digest(x) == next(e for e in GOLD["fields"] if e["field"] == field)["evaluate_keccak256"][str(2 * T + 1)]
        assert np.array_equal(fft.dev_fft(x, inverse=True, out=x).download(MONT), before)
        a = list(co.from_limbs(co.synth(field, SEED, 1, 0, 600)))
        b = list(co.from_limbs(co.synth(field, SEED, 2, 0, 500)))
        got = fft.poly_mul(UnivariatePoly(a, field), UnivariatePoly(b, field), capped)
        assert got.coefficient == fo.poly_mul(field, a, b)
    finally:
        capped.close()


@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("field", [0, FQ, 2])
def test_single_pass_inverse_under_a_stage_cap(monkeypatch, field, stages):
    """n <= 2^stages stays one pass, whose inverse multiplies by n^-1 on the way in
    (no twiddle table to carry it): n = 2 under ZK_FFT_STAGES=1, n = 2 and 4 under 2."""
    monkeypatch.setenv("ZK_FFT_STAGES", str(stages))
    capped = zk_amd.Context(0)
    monkeypatch.delenv("ZK_FFT_STAGES")
    try:
        for k in range(1, min(stages, fo.TWO_ADICITY[field]) + 1):
            x = list(_inputs(field, 1 << k))
            y = fft.fft_evaluate(x, capped, field)
            assert y == fo.fft_evaluate(field, x), k
            assert fft.fft_interpolate(x, field, capped).coefficient == fo.fft_interpolate(field, x), k
            assert fft.fft_interpolate(y, field, capped).coefficient == x, k
    finally:
        capped.close()


# --- the default plan at depth -------------------------------------------------------------
def _digest(table) -> str:
    return co.keccak256(np.ascontiguousarray(table.download(), dtype="<u8").tobytes()).hex()


@pytest.mark.parametrize("k", [T + 1, 2 * T, 2 * T + 1])
@pytest.mark.parametrize("field", FR_FIELDS)
def test_default_plan_against_fixture(ctx, field, k):
    """Two passes, two full passes, three passes: Keccak-256 of the canonical bytes
    of the transform, written by the pure-Python oracle (make_fft_golden.py)."""
    g = next(e for e in GOLD["fields"] if e["field"] == field)
    n = 1 << k
    x = _dev(ctx, field, n)
    y = fft.dev_fft(x)
    assert _digest(y) == g["evaluate_keccak256"][str(k)]
    back = fft.dev_fft(y, inverse=True)
    assert np.array_equal(back.download(MONT), x.download(MONT))


@pytest.mark.parametrize("field", FR_FIELDS)
def test_default_plan_closed_forms(ctx, field):
    """At 2^(2T+1), three passes: x = delta_j gives y[k] = w^(jk); for the synthesised
    table y[0] = sum x, y[n/2] = sum (-1)^j x_j, and two outputs by Horner."""
    p = po.MODULI[field]
    n = 1 << (2 * T + 1)
    w = fo.root_of_unity(field, n)
    for j in (1, n // 2 + 1, n - 1):
        col = np.zeros((n, 4), np.uint64)
        col[j, 0] = 1
        y = fft.dev_fft(ctx.upload(field, col)).to_ints()
        wj, cur, want = pow(w, j, p), 1, []
        for _ in range(n):
            want.append(cur)
            cur = cur * wj % p
        assert y == want, j
    x = _inputs(field, n)
    y = fft.dev_fft(_dev(ctx, field, n)).to_ints()
    assert y[0] == sum(x) % p
    assert y[n // 2] == (sum(x[0::2]) - sum(x[1::2])) % p
    for k in (3, n - 5):
        pt, acc = pow(w, k, p), 0
        for c in reversed(x):
            acc = (acc * pt + c) % p
        assert y[k] == acc, k


def _rows(table, ks) -> list:
    """Rows ks of a device table as canonical ints, one 32-byte download each."""
    out = np.zeros((1, 4), np.uint64)
    got = []
    for k in ks:
        assert 0 <= k < table.count
        assert _lib.lib().zk_dev_download(table.ctx.h, table.field, CANON, C.c_void_p(table.ptr.value + 32 * k), 1, ptr(out)) == 0
        got.append(to_ints(out)[0])
    return got


@pytest.mark.parametrize("field", FR_FIELDS)
def test_default_plan_four_passes(ctx, field):
    """2^25, the first size of the default plan with four passes (widths 7, 6,
    6, 6, the last pass at Ns = 2^19, the twiddle split at h = 13), 1 GiB a
    table, device API only. No Python oracle can run this size: the reference
    is the Horner kernel (poly.dev_evaluate at eight of the 2^25-th roots
    against the same rows of the transform), which tests/poly_oracle.py pins at
    small sizes and tests/test_gpu_poly_scale.py at chunks of many staging
    trips; the input is pinned to the host's synth at seeded rows. A random
    table has no output with an O(1) closed form, so none is checked. The
    inverse runs in place (both scratch tables) and must give the input back,
    every word of it, compared in Montgomery form as downloaded."""
    p = po.MODULI[field]
    k = 25
    n = 1 << k
    passes = -(-k // T)
    widths = [k // passes + (1 if i < k % passes else 0) for i in range(passes)]
    assert passes == 4 and widths == [7, 6, 6, 6] and sum(widths[:-1]) == 19 and (k + 1) // 2 == 13  # fft_plan.hpp, fft.hip
    rng = random.Random(SEED + field)
    x = _dev(ctx, field, n)
    at = [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(4)]
    assert _rows(x, at) == [co.from_limbs(co.synth(field, SEED, 0, i, 1))[0] for i in at]
    y = fft.dev_fft(x)
    w = fo.root_of_unity(field, n)
    ks = [0, 1, 3, 1 << 24, (1 << 24) + 1, n - 5, n - 1, rng.randrange(n)]
    pts = ctx.upload(field, [pow(w, e, p) for e in ks])
    assert _rows(y, ks) == poly.dev_evaluate(x, pts).to_ints()
    before = x.download(MONT)
    assert fft.dev_fft(y, inverse=True, out=y) is y  # in place
    assert np.array_equal(y.download(MONT), before)
    x.free()
    y.free()


# --- the device API --------------------------------------------------------------------------
def test_device_api(ctx):
    field, n = 0, 1 << (T + 2)
    x = _dev(ctx, field, n)
    before = x.download(MONT)
    y = fft.dev_fft(x)
    assert np.array_equal(x.download(MONT), before)  # the input is only read
    assert y is not x and y.count == n and y.to_ints() == list(_want(field, n))
    out = ctx.alloc(field, n)
    assert fft.dev_fft(x, out=out) is out and np.array_equal(out.download(MONT), y.download(MONT))
    assert fft.dev_fft(x, out=x) is x and np.array_equal(x.download(MONT), y.download(MONT))  # in place
    assert fft.dev_fft(x, inverse=True, out=x).download(MONT).tolist() == before.tolist()
    other = zk_amd.Context(0)
    try:
        with pytest.raises(ValueError):
            fft.dev_fft(x, out=other.alloc(field, n))
    finally:
        other.close()
    with pytest.raises(ValueError):
        fft.dev_fft(x, out=ctx.alloc(2, n))
    with pytest.raises(ValueError):
        fft.dev_fft(x, out=ctx.alloc(field, n // 2))
    freed = ctx.alloc(field, n)
    freed.free()
    with pytest.raises(ValueError):
        fft.dev_fft(freed)
    with pytest.raises(ValueError):
        fft.dev_fft(x, out=freed)
    # overlapping, not equal: refused by the library
    L = _lib.lib()
    big = ctx.alloc(field, 2 * n)
    assert L.zk_dev_fft(ctx.h, field, big.ptr, n, 0, C.c_void_p(big.ptr.value + 32 * (n // 2))) == _lib.ZK_EINVAL
    assert L.zk_dev_fft(ctx.h, field, big.ptr, n, 0, C.c_void_p(big.ptr.value + 32 * n)) == 0


# --- poly_mul ----------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FR_FIELDS)
def test_it_multiplies_correctly(ctx, field):
    """univariate_polynomial_dense.rs it_multiplies_correctly :163-183:
    (3 + 4x + 3x^2)(-3 + 4x^3) = -9 - 12x - 9x^2 + 12x^3 + 16x^4 + 12x^5."""
    p = po.MODULI[field]
    a, b = UnivariatePoly([3, 4, 3], field), UnivariatePoly([p - 3, 0, 0, 4], field)
    want = [p - 9, p - 12, p - 9, 12, 16, 12]
    assert (a * b).coefficient == want == fo.poly_mul(field, [3, 4, 3], [p - 3, 0, 0, 4])
    assert fft.poly_mul(b, a, ctx).coefficient == want


@pytest.mark.parametrize("shape", [(1, 1), (3, 4), (100, 29), (257, 256), ((1 << (T - 1)) + 1, 1 << (T - 1))])
@pytest.mark.parametrize("field", FR_FIELDS)
def test_poly_mul_against_schoolbook(ctx, field, shape):
    na, nb = shape
    a = list(co.from_limbs(co.synth(field, SEED, 1, 0, na)))
    b = list(co.from_limbs(co.synth(field, SEED, 2, 0, nb)))
    want = fo.poly_mul(field, a, b)
    got = fft.poly_mul(UnivariatePoly(a, field), UnivariatePoly(b, field), ctx)
    assert got.coefficient == want and len(want) == na + nb - 1 and got.field == field


def test_poly_mul_trims_and_rejects(ctx):
    field = 0
    a, b = [1, 2, 3, 0, 0], [4, 5, 0]
    pa, pb = UnivariatePoly(list(a), field), UnivariatePoly(list(b), field)
    assert fft.poly_mul(pa, pb, ctx).coefficient == fo.poly_mul(field, a, b) == [4, 13, 22, 15]
    assert pa.coefficient == a  # poly_mul leaves its operands alone ...
    assert (pa * pb).coefficient == [4, 13, 22, 15]
    assert pa.coefficient == [1, 2, 3] and pb.coefficient == [4, 5]  # ... the operator trims them, as degree() does
    for zero in ([], [0], [0, 0, 0]):
        with pytest.raises(ValueError):
            fft.poly_mul(UnivariatePoly(list(zero), field), UnivariatePoly([1, 2], field), ctx)
        with pytest.raises(ValueError):
            UnivariatePoly([1, 2], field) * UnivariatePoly(list(zero), field)
    with pytest.raises(ValueError):
        fft.poly_mul(UnivariatePoly([1, po.MODULI[field]], field), UnivariatePoly([1, 2], field), ctx)
    with pytest.raises(ValueError):
        fft.poly_mul(UnivariatePoly([1], 0), UnivariatePoly([1], 2), ctx)
    # BN254 Fq has no domain of 4 points: 1 x 2 fits (N = 2), 2 x 2 does not
    assert fft.poly_mul(UnivariatePoly([3], FQ), UnivariatePoly([4, 5], FQ), ctx).coefficient == [12, 15]
    with pytest.raises(zk_amd.ZkError) as e:
        fft.poly_mul(UnivariatePoly([1, 2], FQ), UnivariatePoly([3, 4], FQ), ctx)
    assert e.value.code == _lib.ZK_EUNSUPPORTED
    # a short output buffer: ZK_EINVAL, the length still reported, nothing written
    L = _lib.lib()
    out = np.full((2, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    n = C.c_uint64(0)
    x, y = as_limbs([1, 2, 3]), as_limbs([4, 5])
    assert L.zk_poly_mul(ctx.h, field, CANON, ptr(x), 3, ptr(y), 2, ptr(out), 2, C.byref(n)) == _lib.ZK_EINVAL
    assert n.value == 4 and (out == 0x5A5A5A5A5A5A5A5A).all()


# --- errors ---------------------------------------------------------------------------------------
def test_transform_rejects(ctx):
    L = _lib.lib()
    p = po.MODULI[0]
    for bad in ([], [1, 2, 3]):
        with pytest.raises(ValueError):
            fft.fft_evaluate(bad, ctx, 0)
        with pytest.raises(ValueError):
            fft.fft_interpolate(bad, 0, ctx)
    with pytest.raises(ValueError):
        fft.fft_evaluate([1, 2, 3, p], ctx, 0)  # a value equal to p
    with pytest.raises(ValueError):
        fft.fft_interpolate([p, 0], 0, ctx)
    with pytest.raises(ValueError):
        fft.fft_evaluate([1, 2, 3, 4], ctx, FQ)  # Fq has no 4th root of unity
    # the length is checked before anything is read: 2^29 with four elements behind the pointer
    x = as_limbs([1, 2, 3, 4])
    out = np.full((4, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    assert L.zk_fft_evaluate(ctx.h, 0, CANON, ptr(x), 1 << 29, ptr(out)) == _lib.ZK_EINVAL  # above the two-adicity
    assert L.zk_fft_evaluate(ctx.h, 2, CANON, ptr(x), 1 << 29, ptr(out)) == _lib.ZK_EUNSUPPORTED
    assert L.zk_fft_interpolate(ctx.h, 2, CANON, ptr(x), 1 << 29, ptr(out)) == _lib.ZK_EUNSUPPORTED
    t = ctx.alloc(0, 4)
    assert L.zk_dev_fft(ctx.h, 0, t.ptr, 3, 0, t.ptr) == _lib.ZK_EINVAL
    assert L.zk_dev_fft(ctx.h, 0, t.ptr, 0, 0, t.ptr) == _lib.ZK_EINVAL
    assert L.zk_dev_fft(ctx.h, 2, t.ptr, 1 << 29, 0, t.ptr) == _lib.ZK_EUNSUPPORTED
    assert L.zk_dev_fft(ctx.h, 0, None, 4, 0, t.ptr) == _lib.ZK_EINVAL
    assert (out == 0x5A5A5A5A5A5A5A5A).all()

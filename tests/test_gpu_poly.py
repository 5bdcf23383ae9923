"""GPU parity of interpolation and batch evaluation over arbitrary points
(zk_amd.poly, csrc/poly.hpp) with univariate_polynomial_dense.rs as restated in
tests/poly_oracle.py. Every result is an exact field element and the
interpolant of distinct x is unique, so every check is plain equality: with the
oracle, with the committed digests of tests/golden/poly.json, or with the
definition (at most n coefficients, trimmed, the value y_i at every x_i). The
kernels are reached at small shapes through contexts created under
ZK_POLY_HOST_MAX=0; the default context's host path is compared with them."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import coracle as co
import poly_oracle as O
import pyoracle as po
from conftest import ROOT

import zk_amd
from zk_amd import _lib, poly
from zk_amd.api import UnivariatePoly
from zk_amd.elems import as_limbs, ptr

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2]
CANON, MONT = 0, 1

with open(os.path.join(ROOT, "tests", "golden", "poly.json")) as _fh:
    GOLD = json.load(_fh)
SEED = GOLD["seed"]
K = 7  # the k of the 2^k - 1, 2^k + 1, 3 2^k shapes
INTERP_SHAPES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, (1 << K) - 1, (1 << K) + 1, 3 << K]


def _ctx_under(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return zk_amd.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dev():
    """Every call on the device, whatever its size."""
    c = _ctx_under(ZK_POLY_HOST_MAX=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev3():
    """... and at most three blocks along x: a kernel grid-strides once its
    shape has more than three tiles of 256 lanes (n or m above 768)."""
    c = _ctx_under(ZK_POLY_HOST_MAX=0, ZK_GRID_CAP=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev1():
    """... and one block along x: it walks every tile of every kernel in turn."""
    c = _ctx_under(ZK_POLY_HOST_MAX=0, ZK_GRID_CAP=1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _points(field: int, n: int) -> tuple:
    """x from table 0 of the seed (the second one replaced by 0), y from table 1: shared, never modified."""
    xs = co.from_limbs(co.synth(field, SEED, 0, 0, n)) if n else []
    ys = co.from_limbs(co.synth(field, SEED, 1, 0, n)) if n else []
    if n > 1:
        xs[1] = 0
    assert len(set(xs)) == n
    return tuple(zip(xs, ys))


@functools.lru_cache(maxsize=None)
def _want(field: int, n: int) -> tuple:
    return tuple(O.interpolate_fast(po.MODULI[field], list(_points(field, n))))


def _mont(field: int, values) -> np.ndarray:
    p = po.MODULI[field]
    return as_limbs([v * (1 << 256) % p for v in values]) if len(values) else np.zeros((1, 4), np.uint64)


def _raw_interpolate(ctx, field, repr_, xs, ys, cap=None):
    """zk_poly_interpolate as is: (code, coefficients as limbs)."""
    n = len(xs)
    conv = (lambda v: _mont(field, v)) if repr_ == MONT else (lambda v: as_limbs(list(v)) if n else np.zeros((1, 4), np.uint64))
    out = np.zeros((max(n, 1), 4), np.uint64)
    cnt = C.c_uint64(77)
    code = _lib.lib().zk_poly_interpolate(ctx.h, field, repr_, ptr(conv(xs)), ptr(conv(ys)), n, ptr(out),
                                          n if cap is None else cap, C.byref(cnt))
    return code, out[: cnt.value] if code == 0 else None


# --- the reference's own tests ----------------------------------------------------------
def test_it_interpolates_points(dev, ctx):  # univariate_polynomial_dense.rs :185-196
    for c in (dev, ctx):
        got = UnivariatePoly.interpolate([(0, 2), (1, 4), (2, 6)], field=1, ctx=c)
        assert got.coefficient == [2, 2] and got.field == 1


def test_it_evaluates_poly(dev, ctx):  # :125-132
    for c in (dev, ctx):
        assert UnivariatePoly([3, 4, 3], 1).evaluate_many([3], ctx=c) == [42]


def test_fibonacci_check(dev):  # sample_tests/src/fibonacci_evaluation.rs
    p = po.MODULI[1]
    fib = [1, 1, 2, 3, 5, 8, 13, 21]
    f = UnivariatePoly.interpolate(list(enumerate(fib)), field=1, ctx=dev)
    v = f.evaluate_many(range(0, 8), ctx=dev)
    assert v == fib
    for x in (2, 5, 7):
        assert v[x] == (v[x - 1] + v[x - 2]) % p


def test_reference_bench_inputs(dev):  # the univariate benches: coefficients 0..99 at 2, ten points on 3 + 2x
    p = po.MODULI[1]
    assert UnivariatePoly(list(range(100)), 1).evaluate_many([2], ctx=dev) == [O.evaluate(p, list(range(100)), 2)]
    assert UnivariatePoly.interpolate([(x, 3 + 2 * x) for x in range(10)], field=1, ctx=dev).coefficient == [3, 2]


# --- interpolation on the device ---------------------------------------------------------
@pytest.mark.parametrize("n", INTERP_SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_interpolate_shapes(dev, field, n):
    pts = _points(field, n)
    want = list(_want(field, n))
    assert poly.interpolate(pts, field, dev).coefficient == want
    xs, ys = [x for x, _ in pts], [y for _, y in pts]
    code, out = _raw_interpolate(dev, field, MONT, xs, ys)
    assert code == 0 and out.shape[0] == len(want)
    if want:
        assert np.array_equal(out, _mont(field, want))


@pytest.mark.parametrize("field", FIELDS)
def test_interpolate_1025_against_fixture_and_definition(dev, field):
    p = po.MODULI[field]
    pts = _points(field, 1025)
    got = poly.interpolate(pts, field, dev).coefficient
    assert O.digest(got) == GOLD["interpolate_sha256"][str(field)]["1025"]
    assert O.is_interpolant(p, got, pts)
    code, out = _raw_interpolate(dev, field, MONT, [x for x, _ in pts], [y for _, y in pts])
    assert code == 0 and np.array_equal(out, _mont(field, got))


@pytest.mark.parametrize("n", [257, 3 << K])
@pytest.mark.parametrize("field", FIELDS)
def test_interpolate_under_a_grid_cap(dev3, field, n):
    """Two tiles under a cap of three: the capped launch path, one trip per block."""
    assert poly.interpolate(_points(field, n), field, dev3).coefficient == list(_want(field, n))


@pytest.mark.parametrize("n", [1025, 3 << 9])
@pytest.mark.parametrize("field", FIELDS)
def test_interpolate_grid_stride(dev, dev3, dev1, field, n):
    """Five and six tiles over three blocks and over one: every kernel's x loop
    takes a second trip (LDS staged again after the trailing barrier, the
    pass-through tile of 1 025 reached by a block that also multiplies, small and
    large tree levels in the same block). 3 2^9 has a short last pair at level 9
    and a pass-through node at level 10."""
    p = po.MODULI[field]
    pts = _points(field, n)
    got = poly.interpolate(pts, field, dev3).coefficient
    assert O.is_interpolant(p, got, pts)
    if n == 1025:
        assert O.digest(got) == GOLD["interpolate_sha256"][str(field)]["1025"]
    assert got == poly.interpolate(pts, field, dev1).coefficient == poly.interpolate(pts, field, dev).coefficient


@pytest.mark.parametrize("field", FIELDS)
def test_duplicate_x_under_grid_stride(dev3, dev1, field):
    pts = list(_points(field, 1025))
    xs, ys = [x for x, _ in pts], [y for _, y in pts]
    xs[1024] = xs[0]  # the first and the last tile, visited by different trips
    for c in (dev3, dev1):
        code, _ = _raw_interpolate(c, field, CANON, xs, ys)
        assert code == _lib.ZK_EINVAL


@pytest.mark.parametrize("field", FIELDS)
def test_interpolate_input_cases(dev, field):
    p = po.MODULI[field]
    xs = [x for x, _ in _points(field, 300)]
    assert poly.interpolate([(x, 0) for x in xs], field, dev).coefficient == []  # every y = 0
    quad = [p - 5, 3, 1]
    assert poly.interpolate([(x, O.horner(p, quad, x)) for x in xs], field, dev).coefficient == quad
    assert poly.interpolate([(x, 9) for x in xs[:70]], field, dev).coefficient == [9]
    assert poly.interpolate([], field, dev).coefficient == []
    assert poly.interpolate([(0, 0)], field, dev).coefficient == []


@pytest.mark.parametrize("field", FIELDS)
def test_duplicate_x_is_einval(dev, dev3, field):
    pts = list(_points(field, 257))
    xs, ys = [x for x, _ in pts], [y for _, y in pts]
    far = list(xs)
    far[256] = far[0]  # positions 0 and n - 1: different blocks, different j tiles
    near = list(xs)
    near[131] = near[130]
    for c in (dev, dev3):
        for bad in (far, near):
            code, _ = _raw_interpolate(c, field, CANON, bad, ys)
            assert code == _lib.ZK_EINVAL
            with pytest.raises(ValueError):
                poly.interpolate(list(zip(bad, ys)), field, c)
        assert poly.interpolate(pts, field, c).coefficient == list(_want(field, 257))  # the flag does not stick
    code, _ = _raw_interpolate(dev, field, CANON, [7, 7], [1, 2])
    assert code == _lib.ZK_EINVAL


def test_interpolate_refusals(dev):
    L = _lib.lib()
    n = (1 << 16) + 1
    buf = np.zeros((n, 4), np.uint64)
    cnt = C.c_uint64(77)
    assert L.zk_poly_interpolate(dev.h, 1, CANON, ptr(buf), ptr(buf), n, ptr(buf), n, C.byref(cnt)) == _lib.ZK_EUNSUPPORTED
    with pytest.raises(zk_amd.ZkError) as e:
        poly.interpolate([(i, i) for i in range(n)], 1, dev)
    assert e.value.code == _lib.ZK_EUNSUPPORTED
    p = po.MODULI[1]
    code, _ = _raw_interpolate(dev, 1, CANON, [1, 2, 3], [4, 5, 6], cap=2)
    assert code == _lib.ZK_EINVAL
    for c in (dev, zk_amd.default_context(0)):  # a value >= p, on the device path and on the host path
        code, _ = _raw_interpolate(c, 1, CANON, [1, p, 3], [4, 5, 6])
        assert code == _lib.ZK_EINVAL
        big = as_limbs([4, 5, (1 << 256) - 1])  # (as is: not a Montgomery image of anything)
        assert L.zk_poly_interpolate(c.h, 1, MONT, ptr(as_limbs([1, 2, 3])), ptr(big), 3, ptr(buf), 3,
                                     C.byref(cnt)) == _lib.ZK_EINVAL
    assert cnt.value == 77


# --- evaluation ----------------------------------------------------------------------------
T = GOLD["eval_tile"]  # kPolyEvalTile (test_poly_cpu.py checks it against the build)


@functools.lru_cache(maxsize=None)
def _coeffs(field: int, d: int) -> tuple:
    return tuple(co.from_limbs(co.synth(field, SEED, 2, 0, d))) if d else ()


def _xs(field: int, m: int) -> list:
    p = po.MODULI[field]
    special = [0, 1, p - 1]
    rnd = co.from_limbs(co.synth(field, SEED, 3, 0, m))
    return (special + rnd)[:m] if m >= 3 else rnd


@pytest.mark.parametrize("d", [0, 1, 2, 100, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_degrees(dev, field, d):
    p = po.MODULI[field]
    cf, xs = list(_coeffs(field, d)), _xs(field, 65)
    want = [O.horner(p, cf, x) for x in xs]
    f = UnivariatePoly(cf, field)
    assert f.evaluate_many(xs, ctx=dev) == want
    assert want[:8] == [f.evaluate(x) for x in xs[:8]]  # the existing one-point evaluate (pow per term)
    if d == 0:
        assert want == [0] * 65


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_point_counts(dev, dev3, field, m):
    p = po.MODULI[field]
    cf, xs = list(_coeffs(field, 100)), _xs(field, m)
    want = [O.horner(p, cf, x) for x in xs]
    f = UnivariatePoly(cf, field)
    assert f.evaluate_many(xs, ctx=dev) == want == f.evaluate_many(xs, ctx=dev3)
    assert want == [f.evaluate(x) for x in xs]
    # Montgomery in, Montgomery out
    out = np.zeros((m, 4), np.uint64)
    assert _lib.lib().zk_poly_evaluate(dev.h, field, MONT, ptr(_mont(field, cf)), 100, ptr(_mont(field, xs)), m, ptr(out)) == 0
    assert np.array_equal(out, _mont(field, want))


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_split_path(dev, dev3, field, m):
    d = 3 * T + 17  # four runs, the last one short
    chunks, length = poly.eval_plan(d, m, dev)
    assert chunks > 1 and length % T == 0 and (chunks - 1) * length < d <= chunks * length
    assert poly.eval_plan(100, m, dev) == (1, 100) and poly.eval_plan(d, 1 << 20, dev) == (1, d)
    p = po.MODULI[field]
    cf = list(_coeffs(field, d))
    xs = [p - 1] if m == 1 else [0, 1, co.from_limbs(co.synth(field, SEED, 3, 0, 1))[0]]
    want = [O.horner(p, cf, x) for x in xs]
    assert poly.evaluate_many(cf, xs, field, dev) == want == poly.evaluate_many(cf, xs, field, dev3)
    assert want == [UnivariatePoly(cf, field).evaluate(x) for x in xs]


@pytest.mark.parametrize("d", [100, 3 * T + 17])
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_grid_stride(dev, dev3, dev1, field, d):
    """1 025 points are five tiles: over three blocks and over one, the Horner
    kernel stages its coefficients again for every further tile, with one run of
    coefficients and on the split path (asserted on the plan), whose combining
    kernel strides as well."""
    p = po.MODULI[field]
    m = 1025
    chunks, _ = poly.eval_plan(d, m, dev3)
    assert (chunks > 1) == (d > T)
    cf, xs = list(_coeffs(field, d)), _xs(field, m)
    want = [O.horner(p, cf, x) for x in xs]
    assert poly.evaluate_many(cf, xs, field, dev3) == want == poly.evaluate_many(cf, xs, field, dev1)
    assert want == poly.evaluate_many(cf, xs, field, dev)


@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_against_fixture(dev, field):
    d, m = GOLD["evaluate_shape"]
    got = poly.evaluate_many(list(_coeffs(field, d)), co.from_limbs(co.synth(field, SEED, 3, 0, m)), field, dev)
    assert O.digest(got) == GOLD["evaluate_sha256"][str(field)]


@pytest.mark.parametrize("field", FIELDS)
def test_device_tables_equal_host_memory(dev, field):
    for d, m in ((100, 257), (3 * T + 17, 3)):
        cf_t = dev.synth(field, d, SEED, 2)
        xs_t = dev.synth(field, m, SEED, 3)
        want = poly.evaluate_many(list(_coeffs(field, d)), co.from_limbs(co.synth(field, SEED, 3, 0, m)), field, dev)
        out = poly.dev_evaluate(cf_t, xs_t)
        assert out.to_ints() == want
        assert xs_t.to_ints() == co.from_limbs(co.synth(field, SEED, 3, 0, m))  # only read
        assert poly.dev_evaluate(cf_t, xs_t, out=xs_t) is xs_t and xs_t.to_ints() == want  # in place
    xs_t, out = dev.synth(field, 5, SEED, 3), dev.alloc(field, 5)
    assert _lib.lib().zk_dev_poly_evaluate(dev.h, field, None, 0, xs_t.ptr, 5, out.ptr) == 0  # no coefficients
    assert out.to_ints() == [0] * 5


def test_dev_evaluate_refusals(dev, ctx):
    cf, xs = dev.synth(1, 8, SEED, 2), dev.synth(1, 5, SEED, 3)
    with pytest.raises(ValueError):
        poly.dev_evaluate(ctx.synth(1, 8, SEED, 2), xs)  # another context
    with pytest.raises(ValueError):
        poly.dev_evaluate(cf, dev.synth(0, 5, SEED, 3))  # another field
    with pytest.raises(ValueError):
        poly.dev_evaluate(cf, xs, out=dev.alloc(1, 4))  # a wrong count
    with pytest.raises(ValueError):
        poly.dev_evaluate(cf, xs, out=dev.alloc(0, 5))
    with pytest.raises(ValueError):
        poly.dev_evaluate(cf, xs, out=ctx.alloc(1, 5))
    L = _lib.lib()
    assert L.zk_dev_poly_evaluate(dev.h, 1, cf.ptr, 8, xs.ptr, 5, cf.ptr) == _lib.ZK_EINVAL  # the output over the coefficients
    assert L.zk_dev_poly_evaluate(dev.h, 1, cf.ptr, 8, cf.ptr, 5, C.c_void_p(cf.ptr.value + 32)) == _lib.ZK_EINVAL
    assert L.zk_dev_poly_evaluate(dev.h, 1, cf.ptr, 8, xs.ptr, 0, None) == 0  # no points: a no-op
    assert L.zk_dev_poly_evaluate(dev.h, 1, cf.ptr, (1 << 28) + 1, xs.ptr, 5, xs.ptr) == _lib.ZK_EUNSUPPORTED
    assert L.zk_dev_poly_evaluate(dev.h, 1, cf.ptr, 1 << 28, xs.ptr, (1 << 12) + 1, xs.ptr) == _lib.ZK_EUNSUPPORTED
    assert xs.to_ints() == co.from_limbs(co.synth(1, SEED, 3, 0, 5))


# --- the host path agrees -------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_host_path_agrees(dev, ctx, field):
    for n in range(0, 17):
        pts = _points(field, n)
        a = poly.interpolate(pts, field, ctx).coefficient
        assert a == poly.interpolate(pts, field, dev).coefficient
        if n in (2, 16):
            assert a == list(_want(field, n))
        xs = _xs(field, max(n, 3))
        assert poly.evaluate_many(a, xs, field, ctx) == poly.evaluate_many(a, xs, field, dev)
    with pytest.raises(ValueError):
        poly.interpolate([(4, 1), (5, 2), (4, 3)], field, ctx)

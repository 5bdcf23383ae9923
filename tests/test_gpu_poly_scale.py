"""Interpolation and batch evaluation (zk_amd.poly, csrc/poly.hpp) and the
Shamir mirror at the sizes where their launch plans change, which
tests/test_gpu_poly.py (at most 1 536 points, at most 2 048 coefficients)
stays below: the round-robin deal of k_poly_tree_level wrapping (a block with
more steps than the level has parts, from n = 2 818), k_poly_weights with
several j0 trips per part (n > 8 192 on 256 CUs), the cap of 2^16 points,
k_poly_eval staging a second tile of one chunk, the split path with many point
tiles, and the host/device crossover of the default context.

The O(n^2) oracle cannot run here (40 s at 4 097 points), so above ~1 000
points the reference is an identity whose other side is the pure-Python NTT of
tests/fft_oracle.py or the input itself:
  (I1) interpolation through n of the N-th roots of unity, N = 2^k >= n, of the
       NTT of f (n coefficients, the top one non-zero) is f: the interpolant
       of distinct x is unique, whatever the subset and its order;
  (I2) Horner at all N-th roots is the forward NTT: evaluate_many, the oracle
       and dev_fft in one equality;
  (I3) on any field, BN254 Fq included: ys = device evaluate_many(f, xs),
       spot-checked by Horner on the host, interpolate back to f: a wrong y
       anywhere has another unique interpolant;
and closed forms on Fq. Every comparison is exact equality.

Each size relies on a plan fact (restated from tests/poly_tree_model.py and the
CU count the context really has, recovered from poly.eval_plan) and asserts it:
on another device the test fails its precondition instead of passing for the
wrong reason."""
from __future__ import annotations

import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import coracle as co
import fft_oracle as fo
import poly_oracle as O
import poly_tree_model as tm
import pyoracle as po

import zk_amd
from zk_amd import _lib, fft, poly, shamir
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2]
FR_FIELDS = [0, 2]  # the fields with a domain
FQ = 1
CANON, MONT = 0, 1
SEED = 37
T = tm.EVAL_TILE  # kPolyEvalTile (test_poly_cpu.py checks the model's constants against the build)
HOST_MAX = 96  # kPolyHostMaxDefault: what a context created without ZK_POLY_HOST_MAX runs on the host


def _ctx_under(**env):
    """A context created under these variables (None: with the variable removed)."""
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
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
    """... and at most three blocks along x."""
    c = _ctx_under(ZK_POLY_HOST_MAX=0, ZK_GRID_CAP=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev1():
    """... and one block along x."""
    c = _ctx_under(ZK_POLY_HOST_MAX=0, ZK_GRID_CAP=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def default(ctx):
    """The default context as it is without ZK_POLY_HOST_MAX: the suite's own
    when the variable is not set, else one created with it removed."""
    if "ZK_POLY_HOST_MAX" not in os.environ:
        yield ctx
        return
    c = _ctx_under(ZK_POLY_HOST_MAX=None)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(dev):
    """The CU count the context plans with, from the planner itself: 513
    coefficients stay one chunk exactly when the point tiles reach 4 CUs."""
    lo, hi = 1, 1 << 20  # tiles; (1 << 20) tiles of 256 points is the evaluation cap
    assert poly.eval_plan(T + 1, lo * tm.BLOCK, dev)[0] > 1 and poly.eval_plan(T + 1, hi * tm.BLOCK, dev)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if poly.eval_plan(T + 1, mid * tm.BLOCK, dev)[0] == 1:
            hi = mid
        else:
            lo = mid
    assert hi % tm.FILL == 0
    n = hi // tm.FILL
    for m, d in ((1, 1553), (3, 513), (1025, 1100), (4096, 4096), (1, 600_000)):
        assert poly.eval_plan(d, m, dev) == tm.eval_plan(m, d, n)
    return n


def _mont(field: int, values) -> np.ndarray:
    p = po.MODULI[field]
    return as_limbs([v * (1 << 256) % p for v in values])


def _raw_interpolate(ctx, field, repr_, xs, ys):
    """zk_poly_interpolate as is: (code, coefficients as limbs)."""
    n = len(xs)
    conv = (lambda v: _mont(field, v)) if repr_ == MONT else (lambda v: as_limbs(list(v)))
    out = np.zeros((n, 4), np.uint64)
    cnt = C.c_uint64(77)
    code = _lib.lib().zk_poly_interpolate(ctx.h, field, repr_, ptr(conv(xs)), ptr(conv(ys)), n, ptr(out), n, C.byref(cnt))
    return code, out[: cnt.value] if code == 0 else None


@functools.lru_cache(maxsize=None)
def _rand(field: int, table: int, n: int) -> tuple:
    """synth(field, SEED, table, 0, n) on the host: shared, never modified."""
    return tuple(co.from_limbs(co.synth(field, SEED, table, 0, n)))


@functools.lru_cache(maxsize=None)
def _poly(field: int, n: int) -> tuple:
    """Exactly n coefficients, the top one non-zero."""
    cf = list(_rand(field, 4, n))
    if cf[-1] == 0:
        cf[-1] = 1
    return tuple(cf)


@functools.lru_cache(maxsize=None)
def _distinct_xs(field: int, n: int) -> tuple:
    """n distinct points, 0, 1 and p - 1 among them."""
    p = po.MODULI[field]
    xs = list(_rand(field, 5, n))
    xs[1], xs[n // 2], xs[n - 2] = 0, 1, p - 1
    assert len(set(xs)) == n
    return tuple(xs)


# --- (I1): the references of the interpolation over roots of unity ----------------------------
def _domain(n: int) -> int:
    return 1 << (n - 1).bit_length()


@functools.lru_cache(maxsize=None)
def _ntt(field: int, n: int) -> tuple:
    """The NTT over the N-th roots, N = 2^k >= n, of _poly(field, n): computed once per (field, n)."""
    return tuple(fo.fft_evaluate(field, list(_poly(field, n)) + [0] * (_domain(n) - n)))


@functools.lru_cache(maxsize=None)
def _root_powers(field: int, N: int) -> tuple:
    p, w = po.MODULI[field], fo.root_of_unity(field, N)
    out, cur = [], 1
    for _ in range(N):
        out.append(cur)
        cur = cur * w % p
    assert cur == 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _root_points(field: int, n: int) -> tuple:
    """(w^i, f(w^i)) at n distinct i of range(N) from a fixed-seed shuffle, not sorted: (xs, ys)."""
    N = _domain(n)
    idx = list(range(N))
    random.Random(SEED * 1_000_003 + n).shuffle(idx)
    idx = idx[:n]
    assert idx != sorted(idx)
    pw, Y = _root_powers(field, N), _ntt(field, n)
    return tuple(pw[i] for i in idx), tuple(Y[i] for i in idx)


def _assert_tree_wraps(n: int, steps: int) -> None:
    """The plan fact of the tree (no CU count in it; its constants are checked
    against the build by test_poly_cpu.py): the most steps a block takes, and
    that they are more than the parts they are dealt over."""
    most, log_len, parts = tm.tree_most_steps(n)
    assert most == steps and parts == tm.TREE_SPLIT and most > parts, (n, most, log_len, parts)


# n: the most steps a block of the tree takes
ROOT_SHAPES = {3072: 10, 4097: 16, 12289: 34, 65535: 256, 65536: 256}


@pytest.mark.parametrize("n", sorted(ROOT_SHAPES))
@pytest.mark.parametrize("field", FR_FIELDS)
def test_interpolate_roots_of_unity(dev, cus, field, n):
    """(I1). 3 072: a node that passes through at level 10, then a = 2 048, b =
    1 024 with 10 steps over 8 parts, the first wrap. 4 097: a = b = 2 048, 16
    steps, every part takes two; a pass-through point at every level; the top
    level is a = 4 096, b = 1. 12 289: three j0 trips per weights part. 65 535:
    a short last node at every level, just under the cap. 65 536: the cap, 256
    steps per block at the top level, weights in parts of 64 trips."""
    _assert_tree_wraps(n, ROOT_SHAPES[n])
    plan = tm.tree_plan(n)
    if n == 3072:
        assert plan[10][5] and not plan[11][5] and plan[11][2] == 1024
    if n == 4097:
        assert all(lv[5] for lv in plan[:12]) and plan[12][1:3] == (2, 1)
    if n == 12289:
        assert tm.weights_plan(n, cus) == (17, 3 * tm.BLOCK) and tm.weights_plan(n, cus)[1] > tm.BLOCK
    if n == 65535:
        assert all(lv[2] == (1 << lv[0]) - 1 for lv in plan[1:])
    if n == 65536:
        assert n == poly.INTERPOLATE_MAX and tm.weights_plan(n, cus) == (4, 64 * tm.BLOCK)
    xs, ys = _root_points(field, n)
    want = list(_poly(field, n))
    assert poly.interpolate(zip(xs, ys), field, dev).coefficient == want
    if n == 4097:  # both representations, through the raw entry
        code, out = _raw_interpolate(dev, field, MONT, xs, ys)
        assert code == 0 and np.array_equal(out, _mont(field, want))


@pytest.mark.parametrize("field", FR_FIELDS)
def test_interpolate_4097_under_grid_caps(dev3, dev1, field):
    """17 tiles over three blocks and over one: the wrapped deal and the x
    loop's further trips meet in one block (accumulators reset per tile, the
    step counter restarted, the barriers matched across skipped steps)."""
    n = 4097
    _assert_tree_wraps(n, ROOT_SHAPES[n])
    assert tm.ceil_div(n, tm.BLOCK) > 3
    xs, ys = _root_points(field, n)
    want = list(_poly(field, n))
    assert poly.interpolate(zip(xs, ys), field, dev3).coefficient == want
    assert poly.interpolate(zip(xs, ys), field, dev1).coefficient == want


# --- Fq, which has no domain --------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 1 << 16])
def test_fq_round_trip(dev, cus, n):
    """(I3): evaluate on the device, spot-check on the host, interpolate back
    to the input. The evaluation is the split path with many point tiles: 17
    times 9 chunks of one staging trip at 4 097, 256 times 4 chunks of 32 trips
    at 2^16 (on 256 CUs)."""
    p = po.MODULI[FQ]
    _assert_tree_wraps(n, ROOT_SHAPES[n])
    chunks, length = poly.eval_plan(n, n, dev)
    assert chunks > 1 and (length > T) == (n > 4097)
    f, xs = list(_poly(FQ, n)), list(_distinct_xs(FQ, n))
    ys = poly.evaluate_many(f, xs, FQ, dev)
    rng = random.Random(SEED + n)
    for i in [0, 1, n // 2, n - 2, n - 1] + [rng.randrange(n) for _ in range(27)]:
        assert ys[i] == O.horner(p, f, xs[i]), i
    assert poly.interpolate(zip(xs, ys), FQ, dev).coefficient == f


@pytest.mark.parametrize("n", [4097, 1 << 16])
def test_fq_top_power(dev, n):
    """y_i = x_i^(n - 1): full length, the top coefficient alone, nothing trimmed."""
    p = po.MODULI[FQ]
    _assert_tree_wraps(n, ROOT_SHAPES[n])
    xs = _distinct_xs(FQ, n)
    got = poly.interpolate([(x, pow(x, n - 1, p)) for x in xs], FQ, dev).coefficient
    assert got == [0] * (n - 1) + [1]


def test_fq_closed_forms_4097(dev):
    p = po.MODULI[FQ]
    n = 4097
    _assert_tree_wraps(n, ROOT_SHAPES[n])
    xs = _distinct_xs(FQ, n)
    quad = [p - 5, 3, 1]
    assert poly.interpolate([(x, O.horner(p, quad, x)) for x in xs], FQ, dev).coefficient == quad
    assert poly.interpolate([(x, 0) for x in xs], FQ, dev).coefficient == []  # every y = 0


# --- duplicates at scale ---------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_duplicate_x_at_12289(dev, cus, field):
    """Two equal x in different weights parts (the second one alone in the last
    part; in a later j0 trip of another part) and in the same part but
    different trips: ZK_EINVAL every time, and the flag does not stick."""
    p = po.MODULI[field]
    n = 12289
    parts, part_len = tm.weights_plan(n, cus)
    assert part_len > tm.BLOCK
    xs, ys = list(_distinct_xs(field, n)), list(_rand(field, 6, n))
    trip = lambda j: (j // part_len, j % part_len // tm.BLOCK)  # (the weights part, its j0 trip) that stages x_j
    last = list(xs)
    last[n - 1] = last[0]  # the last part holds this one point
    assert trip(0) == (0, 0) and trip(n - 1) == (parts - 1, 0) and parts > 1
    far = list(xs)
    far[n - 2] = far[0]
    assert trip(n - 2)[0] != 0 and trip(n - 2)[1] == 2
    near = list(xs)
    near[700] = near[300]
    assert trip(300)[0] == trip(700)[0] and trip(300)[1] != trip(700)[1]
    for bad in (last, far, near):
        code, _ = _raw_interpolate(dev, field, CANON, bad, ys)
        assert code == _lib.ZK_EINVAL
    quad = [p - 5, 3, 1]
    code, out = _raw_interpolate(dev, field, CANON, xs, [O.horner(p, quad, x) for x in xs])
    assert code == 0 and to_ints(out) == quad


# --- evaluation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 8192])
@pytest.mark.parametrize("field", FR_FIELDS)
def test_evaluate_all_roots_is_the_ntt(dev, field, N):
    """(I2): the split path with 16 and 32 point tiles times 8 and 16 chunks."""
    chunks, length = poly.eval_plan(N, N, dev)
    assert chunks > 1 and length == T and tm.ceil_div(N, tm.BLOCK) in (16, 32)
    f = list(_rand(field, 2, N))
    want = fo.fft_evaluate(field, f)
    assert poly.evaluate_many(f, _root_powers(field, N), field, dev) == want == fft.dev_fft(dev.synth(field, N, SEED, 2)).to_ints()


def test_evaluate_all_roots_folds_mod_x_n_minus_1(dev):
    """d = N + 5: the values at the N-th roots are the NTT of f folded mod X^N - 1; nine chunks, the last of five."""
    field, N = 0, 4096
    p = po.MODULI[field]
    d = N + 5
    chunks, length = poly.eval_plan(d, N, dev)
    assert chunks > 1 and d - (chunks - 1) * length == 5
    f = list(_rand(field, 2, d))
    folded = [(f[i] + (f[N + i] if N + i < d else 0)) % p for i in range(N)]
    assert poly.evaluate_many(f, _root_powers(field, N), field, dev) == fo.fft_evaluate(field, folded)


D1 = 2 * T + 76  # one chunk of three staging trips: 512, 512, 76


def _single_chunk_m(dev, cus) -> int:
    """The fewest points at which D1 coefficients stay one chunk on this device."""
    m = (tm.FILL * cus - 1) * tm.BLOCK + 1
    assert poly.eval_plan(D1, m, dev) == (1, D1) and poly.eval_plan(D1, m - 1, dev)[0] > 1
    assert D1 > 2 * T and D1 % T == 76
    return m


@functools.lru_cache(maxsize=None)
def _tiled_case(field: int, m: int):
    """(coefficients, xs as limbs, expected values as limbs): 64 distinct x, 0, 1
    and p - 1 among them, tiled to m points. Lanes are independent, so the
    repeats are legitimate; the reference is Horner at the 64."""
    p = po.MODULI[field]
    cf = list(_rand(field, 2, D1))
    base = [0, 1, p - 1] + list(_rand(field, 3, 61))
    assert len(set(base)) == 64
    want = [O.horner(p, cf, x) for x in base]
    reps = tm.ceil_div(m, 64)
    return cf, np.tile(as_limbs(base), (reps, 1))[:m].copy(), np.tile(as_limbs(want), (reps, 1))[:m].copy()


@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_second_staging_trip_single_chunk(dev, cus, field):
    """k_poly_eval's staging loop refilling its LDS tile inside one chunk: 1 100
    coefficients at the fewest points that keep them one run (261 889 on 256 CUs)."""
    m = _single_chunk_m(dev, cus)
    cf, xs, want = _tiled_case(field, m)
    out = np.zeros((m, 4), np.uint64)
    assert _lib.lib().zk_poly_evaluate(dev.h, field, CANON, ptr(as_limbs(cf)), D1, ptr(xs), m, ptr(out)) == 0
    assert np.array_equal(out, want)


@pytest.mark.parametrize("field", FIELDS)
def test_dev_evaluate_second_staging_trip_in_place(dev, cus, field):
    m = _single_chunk_m(dev, cus)
    cf, xs, want = _tiled_case(field, m)
    cf_t, xs_t = dev.upload(field, as_limbs(cf)), dev.upload(field, xs)
    assert poly.dev_evaluate(cf_t, xs_t, out=xs_t) is xs_t
    assert np.array_equal(xs_t.download(), want)
    assert cf_t.to_ints() == cf  # only read


@pytest.mark.parametrize("field,m", [(0, 1), (1, 1), (2, 1), (1, 3)])
def test_evaluate_second_staging_trip_split_path(dev, cus, field, m):
    """Chunks of two staging trips each on the split path (586 chunks of 1 024
    at 600 000 coefficients on 256 CUs), the last chunk neither full nor one
    tile long (960 = 512 + 448)."""
    p = po.MODULI[field]
    d = 600_000
    if d <= tm.FILL * cus * T:  # another device: chunks of 1 024 need more coefficients
        d = tm.FILL * cus * 2 * T - 64
    chunks, length = poly.eval_plan(d, m, dev)
    assert chunks > 1 and length >= 2 * T and d % length not in (0, T)
    cf = list(_rand(field, 2, d))
    xs = [_rand(field, 3, 2)[1]] if m == 1 else [p - 1, _rand(field, 3, 1)[0], 2]
    assert poly.evaluate_many(cf, xs, field, dev) == [O.horner(p, cf, x) for x in xs]


# --- the default context's crossover ------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_default_context_crossover(default, dev, field):
    """kPolyHostMaxDefault = 96: 95 and 96 points are interpolated on the host,
    97 and 128 on the device; 96 points of 96 coefficients are evaluated on the
    host, 97 on the device. Both sides agree with the oracle and with a context
    that runs everything on the device."""
    p = po.MODULI[field]
    for n in (HOST_MAX - 1, HOST_MAX, HOST_MAX + 1, 128):
        pts = list(zip(_distinct_xs(field, 128)[:n], _rand(field, 6, n)))
        want = O.interpolate_fast(p, pts)
        assert poly.interpolate(pts, field, default).coefficient == want == poly.interpolate(pts, field, dev).coefficient
    cf = list(_rand(field, 2, HOST_MAX))
    for m in (HOST_MAX, HOST_MAX + 1):
        xs = list(_distinct_xs(field, 128)[:m])
        want = [O.horner(p, cf, x) for x in xs]
        assert poly.evaluate_many(cf, xs, field, default) == want == poly.evaluate_many(cf, xs, field, dev)


# --- Shamir at a threshold the tree wraps at -----------------------------------------------------
def test_shamir_threshold_4097(dev):
    p = po.MODULI[FQ]
    t = 4097
    _assert_tree_wraps(t, ROOT_SHAPES[t])
    secret = 0x5EC2E7 * 0x10001 + 5
    rx, ry = _rand(FQ, 7, t - 1), _rand(FQ, 8, t - 1)
    assert len(set(rx)) == t - 1 and 0 not in rx
    f = shamir.create_polynomial(t, secret, 0, list(zip(rx, ry)), ctx=dev)
    assert f.coefficient[0] == secret and f.degree() == t - 1
    rng = random.Random(SEED)
    for i in [0, t - 2] + [rng.randrange(t - 1) for _ in range(30)]:
        assert O.horner(p, f.coefficient, rx[i]) == ry[i], i
    xs = list(_rand(FQ, 9, 5000))
    assert len(set(xs)) == 5000
    shares = shamir.share_points(5000, t, f, xs, ctx=dev)
    assert [x for x, _ in shares] == xs
    for i in (0, 499, 500, 4596, 4999):
        assert shares[i][1] == O.horner(p, f.coefficient, xs[i]), i
    back = shamir.recover_polynomial_all(shares[500:4597], t, ctx=dev)
    assert back.coefficient == f.coefficient and shamir.get_secret(back, 0) == secret

"""CPU checks of interpolation and batch evaluation over arbitrary points
(univariate_polynomial_dense.rs :20-26, :48-74; shamir_secret_sharing.rs): the
checkers of tests/poly_oracle.py against each other and against the
reference's own tests with the randomness passed in, the committed fixture
tests/golden/poly.json, every error code the three entry points return before
any device work, the planner csrc/poly_plan.hpp (compiled on its own, host code
only, with its invariants and the device inversion's constants checked natively),
and tests/poly_tree_model.py, the kernels' index arithmetic, over the planner's
plans against the oracle."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import coracle as co
import poly_oracle as O
import poly_tree_model as tm
import pyoracle as po
from conftest import ROOT

from zk_amd import _lib, poly, shamir
from zk_amd.api import UnivariatePoly
from zk_amd.elems import as_limbs, ptr

FIELDS = [0, 1, 2]
FQ = 1
P = po.MODULI[FQ]
CANON, MONT = 0, 1


def _fixture() -> dict:
    with open(os.path.join(ROOT, "tests", "golden", "poly.json")) as fh:
        return json.load(fh)


def _points(field: int, n: int, seed: int = 23):
    xs = co.from_limbs(co.synth(field, seed, 0, 0, n)) if n else []
    ys = co.from_limbs(co.synth(field, seed, 1, 0, n)) if n else []
    if n > 1:
        xs[1] = 0
    return list(zip(xs, ys))


@functools.lru_cache(maxsize=None)
def _fast(field: int, n: int, seed: int) -> tuple:
    """interpolate_fast of _points, computed once for the tests that share a shape (never modified)."""
    return tuple(O.interpolate_fast(po.MODULI[field], _points(field, n, seed)))


# --- the two oracles ------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_oracles_agree_up_to_48(field):
    """The reference's loop, the independent O(n^2) route and the older closed
    form of oracle/pyoracle.py give the same trimmed polynomial, and it takes y_i
    at every x_i."""
    p = po.MODULI[field]
    for n in range(0, 49):
        pts = _points(field, n, seed=5 + n)
        want = O.interpolate(p, pts)
        assert want == O.interpolate_fast(p, pts), (field, n)
        assert O.is_interpolant(p, want, pts)
        if n in (1, 7, 20):
            assert want == po.interpolate(p, [x for x, _ in pts], [y for _, y in pts])
    assert O.interpolate(p, []) == [] and O.interpolate(p, [(3, 0), (4, 0)]) == []
    low = [(x, O.horner(p, [p - 5, 3, 1], x)) for x, _ in _points(field, 30)]
    assert O.interpolate(p, low) == [p - 5, 3, 1] == O.interpolate_fast(p, low)
    with pytest.raises(ZeroDivisionError):
        O.interpolate(p, [(1, 2), (5, 3), (1, 4)])
    with pytest.raises(ZeroDivisionError):
        O.interpolate_fast(p, [(1, 2), (5, 3), (1, 4)])
    cf, x = co.from_limbs(co.synth(field, 5, 2, 0, 40)), co.from_limbs(co.synth(field, 5, 3, 0, 1))[0]
    assert O.evaluate(p, cf, x) == O.horner(p, cf, x) == po.uni_evaluate(p, cf, x)
    assert O.evaluate(p, [], x) == 0


# --- the reference's own tests --------------------------------------------------------
def test_univariate_reference_tests():  # univariate_polynomial_dense.rs :111-197
    a, b = [3, 4, 3], [P - 3, 0, 0, 4]
    assert O.degree(a) == 2 and UnivariatePoly(list(a), FQ).degree() == 2  # it_returns_degree
    assert O.evaluate(P, a, 3) == 42 == UnivariatePoly(a, FQ).evaluate(3)  # it_evaluates_poly
    assert O.scalar_mul(P, a, 2) == [6, 8, 6] == UnivariatePoly(a, FQ).scalar_mul(2).coefficient  # it_scales
    assert O.add(P, a, b) == [0, 4, 3, 4] == (UnivariatePoly(a, FQ) + UnivariatePoly(b, FQ)).coefficient  # it_adds_correctly
    assert O.mul(P, a, b) == [P - 9, P - 12, P - 9, 12, 16, 12]  # it_multiplies_correctly
    assert O.interpolate(P, [(0, 2), (1, 4), (2, 6)]) == [2, 2]  # it_interpolates_points


def test_shamir_reference_tests():  # shamir_secret_sharing.rs :77-169, the draws passed in
    rnd = list(zip(co.from_limbs(co.synth(FQ, 29, 0, 0, 3)), co.from_limbs(co.synth(FQ, 29, 1, 0, 3))))
    f = O.create_polynomial(4, 40, 6, rnd)  # it_creates_a_correct_polynomial
    assert O.degree(f) == 3 and O.evaluate(P, f, 6) == 40
    pts = [(1, P - 1), (2, 5), (3, 13)]
    assert O.recover_polynomial(pts, 3) == [P - 5, 3, 1]  # it_recreates_polynomial_with_valid_points
    assert O.get_secret([P - 5, 3, 1], 0) == P - 5  # it_returns_right_secret
    xs = co.from_limbs(co.synth(FQ, 29, 2, 0, 10))
    assert len(O.share_points(10, 3, [P - 5, 3, 1], xs)) == 10  # it_share_points_correctly
    wrong = O.recover_polynomial([(1, P - 1), (2, 5), (3, 1)], 3)  # it_doesnt_work_with_wrong_points
    assert wrong != [P - 5, 3, 1] and O.evaluate(P, wrong, 0) != P - 5
    with pytest.raises(ValueError):  # it_doesnt_generate_with_few_points (should_panic)
        O.recover_polynomial([(1, P - 1), (2, 5)], 3)
    # it_all_works_properly
    secret = O.create_polynomial(3, P - 5, 0, rnd[:2])
    shares = O.share_points(10, 3, secret, xs)
    again = O.recover_polynomial(shares[2:6], 3)
    assert again == secret and O.get_secret(again, 0) == P - 5
    with pytest.raises(ValueError):
        O.share_points(2, 3, secret, xs)


def test_fibonacci_check():  # sample_tests/src/fibonacci_evaluation.rs
    fib = [1, 1, 2, 3, 5, 8, 13, 21]
    f = O.interpolate(P, list(enumerate(fib)))
    for x in (2, 5, 7):
        assert O.evaluate(P, f, x) == (O.evaluate(P, f, x - 1) + O.evaluate(P, f, x - 2)) % P


def test_reference_bench_inputs():
    assert O.evaluate(P, list(range(100)), 2) == sum(i << i for i in range(100)) % P
    assert O.interpolate(P, [(x, 3 + 2 * x) for x in range(10)]) == [3, 2]


# --- the Python mirror's own argument rules (no device needed) ---------------------------
def test_shamir_mirror_refuses_like_the_reference():
    with pytest.raises(ValueError, match="Not enough points"):
        shamir.recover_polynomial([(1, P - 1), (2, 5)], 3)
    with pytest.raises(ValueError, match="Not enough points"):
        shamir.recover_polynomial_all([(1, 1)] * 39, 40)
    with pytest.raises(ValueError, match="Num of shares too low"):
        shamir.share_points(2, 3, UnivariatePoly([P - 5, 3, 1], FQ))
    with pytest.raises(ValueError):
        shamir.share_points(4, 3, UnivariatePoly([P - 5, 3, 1], FQ), random_xs=[1, 2, 3])
    with pytest.raises(ValueError):
        shamir.create_polynomial(3, 1, 0, random_points=[(1, 1)])
    assert "departs from the reference" in shamir.recover_polynomial_all.__doc__
    assert shamir.get_secret(UnivariatePoly([P - 5, 3, 1], FQ), 0) == P - 5  # it_returns_right_secret, host only
    assert poly.interpolate([], FQ, ctx=object()).coefficient == []  # no points: no call at all
    assert poly.evaluate_many([1, 2], [], FQ, ctx=object()) == []


# --- the fixture ------------------------------------------------------------------------
def test_fixture_digest_rederived():
    g = _fixture()
    assert g["seed"] == 23 and g["evaluate_shape"] == [2 * g["eval_tile"] + 76, 257]
    d, m = g["evaluate_shape"]
    for field in FIELDS:
        p = po.MODULI[field]
        cf, xs = co.from_limbs(co.synth(field, 23, 2, 0, d)), co.from_limbs(co.synth(field, 23, 3, 0, m))
        assert O.digest([O.horner(p, cf, x) for x in xs]) == g["evaluate_sha256"][str(field)]
        assert sorted(g["interpolate_sha256"][str(field)]) == ["1025"]
    # one of the interpolation digests, at the fixture's own points
    pts = _points(FQ, 1025)
    assert O.digest(O.interpolate_fast(P, pts)) == g["interpolate_sha256"][str(FQ)]["1025"]


# --- error codes returned before any device work -------------------------------------------
def test_entry_points_refuse_before_device_work():
    L = _lib.lib()
    x = as_limbs([1, 2, 3, 4])
    out = np.full((8, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    before = out.copy()
    n, ch, ln = C.c_uint64(77), C.c_uint32(76), C.c_uint64(75)
    big = (1 << 63) + 1
    for field in FIELDS:
        for repr_ in (CANON, MONT):
            # no context
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), 4, ptr(x), 0, ptr(out)) == _lib.ZK_EINVAL
            assert L.zk_poly_interpolate(None, field, repr_, ptr(x), ptr(x), 4, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
            assert L.zk_poly_interpolate(None, field, repr_, ptr(x), ptr(x), 0, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
            # beyond the caps
            assert L.zk_poly_interpolate(None, field, repr_, ptr(x), ptr(x), (1 << 16) + 1, ptr(out), big,
                                         C.byref(n)) == _lib.ZK_EUNSUPPORTED
            assert L.zk_poly_interpolate(None, field, repr_, ptr(x), ptr(x), big, ptr(out), big, C.byref(n)) == _lib.ZK_EUNSUPPORTED
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), (1 << 28) + 1, ptr(x), 1, ptr(out)) == _lib.ZK_EUNSUPPORTED
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), 1, ptr(x), (1 << 28) + 1, ptr(out)) == _lib.ZK_EUNSUPPORTED
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), 1 << 28, ptr(x), (1 << 12) + 1, ptr(out)) == _lib.ZK_EUNSUPPORTED
            assert L.zk_poly_evaluate(None, field, repr_, ptr(x), 1 << 28, ptr(x), 1 << 12, ptr(out)) == _lib.ZK_EINVAL  # (at the cap: the context)
            # cap < n
            assert L.zk_poly_interpolate(None, field, repr_, ptr(x), ptr(x), 4, ptr(out), 3, C.byref(n)) == _lib.ZK_EINVAL
        assert L.zk_dev_poly_evaluate(None, field, ptr(x), 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_dev_poly_evaluate(None, field, ptr(x), big, ptr(x), 4, ptr(out)) == _lib.ZK_EUNSUPPORTED
        # an unknown representation
        assert L.zk_poly_evaluate(None, field, 2, ptr(x), 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_poly_interpolate(None, field, 2, ptr(x), ptr(x), 4, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
    # an unknown field, null buffers
    for bad_field in (3, 7, -1):
        assert L.zk_poly_evaluate(None, bad_field, CANON, ptr(x), 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_dev_poly_evaluate(None, bad_field, ptr(x), 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_poly_interpolate(None, bad_field, CANON, ptr(x), ptr(x), (1 << 16) + 1, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
    assert L.zk_poly_evaluate(None, 0, CANON, None, 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_poly_evaluate(None, 0, CANON, ptr(x), 4, None, 4, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_poly_evaluate(None, 0, CANON, ptr(x), 4, ptr(x), 4, None) == _lib.ZK_EINVAL
    assert L.zk_dev_poly_evaluate(None, 0, None, 4, ptr(x), 4, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_poly_interpolate(None, 0, CANON, None, ptr(x), 4, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
    assert L.zk_poly_interpolate(None, 0, CANON, ptr(x), None, 4, ptr(out), 8, C.byref(n)) == _lib.ZK_EINVAL
    assert L.zk_poly_interpolate(None, 0, CANON, ptr(x), ptr(x), 4, None, 8, C.byref(n)) == _lib.ZK_EINVAL
    assert L.zk_poly_interpolate(None, 0, CANON, ptr(x), ptr(x), 4, ptr(out), 8, None) == _lib.ZK_EINVAL
    assert L.zk_poly_eval_plan(None, 4, 4, C.byref(ch), C.byref(ln)) == _lib.ZK_EINVAL
    assert L.zk_last_error() != b""
    assert np.array_equal(out, before) and (n.value, ch.value, ln.value) == (77, 76, 75)


# --- the planner ----------------------------------------------------------------------------
NAMED = [0, 1, 2, 3, 5, 63, 65, 129, 257, 300, 384, 511, 513, 700, 1025]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not present")
    exe = str(tmp_path_factory.mktemp("ppc") / "poly_plan_check")
    subprocess.run([clang, "-O2", "-std=c++17", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "zk-research-implementations_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "poly_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "0", "1", "96", "65536", "65537", "-2", ""] + ["n=%d" % n for n in NAMED],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "poly_plan_check ok"  # the invariants for n = 0 .. 300 and up to 2^16, checked natively
    consts = {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split()[1:])}
    knobs, trees, weights, evals = {}, {}, {}, {}
    for ln in lines[1:-1]:
        kind, _, rest = ln.partition(" ")
        if kind == "knob":
            k, v = rest.split("=")
            knobs[k] = int(v)
        elif kind == "tree":
            head, *levels = rest.split()
            trees[int(head[2:])] = [tuple(int(v) for v in lv.split(":")) for lv in levels]
        else:
            f = {k: int(v) for k, v in (kv.split("=") for kv in rest.split())}
            if kind == "weights":
                weights[(f["n"], f["cus"])] = (f["parts"], f["len"])
            else:
                evals[(f["m"], f["d"], f["cus"])] = (f["chunks"], f["len"])
    return consts, knobs, trees, weights, evals


def test_planner_and_model_agree(plans):
    consts, knobs, trees, weights, evals = plans
    assert (consts["block"], consts["eval_tile"], consts["tree_tile"], consts["fill"]) == (tm.BLOCK, tm.EVAL_TILE, tm.TREE_TILE, tm.FILL)
    assert consts["tree_split"] == tm.TREE_SPLIT
    assert [tm.tree_split(l) for l in (0, 6, 7, 8, 9, 10, 15)] == [1, 1, 1, 2, 4, 8, 8]
    assert consts["eval_tile"] == _fixture()["eval_tile"]
    assert consts["interp_max"] == 1 << 16 == poly.INTERPOLATE_MAX and consts["table_max_log"] == 28
    assert consts["eval_max_products"] == 1 << 40  # about ten seconds at 116 G products/s
    H = consts["host_max"]
    assert knobs == {"0": 0, "1": 1, "96": 96, "65536": 65536, "65537": H, "-2": H, "": H}
    assert sorted(trees) == NAMED
    for n, levels in trees.items():
        assert levels == [(l, a, b, c, d, int(e)) for l, a, b, c, d, e in tm.tree_plan(n)], n
        assert len(levels) == (max(n, 1) - 1).bit_length()
        # pass-through nodes at several levels at once: 2^k + 1 copies its last point all the way up
        if n == 1025:
            assert [lv[5] for lv in levels] == [1] * 10 + [0]
    assert weights and evals
    for (n, cus), got in weights.items():
        assert got == tm.weights_plan(n, cus)
    for (m, d, cus), got in evals.items():
        assert got == tm.eval_plan(m, d, cus)
    assert evals[(1, 1553, 256)] == (4, 512) and evals[(3, 513, 256)] == (2, 512)  # few points: the split path
    assert tm.eval_plan(1 << 20, 1 << 10, 256) == (1, 1 << 10) and tm.eval_plan(1, 512, 256) == (1, 512)


# --- the kernels' index arithmetic over those plans --------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 63, 65, 129, 257, 300, 384, 513])
def test_tree_model_equals_oracle(plans, n):
    """Leaf, one level, the first pass-through, whole pairs per block, one pair
    over several blocks, a short last node, pass-through nodes at several
    levels, with the full grid and grid-striding over three blocks."""
    _, _, trees, _, _ = plans
    field = n % 3
    p = po.MODULI[field]
    pts = _points(field, n, seed=31)
    want = O.interpolate_fast(p, pts)
    assert [lv[0] for lv in trees[n]] == [lv[0] for lv in tm.tree_plan(n)]
    assert tm.interpolate(p, pts) == want
    if n in (5, 257, 384):  # the capped launch path, one trip per block
        assert tm.interpolate(p, pts, num_cus=8, grid_x=3) == want
    if n in (3, 257):
        bad = list(pts)
        bad[n - 1] = (bad[0][0], 1)
        with pytest.raises(ZeroDivisionError):
            tm.interpolate(p, bad)


@pytest.mark.parametrize("n,grid_x", [(700, 2), (700, 1), (1025, 3)])
def test_tree_model_grid_stride(n, grid_x):
    """Fewer blocks than tiles (3 tiles over 2 and over 1, 5 over 3): blocks take a
    second trip of every kernel's x loop, reach the pass-through tile after a
    multiplying one, and mix small and large levels. The model gives every trip
    fresh LDS, so a read of a slot the trip did not stage fails."""
    field = 1
    p = po.MODULI[field]
    pts = _points(field, n, seed=31)
    assert tm.ceil_div(n, tm.BLOCK) > grid_x
    assert tm.interpolate(p, pts, num_cus=8, grid_x=grid_x) == list(_fast(field, n, 31))


@pytest.mark.parametrize("m,d,grid_x", [(1025, 100, 3), (700, 1553, 2), (600, 513, 1)])
def test_eval_model_grid_stride(m, d, grid_x):
    field = 2
    p = po.MODULI[field]
    cf, xs = co.from_limbs(co.synth(field, 31, 2, 0, d)), co.from_limbs(co.synth(field, 31, 3, 0, m))
    assert tm.ceil_div(m, tm.BLOCK) > grid_x and (tm.eval_plan(m, d, 8)[0] > 1) == (d > tm.EVAL_TILE)
    assert tm.evaluate(p, cf, xs, 8, grid_x=grid_x) == [O.horner(p, cf, x) for x in xs]


@pytest.mark.parametrize("m,d", [(1, 0), (1, 1), (65, 100), (3, 511), (3, 512), (3, 513), (1, 1553), (257, 1100), (300, 2)])
def test_eval_model_equals_oracle(m, d):
    field = (m + d) % 3
    p = po.MODULI[field]
    cf = co.from_limbs(co.synth(field, 31, 2, 0, d)) if d else []
    xs = (co.from_limbs(co.synth(field, 31, 3, 0, m)) + [0, 1, p - 1])[-m:]
    want = [O.horner(p, cf, x) for x in xs]
    assert tm.evaluate(p, cf, xs, 256) == want == tm.evaluate(p, cf, xs, 8, grid_x=3)
    assert want[0] == O.evaluate(p, cf, xs[0])


# --- paths the plans of a 256-CU device reach only at sizes the model cannot afford -----------
def test_eval_model_second_staging_trip():
    """One chunk of more than kPolyEvalTile coefficients with the build's own
    constants: on one CU five point tiles are already 4 CUs' worth, so 1 100
    coefficients stay one run and the staging loop of k_poly_eval takes three
    trips (512, 512, 76), the stage refilled after the trailing barrier."""
    field, m, d = 1, 1025, 1100
    p = po.MODULI[field]
    assert tm.eval_plan(m, d, 1) == (1, d) and d > 2 * tm.EVAL_TILE and d % tm.EVAL_TILE
    cf = co.from_limbs(co.synth(field, 31, 2, 0, d))
    xs = ([0, 1, p - 1] + co.from_limbs(co.synth(field, 31, 3, 0, m)))[:m]
    assert tm.evaluate(p, cf, xs, num_cus=1) == [O.horner(p, cf, x) for x in xs]


@pytest.mark.parametrize("n", [1025, 1536])
def test_tree_model_wrapped_deal(plans, n):
    """The round-robin deal of a large level's steps with more steps than parts:
    with the split constant lowered to 2 a block of a level with len >= 512
    takes up to four (n = 1 025) or six (n = 1 536) steps over two parts, so a
    part takes a second and, at 1 536, a third step (q >= S) with its sums carried across
    the steps it skips. The build's constant (asserted against the build in
    test_planner_and_model_agree) wraps from n = 2 818 on, which the model cannot
    afford; the GPU tests of tests/test_gpu_poly_scale.py run the kernel there."""
    consts = plans[0]
    assert consts["tree_split"] == tm.TREE_SPLIT == 8  # the default stays the build's
    split = 2
    wrapped = [(l, max(tm.tree_steps(n, l), default=0), tm.tree_split(l, split)) for l, *_ in tm.tree_plan(n)]
    assert max(steps for _, steps, _ in wrapped) == (4 if n == 1025 else 6)
    rounds = 1 if n == 1025 else 2  # every part takes a second step; at 1 536 a third one too
    assert any(steps > rounds * parts and parts == split for _, steps, parts in wrapped)
    assert all(steps <= tm.tree_split(l) for l, steps, _ in wrapped)  # the build's constant never wraps here
    assert tm.tree_most_steps(2817)[0] == 8 and tm.tree_most_steps(2818) == (9, 11, 8)  # the first n that does
    field = 1
    p = po.MODULI[field]
    pts = _points(field, n, seed=31)
    want = list(_fast(field, n, 31))
    # 1 025 over three blocks along x: the wrapped deal and the x loop's further trips meet in one block
    assert tm.interpolate(p, pts, num_cus=8, grid_x=3 if n == 1025 else None, split=split) == want


@pytest.mark.parametrize("n,plan", [(513, (2, 512)), (1281, (1, 1536))])
def test_weights_model_several_trips_per_part(n, plan):
    """k_poly_weights with part_len > 256: a part's j0 loop takes a second trip
    (two parts of 512 at n = 513 on one CU, the second one short; one part of
    six trips at n = 1 281), the LDS stage refilled inside one part and the
    j = i skip landing in a later trip. With y = 1 leaf i holds 1 / d_i: checked
    against d_i = prod_{j != i} (x_i - x_j) at lanes of every trip."""
    field, num_cus = 2, 1
    p = po.MODULI[field]
    assert tm.weights_plan(n, num_cus) == plan and plan[1] > tm.BLOCK
    assert all(tm.weights_plan(k, num_cus)[1] == tm.BLOCK for k in range(1, 513))  # 513 is the smallest such n
    xs = [x for x, _ in _points(field, n, seed=31)]
    M, N, dup = tm.leaves(p, xs, [1] * n, num_cus)
    assert dup == 0 and M == [(-x) % p for x in xs]
    for i in (0, 255, 256, 300, 511, 512, n - 1):
        d_i = 1
        for j, xj in enumerate(xs):
            if j != i:
                d_i = d_i * (xs[i] - xj) % p
        assert N[i] * d_i % p == 1, i

"""The GKR round kernels on saturating and boundary-value tables
(tests/extreme_tables.py; the paper side is tests/test_extreme_tables_cpu.py).

Every other GPU test that runs a GKR proof feeds the kernels uniformly random
elements: the int32 tiles of the matrix-core steps are then random walks far
inside their bounds, the digit encoding never ripples a carry over more than
one word, and the lazy ranges never reach their edges. Here the tables hold
the words that do: all comparisons are equalities with the C oracle
(coracle.gkr_prove / prove / partial_evaluate) on the canonical tables
word R^-1 mod p, and after each proof ctx.stats() must show that the kernel
kinds the case is aimed at were launched (a knob that no longer steers is a
failure, not a silent pass).

(a) every family through every schedule at n = 4, 9, 11, 12, 14;
(b) saturated tables with ZK_GRID_CAP=1, where step_grid floors the grid at
    the count that leaves a block exactly its chunk maximum;
(c) plain prove / verify, partial_evaluate and the tensor tables on the same
    words.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import coracle as co
import extreme_tables as xt

import zk_amd
from zk_amd._lib import check, lib
from zk_amd.api import MLE_ADD, MLE_MUL
from zk_amd.context import REPR_MONTGOMERY
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2]
MATRIX_KINDS = ("gkr_d0", "gkr_dm", "gkr_t33")
SINGLE = ("gkr_round", "gkr_round_lanes")  # a single round: either kernel (by the pair count)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _prove(ctx, field: int, tabs) -> tuple[list, list]:
    """As _prove of test_gpu_prelaunch.py, over uploaded Montgomery words."""
    n = tabs[0].words.shape[0].bit_length() - 1
    dev = [ctx.upload(field, t.words, REPR_MONTGOMERY) for t in tabs]
    arr = (C.c_void_p * 4)(*[d.ptr.value for d in dev])
    coeffs = np.zeros((n, 3, 4), np.uint64)
    nco = np.zeros(n, np.uint8)
    ch = np.zeros((n, 4), np.uint64)
    tr = zk_amd.Transcript(field)
    check(lib().zk_dev_gkr_sumcheck_prove_sharded(ctx.h, field, arr, n, 0, ptr(as_limbs([0])), tr.h, ptr(coeffs),
                                                  ptr(nco), ptr(ch)))
    for d in dev:
        d.free()
    return [to_ints(coeffs[k, : nco[k]]) for k in range(n)], to_ints(ch)


_ORACLE: dict = {}


def _oracle(field: int, name: str, n: int, tabs) -> tuple[list, list]:
    key = (field, name, n)
    if key not in _ORACLE:
        polys, chal = co.gkr_prove(field, [t.canon for t in tabs], co.Transcript(), fast=n >= 16)
        _ORACLE[key] = ([list(p) for p in polys], list(chal))
    return _ORACLE[key]


def _launched(ctx) -> set:
    return {k for k, v in ctx.stats()["kernels"].items() if v["launches"] > 0}


def _check_kinds(ctx, must, never, what):
    got = _launched(ctx)
    for k in must:
        alts = k if isinstance(k, tuple) else (k,)
        assert any(a in got for a in alts), f"{what}: no {' / '.join(alts)} launch (launched: {sorted(got)})"
    for k in never:
        assert k not in got, f"{what}: {k} launched (launched: {sorted(got)})"


def _run(monkeypatch, env: dict, field: int, n: int, names, must, never=()):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    ctx = zk_amd.Context(0)
    try:
        for name in names:
            tabs = xt.family(name, field, n)
            want = _oracle(field, name, n, tabs)
            ctx.reset_stats()
            got = _prove(ctx, field, tabs)
            what = f"{name} field {field} n {n} {env}"
            assert got == want, what
            _check_kinds(ctx, must, never, what)
    finally:
        ctx.close()


@pytest.mark.parametrize("field", FIELDS)
def test_canonical_tables_are_what_the_device_holds(ctx, field):
    """The oracle's tables, word R^-1 mod p in Python, are what the device
    makes of the uploaded Montgomery words."""
    tabs = [xt.Table(field, xt.special_list(field))] + xt.family("sprinkled", field, 9) + xt.family("checker_pm1", field, 6)
    for t in tabs:
        d = ctx.upload(field, t.words, REPR_MONTGOMERY)
        assert np.array_equal(d.download(), t.canon)
        assert np.array_equal(d.download(REPR_MONTGOMERY), t.words)
        d.free()


# ---------------------------------------------------------------------------
# (a) every family through every schedule, small
# ---------------------------------------------------------------------------
# The kernel kinds each (setting, n) must launch, from the planner's schedule
# (csrc/gkr_plan.hpp; tests/test_gkr_plan_cpu.py prints it) and the kernel
# choice of host.hpp (gkr_d0 = k_gkr_d0m or k_gkr_d0t, gkr_dm = k_gkr_dm or
# k_gkr_dm3):
#   default    4: D0 DOUBLE | 9: ROUND0 SINGLE SINGLE DTAIL HOST | 11: D0T T32 DTAIL HOST
#              12: D0 DTAIL HOST | 14: D0T T33 T32 DTAIL HOST
#   ZK_D0T=0   11: ROUND0 SINGLE SINGLE DTAIL HOST | 14: D0 DTAIL HOST (others as default)
_DEFAULT = {4: ("gkr_d0", "gkr_dround"), 9: ("gkr_round0", SINGLE, "gkr_dtail"), 11: ("gkr_d0", "gkr_dm", "gkr_dtail"),
            12: ("gkr_d0", "gkr_dtail"), 14: ("gkr_d0", "gkr_t33", "gkr_dm", "gkr_dtail")}
_TWO_ROUND = {4: ("gkr_d0", "gkr_dround"), 9: ("gkr_round0", SINGLE, "gkr_dtail"), 11: ("gkr_round0", SINGLE, "gkr_dtail"),
              12: ("gkr_d0", "gkr_dtail"), 14: ("gkr_d0", "gkr_dtail")}
_VALU = {4: ("gkr_round0", SINGLE, "gkr_dround"), 9: ("gkr_round0", SINGLE, "gkr_dtail"),
         11: ("gkr_round0", SINGLE, "gkr_dtail"), 12: ("gkr_round0", SINGLE, "gkr_dtail"),
         14: ("gkr_round0", SINGLE, "gkr_dtail")}
SETTINGS = {
    "default": ({}, _DEFAULT, ()),
    "d0t0": ({"ZK_D0T": "0"}, _TWO_ROUND, ("gkr_t33",)),
    # As the two-round schedule stands, every double step of these sizes has at
    # most 1024 quads and runs inside the persistent k_gkr_dtail, so
    # ZK_DM_MIN_QUADS alone launches no k_gkr_dm below n = 16 ...
    "d0t0-dm64": ({"ZK_D0T": "0", "ZK_DM_MIN_QUADS": "64"}, _TWO_ROUND, ("gkr_t33",)),
    # ... ZK_DTAIL_MAX_QUADS=16 leaves the double steps of >= 64 quads outside it:
    # k_gkr_dm at n = 12 (256, 64 quads) and 14 (1024, 256, 64); n = 11 starts its
    # doubles with one pending challenge (k_gkr_dround<1>, 64 quads)
    "d0t0-dm64-dtail16": ({"ZK_D0T": "0", "ZK_DM_MIN_QUADS": "64", "ZK_DTAIL_MAX_QUADS": "16"},
                          {4: ("gkr_d0", "gkr_dround"), 9: ("gkr_round0", SINGLE, "gkr_dtail"),
                           11: ("gkr_round0", SINGLE, "gkr_dround", "gkr_dtail"), 12: ("gkr_d0", "gkr_dm", "gkr_dtail"),
                           14: ("gkr_d0", "gkr_dm", "gkr_dtail")}, ("gkr_t33",)),
    "valu": ({"ZK_D0T": "0", "ZK_D0": "0", "ZK_DM": "0"}, _VALU, MATRIX_KINDS),
    "dround0": ({"ZK_DROUND": "0"}, {n: ("gkr_round0", "gkr_tail") for n in (4, 9, 11, 12, 14)},
                MATRIX_KINDS + ("gkr_dround", "gkr_dtail")),
    "host0": ({"ZK_HOST_ROUNDS": "0"}, _DEFAULT, ()),
    "lc0": ({"ZK_LC_LOADS": "0"}, _DEFAULT, ()),
    # (1 is the default; no level of these sizes has a 64-octant chunk per CU, so k_gkr_t33
    # takes 32-octant chunks here either way: the 64-octant loops are in (b))
    "oct64min1": ({"ZK_T33_OCT64_MIN": "1"}, _DEFAULT, ()),
    "prelaunch0": ({"ZK_PRELAUNCH": "0"},
                   {4: ("gkr_d0", "gkr_dround"), 9: ("gkr_round0", SINGLE, "gkr_dround"),
                    11: ("gkr_d0", "gkr_dm", "gkr_dround"), 12: ("gkr_d0", "gkr_dround"),
                    14: ("gkr_d0", "gkr_t33", "gkr_dm", "gkr_dround")}, ("gkr_dtail", "gkr_tail")),
}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("n", [4, 9, 11, 12, 14])
@pytest.mark.parametrize("field", FIELDS)
def test_every_family_through_every_schedule(monkeypatch, field, n, setting):
    """All families at the two-round schedule's smallest size (4), an odd size
    (9), the smallest three-round schedules (11: k_gkr_d0t with lane-contiguous
    loads + k_gkr_dm3; 14: + a 32-octant k_gkr_t33) and the even size between
    that stays on k_gkr_d0m (12). Constant tables stay constant under every
    fold, so const_neg_neg keeps every level of the proof saturated: the
    K = 256 folds with all-maximal B digits, the tails and the host rounds."""
    env, must, never = SETTINGS[setting]
    _run(monkeypatch, env, field, n, list(xt.FAMILIES), must[n], never)


# ---------------------------------------------------------------------------
# (b) saturation at the per-block chunk maximum
# ---------------------------------------------------------------------------
# ZK_GRID_CAP=1 caps every matrix-core step's grid at one block; step_grid
# (host.hpp) floors it at ceil(chunks / k*ChunksMax) (mfma.hpp). Sizes, from
# the constants (kD0TChunksMax 512, kT33ChunksMax 256 / 128, kD0MChunksMax
# 2048, kDMChunksMax 1024) and the schedules above:
#  d0t    n = 17: O = 2^14 octants = 512 chunks of 32 per product; floor
#         2 ceil(512 / 512) = 2 blocks, one per product, 512 chunks each. Two
#         blocks is also the least k_gkr_d0t ever gets, so n = 18 (1024 chunks
#         per product, floor 4 blocks of 512) is the smallest size at which
#         the blocks stay at the maximum only because of the floor.
#  dm3    n = 19 (D0T T32 DOUBLE ...; no k_gkr_t33 at 19 variables): Q = 2^14
#         quads = 256 chunks of 64 in ONE block, the most k_gkr_dm3 gets below
#         25 variables (its maximum, 1024, is out of reach of the schedule).
#  t33<32> n = 20 with ZK_T33_OCT64_MIN=4 (32-octant chunks while a level has
#         fewer than 4 x 256 chunks of 64): the first k_gkr_t33 folds to
#         O = 2^14 octants = 512 chunks of 32; floor ceil(512 / 256) = 2
#         blocks of 256. (At 18 variables it has 128 chunks, at 19 none.)
#  t33<64> n = 20: O = 2^14 = 256 chunks of 64; floor ceil(256 / 128) = 2 blocks
#         of 128: the pipelined loop with lane-contiguous loads (default),
#         without them (ZK_LC_LOADS=0), and the plain loop (ZK_T33_PIPE=0).
#  d0m, dm n = 20 with ZK_D0T=0: k_gkr_d0m has Q = 2^18 quads = 8192 chunks of
#         32; floor ceil(8192 / (2 x 2048)) = 2 blocks, each wave 2048 chunks.
#         The first double step has Q = 2^16 quads = 1024 chunks of 64: one
#         block at kDMChunksMax, once ZK_DM_MIN_QUADS (default 2^17) admits it.
CHUNK_MAX = {
    "d0t-17": (17, {}, ("gkr_d0", "gkr_dm", "gkr_dtail"), ("gkr_t33",)),
    "d0t-18": (18, {}, ("gkr_d0", "gkr_t33", "gkr_dm", "gkr_dtail"), ()),
    "dm3-19": (19, {}, ("gkr_d0", "gkr_dm", "gkr_dround", "gkr_dtail"), ("gkr_t33",)),
    "t33oct32-20": (20, {"ZK_T33_OCT64_MIN": "4"}, ("gkr_d0", "gkr_t33", "gkr_dm"), ()),
    "t33oct64-lc-20": (20, {}, ("gkr_d0", "gkr_t33", "gkr_dm"), ()),
    "t33oct64-pipe-20": (20, {"ZK_LC_LOADS": "0"}, ("gkr_d0", "gkr_t33", "gkr_dm"), ()),
    "t33oct64-plain-20": (20, {"ZK_T33_PIPE": "0"}, ("gkr_d0", "gkr_t33", "gkr_dm"), ()),
    "d0m-dm-20": (20, {"ZK_D0T": "0", "ZK_DM_MIN_QUADS": "65536"}, ("gkr_d0", "gkr_dm", "gkr_dround"), ("gkr_t33",)),
}
# field 1 shares field 0's code path (both lazy): const_neg_neg is enough there
CHUNK_MAX_CASES = [(f, name) for f in (0, 2) for name in ("const_neg_neg", "const_pos_neg", "checker_sat_top3")] + \
                  [(1, "const_neg_neg")]


@pytest.mark.parametrize("field,name", CHUNK_MAX_CASES)
@pytest.mark.parametrize("case", list(CHUNK_MAX))
def test_saturated_tiles_at_the_chunk_maximum(monkeypatch, case, field, name):
    """sat- * sat- adds exactly 2^19 per MFMA to every tile entry below digit
    31, so a block at its chunk maximum reaches the 2^30 the int32 tiles are
    sized for (const_neg_neg: every entry positive; const_pos_neg: every entry
    negative, G < 0 through the + M offset; checker_sat_top3: the corners
    differ in sign, so the moment / category tiles differ from each other)."""
    n, env, must, never = CHUNK_MAX[case]
    _run(monkeypatch, dict(env, ZK_GRID_CAP="1"), field, n, [name], must, never)


# ---------------------------------------------------------------------------
# (c) the other consumers of the same arithmetic
# ---------------------------------------------------------------------------
def _plain_prove(ctx, field: int, t) -> None:
    n = t.words.shape[0].bit_length() - 1
    rp = np.zeros((2 * n, 4), np.uint64)
    cs = np.zeros((1, 4), np.uint64)
    check(lib().zk_sumcheck_prove(ctx.h, field, REPR_MONTGOMERY, ptr(t.words), n, ptr(rp), ptr(cs)))
    want_rp, want_cs = co.prove(field, t.canon)
    # outputs come back in Montgomery form: convert through the device
    assert ctx.upload(field, rp, REPR_MONTGOMERY).to_ints() == co.from_limbs(want_rp.reshape(-1, 4))
    assert ctx.upload(field, cs, REPR_MONTGOMERY).to_ints() == [want_cs]
    ok = C.c_int(0)
    check(lib().zk_sumcheck_verify(ctx.h, field, REPR_MONTGOMERY, ptr(t.words), n, ptr(rp), n, 2, ptr(cs), C.byref(ok)))
    assert ok.value == 1
    assert co.verify(field, t.canon, want_rp, want_cs) == 1


@pytest.mark.parametrize("name", ["const_pm1", "checker_pm1", "sprinkled"])
@pytest.mark.parametrize("n", [9, 16])
@pytest.mark.parametrize("field", FIELDS)
def test_plain_sumcheck_on_extreme_tables(ctx, field, n, name):
    _plain_prove(ctx, field, xt.family(name, field, n)[0])


def test_plain_sumcheck_const_pm1_20var(ctx):
    _plain_prove(ctx, 1, xt.family("const_pm1", 1, 20)[0])


@pytest.mark.parametrize("name", ["checker_pm1", "const_neg_neg"])
@pytest.mark.parametrize("field", FIELDS)
def test_partial_evaluate_on_extreme_tables(ctx, field, name):
    p = xt.modulus(field)
    rs = [0, 1, p - 1, xt.canonical(field, xt.specials(field)["sat-"])]
    for n, bits in ((7, range(7)), (13, [0])):
        t = xt.family(name, field, n)[0]
        d_in = ctx.upload(field, t.words, REPR_MONTGOMERY)
        d_out = ctx.alloc(field, 1 << (n - 1))
        for bit in bits:
            for r in rs:
                check(lib().zk_dev_mle_partial_evaluate(ctx.h, field, d_in.ptr, n, bit, 0, ptr(as_limbs([r])), d_out.ptr))
                assert np.array_equal(d_out.download(), co.partial_evaluate(field, t.canon, bit, r)), (n, bit, hex(r))
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("field", FIELDS)
def test_tensor_tables_on_extreme_tables(ctx, field):
    p, h = xt.modulus(field), 6
    a, b = xt.family("checker_sat_lane", field, h)[:2]  # a: sat- / sat+ alternating, b: all sat-
    da, db = ctx.upload(field, a.words, REPR_MONTGOMERY), ctx.upload(field, b.words, REPR_MONTGOMERY)
    out = ctx.alloc(field, 1 << (2 * h))
    av, bv = a.canon_ints(), b.canon_ints()
    for op, f in ((MLE_ADD, lambda x, y: (x + y) % p), (MLE_MUL, lambda x, y: x * y % p)):
        for (dx, xv), (dy, yv) in (((da, av), (db, bv)), ((da, av), (da, av))):
            check(lib().zk_dev_mle_tensor(ctx.h, field, op, dx.ptr, 1 << h, dy.ptr, 1 << h, out.ptr))
            assert out.to_ints() == [f(x, y) for x in xv for y in yv]
    for d in (da, db, out):
        d.free()

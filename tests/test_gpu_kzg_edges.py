"""The KZG path at its edges, through the public ABI only (csrc/msm.hpp and the
device half of csrc/kzg.hip; cases and oracles from tests/ec_cases.py).

Width sweep: msm_g1 at every signed-digit window width, forced by ZK_MSM_C
(6, 7, 9, 11, 12, 14, 15, 16, 18, 19, 20; 17 rounds to 16) or chosen by
msm_window_bits (8, 10, 13), with that width's whole scalar family — every
window at 2^(c-1) (bucket 0, weighed apart), one above (all negative), 2^254 - 1
(digits of 2^c that are skipped and still carry), r - 1, ... — sprinkled over
random scalars, on bases that mix k G, the order-3 point (0, 2), two points
with boundary-word x-coordinates and infinity; two blocks of the bucket sort,
the second partial. Also on contexts under ZK_MSM_BALANCED=0 and
ZK_MSM_WIN_TASK=2 and 7.

Level-batched widths: get_proof at 12 variables at its own width (6), under
ZK_MSM_C=12 (the sort's LDS bin table exactly full) and 13.

Degenerate setups: taus from {0, 1, r - 1} make most of the Lagrange basis the
point at infinity — k_fixed_base8 / k_fixed_base20 on scalar 0, k_pair_sum on
infinities, k_batch_normalize's Z = 0 skip inside a shared inversion (18 and 20
variables), MSMs over mostly-infinity bases, a verifier with tau G2 at
infinity. taus = [t, 1, .., 1] hand the fixed-base kernels a chosen scalar t.

Zero quotients: constant tables, tables of the last variable only, and
openings at points of {0, 1, r - 1}.

All exact: every comparison is equality of group elements."""
from __future__ import annotations

import random

import numpy as np
import pytest

import ec_cases as ec
import kzg_oracle as ko
import pairing_oracle as pao
import pyoracle as po

import zk_amd
from zk_amd._lib import check, lib
from zk_amd.context import REPR_CANONICAL
from zk_amd.elems import ptr, to_ints
from zk_amd.kzg import KZG, _points, msm_g1

pytestmark = pytest.mark.gpu
R = ko.R
G = ko.G1

# ---- width sweep ------------------------------------------------------------------------------
FORCED = (6, 7, 9, 11, 12, 14, 15, 16, 18, 19, 20)
DEFAULT_N = {8: 4500, 10: 8000, 13: 58000}  # n for which msm_window_bits picks the width (pinned in test_ec_cases_cpu.py)
SWEEP_N = 1500  # two sort blocks of 1024 points, the second partial
POOL = [ec.base_g(1), ec.base_g(2), ec.base_g(0x1234567), ec.BASE_T, ec.base_palette(5), ec.base_palette(17),
        ec.BASE_INF, ec.base_g(R - 1)]


def sweep_case(c: int, n: int):
    """-> (points, scalars, expected) for width c: random scalars, the family of c at a stride
    coprime to the pool (every family member meets every kind of base)"""
    rng = random.Random(1000 + c)
    bases = [POOL[i % len(POOL)] for i in range(n)]
    scalars = [rng.randrange(R) for _ in range(n)]
    fam = ec.scalar_family(c)
    for j in range(len(fam) * len(POOL)):
        scalars[(j * 7 + 3) % n] = fam[j % len(fam)]
    # equal bases with equal scalars meet in one bucket (the doubling branch); G and -G (pool
    # entries 0 and 7) with equal scalars cancel there
    for j in range(0, 64, 8):
        scalars[n - 1 - j] = fam[0]
    for m in range(100, 108):  # (past the sprinkled family)
        scalars[8 * m + 7] = scalars[8 * m]
    return [b.pt for b in bases], scalars, ec.msm_expected(bases, scalars)


@pytest.mark.parametrize("c", FORCED)
def test_msm_at_a_forced_width(ctx, monkeypatch, c):
    pts, scalars, want = sweep_case(c, SWEEP_N)
    monkeypatch.setenv("ZK_MSM_C", str(c))
    assert msm_g1(pts, scalars, ctx) == want


@pytest.mark.parametrize("c", sorted(DEFAULT_N))
def test_msm_at_a_default_width(ctx, monkeypatch, c):
    monkeypatch.delenv("ZK_MSM_C", raising=False)
    n = DEFAULT_N[c]
    assert ec.msm_window_bits(n) == c
    pts, scalars, want = sweep_case(c, n)
    assert msm_g1(pts, scalars, ctx) == want


@pytest.mark.parametrize("name,value", [("ZK_MSM_BALANCED", "0"), ("ZK_MSM_WIN_TASK", "2"), ("ZK_MSM_WIN_TASK", "7")])
def test_msm_widths_on_other_reduction_paths(monkeypatch, name, value):
    """The per-bucket bucket sums (ZK_MSM_BALANCED=0) and window sums in tasks of
    2 and of 7 points (ZK_MSM_WIN_TASK; 4 by default), read when a context is made."""
    monkeypatch.setenv(name, value)
    ctx = zk_amd.Context(0)
    try:
        for c in (6, 11, 16):
            pts, scalars, want = sweep_case(c, SWEEP_N)
            monkeypatch.setenv("ZK_MSM_C", str(c))
            assert msm_g1(pts, scalars, ctx) == want, c
    finally:
        ctx.close()


# ---- level-batched widths ---------------------------------------------------------------------
def quotient_points(evals, v, point, taus):
    """q_i(taus[i + 1:]) * G for every quotient of get_proof (kzg.rs:59-95)"""
    cur = [(e - v) % R for e in evals]
    out = []
    for i in range(len(point)):
        q = ko.get_quotient(cur)
        out.append(ko.mul(po.evaluate(R, q, taus[i + 1:]) if len(q) > 1 else q[0], G))
        cur = ko.get_remainder(cur, point[i])
    return out


@pytest.fixture(scope="module")
def opening12():
    rng = random.Random(1212)
    n = 12
    taus = [rng.randrange(R) for _ in range(n)]
    evals = [rng.randrange(R) for _ in range(1 << n)]
    fam = ec.scalar_family(12) + ec.scalar_family(13) + ec.scalar_family(6)
    for j, s in enumerate(fam):
        evals[(j * 101 + 7) % len(evals)] = s
    point = [rng.randrange(R) for _ in range(n)]
    v = po.evaluate(R, evals, point)
    return taus, evals, point, v, quotient_points(evals, v, point, taus)


@pytest.mark.parametrize("c", [None, 12, 13])
def test_get_proof_level_batched_at_width(ctx, monkeypatch, opening12, c):
    """12 batched levels: width 6 by default; ZK_MSM_C=12 fills the sort's coarse-bin
    table exactly (12 x 22 windows << 6 = 16896 = kSortBinsMax), 13 takes 15360."""
    taus, evals, point, v, want = opening12
    assert ec.msm_window_bits(4095, levels=12) == 6 and ec.sort_bins(12, 12) == ec.SORT_BINS_MAX
    k = KZG(taus, ctx)
    try:
        if c is None:
            monkeypatch.delenv("ZK_MSM_C", raising=False)
        else:
            monkeypatch.setenv("ZK_MSM_C", str(c))
        assert k.get_proof(v, point, evals) == want
    finally:
        k.close()


def test_a_forced_width_whose_bins_do_not_fit_is_refused(ctx, monkeypatch, opening12):
    """ZK_MSM_C=16 over 12 levels would need 12 x 16 windows << 8 = 49152 coarse bins: the
    host refuses before any sort kernel runs (so the widths above did take effect: the
    variable is read), and the context goes on working."""
    taus, evals, point, v, want = opening12
    assert ec.sort_bins(16, 12) == 49152 > ec.SORT_BINS_MAX
    k = KZG(taus, ctx)
    try:
        monkeypatch.setenv("ZK_MSM_C", "16")
        with pytest.raises(ValueError, match="coarse bins exceed"):
            k.get_proof(v, point, evals)
        monkeypatch.delenv("ZK_MSM_C")
        assert k.get_proof(v, point, evals) == want
    finally:
        k.close()


# ---- degenerate taus --------------------------------------------------------------------------
def sparse_eq(taus: list[int]) -> dict[int, int]:
    """{i: eq(taus, i)} over the non-zero entries only (MSB first, as kzg_oracle.lagrange_scalars)"""
    cur = {0: 1}
    for t in taus:
        nxt = {}
        for i, e in cur.items():
            for bit, f in ((0, (1 - t) % R), (1, t % R)):
                if f:
                    nxt[2 * i + bit] = e * f % R
        cur = nxt
    return cur


_mul_cache: dict[int, tuple] = {}


def mul_g(s: int):
    if s not in _mul_cache:
        _mul_cache[s] = ko.mul(s, G)
    return _mul_cache[s]


def basis_rows(ctx, k: KZG, v: int) -> np.ndarray:
    out = np.zeros((1 << v, 12), np.uint64)
    check(lib().zk_kzg_lagrange_basis(ctx.h, k.h, v, ptr(out)))
    return out


def check_basis(ctx, k: KZG, taus: list[int]):
    """every suffix level: infinity exactly where eq is 0 (numpy mask), eq * G elsewhere"""
    nv = len(taus)
    for v in range(nv + 1):
        rows = basis_rows(ctx, k, v)
        want = sparse_eq(taus[nv - v:])
        nz = np.flatnonzero(rows.any(axis=1))
        assert nz.tolist() == sorted(want), v
        got = _points(rows[nz])
        assert got == [mul_g(want[i]) for i in sorted(want)], v
    assert _points(basis_rows(ctx, k, 0)) == [G]


def degenerate_taus(nv: int, seed: int) -> list[int]:
    """mostly 0 and 1, two r - 1 and (from 6 variables) two free values"""
    rng = random.Random(seed)
    taus = [rng.randrange(2) for _ in range(nv)]
    special = [R - 1, R - 1] + ([rng.randrange(R), rng.randrange(R)] if nv >= 6 else [])
    for pos, s in zip(rng.sample(range(nv), len(special)), special):
        taus[pos] = s
    return taus


SMALL_TAUS = [[0, 1, R - 1], [1, 0, 0], [0, 0, 0], [1, 1, 1], [R - 1, 7, 0],
              [0, 0x123456789, 1, R - 1, 1, 0], degenerate_taus(6, 6)]


@pytest.mark.parametrize("taus", SMALL_TAUS, ids=lambda t: "-".join("r1" if x == R - 1 else str(x)[:6] for x in t))
def test_degenerate_small_setup(ctx, taus):
    """3 and 6 variables (k_fixed_base8): basis, commit, get_proof against the
    literal oracle, and the verifier — tau G2 is infinity where tau is 0."""
    nv = len(taus)
    rng = random.Random(nv * 100 + sum(t % 5 for t in taus))
    k = KZG(taus, ctx)
    try:
        check_basis(ctx, k, taus)
        basis = ko.get_lagrange_basis(taus)
        assert k.lagrange_basis() == basis
        evals = [rng.randrange(R) for _ in range(1 << nv)]
        c = k.commit(evals)
        assert c == mul_g(po.evaluate(R, evals, taus))
        g2t = k.g2_taus
        assert g2t == pao.g2_taus(taus)
        for point in ([rng.randrange(R) for _ in range(nv)], [(0, 1, R - 1)[(i + nv) % 3] for i in range(nv)]):
            v = k.open(point, evals)
            assert v == po.evaluate(R, evals, point)
            proof = k.get_proof(v, point, evals)
            assert proof == ko.get_proof(evals, v, point, basis)
            assert KZG.verify(c, v, proof, point, g2t)
            assert not KZG.verify(c, (v + 1) % R, proof, point, g2t)
    finally:
        k.close()


@pytest.mark.parametrize("nv", [16, 18, 20])
def test_degenerate_large_setup(ctx, nv):
    """k_fixed_base20 with scalar 0 nearly everywhere; the basis normalised 1, 2 and
    8 points per inversion (16, 18, 20 variables), most of them Z = 0; a commitment
    over a basis that is infinity except at 16 points."""
    taus = degenerate_taus(nv, nv)
    k = KZG(taus, ctx)
    try:
        check_basis(ctx, k, taus)
        N = 1 << nv
        evals = np.random.default_rng(nv).integers(0, 1 << 63, size=(N, 4), dtype=np.uint64)
        evals[:, 3] &= np.uint64((1 << 60) - 1)  # below 2^252 < r
        out = np.zeros((1, 12), np.uint64)
        check(lib().zk_kzg_commit(ctx.h, k.h, REPR_CANONICAL, ptr(evals), ptr(out)))
        eq = sparse_eq(taus)
        idx = sorted(eq)
        f = to_ints(evals[idx])
        assert _points(out)[0] == mul_g(sum(fi * eq[i] for fi, i in zip(f, idx)) % R)
    finally:
        k.close()


# ---- chosen fixed-base scalars ----------------------------------------------------------------
def check_chosen_scalar(ctx, nv: int, t: int):
    k = KZG([t] + [1] * (nv - 1), ctx)
    try:
        rows = basis_rows(ctx, k, nv)
        want = {i: p for i, p in (((1 << (nv - 1)) - 1, mul_g((1 - t) % R)), ((1 << nv) - 1, mul_g(t))) if p is not None}
        nz = np.flatnonzero(rows.any(axis=1))
        assert nz.tolist() == sorted(want), hex(t)
        assert _points(rows[nz]) == [want[i] for i in sorted(want)], hex(t)
    finally:
        k.close()


def test_fixed_base20_on_the_20_bit_family(ctx):
    """taus = [t, 1, .., 1]: the basis is (1 - t) G at 2^(nv-1) - 1, t G at 2^nv - 1 and
    infinity elsewhere, so k_fixed_base20 (16 variables) gets t and 1 - t as scalars."""
    for t in ec.scalar_family(20):
        check_chosen_scalar(ctx, 16, t)


def test_fixed_base8_on_the_byte_family(ctx):
    for t in ec.byte_family():
        check_chosen_scalar(ctx, 6, t)


# ---- zero quotients ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(12, None), (16, "0")], ids=["12", "16-unbatched"])
def opening_setup(request):
    nv, batch = request.param
    rng = random.Random(40 + nv)
    taus = [rng.randrange(R) for _ in range(nv)]
    return nv, batch, taus


def test_zero_quotients(ctx, monkeypatch, opening_setup):
    nv, batch, taus = opening_setup
    if batch is not None:
        monkeypatch.setenv("ZK_PROOF_BATCH_LEVELS", batch)
    rng = random.Random(50 + nv)
    N = 1 << nv
    k = KZG(taus, ctx)
    try:
        g2t = k.g2_taus
        # a constant table: every quotient is zero
        v = rng.randrange(R)
        point = [rng.randrange(R) for _ in range(nv)]
        proof = k.get_proof(v, point, [v] * N)
        assert proof == [None] * nv
        assert KZG.verify(mul_g(v), v, proof, point, g2t)
        assert not KZG.verify(mul_g(v), (v + 1) % R, proof, point, g2t)
        # a table of the last variable only: one non-zero quotient, the constant b - a
        a, b = rng.randrange(R), rng.randrange(R)
        evals = [a, b] * (N // 2)
        v = (a + (b - a) * point[-1]) % R
        assert k.open(point, evals) == v
        proof = k.get_proof(v, point, evals)
        assert proof == [None] * (nv - 1) + [mul_g((b - a) % R)]
        assert KZG.verify(k.commit(evals), v, proof, point, g2t)
        # a point of 0, 1 and r - 1 only
        evals = [rng.randrange(R) for _ in range(N)]
        point = [(0, 1, R - 1)[(i * 5 + nv) % 3] for i in range(nv)]
        v = k.open(point, evals)
        assert v == po.evaluate(R, evals, point)
        proof = k.get_proof(v, point, evals)
        assert proof == quotient_points(evals, v, point, taus)
        assert KZG.verify(k.commit(evals), v, proof, point, g2t)
    finally:
        k.close()

"""tests/ec_cases.py itself, and csrc/ec.hpp compiled for the host, on the CPU.

1. The case tables are what they claim: 56 palette words below p, 29 palette
   points on the curve, T of order 3, and the scalar families drive the Python
   model of msm.hpp's signed_digits to the edges they are named for, at every
   width the GPU sweep runs (tests/test_gpu_kzg_edges.py).
2. The restatement of kzg.hip's msm_window_bits is pinned: its constants are
   read back from the sources, and the widths the GPU tests rely on are stated.
3. The host legs of the ec.hpp probe (tests/native/ec_probe.hip): every Fq op
   on all 56 x 56 pairs (binary) or 56 words (unary) and every G1 op on all
   group-law cases, against Python integers. The host leg takes fqh::mul
   (6 x 64-bit); tests/test_gpu_ec_probe.py runs the same cases through the
   device leg (the 12 x 32-bit CIOS), so a failure there and none here puts the
   fault in the 32-bit path or in its generated code.

Without hipcc the probe cannot be built and part 3 skips."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

import ec_cases as ec
import kzg_oracle as ko

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ec.PKG, "csrc")
SWEEP_WIDTHS = (6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20)


# ---- 1. the tables ----------------------------------------------------------------------
def test_palette_is_56_words_below_p():
    pal = ec.PALETTE
    assert len(pal) == len(set(pal)) == 56 and all(0 <= w < ec.P for w in pal)
    top = (((ec.P >> 352) - 1) << 352) | ((1 << 352) - 1)
    assert top in pal and top + (1 << 352) >= ec.P
    for k in range(1, 12):
        assert {1 << 32 * k, (1 << 32 * k) - 1, ec.P - (1 << 32 * k), ec.P - (1 << 32 * k) + 1} <= set(pal)


def test_points_are_on_the_curve():
    assert len(ec.PALETTE_POINTS) == 29
    assert all(ko.on_curve(pt) for pt in ec.POINTS) and None not in ec.POINTS
    assert {ec.mont(x) for x, _ in ec.PALETTE_POINTS} <= set(ec.PALETTE)
    T = ec.T
    assert ko.on_curve(T) and ko.add(T, T) == ko.neg(T) and ko.add(T, ko.add(T, T)) is None
    assert ec.mul_int(3, T) is None and ec.mul_int(ko.R, ko.G1) is None and ec.mul_int(5, ko.G1) == ko.mul(5, ko.G1)


def test_group_law_cases_cover_the_exceptional_branches():
    cs = {label: (a, b, want) for label, a, b, want in ec.pair_cases()}
    assert cs["T+T"][2] == ko.neg(ec.T) and cs["T+2T"][2] is None
    assert cs["inf+inf"][2] is None and cs["ginf+ginf"][2] is None
    n = len(ec.POINTS)
    for i in range(n):
        a, b, want = cs[f"P{i}+P other Z"]
        assert a.pt == b.pt and a.lam != b.lam and want == ko.add(a.pt, a.pt) and want is not None
        a, b, want = cs[f"P{i}-P other Z"]
        assert a.lam != b.lam and want is None
        assert cs[f"ginf+P{i}"][2] == ec.POINTS[i] == cs[f"P{i}+inf"][2]
    # an encoded operand decodes to its point whatever its Z, and garbage under Z = 0 is infinity
    for o in ec.unary_operands():
        assert ec.dec_jac(ec.enc_jac(o)) == o.pt == ec.dec_xyzz(ec.enc_xyzz(o))
    assert all(w != 0 for w in ec.enc_jac(ec.GINF)[:2]) and ec.enc_jac(ec.GINF)[2] == 0
    assert {k for _, k, _ in ec.mul_small_cases()} == {0, 1, 2, 3, 1 << 31, (1 << 32) - 1}


@pytest.mark.parametrize("c", SWEEP_WIDTHS)
def test_scalar_families_reach_the_signed_digit_edges(c):
    W, cb = ec.window_shape(c)
    assert cb == c and W * c >= 256
    half = 1 << (c - 1)
    fam = ec.scalar_family(c)
    for s in fam:  # every member: canonical, no carry lost, digits sum back to it
        d, carry = ec.signed_digits(s, c, W)
        assert 0 <= s < ko.R and carry == 0
        assert sum((-m if neg else m) << (c * w) for w, _, m, neg in d) == s
        assert all(m <= half for _, _, m, _ in d)
    # the windows that lie wholly below bit 254: all but the top one, W - 1 — except at c = 15, where
    # 17 windows cover the 255 bits exactly and the 18th (W c >= 256) never holds more than a carry
    full = 254 // c
    assert full == (W - 2 if c == 15 else W - 1)
    rest = W - full - 1
    h = ec.half_all(c)
    d, _ = ec.signed_digits(h, c, W)
    assert [(m, neg) for _, _, m, neg in d] == [(half, 0)] * full + [(0, 0)] * (rest + 1)  # all in bucket 0
    d, _ = ec.signed_digits(h + 1, c, W)
    assert [(m, neg) for _, _, m, neg in d] == [(half - 1, 1)] * full + [(1, 0)] + [(0, 0)] * rest
    d, _ = ec.signed_digits((1 << 254) - 1, c, W)
    assert sum(1 for _, raw, m, neg in d if raw == 1 << c and m == 0 and neg) == full - 1  # skipped, still carrying
    d, _ = ec.signed_digits(ko.R - 1, c, W)
    assert d[-1][2] <= half  # the top window holds the last carry


def test_forced_and_batched_widths_fit_the_sort_bins():
    for c in SWEEP_WIDTHS:
        assert ec.sort_bins(c) <= 13312, c  # kSortBinsSingle
    assert ec.sort_bins(12, levels=12) == 16896 == ec.SORT_BINS_MAX  # exactly full
    assert ec.sort_bins(13, levels=12) == 15360
    assert ec.sort_bins(6, levels=12) <= ec.SORT_BINS_MAX < ec.sort_bins(16, levels=12)
    assert ec.window_shape(17) == (16, 16)  # why the sweep leaves 17 out


# ---- 2. the window-width restatement -------------------------------------------------------
def test_msm_window_bits_restates_the_source():
    src = open(os.path.join(CSRC, "kzg.hip")).read()
    body = src[src.index("inline uint32_t msm_window_bits"):]
    body = body[: body.index("\n}\n")]
    cands = re.search(r"for \(uint32_t cc : \{([^}]*)\}\)", body).group(1)
    assert tuple(int(x.strip().rstrip("u")) for x in cands.split(",")) == ec.MSM_WIDTHS
    assert float(re.search(r"constexpr double kBucketCost = ([0-9.]+);", src).group(1)) == ec.BUCKET_COST
    assert "if (f >= 6 && f <= 20) return f;" in body
    assert "if (lg < 12 && levels == 0) return std::min<uint32_t>(20, std::max<uint32_t>(6, lg > 9 ? lg - 3 : 6));" in body
    assert "if (levels == 0 && cc == 6) continue;" in body
    assert "const double cost = (double)n * W + kBucketCost * Wt * (double)(1ull << bb);" in body
    msm = open(os.path.join(CSRC, "msm.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kSortBinsMax = (\d+);", msm).group(1)) == ec.SORT_BINS_MAX
    assert "sort_fine_bits(uint32_t b) { return b / 2; }" in msm


def test_msm_window_bits_values():
    assert ec.msm_window_bits(2 * 16384 + 777) == 10 and ec.window_shape(10) == (26, 10)
    assert ec.msm_window_bits(1500) == 7 and ec.msm_window_bits(1 << 9) == 6
    assert [ec.msm_window_bits(n) for n in (4096, 4500, 7679)] == [8, 8, 8]
    assert [ec.msm_window_bits(n) for n in (7681, 8000, 57000)] == [10, 10, 10]
    assert [ec.msm_window_bits(n) for n in (57200, 58000, 1 << 19)] == [13, 13, 13]
    assert ec.msm_window_bits(1 << 22) == 16 and ec.msm_window_bits(1 << 24) == 20
    assert ec.msm_window_bits((1 << 12) - 1, levels=12) == 6  # get_proof's batched pass at 12 variables
    assert ec.msm_window_bits(1500, forced=19) == 19 and ec.msm_window_bits(1500, forced=21) == 7


# ---- 3. the host legs ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """The built probe; a tree that has not been built gets one in a temporary directory."""
    if os.path.exists(ec.PROBE_PATH):
        return ec.Probe()
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("ecprobe") / "libzkecprobe.so")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-shared", "-o", so,
                    ec.PROBE_SRC], check=True, capture_output=True, timeout=600)
    return ec.Probe(so)


@pytest.mark.parametrize("op", ec.FQ_OPS)
def test_fq_host_leg_equals_python_integers(probe, op):
    a, b, _ = ec.fq_cases(op)
    assert len(a) >= (56 * 56 if op in ec.FQ_BINARY else 56)
    bad = ec.fq_failures(probe, op, 0)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("op", ec.G1_OPS)
def test_g1_host_leg_equals_the_python_group_law(probe, op):
    assert probe.g1_shape(op) == ec.G1_SHAPES[op]
    bad = ec.g1_failures(probe, op, 0)
    assert not bad, (len(bad), bad[:5])


def test_probe_refuses_bad_arguments(probe):
    assert probe.lib.zk_ecprobe_fq(len(ec.FQ_OPS), 0, None, None, 1, None) == 1
    assert probe.lib.zk_ecprobe_g1(-1, 0, None, None, 1, None) == 1
    assert probe.lib.zk_ecprobe_fq(0, 0, None, None, 1, None) == 2
    assert probe.lib.zk_ecprobe_g1(1, 0, None, None, 0, None) == 0  # nothing to do

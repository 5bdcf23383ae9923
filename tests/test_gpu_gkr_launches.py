"""Which kernels a GKR sum-check proof launches, in order, at the sizes where
the step schedule changes shape (csrc/gkr_plan.hpp plan_phase, enqueued by
host.hpp gkr_phase): BN254 Fr, default knobs, device-resident tables. Each
proof must also equal the oracle's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import coracle as co

from zk_amd import Transcript
from zk_amd._lib import check, lib
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu
FIELD = 0

# n = 8: rounds 0-1 in one pass, the double steps in the persistent kernel (the
# last rounds on the host); 9: round 0, two single rounds; 11: the smallest
# three-round input pass (counted under gkr_d0), then the two-round step that
# folds by three (gkr_dm); 16: the smallest size with a k_gkr_t33 step
LAUNCHES = {
    8: ["gkr_d0", "gkr_dtail"],
    9: ["gkr_round0", "gkr_round_lanes", "gkr_round_lanes", "gkr_dtail"],
    11: ["gkr_d0", "gkr_dm", "gkr_dtail"],
    16: ["gkr_d0", "gkr_t33", "gkr_dm", "gkr_dtail"],
}


@pytest.mark.parametrize("n", sorted(LAUNCHES))
def test_gkr_launch_sequence(ctx, n):
    dev = [ctx.synth(FIELD, 1 << n, seed=41, table=t) for t in range(4)]
    arr = (C.c_void_p * 4)(*[d.ptr.value for d in dev])
    coeffs = np.zeros((n, 3, 4), np.uint64)
    nco = np.zeros(n, np.uint8)
    ch = np.zeros((n, 4), np.uint64)
    tr = Transcript(FIELD)
    ctx.set_timing(True)
    try:
        ctx.reset_stats()  # (the tables are resident: only the proof's launches are logged)
        check(lib().zk_dev_gkr_sumcheck_prove(ctx.h, FIELD, arr, n, 0, ptr(as_limbs([0])), tr.h, ptr(coeffs), ptr(nco),
                                              ptr(ch)))
        kinds = [x["kind"] for x in ctx.launches() if x["kind"].startswith("gkr_")]
    finally:
        ctx.set_timing(False)
    print(n, kinds)
    assert kinds == LAUNCHES[n]
    polys, chal = co.gkr_prove(FIELD, [co.synth(FIELD, 41, t, 0, 1 << n) for t in range(4)], co.Transcript())
    assert [to_ints(coeffs[k, : nco[k]]) for k in range(n)] == polys
    assert to_ints(ch) == chal

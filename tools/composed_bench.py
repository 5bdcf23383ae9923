"""The composed sum-check on one GPU: what the general prover
costs beside the four-table prover on the shape both can prove, and how close
its round kernels come to the memory system on degree-3 shapes.

usage: python tools/composed_bench.py [--min-seconds 1.0] [--nvars 20 24] [--big 24] [--out FILE]
(the JSON lines also go to --out, by default profiles/composed_bench.json)

One JSON line per case, all over BN254 Fr, tables synthesised on the device
(zk_dev_synth_fill) and proved in place through the device-resident calls:
  gkr4_2^n      four tables, factors [[0,1],[2,3]], through
                zk_dev_composed_sumcheck_prove (composed_ms) and
                zk_dev_gkr_sumcheck_prove (gkr_ms) in the same process, the two
                alternating; same_bytes: coefficients, counts, challenges and
                the transcript state after the proof are equal (asserted);
                composed_over_gkr = composed_ms / gkr_ms.
  eq_a_b        three tables, one term, degree 3.
  eq_ab_eq_cd   five tables, factors [[0,1,2],[0,3,4]]: eq shared by two terms.
Each *_ms is the median host-clock time of the synchronous C call after two
warm-up calls, timed over at least --min-seconds in total; *_ms_min the fastest
call. *_kernel_ms, *_alg_bytes and *_launches are the round kernels' event-timed
device time, algorithmic bytes and count from one further call with launch
timing on; frac_of_8TBps = alg_bytes / kernel time / 8e12; outside_kernels =
1 - kernel_ms / ms, the share of the call that is not round-kernel time
(launch, hand-off, transcript, host rounds).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zk-research-implementations_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 23
FIELD = 0
ROUND_KINDS = ("gkr_round0", "gkr_round", "gkr_round_lanes", "gkr_tail", "gkr_dround", "gkr_dtail", "gkr_d0", "gkr_dm",
               "gkr_t33")


def timed_pair(fns, min_seconds: float, min_reps: int = 5) -> list[list[float]]:
    """Times the functions in turn (a, b, a, b, ...): drift hits both alike."""
    ts, total = [[] for _ in fns], 0.0
    while total < min_seconds or len(ts[0]) < min_reps:
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            ts[i].append(dt)
            total += dt
    return ts


class Out:
    def __init__(self, n: int, width: int, ntables: int):
        self.coeffs = np.zeros((n, width, 4), np.uint64)
        self.nco = np.zeros(n, np.uint8)
        self.ch = np.zeros((n, 4), np.uint64)
        self.ev = np.zeros((ntables, 4), np.uint64)
        self.cs = np.zeros((1, 4), np.uint64)
        self.state = b""

    def same(self, o: "Out") -> bool:
        return (np.array_equal(self.coeffs, o.coeffs) and np.array_equal(self.nco, o.nco)
                and np.array_equal(self.ch, o.ch) and self.state == o.state)


def composed_call(ctx, tables, factors, nvars):
    import zk_amd
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr

    degree = len(factors[0])
    fac = np.array([f for t in factors for f in t], np.uint8)
    arr = (C.c_void_p * len(tables))(*[t.ptr.value for t in tables])
    o = Out(nvars, degree + 1, len(tables))
    claim = as_limbs([1])

    def call():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, arr, len(tables), nvars, ptr(fac), len(factors), degree,
                                                   ptr(claim), t.h, ptr(o.coeffs), ptr(o.nco), ptr(o.ch), ptr(o.ev),
                                                   ptr(o.cs)))
        o.state = t.to_bytes()
    return call, o


def gkr_call(ctx, tables, nvars):
    import zk_amd
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr

    arr = (C.c_void_p * 4)(*[t.ptr.value for t in tables])
    o = Out(nvars, 3, 4)
    claim = as_limbs([1])

    def call():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_gkr_sumcheck_prove(ctx.h, FIELD, arr, nvars, 0, ptr(claim), t.h, ptr(o.coeffs), ptr(o.nco),
                                              ptr(o.ch)))
        o.state = t.to_bytes()
    return call, o


def kernel_stats(ctx, call, name: str) -> dict:
    """One more call of its own with every launch event-timed (not one of the timed calls)."""
    ctx.set_timing(True)
    ctx.reset_stats()
    call()
    k = ctx.stats()["kernels"]
    ctx.set_timing(False)
    rk = [k[x] for x in ROUND_KINDS]
    return {f"{name}_launches": sum(v["launches"] for v in rk), f"{name}_kernel_ms": sum(v["ms"] for v in rk),
            f"{name}_alg_bytes": sum(v["alg_bytes"] for v in rk)}


def summary(name: str, ts: list[float]) -> dict:
    return {f"{name}_ms": statistics.median(ts) * 1e3, f"{name}_ms_min": min(ts) * 1e3, f"{name}_reps": len(ts)}


def derived(res: dict, name: str) -> None:
    res[f"{name}_frac_of_8TBps"] = res[f"{name}_alg_bytes"] / (res[f"{name}_kernel_ms"] * 1e-3) / 8e12
    res[f"{name}_outside_kernels"] = 1.0 - res[f"{name}_kernel_ms"] / res[f"{name}_ms"]


def bench_gkr4(ctx, nvars: int, min_seconds: float) -> dict:
    tables = [ctx.synth(FIELD, 1 << nvars, SEED, t) for t in range(4)]
    ccall, co = composed_call(ctx, tables, [[0, 1], [2, 3]], nvars)
    gcall, go = gkr_call(ctx, tables, nvars)
    for _ in range(2):
        ccall()
        gcall()
    if not co.same(go):
        raise RuntimeError("the composed prover's proof of the four-table shape differs from zk_dev_gkr_sumcheck_prove's")
    tc, tg = timed_pair([ccall, gcall], min_seconds)
    res = {"tool": "composed_bench", "case": f"gkr4_2^{nvars}", "nvars": nvars, "same_bytes": True,
           **summary("composed", tc), **summary("gkr", tg), **kernel_stats(ctx, ccall, "composed"),
           **kernel_stats(ctx, gcall, "gkr")}
    res["composed_over_gkr"] = res["composed_ms"] / res["gkr_ms"]
    derived(res, "composed")
    derived(res, "gkr")
    for t in tables:
        t.free()
    return res


def bench_shape(ctx, name: str, ntables: int, factors, nvars: int, min_seconds: float) -> dict:
    import zk_amd

    tables = [ctx.synth(FIELD, 1 << nvars, SEED, t) for t in range(ntables)]
    call, o = composed_call(ctx, tables, factors, nvars)
    for _ in range(2):
        call()
    # what is timed is a proof that passes the verifier's final check: its last round polynomial at the last
    # challenge is the combination of its table evaluations
    from zk_amd.elems import to_ints

    polys = [zk_amd.UnivariatePoly(to_ints(o.coeffs[k, : o.nco[k]]), FIELD) for k in range(nvars)]
    ch, ev = to_ints(o.ch), to_ints(o.ev)
    if polys[-1].evaluate(ch[-1]) != zk_amd.composed_combine(ev, factors, FIELD):
        raise RuntimeError("the benchmarked proof fails the final check")
    (ts,) = timed_pair([call], min_seconds)
    res = {"tool": "composed_bench", "case": name, "nvars": nvars, "ntables": ntables, "factors": factors,
           **summary(name, ts), **kernel_stats(ctx, call, name)}
    derived(res, name)
    for t in tables:
        t.free()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--nvars", type=int, nargs="*", default=[20, 24], help="sizes of the four-table comparison")
    ap.add_argument("--big", type=int, default=24, help="size of the degree-3 shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composed_bench.json"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    res = [bench_gkr4(ctx, n, a.min_seconds) for n in a.nvars]
    res.append(bench_shape(ctx, "eq_a_b", 3, [[0, 1, 2]], a.big, a.min_seconds))
    res.append(bench_shape(ctx, "eq_ab_eq_cd", 5, [[0, 1, 2], [0, 3, 4]], a.big, a.min_seconds))
    lines = [json.dumps(r) for r in res]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

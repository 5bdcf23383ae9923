"""The committed sum-check on one GPU: the rate of the
linear-combination kernel, what a batched KZG opening costs beside single
openings, and one whole proof split into its parts.

usage: python tools/committed_bench.py [--min-seconds 1.0] [--lincomb 20 24] [--nvars 20] [--out FILE]
(the JSON lines also go to --out, by default profiles/committed_bench.json)

One JSON line per case, all over BLS12-381 Fr, tables synthesised on the device
(zk_dev_synth_fill) and used in place:
  lincomb_2^n_k     zk_dev_mle_lincomb of k = 4 and 16 tables of 2^n entries, the
                    two alternating. kernel_ms: the median event-timed duration
                    of the k_lincomb launch (launch events, timing on for the
                    kind); alg_bytes = 32 (k + 1) 2^n; frac_of_8TBps = alg_bytes
                    / kernel time / 8e12; ms: the median host-clock time of the
                    synchronous call.
  batch_open_2^n    one KZG setup of n variables, 16 tables. In turn, in the same
                    run: one zk_dev_kzg_get_proof (single), zk_dev_kzg_batch_open
                    of 4 and of 16 tables (batch4, batch16), and 4 and 16 single
                    openings one after the other (singles4, singles16). The
                    point and the opened values come from a degree-1 composed
                    sum-check over the same tables; the 16-table batched proof
                    is checked by zk_kzg_batch_verify (asserted).
                    batch16_over_single is the issue's condition (<= 1.25).
  zero_check_2^n    eq a b + neq c one with a, b, c committed (c = a b, made on
                    the host once): zk_dev_committed_sumcheck_prove (whole) and,
                    alternating with it, its three parts through the public
                    calls: zk_dev_kzg_commit_batch (commit), the sum-check
                    (sumcheck) and zk_dev_kzg_batch_open (open). The proof is
                    checked by zk_committed_sumcheck_verify (asserted).
Each *_ms is a median after two warm-up rounds, timed over at least
--min-seconds in total and at least five rounds; *_ms_min the fastest call.
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

SEED = 29
FIELD = 2


def timed_round(fns, min_seconds: float, min_reps: int = 5) -> list[list[float]]:
    """Times the functions in turn (a, b, c, a, b, c, ...): drift hits all alike."""
    ts, total = [[] for _ in fns], 0.0
    while total < min_seconds or len(ts[0]) < min_reps:
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            ts[i].append(dt)
            total += dt
    return ts


def summary(name: str, ts: list[float]) -> dict:
    return {f"{name}_ms": statistics.median(ts) * 1e3, f"{name}_ms_min": min(ts) * 1e3, f"{name}_reps": len(ts)}


def pointers(tables):
    return (C.c_void_p * len(tables))(*[t.ptr.value for t in tables])


def bench_lincomb(ctx, lg: int, min_seconds: float) -> list[dict]:
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr

    n = 1 << lg
    tables = [ctx.synth(FIELD, n, SEED, t) for t in range(16)]
    out = ctx.alloc(FIELD, n)
    coeffs = as_limbs([3 + 5 * i for i in range(16)])
    const = as_limbs([7])
    kernel_ms = {4: [], 16: []}

    def call(k):
        arr = pointers(tables[:k])

        def go():
            ctx.reset_stats()
            check(lib().zk_dev_mle_lincomb(ctx.h, FIELD, 0, arr, k, ptr(coeffs), ptr(const), n, out.ptr))
            kernel_ms[k] += [x["ms"] for x in ctx.launches() if x["kind"] == "fold"]
        return go

    ctx.set_timing_kinds(["fold"])
    calls = [call(4), call(16)]
    for fn in calls * 2:
        fn()
    for v in kernel_ms.values():
        v.clear()
    ts = timed_round(calls, min_seconds)
    ctx.set_timing(False)
    res = []
    for k, t in zip((4, 16), ts):
        alg = 32.0 * (k + 1) * n
        km = statistics.median(kernel_ms[k])
        res.append({"tool": "committed_bench", "case": f"lincomb_2^{lg}_{k}", "log2_entries": lg, "ntables": k,
                    **summary("call", t), "kernel_ms": km, "kernel_ms_min": min(kernel_ms[k]),
                    "kernel_launches_timed": len(kernel_ms[k]), "alg_bytes": alg,
                    "frac_of_8TBps": alg / (km * 1e-3) / 8e12, "TBps": alg / (km * 1e-3) / 1e12})
    for t in tables + [out]:
        t.free()
    return res


def degree1_evals(ctx, tables, nvars):
    """(challenges, table i at the challenges) from a degree-1 composed sum-check over the tables"""
    import zk_amd
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr

    k = len(tables)
    fac = np.arange(k, dtype=np.uint8)
    coeffs, nco = np.zeros((nvars, 2, 4), np.uint64), np.zeros(nvars, np.uint8)
    ch, ev, cs = np.zeros((nvars, 4), np.uint64), np.zeros((k, 4), np.uint64), np.zeros((1, 4), np.uint64)
    t = zk_amd.Transcript(FIELD)
    check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, pointers(tables), k, nvars, ptr(fac), k, 1,
                                               ptr(as_limbs([0])), t.h, ptr(coeffs), ptr(nco), ptr(ch), ptr(ev), ptr(cs)))
    return ch, ev


def bench_batch_open(ctx, nvars: int, min_seconds: float) -> dict:
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr
    from zk_amd.kzg import KZG

    n = 1 << nvars
    kzg = KZG([5 + 2 * i for i in range(nvars)], ctx)
    tables = [ctx.synth(FIELD, n, SEED, t) for t in range(16)]
    point, evals = degree1_evals(ctx, tables, nvars)
    rho = as_limbs([0x1234567890ABCDEF1234567890ABCDEF])
    out = np.zeros((nvars, 12), np.uint64)

    def single(i):
        check(lib().zk_dev_kzg_get_proof(ctx.h, kzg.h, 0, tables[i].ptr, ptr(evals[i:i + 1]), ptr(point), ptr(out)))

    def batch(k):
        arr = pointers(tables[:k])
        return lambda: check(lib().zk_dev_kzg_batch_open(ctx.h, kzg.h, 0, arr, k, ptr(rho), ptr(evals), ptr(point),
                                                         ptr(out)))

    def singles(k):
        def go():
            for i in range(k):
                single(i)
        return go

    names = ["single", "batch4", "batch16", "singles4", "singles16"]
    calls = [lambda: single(0), batch(4), batch(16), singles(4), singles(16)]
    for fn in calls * 2:
        fn()
    # the benchmarked batch is a valid opening: 16 commitments, one proof
    cms = np.zeros((16, 12), np.uint64)
    check(lib().zk_dev_kzg_commit_batch(ctx.h, kzg.h, pointers(tables), 16, ptr(cms)))
    calls[2]()
    g2 = np.zeros((nvars, 24), np.uint64)
    check(lib().zk_kzg_g2_taus(kzg.h, ptr(g2)))
    ok = C.c_int(0)
    check(lib().zk_kzg_batch_verify(0, ptr(cms), 16, ptr(rho), ptr(evals), ptr(out), nvars, ptr(point), nvars, ptr(g2),
                                    C.byref(ok)))
    if not ok.value:
        raise RuntimeError("the benchmarked batched opening does not verify")
    ts = timed_round(calls, min_seconds)
    res = {"tool": "committed_bench", "case": f"batch_open_2^{nvars}", "nvars": nvars, "verified": True}
    for name, t in zip(names, ts):
        res.update(summary(name, t))
    res["batch4_over_single"] = res["batch4_ms"] / res["single_ms"]
    res["batch16_over_single"] = res["batch16_ms"] / res["single_ms"]
    res["batch16_over_singles16"] = res["batch16_ms"] / res["singles16_ms"]
    res["condition_batch16_le_1.25_single"] = bool(res["batch16_over_single"] <= 1.25)
    # the extra pass by itself, event-timed inside one batched opening
    ctx.set_timing_kinds(["fold"])
    ctx.reset_stats()
    calls[2]()
    folds = [x for x in ctx.launches() if x["kind"] == "fold"]
    ctx.set_timing(False)
    res["batch16_lincomb_kernel_ms"] = folds[0]["ms"]  # (the first launch of the kind: cur = g - v)
    res["batch16_lincomb_alg_bytes"] = folds[0]["alg_bytes"]
    for t in tables:
        t.free()
    kzg.close()
    return res


def bench_zero_check(ctx, nvars: int, min_seconds: float) -> dict:
    import zk_amd
    from zk_amd._lib import check, lib
    from zk_amd.api import modulus
    from zk_amd.elems import as_limbs, ptr
    from zk_amd.kzg import KZG

    n, p = 1 << nvars, modulus(FIELD)
    kzg = KZG([5 + 2 * i for i in range(nvars)], ctx)
    a, b = ctx.synth(FIELD, n, SEED, 0), ctx.synth(FIELD, n, SEED, 1)
    c = ctx.upload(FIELD, [x * y % p for x, y in zip(a.to_ints(), b.to_ints())])
    eq = zk_amd.DeviceTable.eq(ctx, FIELD, [11 + 3 * i for i in range(nvars)])
    neq = zk_amd.DeviceTable.lincomb([eq], [p - 1])
    one = zk_amd.DeviceTable.lincomb([eq], [0], 1)
    tables = [eq, a, b, neq, c, one]
    factors, mask, committed = [[0, 1, 2], [3, 4, 5]], 0b010110, [a, b, c]
    fac = np.array(factors, np.uint8).reshape(-1)
    coeffs, nco = np.zeros((nvars, 4, 4), np.uint64), np.zeros(nvars, np.uint8)
    ch, ev, cs = np.zeros((nvars, 4), np.uint64), np.zeros((6, 4), np.uint64), np.zeros((1, 4), np.uint64)
    cms, op = np.zeros((3, 12), np.uint64), np.zeros((nvars, 12), np.uint64)
    zero, rho = as_limbs([0]), as_limbs([0xFEDCBA9876543210])
    arr, carr = pointers(tables), pointers(committed)

    def whole():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_committed_sumcheck_prove(ctx.h, kzg.h, 0, arr, 6, nvars, ptr(fac), 2, 3, mask, None, ptr(zero),
                                                    t.h, ptr(coeffs), ptr(nco), ptr(ch), ptr(ev), ptr(cs), ptr(cms),
                                                    ptr(op)))

    scratch_cm, scratch_op = np.zeros((3, 12), np.uint64), np.zeros((nvars, 12), np.uint64)
    s_coeffs, s_nco = np.zeros((nvars, 4, 4), np.uint64), np.zeros(nvars, np.uint8)
    s_ch, s_ev = np.zeros((nvars, 4), np.uint64), np.zeros((6, 4), np.uint64)

    def commit():
        check(lib().zk_dev_kzg_commit_batch(ctx.h, kzg.h, carr, 3, ptr(scratch_cm)))

    def sumcheck():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, arr, 6, nvars, ptr(fac), 2, 3, ptr(zero), t.h,
                                                   ptr(s_coeffs), ptr(s_nco), ptr(s_ch), ptr(s_ev), ptr(cs)))

    def opening():
        check(lib().zk_dev_kzg_batch_open(ctx.h, kzg.h, 0, carr, 3, ptr(rho), ptr(s_ev[[1, 2, 4]].copy()), ptr(s_ch),
                                          ptr(scratch_op)))

    calls = [whole, commit, sumcheck, opening]
    for fn in calls * 2:
        fn()
    whole()
    g2 = np.zeros((nvars, 24), np.uint64)
    check(lib().zk_kzg_g2_taus(kzg.h, ptr(g2)))
    ok = C.c_int(0)
    vch = np.zeros((nvars, 4), np.uint64)
    vt = zk_amd.Transcript(FIELD)
    check(lib().zk_committed_sumcheck_verify(0, 3, ptr(coeffs), ptr(nco), nvars, ptr(zero), ptr(fac), 2, 6, ptr(ev), mask,
                                             ptr(cms), ptr(op), ptr(g2), vt.h, C.byref(ok), ptr(vch)))
    if not ok.value or not np.array_equal(vch, ch):
        raise RuntimeError("the benchmarked proof does not verify")
    ts = timed_round(calls, min_seconds)
    res = {"tool": "committed_bench", "case": f"zero_check_2^{nvars}", "nvars": nvars, "ntables": 6, "committed": 3,
           "verified": True}
    for name, t in zip(["whole", "commit", "sumcheck", "open"], ts):
        res.update(summary(name, t))
    res["parts_over_whole"] = (res["commit_ms"] + res["sumcheck_ms"] + res["open_ms"]) / res["whole_ms"]
    for t in tables:
        t.free()
    kzg.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--lincomb", type=int, nargs="*", default=[20, 24], help="log2 sizes of the k_lincomb cases")
    ap.add_argument("--nvars", type=int, default=20, help="size of the opening and whole-proof cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "committed_bench.json"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    res = []
    for lg in a.lincomb:
        res += bench_lincomb(ctx, lg, a.min_seconds)
    res.append(bench_batch_open(ctx, a.nvars, a.min_seconds))
    res.append(bench_zero_check(ctx, a.nvars, a.min_seconds))
    lines = [json.dumps(r) for r in res]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

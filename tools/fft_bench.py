"""NTT on one GPU: forward and inverse transforms of a device-resident table and
the polynomial product built on them, beside the one-core Python oracle.

usage: python tools/fft_bench.py [--sizes 0:20,0:24,2:20,2:24] [--mul 0:23] [--min-seconds 1.5]
                                 [--out profiles/fft_bench.json]

Per (field, log2 n) one JSON line:
  forward_ms / inverse_ms  zk_dev_fft over a synthesised DeviceTable of 2^k
                  elements into a second table (the passes of csrc/fft_plan.hpp and
                  one synchronise); median of the timed repeats, host clock around
                  the synchronous call
  inplace_ms      the forward transform with the table as its own output
  butterflies_per_s   k 2^(k-1) / forward time
  model_mul_ms    the multiplications of the plan (butterflies that multiply, two
                  per element for an inter-pass twiddle) at 120 G modmul/s
  model_hbm_ms    the passes' traffic (64 B per element and pass) at 4.75 TB/s
  oracle_ms       tests/fft_oracle.py fft_evaluate on one core of this host,
                  measured at 2^16 and extrapolated with n log n
  round_trip_ok   (largest size of the run) inverse(forward(x)) == x, every limb
Per --mul item (field, log2 terms) one line: zk_poly_mul of two polynomials of
2^k terms from host memory (upload, two forward transforms of 2^(k+1) points, the
pointwise product, one inverse, download), and the device part alone.
Warm-up calls come first; each figure is timed over at least --min-seconds in total.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zk-research-implementations_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 11
PLAN_HPP = os.path.join(ROOT, "zk-research-implementations_amd", "csrc", "fft_plan.hpp")
with open(PLAN_HPP) as _fh:  # the build's own constant, not a copy of it
    TILE_LOG = int(re.search(r"constexpr uint32_t kFftTileLog = (\d+);", _fh.read()).group(1))
FIELD_NAMES = {0: "bn254_fr", 1: "bn254_fq", 2: "bls12_381_fr"}
MODMUL_PER_S, HBM_BYTES_PER_S = 120e9, 4.75e12  # profiles/r1_arith_rates.txt, the measured copy rate


def timed(fn, min_seconds: float, min_reps: int = 5) -> list[float]:
    ts, total = [], 0.0
    while total < min_seconds or len(ts) < min_reps:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        ts.append(dt)
        total += dt
    return ts


def stage_cap() -> int:
    """fft_stage_cap of csrc/fft_plan.hpp: ZK_FFT_STAGES in 1 .. kFftTileLog, else kFftTileLog."""
    try:
        knob = int(os.environ.get("ZK_FFT_STAGES", "0"), 0)
    except ValueError:
        knob = 0
    return knob if 1 <= knob <= TILE_LOG else TILE_LOG


def plan_widths(k: int, stages: int | None = None) -> list[int]:
    """The pass widths fft_plan gives 2^k (tests/test_fft_cpu.py holds the two together)."""
    stages = stage_cap() if stages is None else stages
    if k == 0:
        return []
    passes = -(-k // stages)
    base, rem = divmod(k, passes)
    return [base + (1 if i < rem else 0) for i in range(passes)]


def model(k: int) -> dict:
    n = 1 << k
    widths = plan_widths(k)
    muls = sum((a - 1) * n // 2 for a in widths) + 2 * n * (len(widths) - 1)
    return {"passes": widths, "field_muls": muls, "model_mul_ms": muls / MODMUL_PER_S * 1e3,
            "model_hbm_ms": 64.0 * n * len(widths) / HBM_BYTES_PER_S * 1e3}


def oracle_seconds_per_nlogn(field: int) -> float:
    import coracle as co
    import fft_oracle as fo

    k = 16
    x = co.from_limbs(co.synth(field, SEED, 0, 0, 1 << k))
    t0 = time.perf_counter()
    fo.fft_evaluate(field, x)
    return (time.perf_counter() - t0) / (k << k)


def bench(ctx, field: int, k: int, min_seconds: float, check_round_trip: bool) -> dict:
    from zk_amd.fft import dev_fft

    n = 1 << k
    x = ctx.synth(field, n, seed=SEED, table=0)
    y = ctx.alloc(field, n)
    z = ctx.alloc(field, n)
    for _ in range(2):  # warm-up: code objects, the occupancy query, the twiddle tables, the scratch
        dev_fft(x, out=y)
        dev_fft(y, inverse=True, out=z)
    tf = timed(lambda: dev_fft(x, out=y), min_seconds)
    ti = timed(lambda: dev_fft(y, inverse=True, out=z), min_seconds)
    res = {"tool": "fft_bench", "field": FIELD_NAMES[field], "log_n": k,
           "forward_ms": statistics.median(tf) * 1e3, "forward_ms_min": min(tf) * 1e3, "forward_reps": len(tf),
           "inverse_ms": statistics.median(ti) * 1e3, "inverse_ms_min": min(ti) * 1e3, "inverse_reps": len(ti)}
    if check_round_trip:
        ok = bool(np.array_equal(z.download(1), x.download(1)))
        res["round_trip_ok"] = ok
        if not ok:
            raise RuntimeError("inverse(forward(x)) differs from x")
    dev_fft(z, out=z)
    tp = timed(lambda: dev_fft(z, out=z), min_seconds / 2)
    res["inplace_ms"] = statistics.median(tp) * 1e3
    res["butterflies_per_s"] = k * (n // 2) / statistics.median(tf)
    res.update(model(k))
    res["fraction_of_mul_model"] = res["model_mul_ms"] / res["forward_ms"]
    for t in (x, y, z):
        t.free()
    return res


def bench_mul(ctx, field: int, k: int, min_seconds: float) -> dict:
    from zk_amd._lib import check, lib
    from zk_amd.elems import ptr
    from zk_amd.fft import dev_fft

    n = 1 << k
    ta, tb = ctx.synth(field, n, seed=SEED, table=1), ctx.synth(field, n, seed=SEED, table=2)
    a, b = ta.download(1), tb.download(1)  # Montgomery images: no conversion on the way in or out
    ta.free()
    tb.free()
    out = np.zeros((2 * n - 1, 4), np.uint64)
    got = C.c_uint64(0)

    def mul():
        check(lib().zk_poly_mul(ctx.h, field, 1, ptr(a), n, ptr(b), n, ptr(out), 2 * n - 1, C.byref(got)))

    mul()
    tm = timed(mul, min_seconds, 3)
    t = ctx.synth(field, 2 * n, seed=SEED, table=3)

    def device_part():  # the three transforms of the product (the pointwise pass is one more read and write)
        dev_fft(t, out=t)
        dev_fft(t, out=t)
        dev_fft(t, inverse=True, out=t)

    device_part()
    td = timed(device_part, min_seconds / 2, 3)
    t.free()
    return {"tool": "fft_bench", "op": "poly_mul", "field": FIELD_NAMES[field], "log_terms": k, "out_len": int(got.value),
            "poly_mul_ms": statistics.median(tm) * 1e3, "poly_mul_reps": len(tm),
            "three_transforms_ms": statistics.median(td) * 1e3, "host_bytes_moved": 32 * (4 * n - 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0:20,0:24,2:20,2:24", help="field:log2(n), comma separated")
    ap.add_argument("--mul", default="0:23", help="field:log2(terms) of the product's operands, comma separated ('' for none)")
    ap.add_argument("--min-seconds", type=float, default=1.5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    sizes = [tuple(int(v) for v in item.split(":")) for item in a.sizes.split(",") if item]
    largest = max(k for _, k in sizes) if sizes else 0
    per = {}
    lines = []
    for f, k in sizes:
        r = bench(ctx, f, k, a.min_seconds, k == largest)
        if f not in per:
            per[f] = oracle_seconds_per_nlogn(f)
        r["oracle_ms"] = per[f] * (k << k) * 1e3
        r["oracle_measured_at_log_n"] = 16
        r["speedup_vs_oracle"] = r["oracle_ms"] / r["forward_ms"]
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    for item in a.mul.split(","):
        if not item:
            continue
        f, k = (int(v) for v in item.split(":"))
        lines.append(json.dumps(bench_mul(ctx, f, k, a.min_seconds)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

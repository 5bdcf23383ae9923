"""Interpolation and batch evaluation over arbitrary points on one GPU, beside the
multiply model and the one-core Python oracle.

usage: python tools/poly_bench.py [--interp 1:10,1:12,1:14,1:16,0:10,0:12,0:14,0:16]
                                  [--eval 1:20:10,1:10:20,1:24:2] [--crossover 1] [--min-seconds 1.5]
                                  [--out profiles/poly_bench.json]

Per --interp item (field, log2 n) one JSON line:
  interpolate_ms  zk_poly_interpolate of n synthesised points from host memory in
                  the Montgomery representation (two uploads with their range
                  check, the weights, the leaves with one inversion each, the
                  tree's levels, the download; it synchronises): median of the
                  timed repeats, host clock around the synchronous call
  model_ms        2.5 n^2 + n (products of one inversion) field products at
                  120 G modmul/s (profiles/r1_arith_rates.txt: 116-128)
  oracle_ms       tests/poly_oracle.py interpolate, the reference's own O(n^3)
                  loop, on one core of this host: measured at n = 24, extrapolated
                  by n^3
  definition_ok   (the largest n of the run) the result takes y_i at 64 of the x_i
Per --eval item (field, log2 m, log2 d) one line:
  evaluate_ms     zk_dev_poly_evaluate over synthesised DeviceTables
  model_ms        m d products at 120 G/s;   hbm_ms  the 32 (2 m + d) bytes at 4.75 TB/s
  oracle_ms       poly_oracle.evaluate (a pow per term) measured at 16 points of 1024
                  coefficients, extrapolated by m d log2 d
--crossover FIELD: for n = 2 .. 256 the same interpolation on a context that runs
everything on the host (ZK_POLY_HOST_MAX=65536) and on one that runs everything on
the device (0), alternating; likewise one evaluation shape per n (n points, n coefficients).
Warm-up calls come first; each figure is timed over at least --min-seconds in total.
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
for p in (os.path.join(ROOT, "zk-research-implementations_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 23
FIELD_NAMES = {0: "bn254_fr", 1: "bn254_fq", 2: "bls12_381_fr"}
MODMUL_PER_S, HBM_BYTES_PER_S = 120e9, 4.75e12  # profiles/r1_arith_rates.txt, the measured copy rate
MONT = 1


def timed(fn, min_seconds: float, min_reps: int = 5) -> list[float]:
    ts, total = [], 0.0
    while total < min_seconds or len(ts) < min_reps:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        ts.append(dt)
        total += dt
    return ts


def inversion_products(field: int) -> int:
    """fe_inv of csrc/field.hpp: a squaring per bit of a 256-bit exponent word
    walk and a product per set bit of p - 2."""
    import pyoracle as po

    return 256 + bin(po.MODULI[field] - 2).count("1")


def ctx_under(**env):
    import zk_amd

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


def mont_points(ctx, field: int, n: int):
    """n points as Montgomery images in host memory (x: table 0, y: table 1 of the seed)."""
    tx, ty = ctx.synth(field, n, SEED, 0), ctx.synth(field, n, SEED, 1)
    xs, ys = tx.download(MONT), ty.download(MONT)
    tx.free()
    ty.free()
    return xs, ys


def interpolate_call(ctx, field: int, xs, ys):
    from zk_amd._lib import check, lib
    from zk_amd.elems import ptr

    n = xs.shape[0]
    out = np.zeros((n, 4), np.uint64)
    got = C.c_uint64(0)

    def call():
        check(lib().zk_poly_interpolate(ctx.h, field, MONT, ptr(xs), ptr(ys), n, ptr(out), n, C.byref(got)))

    return call, out, got


def oracle_interp_seconds_per_n3(field: int) -> float:
    import coracle as co
    import poly_oracle as O
    import pyoracle as po

    n = 24
    pts = list(zip(co.from_limbs(co.synth(field, SEED, 0, 0, n)), co.from_limbs(co.synth(field, SEED, 1, 0, n))))
    t0 = time.perf_counter()
    O.interpolate(po.MODULI[field], pts)
    return (time.perf_counter() - t0) / n ** 3


def oracle_eval_seconds_per_term_bit(field: int) -> float:
    import coracle as co
    import poly_oracle as O
    import pyoracle as po

    d, m = 1024, 16
    cf, xs = co.from_limbs(co.synth(field, SEED, 2, 0, d)), co.from_limbs(co.synth(field, SEED, 3, 0, m))
    t0 = time.perf_counter()
    for x in xs:
        O.evaluate(po.MODULI[field], cf, x)
    return (time.perf_counter() - t0) / (m * d * 10)


def bench_interp(ctx, field: int, k: int, min_seconds: float, check: bool) -> dict:
    import pyoracle as po

    n = 1 << k
    xs, ys = mont_points(ctx, field, n)
    call, out, got = interpolate_call(ctx, field, xs, ys)
    call()
    call()  # warm-up: code objects, the occupancy queries, the scratch tables
    ts = timed(call, min_seconds, 3)
    muls = 2.5 * n * n + n * inversion_products(field)
    res = {"tool": "poly_bench", "op": "interpolate", "field": FIELD_NAMES[field], "log_n": k, "ncoeffs": int(got.value),
           "interpolate_ms": statistics.median(ts) * 1e3, "interpolate_ms_min": min(ts) * 1e3, "reps": len(ts),
           "field_muls_model": muls, "model_ms": muls / MODMUL_PER_S * 1e3}
    res["fraction_of_mul_model"] = res["model_ms"] / res["interpolate_ms"]
    if check:
        from zk_amd.elems import to_ints

        p = po.MODULI[field]
        rinv = pow(1 << 256, -1, p)
        cf = [v * rinv % p for v in to_ints(out[: got.value])]
        ok = True
        for i in range(0, n, max(1, n // 64)):
            x, y = (v * rinv % p for v in to_ints(np.stack([xs[i], ys[i]])))
            acc = 0
            for c in reversed(cf):
                acc = (acc * x + c) % p
            ok = ok and acc == y
        res["definition_ok"] = ok
        if not ok:
            raise RuntimeError("the interpolant misses a point")
    return res


def bench_eval(ctx, field: int, log_m: int, d: int, min_seconds: float) -> dict:
    from zk_amd.poly import dev_evaluate, eval_plan

    m = 1 << log_m
    cf, xs, out = ctx.synth(field, d, SEED, 2), ctx.synth(field, m, SEED, 3), ctx.alloc(field, m)
    for _ in range(2):
        dev_evaluate(cf, xs, out=out)
    ts = timed(lambda: dev_evaluate(cf, xs, out=out), min_seconds, 3)
    chunks, length = eval_plan(d, m, ctx)
    res = {"tool": "poly_bench", "op": "evaluate", "field": FIELD_NAMES[field], "npoints": m, "ncoeffs": d,
           "chunks": chunks, "chunk_len": length,
           "evaluate_ms": statistics.median(ts) * 1e3, "evaluate_ms_min": min(ts) * 1e3, "reps": len(ts),
           "field_muls_model": float(m) * d, "model_ms": float(m) * d / MODMUL_PER_S * 1e3,
           "hbm_ms": 32.0 * (2 * m + d) / HBM_BYTES_PER_S * 1e3}
    res["fraction_of_mul_model"] = res["model_ms"] / res["evaluate_ms"]
    for t in (cf, xs, out):
        t.free()
    return res


def crossover(field: int, min_seconds: float) -> list[dict]:
    from zk_amd._lib import check, lib
    from zk_amd.elems import ptr

    host, dev = ctx_under(ZK_POLY_HOST_MAX=65536), ctx_under(ZK_POLY_HOST_MAX=0)
    lines = []
    for n in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256):
        xs, ys = mont_points(dev, field, n)
        row = {"tool": "poly_bench", "op": "crossover", "field": FIELD_NAMES[field], "n": n}
        calls = {}
        for name, c in (("host", host), ("device", dev)):
            calls[name + "_interpolate"] = interpolate_call(c, field, xs, ys)[0]
            out = np.zeros((n, 4), np.uint64)
            calls[name + "_evaluate"] = (lambda c=c, out=out: check(lib().zk_poly_evaluate(
                c.h, field, MONT, ptr(ys), n, ptr(xs), n, ptr(out))))
        for fn in calls.values():
            fn()
        for leg in (1, 2):  # alternating
            for name, fn in calls.items():
                ts = timed(fn, min_seconds / 8, 5)
                row["%s_us_leg%d" % (name, leg)] = statistics.median(ts) * 1e6
        lines.append(row)
    host.close()
    dev.close()
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--interp", default="1:10,1:12,1:14,1:16,0:10,0:12,0:14,0:16", help="field:log2(n), comma separated")
    ap.add_argument("--eval", default="1:20:10,1:10:20,1:24:2", help="field:log2(points):log2(coefficients), comma separated")
    ap.add_argument("--crossover", default="", help="field: the host path against the device path for n = 2 .. 256")
    ap.add_argument("--min-seconds", type=float, default=1.5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()

    lines = []

    def emit(r: dict) -> None:
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    import zk_amd

    ctx = zk_amd.default_context()
    interp = [tuple(int(v) for v in item.split(":")) for item in a.interp.split(",") if item]
    largest = max((k for _, k in interp), default=0)
    per = {}
    for f, k in interp:
        r = bench_interp(ctx, f, k, a.min_seconds, k == largest)
        if f not in per:
            per[f] = oracle_interp_seconds_per_n3(f)
        r["oracle_ms"] = per[f] * float(1 << k) ** 3 * 1e3
        r["oracle_measured_at_n"] = 24
        r["oracle_extrapolated"] = True
        r["speedup_vs_oracle"] = r["oracle_ms"] / r["interpolate_ms"]
        emit(r)
    per = {}
    for item in a.eval.split(","):
        if not item:
            continue
        f, lm, ld = (int(v) for v in item.split(":"))
        d = 1 << ld
        r = bench_eval(ctx, f, lm, d, a.min_seconds)
        if f not in per:
            per[f] = oracle_eval_seconds_per_term_bit(f)
        r["oracle_ms"] = per[f] * float(1 << lm) * d * max(ld, 1) * 1e3
        r["oracle_measured_at"] = [16, 1024]
        r["oracle_extrapolated"] = True
        r["speedup_vs_oracle"] = r["oracle_ms"] / r["evaluate_ms"]
        emit(r)
    if a.crossover != "":
        for r in crossover(int(a.crossover), a.min_seconds):
            emit(r)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The lookup argument on one GPU: the batched inversion beside
one Fermat power per element, the rate of the probe kernel, and one whole proof
split into its parts.

usage: python tools/lookup_bench.py [--min-seconds 1.0] [--inverse 12 16 20 24] [--probe 20 24]
                                    [--nvars 20] [--table-log 16] [--out FILE]
(the JSON lines also go to --out, by default profiles/lookup_bench.json)

One JSON line per case, all over BLS12-381 Fr:
  inverse_2^n    zk_dev_fe_batch_inverse (out of place) alternating with the
                 baseline, a tool-local kernel with one fe_inv per element, one
                 lane each (tools/lookup_baseline.hip, built into
                 tools/mb_lookup_baseline.so on first use). batch_kernel_ms: the
                 median event-timed duration of the k_batch_inverse launch;
                 baseline_kernel_ms: the median of the baseline launch's own
                 events; baseline_over_batch their ratio. The two results are
                 compared (asserted equal).
  probe_2^n_*    zk_dev_lookup_multiplicities of 2^n entries against a table of
                 2^table_log distinct values: `uniform` draws the entries
                 uniformly from the table, `repeated` is one value throughout
                 (every add lands on one counter). probe_kernel_ms: the median
                 event-timed duration of the k_lookup_probe launch;
                 entries_per_s from it.
  proof_2^n      one whole zk_dev_lookup_prove of a uniform column (whole),
                 verified by a host-only handle (asserted), and, alternating
                 with it, its parts through the public calls: the four
                 commitments as the prover makes them, two and two (commit), the
                 multiplicities (count), the helper columns' two linear
                 combinations and two batched inversions (helpers; the padding
                 and the product by m, two plain streams, are not public and
                 not in it: the tool makes the true h_t once, on the host, for
                 the commitment, the sum-check and the opening), the six public
                 tables (public), the composed sum-check over eleven tables
                 (sumcheck) and the batched opening of four (open).
                 parts_over_whole = their sum / whole.
Each *_ms is a median after two warm-up rounds, timed over at least
--min-seconds in total and at least five rounds; *_ms_min the fastest call.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zk-research-implementations_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 31
FIELD = 2
BASELINE_SRC = os.path.join(ROOT, "tools", "lookup_baseline.hip")
BASELINE_LIB = os.path.join(ROOT, "tools", "mb_lookup_baseline.so")


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


def baseline_lib():
    if not os.path.exists(BASELINE_LIB) or os.path.getmtime(BASELINE_LIB) < os.path.getmtime(BASELINE_SRC):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC",
                        "--offload-arch=gfx950", "-shared", "-I" + os.path.join(ROOT, "zk-research-implementations_amd", "csrc"),
                        "-o", BASELINE_LIB, BASELINE_SRC], check=True)
    L = C.CDLL(BASELINE_LIB)
    L.lookup_baseline_inverse_ms.restype = C.c_float
    L.lookup_baseline_inverse_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    return L


def layer_ms(ctx) -> list[float]:
    return [x["ms"] for x in ctx.launches() if x["kind"] == "layer"]


def bench_inverse(ctx, lg: int, min_seconds: float) -> dict:
    from zk_amd._lib import check, lib

    B = baseline_lib()
    n = 1 << lg
    src = ctx.synth(FIELD, n, SEED, 0)
    out, ref = ctx.alloc(FIELD, n), ctx.alloc(FIELD, n)
    batch_ms, base_ms = [], []

    def batch():
        ctx.reset_stats()
        check(lib().zk_dev_fe_batch_inverse(ctx.h, FIELD, src.ptr, n, out.ptr))
        batch_ms.extend(layer_ms(ctx))

    def baseline():
        ms = B.lookup_baseline_inverse_ms(src.ptr, ref.ptr, n)
        if ms < 0:
            raise RuntimeError("the baseline kernel failed")
        base_ms.append(ms)

    ctx.set_timing_kinds(["layer"])
    for fn in (batch, baseline) * 2:
        fn()
    if not np.array_equal(out.download(1), ref.download(1)):
        raise RuntimeError("the batched inversion and the baseline differ")
    batch_ms.clear()
    base_ms.clear()
    ts = timed_round([batch, baseline], min_seconds)
    ctx.set_timing(False)
    bk, sk = statistics.median(batch_ms), statistics.median(base_ms)
    res = {"tool": "lookup_bench", "case": f"inverse_2^{lg}", "log2_entries": lg, "equal": True,
           **summary("batch_call", ts[0]), **summary("baseline_call", ts[1]), "batch_kernel_ms": bk,
           "batch_kernel_ms_min": min(batch_ms), "baseline_kernel_ms": sk, "baseline_kernel_ms_min": min(base_ms),
           "kernel_launches_timed": len(batch_ms), "baseline_over_batch": sk / bk,
           "batch_elements_per_s": n / (bk * 1e-3), "batch_faster": bool(bk < sk)}
    for t in (src, out, ref):
        t.free()
    return res


def upload_limbs(ctx, limbs: np.ndarray):
    from zk_amd._lib import check, lib

    limbs = np.ascontiguousarray(limbs, np.uint64)
    t = ctx.alloc(FIELD, limbs.shape[0])
    check(lib().zk_dev_upload(ctx.h, FIELD, 0, limbs.ctypes.data_as(C.c_void_p), limbs.shape[0], t.ptr))
    return t


def table_and_lookup(ctx, table_log: int):
    """2^table_log distinct pseudo-random values -> (their limbs, the handle)"""
    from zk_amd import Lookup

    src = ctx.synth(FIELD, 1 << table_log, SEED, 3)
    limbs = src.download()
    src.free()
    table = [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in limbs]
    if len(set(table)) != len(table):
        raise RuntimeError("the synthetic table has duplicates")
    return limbs, Lookup(table, ctx)


def bench_probe(ctx, lg: int, table_log: int, min_seconds: float) -> list[dict]:
    from zk_amd._lib import check, lib

    n = 1 << lg
    limbs, lk = table_and_lookup(ctx, table_log)
    rng = np.random.default_rng(SEED)
    cols = {"uniform": upload_limbs(ctx, limbs[rng.integers(0, len(limbs), n)]),
            "repeated": upload_limbs(ctx, limbs[np.full(n, 12345 % len(limbs))])}
    m = ctx.alloc(FIELD, n)
    kernel_ms = {k: [] for k in cols}
    missing = C.c_uint64(0)

    def call(name):
        def go():
            ctx.reset_stats()
            check(lib().zk_dev_lookup_multiplicities(lk.h, cols[name].ptr, n, m.ptr, lg, C.byref(missing)))
            if missing.value:
                raise RuntimeError("a member was not found")
            kernel_ms[name].append(layer_ms(ctx)[0])  # (the first launch of the kind: the probe)
        return go

    ctx.set_timing_kinds(["layer"])
    calls = [call(k) for k in cols]
    for fn in calls * 2:
        fn()
    for v in kernel_ms.values():
        v.clear()
    ts = timed_round(calls, min_seconds)
    ctx.set_timing(False)
    res = []
    for name, t in zip(cols, ts):
        km = statistics.median(kernel_ms[name])
        res.append({"tool": "lookup_bench", "case": f"probe_2^{lg}_{name}", "log2_entries": lg, "log2_table": table_log,
                    **summary("call", t), "probe_kernel_ms": km, "probe_kernel_ms_min": min(kernel_ms[name]),
                    "kernel_launches_timed": len(kernel_ms[name]), "entries_per_s": n / (km * 1e-3)})
    for t in list(cols.values()) + [m]:
        t.free()
    lk.close()
    return res


def bench_proof(ctx, nvars: int, table_log: int, min_seconds: float) -> dict:
    import zk_amd
    from zk_amd import DeviceTable, Lookup
    from zk_amd._lib import check, lib
    from zk_amd.api import modulus
    from zk_amd.elems import as_limbs, ptr
    from zk_amd.kzg import KZG

    n, p = 1 << nvars, modulus(FIELD)
    kzg = KZG([5 + 2 * i for i in range(nvars)], ctx)
    limbs, lk = table_and_lookup(ctx, table_log)
    rng = np.random.default_rng(SEED + 1)
    f = upload_limbs(ctx, limbs[rng.integers(0, len(limbs), n)])
    t_pad = upload_limbs(ctx, limbs[np.minimum(np.arange(n), len(limbs) - 1)])

    proof = {}

    def whole():
        proof["p"] = lk.prove(f, zk_amd.Transcript(FIELD), kzg)

    # the parts, on tables of the same shapes (their values do not matter to the time)
    alpha, minus1 = as_limbs([0x123456789ABCDEF0FEDCBA9876543210]), as_limbs([p - 1])
    m, tmp, hf, ht = (ctx.alloc(FIELD, n) for _ in range(4))
    missing = C.c_uint64(0)
    cms = np.zeros((4, 12), np.uint64)

    ht_true = {}  # h_t itself, m / (alpha - t_pad): zero wherever m is, which an MSM is quick to skip

    def commit():
        check(lib().zk_dev_kzg_commit_batch(ctx.h, kzg.h, pointers([f, m]), 2, ptr(cms)))
        check(lib().zk_dev_kzg_commit_batch(ctx.h, kzg.h, pointers([hf, ht_true["t"]]), 2, ptr(cms[2:])))

    def count():
        check(lib().zk_dev_lookup_multiplicities(lk.h, f.ptr, n, m.ptr, nvars, C.byref(missing)))

    def helpers():
        for src, dst in ((f, hf), (t_pad, ht)):
            check(lib().zk_dev_mle_lincomb(ctx.h, FIELD, 0, pointers([src]), 1, ptr(minus1), ptr(alpha), n, tmp.ptr))
            check(lib().zk_dev_fe_batch_inverse(ctx.h, FIELD, tmp.ptr, n, dst.ptr))

    pub = {}

    def public():
        for t in pub.values():
            t.free()
        eq = DeviceTable.eq(ctx, FIELD, [11 + 3 * i for i in range(nvars)])
        pub.update({f"e{i}": DeviceTable.lincomb([eq], [3 + i]) for i in range(4)})
        eq.free()
        pub["one"] = DeviceTable.lincomb([f], [0], 1)
        pub["neg"] = DeviceTable.lincomb([f], [0], p - 1)

    fac = np.array([0, 5, 5, 1, 6, 5, 7, 0, 5, 8, 0, 2, 8, 5, 5, 9, 1, 5, 10, 1, 4, 10, 3, 5], np.uint8)
    coeffs, nco = np.zeros((nvars, 4, 4), np.uint64), np.zeros(nvars, np.uint8)
    ch, ev, cs = np.zeros((nvars, 4), np.uint64), np.zeros((11, 4), np.uint64), np.zeros((1, 4), np.uint64)
    zero, rho = as_limbs([0]), as_limbs([0xFEDCBA9876543210])
    op = np.zeros((nvars, 12), np.uint64)

    def tables():
        return [hf, ht_true["t"], f, m, t_pad, pub["one"], pub["neg"], pub["e0"], pub["e1"], pub["e2"], pub["e3"]]

    def sumcheck():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, pointers(tables()), 11, nvars, ptr(fac), 8, 3,
                                                   ptr(zero), t.h, ptr(coeffs), ptr(nco), ptr(ch), ptr(ev), ptr(cs)))

    def opening():
        check(lib().zk_dev_kzg_batch_open(ctx.h, kzg.h, 0, pointers([hf, ht_true["t"], f, m]), 4, ptr(rho), ptr(ev[:4].copy()),
                                          ptr(ch), ptr(op)))

    # the product by m is not public: made here once, on the host, over the table's T entries (m is zero past them)
    count()
    helpers()
    T = len(limbs)
    inv_t, m_t = ht.to_ints()[:T], m.to_ints()[:T]
    ht_limbs = np.zeros((n, 4), np.uint64)
    ht_limbs[:T] = as_limbs([a * b % p for a, b in zip(inv_t, m_t)])
    ht_true["t"] = upload_limbs(ctx, ht_limbs)

    names = ["whole", "commit", "count", "helpers", "public", "sumcheck", "open"]
    calls = [whole, commit, count, helpers, public, sumcheck, opening]
    for fn in calls * 2:
        fn()
    whole()
    host = Lookup([int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in limbs])
    if proof["p"].missing or not host.verify(proof["p"], zk_amd.Transcript(FIELD), kzg.g2_taus).verified:
        raise RuntimeError("the benchmarked proof does not verify")
    ts = timed_round(calls, min_seconds)
    res = {"tool": "lookup_bench", "case": f"proof_2^{nvars}", "nvars": nvars, "log2_table": table_log, "ntables": 11,
           "committed": 4, "verified": True}
    for name, t in zip(names, ts):
        res.update(summary(name, t))
    parts = sum(res[f"{k}_ms"] for k in names[1:])
    res["parts_over_whole"] = parts / res["whole_ms"]
    res["kzg_share_of_parts"] = (res["commit_ms"] + res["open_ms"]) / parts
    for t in [f, t_pad, m, tmp, hf, ht, ht_true["t"]] + list(pub.values()):
        t.free()
    host.close()
    lk.close()
    kzg.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--inverse", type=int, nargs="*", default=[12, 16, 20, 24], help="log2 sizes of the inversion cases")
    ap.add_argument("--probe", type=int, nargs="*", default=[20, 24], help="log2 sizes of the probe cases")
    ap.add_argument("--nvars", type=int, default=20, help="size of the whole-proof case (0: skip it)")
    ap.add_argument("--table-log", type=int, default=16, help="log2 of the table of the probe and proof cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    res = []
    for lg in a.inverse:
        res.append(bench_inverse(ctx, lg, a.min_seconds))
    for lg in a.probe:
        res += bench_probe(ctx, lg, a.table_log, a.min_seconds)
    if a.nvars:
        res.append(bench_proof(ctx, a.nvars, a.table_log, a.min_seconds))
    lines = [json.dumps(r) for r in res]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

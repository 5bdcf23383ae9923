"""The R1CS prover on one GPU: the rate of the gather kernel
beside the wired prover's phase-1 gather, what a split column costs, and one
whole committed proof split into its parts.

usage: python tools/r1cs_bench.py [--min-seconds 1.0] [--log-rows 20] [--out FILE]
(the JSON lines also go to --out, by default profiles/r1cs_bench.json)

One JSON line per case, all over BLS12-381 Fr. kernel times are the launches'
own events (timing on for the kind "layer"), a launch picked out of a call's
log by its alg_bytes, which the driver computes from the entry and chunk counts;
*_ms are host-clock medians of the synchronous calls. Calls alternate (a, b, a,
b, ...) after two warm-up rounds, for at least --min-seconds in all and at
least five rounds.
  gather_rows_2^n   k_r1cs_gather by rows (zk_dev_r1cs_mul) on a uniform instance
                    of 2^n rows, 3 entries per row per matrix (9 2^n entries, random
                    columns of 2^(n+1)), alternating with a wired GKR proof of
                    one layer of 9 2^n gates whose left inputs have fan-out 9 (2^n
                    rows of 9 gates for k_wired_phase1, random right inputs).
                    ns_per_entry = kernel time / entries for each;
                    r1cs_over_phase1 their ratio (the issue expects <= 1).
  gather_chain_2^n  the squaring chain of 2^n constraints: every constraint reads
                    the constant-1 column, so in the column pass one column holds
                    2^n entries (2^(n-8) chunks and slots). The row pass and the
                    column pass (zk_r1cs_matrix_evals: three sums kept apart) of
                    the same instance, alternating: gather and combine kernels.
  proof_chain_2^n   one committed proof of that chain (zk_dev_r1cs_prove, whole)
                    and, alternating with it, its parts through the public
                    calls: the commitment (zk_dev_kzg_commit), the row pass
                    (zk_dev_r1cs_mul), sum-check 1 over six tables of 2^n, the
                    column pass (zk_r1cs_matrix_evals, which also builds two eq
                    tables and takes three dot products: an upper bound of the
                    prover's), sum-check 2 over two tables of 2^(n+1), the opening
                    (zk_dev_kzg_get_proof). The proof is checked by
                    zk_r1cs_verify (asserted). rows_in_proof, cols_in_proof and
                    combine_in_proof are the prover's own gather and combine
                    launches (the column pass with a + rho b + rho^2 c written),
                    event-timed inside nine more whole proofs.
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

SEED = 31
FIELD = 2
CHUNK = 256  # kWiredChunk


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


def limbs(rng: np.random.Generator, n: int) -> np.ndarray:
    x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    x[:, 3] >>= np.uint64(11)  # below 2^252: canonical in every field
    return x


def nchunks_of(keys: np.ndarray) -> tuple[int, int, int]:
    """(chunks, slots, split rows) of the grouping of `keys` (wired_plan.hpp wired_csr)"""
    cnt = np.bincount(keys)
    cnt = cnt[cnt > 0]
    per = (cnt + CHUNK - 1) // CHUNK
    split = per[per > 1]
    return int(per.sum()), int(split.sum()), int(len(split))


def gather_bytes(n: int, nchunks: int, nc: int) -> float:
    return 68.0 * n + (12.0 + 32.0 * nc) * nchunks  # r1cs.hip gather_pass


def logged(ctx, sink: dict, picks: dict):
    """after a call: append the event time of the launch whose alg_bytes is picks[name]. The driver's
    launches carry no name, so a launch is known by its byte count (the formulas of r1cs.hip and
    wired.hip gather_pass, restated above and below): exactly one launch of the call must carry it,
    anything else — a formula that has changed, two launches of equal bytes — is an error, not a figure."""
    log = [x for x in ctx.launches() if x["kind"] == "layer"]
    for name, b in picks.items():
        hit = [x["ms"] for x in log if x["alg_bytes"] == b]
        if len(hit) != 1:
            raise RuntimeError(f"{name}: {len(hit)} launches of {b:.0f} bytes in the call's log of {len(log)}, expected 1")
        sink.setdefault(name, []).append(hit[0])


def kernel_summary(name: str, ms: list[float], entries: int) -> dict:
    med = statistics.median(ms)
    return {f"{name}_kernel_ms": med, f"{name}_kernel_ms_min": min(ms), f"{name}_kernel_ms_max": max(ms),
            f"{name}_launches_timed": len(ms), f"{name}_ns_per_entry": med * 1e6 / entries}


def chain_arrays(lg: int):
    """the squaring chain v_(i+1) = v_i^2 + 7 in 2^lg constraints as array triples, its witness and io"""
    from zk_amd.api import modulus
    from zk_amd.elems import as_limbs

    p = modulus(FIELD)
    nrows = 1 << lg
    n, H = nrows - 1, nrows
    v = [2]
    for _ in range(n):
        v.append((v[-1] * v[-1] + 7) % p)
    i = np.arange(n, dtype=np.uint32)
    one, minus_c = as_limbs([1]), as_limbs([p - 7])
    rep = lambda x, k: np.repeat(x, k, axis=0)  # noqa: E731
    A = (np.append(i, n).astype(np.uint32), np.append(i, n).astype(np.uint32), rep(one, n + 1))
    B = (np.append(i, n).astype(np.uint32), np.append(i, H).astype(np.uint32), rep(one, n + 1))
    C_ = (np.concatenate([i, i, [n]]).astype(np.uint32), np.concatenate([i + 1, np.full(n, H), [H + 1]]).astype(np.uint32),
          np.concatenate([rep(one, n), rep(minus_c, n), one]))
    return (A, B, C_), v, [v[-1]]


def bench_gather_rows(ctx, lg: int, min_seconds: float) -> dict:
    from zk_amd import R1CS
    from zk_amd._lib import check, lib
    from zk_amd.elems import ptr
    from zk_amd.gkr import WiredCircuit

    rng = np.random.default_rng(SEED)
    nrows, sy = 1 << lg, lg + 1
    per = 3 * nrows
    mats = [(np.repeat(np.arange(nrows, dtype=np.uint32), 3), rng.integers(0, 1 << sy, per, dtype=np.uint32),
             limbs(rng, per)) for _ in range(3)]
    r = R1CS(FIELD, nrows, sy, 0, *mats, ctx=ctx)
    n = 3 * per
    dz = ctx.synth(FIELD, 1 << sy, SEED, 0)
    outs = [ctx.alloc(FIELD, nrows) for _ in range(3)]
    ms: dict = {}
    pick_r = {"r1cs": gather_bytes(n, nrows, 3)}

    def mul():
        ctx.reset_stats()
        check(lib().zk_dev_r1cs_mul(r.h, dz.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr))
        logged(ctx, ms, pick_r)

    G = n  # as many gates as entries, fan-out 9 of every left input
    left = rng.permutation(np.repeat(np.arange(nrows, dtype=np.uint32), 9))
    circ = WiredCircuit([(rng.integers(0, 2, G, dtype=np.uint8), left, rng.integers(0, nrows, G, dtype=np.uint32))],
                        nrows, FIELD)
    x = limbs(rng, nrows)
    h = circ.device(ctx)
    outp = np.zeros((1 << circ.output_vars, 4), np.uint64)
    coeffs, nco = np.zeros((circ.total_rounds, 3, 4), np.uint64), np.zeros(circ.total_rounds, np.uint8)
    ch, claims, ins = np.zeros((circ.total_rounds, 4), np.uint64), np.zeros((1, 4), np.uint64), np.zeros((2, 4), np.uint64)
    pick_w = {"phase1": 72.0 * G + 76.0 * nrows}  # wired.hip gather_pass; by left: 2^lg rows of 9, one chunk each

    def wired():
        ctx.reset_stats()
        check(lib().zk_gkr_wired_prove(h.h, FIELD, 0, ptr(x), ptr(outp), ptr(coeffs), ptr(nco), ptr(ch), ptr(claims),
                                       ptr(ins)))
        logged(ctx, ms, pick_w)

    ctx.set_timing_kinds(["layer"])
    for fn in (mul, wired) * 2:
        fn()
    ms.clear()
    ts = timed_round([mul, wired], min_seconds)
    ctx.set_timing(False)
    res = {"tool": "r1cs_bench", "case": f"gather_rows_2^{lg}", "log2_rows": lg, "entries": n, "gates": G,
           **summary("mul_call", ts[0]), **summary("wired_proof", ts[1]), **kernel_summary("r1cs", ms["r1cs"], n),
           **kernel_summary("phase1", ms["phase1"], G)}
    res["r1cs_over_phase1"] = res["r1cs_ns_per_entry"] / res["phase1_ns_per_entry"]
    res["r1cs_min_over_phase1_max"] = res["r1cs_kernel_ms_min"] / res["phase1_kernel_ms_max"]
    r.close()
    circ.close()
    for t in [dz] + outs:
        t.free()
    return res


def bench_chain(ctx, lg: int, min_seconds: float) -> list[dict]:
    import zk_amd
    from zk_amd import R1CS
    from zk_amd._lib import check, lib
    from zk_amd.elems import as_limbs, ptr
    from zk_amd.kzg import KZG

    mats, w, io = chain_arrays(lg)
    nrows, sx, sy = 1 << lg, lg, lg + 1
    r = R1CS(FIELD, nrows, sy, 1, *mats, ctx=ctx)
    rows = np.concatenate([m[0] for m in mats])
    cols = np.concatenate([m[1] for m in mats])
    n = len(rows)
    row_chunks, _, _ = nchunks_of(rows)
    col_chunks, col_slots, col_split = nchunks_of(cols)
    dw = ctx.upload(FIELD, w)
    dz = ctx.upload(FIELD, r.z(w, io))
    outs = [ctx.alloc(FIELD, nrows) for _ in range(3)]
    rx, ry = as_limbs([11 + 3 * i for i in range(sx)]), as_limbs([13 + 5 * i for i in range(sy)])
    me = np.zeros((3, 4), np.uint64)
    ms: dict = {}
    picks = {"rows": gather_bytes(n, row_chunks, 3), "cols": gather_bytes(n, col_chunks, 3),
             "combine": 32.0 * 3 * (col_slots + col_split)}

    def mul():
        ctx.reset_stats()
        check(lib().zk_dev_r1cs_mul(r.h, dz.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr))
        logged(ctx, ms, {"rows": picks["rows"]})

    def evals():
        ctx.reset_stats()
        check(lib().zk_r1cs_matrix_evals(r.h, 0, ptr(rx), ptr(ry), ptr(me)))
        logged(ctx, ms, {"cols": picks["cols"], "combine": picks["combine"]})

    ctx.set_timing_kinds(["layer"])
    for fn in (mul, evals) * 2:
        fn()
    ms.clear()
    ts = timed_round([mul, evals], min_seconds)
    ctx.set_timing(False)
    gather = {"tool": "r1cs_bench", "case": f"gather_chain_2^{lg}", "log2_rows": lg, "entries": n,
              "row_chunks": row_chunks, "col_chunks": col_chunks, "col_slots": col_slots, "col_split_rows": col_split,
              **summary("mul_call", ts[0]), **summary("matrix_evals_call", ts[1]),
              **kernel_summary("rows", ms["rows"], n), **kernel_summary("cols", ms["cols"], n),
              **kernel_summary("combine", ms["combine"], n)}
    gather["cols_plus_combine_over_rows"] = (gather["cols_kernel_ms"] + gather["combine_kernel_ms"]) / gather["rows_kernel_ms"]

    # the whole committed proof and its parts
    kzg = KZG([5 + 2 * i for i in range(sy - 1)], ctx)
    c1, n1 = np.zeros((sx, 4, 4), np.uint64), np.zeros(sx, np.uint8)
    c2, n2 = np.zeros((sy, 3, 4), np.uint64), np.zeros(sy, np.uint8)
    ev, prx, pry = np.zeros((4, 4), np.uint64), np.zeros((sx, 4), np.uint64), np.zeros((sy, 4), np.uint64)
    cm, op = np.zeros((1, 12), np.uint64), np.zeros((sy - 1, 12), np.uint64)
    iol = as_limbs(io)

    def whole():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_r1cs_prove(r.h, 0, dw.ptr, ptr(iol), kzg.h, None, t.h, ptr(c1), ptr(n1), ptr(c2), ptr(n2),
                                      ptr(ev), ptr(prx), ptr(pry), ptr(cm), ptr(op)))

    scm, sop = np.zeros((1, 12), np.uint64), np.zeros((sy - 1, 12), np.uint64)

    def commit():
        check(lib().zk_dev_kzg_commit(ctx.h, kzg.h, dw.ptr, ptr(scm)))

    eq = zk_amd.DeviceTable.eq(ctx, FIELD, [11 + 3 * i for i in range(sx)])
    p = zk_amd.api.modulus(FIELD)
    neq = zk_amd.DeviceTable.lincomb([eq], [p - 1])
    ones = zk_amd.DeviceTable.lincomb([eq], [0], 1)
    check(lib().zk_dev_r1cs_mul(r.h, dz.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr))  # Az, Bz, Cz for sum-check 1
    t1 = (C.c_void_p * 6)(*[t.ptr.value for t in (eq, outs[0], outs[1], neq, outs[2], ones)])
    m_tab = ctx.synth(FIELD, 1 << sy, SEED, 1)  # (any table of 2^sy times the cost of M's)
    t2 = (C.c_void_p * 2)(m_tab.ptr.value, dz.ptr.value)
    f1, f2 = np.arange(6, dtype=np.uint8), np.arange(2, dtype=np.uint8)
    s1c, s1n, s1h, s1e = np.zeros((sx, 4, 4), np.uint64), np.zeros(sx, np.uint8), np.zeros((sx, 4), np.uint64), np.zeros((6, 4), np.uint64)
    s2c, s2n, s2h, s2e = np.zeros((sy, 3, 4), np.uint64), np.zeros(sy, np.uint8), np.zeros((sy, 4), np.uint64), np.zeros((2, 4), np.uint64)
    cs, zero = np.zeros((1, 4), np.uint64), as_limbs([0])

    def sumcheck1():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, t1, 6, sx, ptr(f1), 2, 3, ptr(zero), t.h, ptr(s1c),
                                                   ptr(s1n), ptr(s1h), ptr(s1e), ptr(cs)))

    def sumcheck2():
        t = zk_amd.Transcript(FIELD)
        check(lib().zk_dev_composed_sumcheck_prove(ctx.h, FIELD, 0, t2, 2, sy, ptr(f2), 1, 2, ptr(zero), t.h, ptr(s2c),
                                                   ptr(s2n), ptr(s2h), ptr(s2e), ptr(cs)))

    def opening():
        check(lib().zk_dev_kzg_get_proof(ctx.h, kzg.h, 0, dw.ptr, ptr(ev[3:4]), ptr(pry[1:]), ptr(sop)))

    def rows_pass():
        check(lib().zk_dev_r1cs_mul(r.h, dz.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr))

    def cols_pass():
        check(lib().zk_r1cs_matrix_evals(r.h, 0, ptr(rx), ptr(ry), ptr(me)))

    whole()  # (ev and pry: the opening's inputs)
    names = ["whole", "commit", "rows", "sumcheck1", "cols", "sumcheck2", "open"]
    calls = [whole, commit, rows_pass, sumcheck1, cols_pass, sumcheck2, opening]
    for fn in calls * 2:
        fn()
    whole()
    g2 = np.zeros((sy - 1, 24), np.uint64)
    check(lib().zk_kzg_g2_taus(kzg.h, ptr(g2)))
    ok = C.c_int(0)
    vrx, vry = np.zeros((sx, 4), np.uint64), np.zeros((sy, 4), np.uint64)
    vt = zk_amd.Transcript(FIELD)
    check(lib().zk_r1cs_verify(r.h, 0, ptr(iol), ptr(c1), ptr(n1), ptr(c2), ptr(n2), ptr(ev), ptr(cm), ptr(op), ptr(g2),
                               vt.h, C.byref(ok), ptr(vrx), ptr(vry)))
    if not ok.value or not np.array_equal(vry, pry):
        raise RuntimeError("the benchmarked proof does not verify")
    ts = timed_round(calls, min_seconds)
    proof = {"tool": "r1cs_bench", "case": f"proof_chain_2^{lg}", "log2_rows": lg, "sx": sx, "sy": sy, "entries": n,
             "verified": True}
    for name, t in zip(names, ts):
        proof.update(summary(name, t))
    proof["parts_over_whole"] = sum(proof[f"{k}_ms"] for k in names[1:]) / proof["whole_ms"]
    ctx.set_timing(True)
    ctx.reset_stats()
    whole()
    k = ctx.stats()["kernels"]
    ctx.set_timing(False)
    proof["whole_all_kernel_ms"] = sum(v["ms"] for v in k.values())
    proof["whole_launches"] = sum(v["launches"] for v in k.values())
    # the prover's own matrix passes (the column pass is NC = 1 there), event-timed inside whole proofs
    inside: dict = {}
    own = {"rows_in_proof": picks["rows"], "cols_in_proof": gather_bytes(n, col_chunks, 1),
           "combine_in_proof": 32.0 * 1 * (col_slots + col_split)}
    ctx.set_timing_kinds(["layer"])
    for _ in range(9):
        ctx.reset_stats()
        whole()
        logged(ctx, inside, own)
    ctx.set_timing(False)
    for name, v in inside.items():
        proof.update(kernel_summary(name, v, n))
    r.close()
    kzg.close()
    return [gather, proof]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_bench.json"),
                    help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    res = [bench_gather_rows(ctx, a.log_rows, a.min_seconds)] + bench_chain(ctx, a.log_rows, a.min_seconds)
    lines = [json.dumps(x) for x in res]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

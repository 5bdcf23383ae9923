"""Keccak Merkle tree on one GPU: build, batched openings and batched updates,
beside the same build by the one-core oracle on the same host.

usage: python tools/merkle_bench.py [--sizes 0:20,0:24,2:24] [--min-seconds 1.5]
                                    [--full-oracle] [--out profiles/merkle_bench.json]

Per (field, depth) one JSON line:
  build_ms        MerkleTree.new_with_inputs over a synthesised DeviceTable of
                  2^depth elements (zk_dev_merkle_new: allocation of the tree,
                  2^depth leaf hashes, 2^depth - 1 pair hashes, one synchronise);
                  median of the timed repeats, host clock around the synchronous call
  alloc_ms        the tree's allocation alone (a device allocation of the same
                  size, timed the same way): build_ms - alloc_ms is the hashing
  hashes_per_s    (2^(depth+1) - 1) / build time; hashing_hashes_per_s without the allocation
  open1024_ms     zk_merkle_create_proofs of 1 024 leaves in one call
  update1024_ms   zk_merkle_update_leaves of 1 024 distinct leaves in one call
  oracle_build_ms the same tree by the oracle on one core of this host (its C
                  Keccak-256 per hash; the reduction mod p and the loop are
                  Python, about 1 us per hash of glue). Measured at depth <= 20
                  (and the roots compared); above that extrapolated from the
                  measured time per hash unless --full-oracle
Warm-up builds come first; each figure is timed over at least --min-seconds in total.
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
for p in (os.path.join(ROOT, "zk-research-implementations_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 11
FIELD_NAMES = {0: "bn254_fr", 1: "bn254_fq", 2: "bls12_381_fr"}


def oracle_build(field: int, depth: int) -> tuple[int, float, int]:
    """(root, seconds, hashes): merkle_tree.rs new_with_inputs over synth(field, SEED, 0, 0, 2^depth), one core."""
    import coracle as co
    import pyoracle as po

    L, p = co.lib(), po.MODULI[field]
    n = 1 << depth
    inputs = co.synth(field, SEED, 0, 0, n)
    out = (C.c_uint8 * 32)()
    out_addr = C.addressof(out)
    keccak, from_bytes = L.or_keccak256, int.from_bytes

    def level(cur: bytearray, msg: int) -> bytearray:  # one Keccak-256 per msg bytes, reduced mod p
        count = len(cur) // msg
        src = C.addressof((C.c_uint8 * len(cur)).from_buffer(cur))
        nxt = bytearray(32 * count)
        for j in range(count):
            keccak(src + msg * j, msg, out_addr)
            nxt[32 * j: 32 * j + 32] = (from_bytes(bytes(out), "little") % p).to_bytes(32, "little")
        return nxt

    t0 = time.perf_counter()
    cur = level(bytearray(inputs.tobytes()), 32)  # leaves: compute_hash
    hashes = n
    while len(cur) > 32:  # levels: hash_pair
        cur = level(cur, 64)
        hashes += len(cur) // 32
    return from_bytes(bytes(cur), "little"), time.perf_counter() - t0, hashes


def timed(fn, min_seconds: float, min_reps: int = 5) -> list[float]:
    ts, total = [], 0.0
    while total < min_seconds or len(ts) < min_reps:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        ts.append(dt)
        total += dt
    return ts


def bench(ctx, field: int, depth: int, min_seconds: float, full_oracle: bool, per_hash_s: float | None) -> dict:
    import coracle as co

    from zk_amd._lib import check, lib
    from zk_amd.elems import ptr
    from zk_amd.merkle import MerkleTree, verify_proof

    n = 1 << depth
    hashes = 2 * n - 1
    table = ctx.synth(field, n, seed=SEED, table=0)

    def build():
        MerkleTree.new_with_inputs(field, depth, table, ctx).close()

    def alloc():
        ctx.alloc(field, 2 * n - 1).free()

    for _ in range(2):  # warm-up: code objects, the occupancy query, the allocator
        build()
        alloc()
    tb = timed(build, min_seconds)
    ta = timed(alloc, min_seconds / 4)
    build_s, alloc_s = statistics.median(tb), statistics.median(ta)

    tree = MerkleTree.new_with_inputs(field, depth, table, ctx)
    root = tree.get_root_hash()
    k = 1024
    ids = np.array([(i * (n // k) + (i % 7)) % n for i in range(k)] if n >= 8 * k else list(range(min(k, n))), np.uint64)
    k = len(ids)
    data = np.concatenate([co.synth(field, SEED, 0, int(i), 1) for i in ids])
    sib = np.zeros((k * depth, 4), np.uint64)
    sides = np.zeros(k * depth, np.uint8)

    def open_batch():
        check(lib().zk_merkle_create_proofs(tree.h, 0, ptr(data), ptr(ids), k, ptr(sib), ptr(sides)))

    open_batch()
    to = timed(open_batch, min_seconds / 2)
    proof = tree.create_proof(int.from_bytes(data[5].tobytes(), "little"), int(ids[5]))
    if not verify_proof(root, proof, field):
        raise RuntimeError("an opening of the built tree does not verify")

    new = co.synth(field, SEED + 1, 1, 0, k)
    flags = np.zeros(k, np.uint8)

    def update_batch():
        check(lib().zk_merkle_update_leaves(tree.h, 0, ptr(ids), ptr(new), ptr(flags), k))

    update_batch()
    tu = timed(update_batch, min_seconds / 2)
    tree.close()
    table.free()

    res = {
        "tool": "merkle_bench", "field": FIELD_NAMES[field], "depth": depth, "hashes": hashes,
        "build_ms": build_s * 1e3, "build_ms_min": min(tb) * 1e3, "build_reps": len(tb), "alloc_ms": alloc_s * 1e3,
        "hashes_per_s": hashes / build_s, "hashing_hashes_per_s": hashes / max(build_s - alloc_s, 1e-9),
        "open1024_ms": statistics.median(to) * 1e3, "open_reps": len(to),
        "update1024_ms": statistics.median(tu) * 1e3, "update_reps": len(tu), "batch": k,
        "root": "0x%064x" % root,
    }
    if depth <= 20 or full_oracle:
        oroot, secs, oh = oracle_build(field, depth)
        assert oh == hashes
        res.update(oracle_build_ms=secs * 1e3, oracle_measured=True, root_matches_oracle=(oroot == root))
        if oroot != root:
            raise RuntimeError(f"root differs from the oracle's: {root:#x} vs {oroot:#x}")
    elif per_hash_s is not None:
        res.update(oracle_build_ms=per_hash_s * hashes * 1e3, oracle_measured=False, root_matches_oracle=None)
    if "oracle_build_ms" in res:
        res["speedup_vs_oracle"] = res["oracle_build_ms"] / res["build_ms"]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0:20,0:24,2:24", help="field:depth, comma separated")
    ap.add_argument("--min-seconds", type=float, default=1.5)
    ap.add_argument("--full-oracle", action="store_true", help="run the oracle build at every size (minutes at depth 24)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()

    import zk_amd

    ctx = zk_amd.default_context()
    per_hash = None
    lines = []
    for item in a.sizes.split(","):
        f, d = (int(v) for v in item.split(":"))
        r = bench(ctx, f, d, a.min_seconds, a.full_oracle, per_hash)
        if r.get("oracle_measured"):
            per_hash = r["oracle_build_ms"] / 1e3 / r["hashes"]
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

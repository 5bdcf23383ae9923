"""Writes tests/golden/merkle.json from the pure-Python oracle alone
(oracle/pyoracle.py: its own Keccak-f[1600]): per field the root of the
depth-10 tree of merkle_tree.rs over synth(field, seed 11, table 0, 0, 1024)
and the set of quotients floor(digest / p) met while building it (the
branches of from_le_bytes_mod_order's reduction).

    python tests/golden/make_merkle_golden.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

import pyoracle as po  # noqa: E402

DEPTH, SEED = 10, 11


def build(field: int) -> dict:
    p = po.MODULI[field]
    quotients = set()

    def h(data: bytes) -> int:
        d = int.from_bytes(po.keccak256(data), "little")
        quotients.add(d // p)
        return d % p

    inputs = po.synth(field, SEED, 0, 0, 1 << DEPTH)
    cur = [h(v.to_bytes(32, "little")) for v in inputs]  # compute_hash :201-206
    for _ in range(DEPTH):  # hash_pair :208-214
        cur = [h(cur[j].to_bytes(32, "little") + cur[j + 1].to_bytes(32, "little")) for j in range(0, len(cur), 2)]
    return {"field": field, "root": "0x%064x" % cur[0], "quotients": sorted(quotients)}


def main() -> None:
    out = {"depth": DEPTH, "seed": SEED, "table": 0, "index0": 0, "count": 1 << DEPTH,
           "trees": [build(f) for f in (0, 1, 2)]}
    with open(os.path.join(HERE, "merkle.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

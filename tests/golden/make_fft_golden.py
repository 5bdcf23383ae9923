"""Writes tests/golden/fft.json from the pure-Python oracles alone
(tests/fft_oracle.py over oracle/pyoracle.py): for BN254 Fr and BLS12-381 Fr
the constant g^((p - 1) / 2^s) every root of unity is squared down from, and
the Keccak-256 of the canonical little-endian bytes of
fft_evaluate(synth(field, seed 11, table 0, 0, n)) at n = 2^12 and at the sizes
where the GPU plan changes shape: 2^(T+1) (two passes), 2^(2T) (two full
passes) and 2^(2T+1) (three), T = kFftTileLog of csrc/fft_plan.hpp.

    python tests/golden/make_fft_golden.py      (about a minute)
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import fft_oracle as fo  # noqa: E402
import pyoracle as po  # noqa: E402

SEED = 11
with open(os.path.join(HERE, "..", "..", "zk-research-implementations_amd", "csrc", "fft_plan.hpp")) as _fh:
    TILE_LOG = int(re.search(r"constexpr uint32_t kFftTileLog = (\d+);", _fh.read()).group(1))
LOGS = sorted({12, TILE_LOG + 1, 2 * TILE_LOG, 2 * TILE_LOG + 1})


def build(field: int) -> dict:
    inputs = po.synth(field, SEED, 0, 0, 1 << LOGS[-1])
    digests = {}
    for k in LOGS:
        y = fo.fft_evaluate(field, inputs[: 1 << k])
        digests[str(k)] = po.keccak256(fo.table_bytes(y)).hex()
    return {"field": field, "two_adicity": fo.TWO_ADICITY[field], "generator": fo.GENERATOR[field],
            "two_adic_root": "0x%064x" % fo.two_adic_root(field), "evaluate_keccak256": digests}


def main() -> None:
    out = {"tile_log": TILE_LOG, "seed": SEED, "table": 0, "index0": 0, "fields": [build(f) for f in (0, 2)]}
    with open(os.path.join(HERE, "fft.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Writes tests/golden/poly.json from the pure-Python oracles alone
(tests/poly_oracle.py over oracle/pyoracle.py): for each field the SHA-256 of
the canonical little-endian bytes of
  interpolate((x_i, y_i), i < 1025), x = synth(field, seed 23, table 0) with
      x_1 replaced by 0, y = synth(field, seed 23, table 1)
  evaluate(coefficients synth(.., table 2)[:d], points synth(.., table 3)[:m])
      at (d, m) = (2 kPolyEvalTile + 76, 257),
with kPolyEvalTile read from csrc/poly_plan.hpp. Inputs are named by seed and
table (the generator oracle/coracle.py and the library share), not stored.

    python tests/golden/make_poly_golden.py      (a few seconds)
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import poly_oracle as O  # noqa: E402
import pyoracle as po  # noqa: E402

SEED = 23
N = 1025
with open(os.path.join(HERE, "..", "..", "zk-research-implementations_amd", "csrc", "poly_plan.hpp")) as _fh:
    EVAL_TILE = int(re.search(r"constexpr uint32_t kPolyEvalTile = (\d+);", _fh.read()).group(1))
SHAPE = (2 * EVAL_TILE + 76, 257)


def points(field: int, n: int):
    xs, ys = po.synth(field, SEED, 0, 0, n), po.synth(field, SEED, 1, 0, n)
    if n > 1:
        xs[1] = 0
    return list(zip(xs, ys))


def main() -> None:
    interp, ev = {}, {}
    for field in (0, 1, 2):
        p = po.MODULI[field]
        pts = points(field, N)
        coeffs = O.interpolate_fast(p, pts)
        assert O.is_interpolant(p, coeffs, pts)
        interp[str(field)] = {str(N): O.digest(coeffs)}
        cf, xs = po.synth(field, SEED, 2, 0, SHAPE[0]), po.synth(field, SEED, 3, 0, SHAPE[1])
        ev[str(field)] = O.digest([O.horner(p, cf, x) for x in xs])
    out = {"seed": SEED, "eval_tile": EVAL_TILE, "interpolate_sha256": interp, "evaluate_shape": list(SHAPE),
           "evaluate_sha256": ev}
    with open(os.path.join(HERE, "poly.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

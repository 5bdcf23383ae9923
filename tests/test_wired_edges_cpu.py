"""The chunk-edge circuits of tests/wired_edge_circuits.py have the rows their
names say: a recount of the wiring arrays, with wired_csr's cut rule
(csrc/wired_plan.hpp; the rule itself is checked by
tests/native/wired_plan_check.cpp) restated in row_chunks."""
from __future__ import annotations

import numpy as np
import pytest

import wired_edge_circuits as we

CASES = {**we.CHUNK_EDGES_DENSE, **we.CHUNK_EDGES_HOST}
WANT = {"row256": {1: [256]}, "row257": {2: [256, 1]}, "rows512+513": {0: [256, 256], 3: [256, 256, 1]},
        "row65537": {1: [256] * 256 + [1]}}


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_are_what_the_names_say(name, side):
    ninputs, gates, heavy = CASES[name]
    layers = we.skewed_circuit(1, ninputs, gates, heavy, side)
    assert [len(x[0]) for x in layers] == [gates, 2]
    ops, left, right = layers[0]
    key, other = (left, right) if side == "left" else (right, left)
    rows = we.row_chunks(key, ninputs)
    assert sum(sum(c) for c in rows.values()) == gates
    for wire, chunks in WANT[name].items():
        assert rows[wire] == chunks
    for wire, chunks in rows.items():  # the rest is spread: no other row on this side is split
        assert wire in heavy or len(chunks) == 1
    assert 0 < int(ops.sum()) < gates and len(np.unique(other)) == ninputs  # mixed ops, the other side random
    assert int(max(left.max(), right.max())) < ninputs
    assert sorted(np.flatnonzero(key == next(iter(heavy))).tolist()) != list(range(heavy[next(iter(heavy))]))  # shuffled
    if name == "row65537":
        assert len(rows[1]) == 257 > we.CHUNK  # slots of the row: k_wired_combine's loop runs twice


def test_row_chunks_is_the_cut_rule():
    key = np.array([0] * 1 + [2] * 256 + [3] * 257 + [5] * 600, np.uint32)
    assert we.row_chunks(key, 7) == {0: [1], 2: [256], 3: [256, 1], 5: [256, 256, 88]}

"""Wired circuits whose gate rows sit on the edges of the chunking
(csrc/wired_plan.hpp wired_csr, kWiredChunk = 256), as numpy arrays (test
helper, not a test module; the GPU side is tests/test_gpu_wired_edges.py, the
recount of the rows tests/test_wired_edges_cpu.py).

A row is the list of a layer's gates that read one wire on one side: phase 1
gathers through the rows by left input, phase 2 through those by right input.
A row of at most 256 gates is one chunk, written straight into the table; a
longer one is cut into chunks of 256 and a rest, each summed into a slot, and
one block of 256 threads adds a row's slots (k_wired_combine)."""
from __future__ import annotations

import numpy as np

CHUNK = 256  # kWiredChunk


def skewed_layer(rng: np.random.Generator, below: int, gates: int, heavy: dict, side: str):
    """One layer (ops, left, right) of `gates` gates over `below` wires: wire w
    feeds exactly heavy[w] gates on `side` ("left" or "right"), the other gates'
    wires on that side go round the remaining wires, the gates are in random
    order, the ops mixed and the wires of the other side random."""
    assert side in ("left", "right") and sum(heavy.values()) <= gates and all(0 <= w < below for w in heavy)
    rest = np.array([w for w in range(below) if w not in heavy], np.uint32)
    nrest = gates - sum(heavy.values())
    assert nrest == 0 or len(rest) > 0
    key = np.concatenate([np.full(c, w, np.uint32) for w, c in sorted(heavy.items())] +
                         [rest[np.arange(nrest) % max(len(rest), 1)] if nrest else np.zeros(0, np.uint32)])
    key = np.ascontiguousarray(key[rng.permutation(gates)])
    other = rng.integers(0, below, gates, dtype=np.uint32)
    ops = rng.integers(0, 2, gates, dtype=np.uint8)
    return (ops, key, other) if side == "left" else (ops, other, key)


def top_layer(rng: np.random.Generator, below: int, gates: int = 2):
    """A small layer above: mixed ops, random wires."""
    ops = (np.arange(gates) % 2).astype(np.uint8)
    return ops, rng.integers(0, below, gates, dtype=np.uint32), rng.integers(0, below, gates, dtype=np.uint32)


def skewed_circuit(seed: int, ninputs: int, gates: int, heavy: dict, side: str):
    """-> layers [gates, 2] with the first one skewed_layer"""
    rng = np.random.default_rng(seed)
    return [skewed_layer(rng, ninputs, gates, heavy, side), top_layer(rng, gates)]


def row_chunks(key: np.ndarray, nrows: int) -> dict:
    """wired_csr's cut, recounted: {row: [its chunks' gate counts]} for every row that has a gate."""
    counts = np.bincount(key, minlength=nrows)
    return {int(r): [CHUNK] * (int(n) // CHUNK) + ([int(n) % CHUNK] if int(n) % CHUNK else [])
            for r, n in enumerate(counts) if n}


# name -> (ninputs, gates of the first layer, {wire: gates it feeds}); each runs on the left and on the right
CHUNK_EDGES_DENSE = {      # against the dense model (4 inputs, layers [300, 2])
    "row256": (4, 300, {1: 256}),          # a whole row of exactly one full chunk: not split
    "row257": (4, 300, {2: 257}),          # split: 256 + 1
}
CHUNK_EDGES_HOST = {       # against the host path
    "rows512+513": (4, 1100, {0: 512, 3: 513}),   # two full chunks; two full chunks and a last one of 1
    "row65537": (4, 65600, {1: 65537}),           # 257 slots: more than the combining block has threads
}

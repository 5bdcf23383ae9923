"""The wired GKR prover (csrc/wired.hpp) and the tree prover
(csrc/gkr_circuit.hip) where tests/test_gpu_wired.py and
tests/test_gpu_gkr_circuit.py do not reach their device code. Every comparison
is an equality of field elements: with the dense model
(tests/gkr_wired_oracle.py, oracle/gkr_oracle.py) where its tables are small
enough, otherwise between every layer on the device (ZK_CIRCUIT_HOST_LGL=0)
and every layer on the host (20), an independent fill of the same tables, plus
the host verifier.

(a) boundary inputs in place of random ones: all 0 (every round polynomial
    trims to nothing), all 1, all p - 1, alternating 0 / p - 1, and the
    boundary palette (tests/extreme_tables.py);
(b) rows on the edges of the chunking (tests/wired_edge_circuits.py): 256 gates
    (one whole chunk) against 257 (split, a last chunk of 1), 512, 513, and
    65 537, whose 257 slots make the combining block's loop run twice; each on
    the left (phase 1) and on the right (phase 2);
(c) the zero fill of k_wired_layer past the last gate, within a block and
    across a block boundary, and k_eq_table over 1 to 6, 8, 9, 10 and 17
    coordinates (every split into passes of 1, 2 and 3);
(d) the tree prover's kernels on the inputs of (a).
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import extreme_tables as xt
import gkr_oracle as go
import gkr_wired_oracle as wo
import wired_edge_circuits as we
from test_gpu_gkr_circuit import OPS, _circuit
from test_gpu_wired import SHAPES, _context, _equals_dense, _fields, _limbs, _numpy_layers, _special

from zk_amd.elems import to_ints
from zk_amd.gkr import Circuit, WiredCircuit, prove, verify

pytestmark = pytest.mark.gpu
FIELDS = (0, 1, 2)
HOST_ALL = "20"  # every layer of every circuit here has kb <= 20: all on the host


def boundary_inputs(field: int, n: int) -> dict:
    p = go.MODULI[field]
    pal = xt.palette(field)
    return {"zeros": [0] * n, "ones": [1] * n, "pm1": [p - 1] * n, "alternating": [(p - 1) * (i & 1) for i in range(n)],
            "palette": [xt.canonical(field, pal[i % len(pal)]) for i in range(n)]}


# ---- (a) boundary inputs against the dense model ---------------------------------------
def _one_op(op: int):
    rng = random.Random(f"one-op{op}")
    return 5, [[(op, rng.randrange(b), rng.randrange(b)) for _ in range(g)] for b, g in ((5, 6), (6, 4), (4, 2))]


def _shape(shape):
    if shape == "mul-only":
        return _one_op(1)
    if shape == "add-only":
        return _one_op(0)
    if isinstance(shape, str):
        return _special(shape)
    return shape[0], wo.random_layers(random.Random(f"edges{shape}"), *shape)


@pytest.mark.parametrize("host_lgl", ["0", None])
@pytest.mark.parametrize("shape", SHAPES + ["mul-only", "add-only"],
                         ids=lambda s: s if isinstance(s, str) else f"{s[0]};{','.join(map(str, s[1]))}")
def test_boundary_inputs_equal_the_dense_model(monkeypatch, shape, host_lgl):
    ninputs, layers = _shape(shape)
    ctx = _context(monkeypatch, host_lgl)
    try:
        for field in FIELDS:
            circ = WiredCircuit(layers, ninputs, field)
            for name, inputs in boundary_inputs(field, ninputs).items():
                want = wo.prove(field, layers, ninputs, inputs)
                got = prove(circ, inputs, ctx)
                _equals_dense(got, want)
                assert verify(got, circ, inputs) and verify(got, circ), (field, name)
                if name == "zeros":  # the model's polynomials are empty, and so must the device's be
                    assert all(q == [] for layer in want["proof_polynomials"] for q in layer)
                    assert all(q.coefficient == [] for layer in got.proof_polynomials for q in layer)
            circ.close()
    finally:
        ctx.close()


# ---- (b) chunk edges -----------------------------------------------------------------------
def _edge_circuit(cases, name, side):
    ninputs, gates, heavy = cases[name]
    layers = we.skewed_circuit(len(name) + (side == "right"), ninputs, gates, heavy, side)
    key = layers[0][1 if side == "left" else 2]
    rows = we.row_chunks(key, ninputs)
    for wire, count in heavy.items():  # the rows the case is about are what the layer has
        assert sum(rows[wire]) == count and len(rows[wire]) == -(-count // we.CHUNK)
    return ninputs, layers


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", sorted(we.CHUNK_EDGES_DENSE))
def test_chunk_edges_equal_the_dense_model(monkeypatch, name, side):
    ninputs, layers = _edge_circuit(we.CHUNK_EDGES_DENSE, name, side)
    field = (sorted(we.CHUNK_EDGES_DENSE).index(name) + (side == "right")) % 3
    inputs = to_ints(_limbs(np.random.default_rng(256), ninputs))
    tuples = [list(zip(*(a.tolist() for a in layer))) for layer in layers]
    want = wo.prove(field, tuples, ninputs, inputs)
    ctx = _context(monkeypatch, "0")
    try:
        circ = WiredCircuit(layers, ninputs, field)
        got = prove(circ, inputs, ctx)
        _equals_dense(got, want)
        assert verify(got, circ, inputs) and verify(got, circ)
        circ.close()
    finally:
        ctx.close()


def _device_equals_host(monkeypatch, circuits):
    """[(circuit, inputs)]: one proof with every layer on the device, one with every layer on the
    host; equal in every field, accepted, and rejected once an input changes."""
    proofs = []
    for host_lgl in ("0", HOST_ALL):
        ctx = _context(monkeypatch, host_lgl)
        try:
            proofs.append([prove(circ, inputs, ctx) for circ, inputs in circuits])
        finally:
            for circ, _ in circuits:
                circ.close()
            ctx.close()
    for (circ, inputs), dev, host in zip(circuits, *proofs):
        what = (int(circ.field), circ.ninputs, circ.gates.tolist())
        assert _fields(dev) == _fields(host), what
        assert verify(dev, circ, inputs), what
        bad = inputs.copy()
        bad[len(bad) // 2, 0] ^= np.uint64(1)
        assert not verify(dev, circ, bad), what


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", sorted(we.CHUNK_EDGES_HOST))
def test_chunk_edges_equal_the_host_path(monkeypatch, name, side):
    ninputs, layers = _edge_circuit(we.CHUNK_EDGES_HOST, name, side)
    field = (side == "right") * 2  # (a lazy-digit field and the reduced one)
    inputs = _limbs(np.random.default_rng(512), ninputs)
    _device_equals_host(monkeypatch, [(WiredCircuit(layers, ninputs, field), inputs)])


# ---- (c) padding and eq passes -------------------------------------------------------------
WIDTHS = [2, 3, 5, 9, 17, 33, 64]  # inputs: kb = 1 .. 6


@pytest.mark.parametrize("ninputs", WIDTHS)
def test_every_input_width_equals_the_dense_model(monkeypatch, ninputs):
    """Layers of 61 or 64 gates (a zero fill of 3 or none) and 3 over each width: eq tables over
    kb = 1 .. 6 and ka = 6 coordinates."""
    i = WIDTHS.index(ninputs)
    field, gates = i % 3, [64 if i % 2 == 0 else 61, 3]
    rng = random.Random(f"width{ninputs}")
    layers = wo.random_layers(rng, ninputs, gates)
    inputs = [rng.randrange(go.MODULI[field]) for _ in range(ninputs)]
    want = wo.prove(field, layers, ninputs, inputs)
    ctx = _context(monkeypatch, "0")
    try:
        circ = WiredCircuit(layers, ninputs, field)
        got = prove(circ, inputs, ctx)
        _equals_dense(got, want)
        assert verify(got, circ, inputs) and verify(got, circ)
        circ.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("gates", [255, 256, 257])
def test_every_input_width_under_a_wide_layer(monkeypatch, gates):
    """255, 256 and 257 gates over each width: the zero fill of the last thread of a block, none,
    and of 255 threads of a second block; eq tables over ka = 8, 8 and 9 coordinates."""
    circuits = []
    for i, ninputs in enumerate(WIDTHS):
        rng = np.random.default_rng(1000 * gates + ninputs)
        circuits.append((WiredCircuit(_numpy_layers(rng, ninputs, [gates, 2]), ninputs, (i + gates) % 3),
                         _limbs(rng, ninputs)))
    _device_equals_host(monkeypatch, circuits)


def test_zero_fill_across_a_block_boundary(monkeypatch):
    """257 inputs, layers 513 and 3: the first layer's values are zero from 513 to 1024, through the
    rest of one block and the whole of the next; kb = 9 and 10, ka = 10."""
    circuits = []
    for field in FIELDS:
        rng = np.random.default_rng(513 + field)
        circuits.append((WiredCircuit(_numpy_layers(rng, 257, [513, 3]), 257, field), _limbs(rng, 257)))
    _device_equals_host(monkeypatch, circuits)


# ---- (d) the tree prover on boundary inputs ------------------------------------------------
@pytest.mark.parametrize("field,depth,out_gates", [(2, 3, 1), (0, 3, 1), (1, 4, 2), (2, 5, 1), (0, 1, 1), (0, 1, 2),
                                                   (2, 2, 2), (0, 5, 2)])
def test_tree_prover_on_boundary_inputs(monkeypatch, field, depth, out_gates):
    """test_gpu_gkr_circuit.py's circuits with every layer on the device (k_layer_tables,
    k_phase1_tables, k_phase2_tables, k_mle_eval2, k_gate_weights), on all 0, all p - 1 and
    alternating inputs, against gkr_oracle.prove. (No KZG step: it is no part of these kernels.)"""
    structure = _circuit(random.Random(1000 * field + 10 * depth + out_gates), depth, out_gates)
    circ = Circuit([[OPS[o] for o in layer] for layer in structure], field)
    ctx = _context(monkeypatch, "0")
    try:
        for name, inputs in boundary_inputs(field, 2 * len(structure[0])).items():
            if name not in ("zeros", "pm1", "alternating"):
                continue
            want = go.prove(field, structure, inputs)
            got = prove(circ, inputs, ctx, taus=None)
            assert got.output_poly == want["output_poly"], name
            assert [[q.coefficient for q in layer] for layer in got.proof_polynomials] == \
                [[list(q) for q in layer] for layer in want["proof_polynomials"]], name
            assert got.claimed_evaluations == [tuple(c) for c in want["claimed_evaluations"]], name
            assert got.input_evaluations == tuple(want["input_evaluations"]), name
            assert verify(got, circ, inputs), name
            if name == "zeros":
                assert all(q.coefficient == [] for layer in got.proof_polynomials for q in layer)
    finally:
        ctx.close()

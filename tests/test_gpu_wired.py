"""Wired GKR circuits on the GPU: layer evaluation, gate
weights and both phases' tables by gather through the wiring, through the C
ABI. Tree-shaped wirings must give the tree prover's bytes; small circuits of
any shape must equal the dense model (tests/gkr_wired_oracle.py) exactly;
larger ones must agree between the device path and the host path (which fills
the same tables without any grouping) and pass the host verifier."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import gkr_oracle as go
import gkr_wired_oracle as wo

from zk_amd._lib import ZK_EINVAL, ZK_EUNSUPPORTED, ZkError, lib
from zk_amd.gkr import Circuit, Operation, WiredCircuit, prove, verify

pytestmark = pytest.mark.gpu
A, M = go.ADD, go.MUL


def _context(monkeypatch, host_lgl):
    import zk_amd

    if host_lgl is None:
        monkeypatch.delenv("ZK_CIRCUIT_HOST_LGL", raising=False)
    else:
        monkeypatch.setenv("ZK_CIRCUIT_HOST_LGL", host_lgl)
    return zk_amd.Context(0)


def _fields(pr):
    return (pr.output_poly, [[q.coefficient for q in layer] for layer in pr.proof_polynomials], pr.claimed_evaluations,
            pr.input_evaluations, pr.random_challenges)


def _equals_dense(pr, want):
    assert pr.output_poly == want["output_poly"]
    assert [[q.coefficient for q in layer] for layer in pr.proof_polynomials] == \
        [[list(q) for q in layer] for layer in want["proof_polynomials"]]
    assert pr.claimed_evaluations == [tuple(c) for c in want["claimed_evaluations"]]
    assert pr.input_evaluations == tuple(want["input_evaluations"])
    assert pr.random_challenges[-1] == want["final_rb"] + want["final_rc"]
    assert pr.input_proof is None


# ---- tree parity ------------------------------------------------------------
def _tree_case(field, depth, out_gates):
    rng = random.Random(7000 + 100 * field + 10 * depth + out_gates)
    structure = [[rng.choice((A, M)) for _ in range(out_gates << (depth - 1 - i))] for i in range(depth)]
    inputs = [rng.randrange(go.MODULI[field]) for _ in range(2 * len(structure[0]))]
    circ = Circuit([[Operation.Mul if o == M else Operation.Add for o in ops] for ops in structure], field)
    return structure, inputs, circ


@pytest.mark.parametrize("host_lgl", ["0", "3", None])
@pytest.mark.parametrize("depth,out_gates", [(d, o) for d in (1, 2, 3, 5) for o in (1, 2)])
def test_tree_wiring_gives_the_tree_provers_bytes(monkeypatch, depth, out_gates, host_lgl):
    ctx = _context(monkeypatch, host_lgl)
    try:
        for field in (0, 1, 2):
            structure, inputs, circ = _tree_case(field, depth, out_gates)
            wired = WiredCircuit.from_tree(circ)
            got, tree = prove(wired, inputs, ctx), prove(circ, inputs, ctx, taus=None)
            assert _fields(got) == _fields(tree)
            _equals_dense(got, go.prove(field, structure, inputs))
            assert verify(got, wired, inputs) and verify(got, circ, inputs)
            wired.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("host_lgl", ["0", "3", None])
def test_tree_wiring_depth_10(monkeypatch, host_lgl):
    ctx = _context(monkeypatch, host_lgl)
    try:
        _, inputs, circ = _tree_case(2, 10, 1)
        wired = WiredCircuit.from_tree(circ)
        got = prove(wired, inputs, ctx)
        assert _fields(got) == _fields(prove(circ, inputs, ctx, taus=None))
        assert verify(got, wired, inputs)
    finally:
        ctx.close()


# ---- dense-model parity -------------------------------------------------------
def _special(kind):
    rng = random.Random(kind)
    op = lambda: rng.randrange(2)  # noqa: E731
    if kind == "left0":  # every gate of the middle layer reads wire 0 on the left
        return 8, [[(op(), rng.randrange(8), rng.randrange(8)) for _ in range(8)],
                   [(op(), 0, rng.randrange(8)) for _ in range(8)], [(op(), rng.randrange(8), rng.randrange(8))]]
    if kind == "same":  # left == right everywhere
        return 6, [[(op(), g % 6, g % 6) for g in range(7)], [(op(), g, g) for g in range(5)], [(op(), 3, 3)] * 2]
    if kind == "pair":  # one (left, right) pair under an Add and two Muls
        return 6, [[(0, 2, 5), (1, 2, 5), (1, 2, 5), (op(), 1, 4)], [(op(), rng.randrange(4), rng.randrange(4)) for _ in range(2)]]
    assert kind == "unused"  # half the wires of the first layer are never read
    return 8, [[(op(), rng.randrange(4), rng.randrange(4)) for _ in range(6)],
               [(op(), rng.randrange(3), rng.randrange(3)) for _ in range(3)]]


SHAPES = [(6, [5, 3, 1]), (4, [16, 4]), (8, [8, 8, 3]), (2, [1]), (1, [1, 1]), "left0", "same", "pair", "unused"]


@pytest.mark.parametrize("host_lgl", ["0", None])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else f"{s[0]};{','.join(map(str, s[1]))}")
def test_device_proof_equals_dense_model(monkeypatch, shape, host_lgl):
    ctx = _context(monkeypatch, host_lgl)
    try:
        for field in (0, 1, 2):
            rng = random.Random(f"{shape}{field}")
            ninputs, layers = _special(shape) if isinstance(shape, str) else (shape[0], wo.random_layers(rng, *shape))
            inputs = [rng.randrange(go.MODULI[field]) for _ in range(ninputs)]
            circ = WiredCircuit(layers, ninputs, field)
            got = prove(circ, inputs, ctx)
            _equals_dense(got, wo.prove(field, layers, ninputs, inputs))
            assert verify(got, circ, inputs) and verify(got, circ)
            circ.close()
    finally:
        ctx.close()


# ---- the device path at size --------------------------------------------------
def _limbs(rng: np.random.Generator, n: int) -> np.ndarray:
    """n canonical field elements (below 2^252, under every modulus) as uint64[n, 4]."""
    x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    x[:, 3] >>= np.uint64(11)
    return x


def _numpy_layers(rng: np.random.Generator, ninputs: int, gates, const_wire=False):
    layers, below = [], ninputs
    for i, g in enumerate(gates):
        ops = rng.integers(0, 2, g, dtype=np.uint8)
        left = rng.integers(0, below, g, dtype=np.uint32)
        right = rng.integers(0, below, g, dtype=np.uint32)
        if const_wire:  # one wire feeds every gate: on the left (phase 1's rows) or the right (phase 2's), by layer
            (left if i % 2 == 0 else right)[:] = 5 % below
        layers.append((ops, left, right))
        below = g
    return layers


@pytest.mark.parametrize("field", [0, 2])
@pytest.mark.parametrize("const_wire", [False, True], ids=["uniform", "const-wire"])
def test_device_layers_equal_host_layers(monkeypatch, field, const_wire):
    """2^12 inputs, layers 4096, 4096, 64, 8. Every layer on the device (0), the
    default split, and every layer on the host (13; no grouping there: an
    independent fill of the same tables) give one proof. With one wire feeding
    all 4096 gates of a layer its row is 16 chunks and goes through the
    combining pass."""
    rng = np.random.default_rng(40 + field)
    circ = WiredCircuit(_numpy_layers(rng, 4096, [4096, 4096, 64, 8], const_wire), 4096, field)
    inputs = _limbs(rng, 4096)
    proofs = []
    for host_lgl in ("0", None, "13"):
        ctx = _context(monkeypatch, host_lgl)
        try:
            proofs.append(prove(circ, inputs, ctx))
        finally:
            circ.close()
            ctx.close()
    assert _fields(proofs[0]) == _fields(proofs[1]) == _fields(proofs[2])
    assert len(proofs[0].output_poly) == 8 and [len(x) for x in proofs[0].proof_polynomials] == [12, 24, 24, 24]
    assert verify(proofs[0], circ, inputs)


def test_beyond_the_tree_provers_cap(ctx):
    """2^16 inputs, layers 2^16, 2^16, 2 (the tree prover stops at 2^14 inputs)."""
    n = 1 << 16
    rng = np.random.default_rng(16)
    circ = WiredCircuit(_numpy_layers(rng, n, [n, n, 2]), n, 0)
    p = go.MODULI[0]
    pyr = random.Random(16)
    inputs = [pyr.randrange(p) for _ in range(n)]
    pr = prove(circ, inputs, ctx)
    assert pr.output_poly == circ.evaluate(inputs)[-1]
    assert [len(x) for x in pr.proof_polynomials] == [32, 32, 32]
    assert verify(pr, circ, inputs)
    bad = list(inputs)
    bad[12345] = (bad[12345] + 1) % p
    assert not verify(pr, circ, bad)
    c0 = pr.proof_polynomials[1][7].coefficient
    c0[0] = (c0[0] + 1) % p
    assert not verify(pr, circ, inputs)
    circ.close()


def test_largest_shape(ctx):
    """2^20 inputs, layers 2^20, 2, from numpy arrays (no per-gate Python work):
    the largest shape that is tested."""
    n = 1 << 20
    rng = np.random.default_rng(20)
    circ = WiredCircuit(_numpy_layers(rng, n, [n, 2]), n, 2)
    inputs = _limbs(rng, n)
    pr = prove(circ, inputs, ctx)
    assert [len(x) for x in pr.proof_polynomials] == [40, 40] and len(pr.output_poly) == 2
    assert verify(pr, circ, inputs)
    circ.close()


# ---- errors -------------------------------------------------------------------
def test_errors_write_nothing(ctx):
    import zk_amd

    L = lib()
    gates = np.array([2, 1], np.uint32)
    ops, left, right = np.array([0, 1, 0], np.uint8), np.array([0, 1, 0], np.uint32), np.array([1, 2, 1], np.uint32)

    def new(nlayers=2, gates=gates, ops=ops, left=left, right=right, ninputs=3):
        h = C.c_void_p(0xDEAD)
        rc = L.zk_gkr_wired_new(ctx.h, nlayers, gates.ctypes.data, ops.ctypes.data, left.ctypes.data,
                                right.ctypes.data, ninputs, C.byref(h))
        return rc, h

    rc, h = new()
    assert rc == 0 and h.value not in (None, 0xDEAD)
    L.zk_gkr_wired_free(h)
    for kw in ({"right": np.array([1, 3, 1], np.uint32)},      # an index >= n_below (first layer)
               {"left": np.array([0, 1, 2], np.uint32)},       # ... (second layer: two wires below)
               {"ops": np.array([0, 2, 0], np.uint8)},         # an op of 2
               {"gates": np.array([3, 0], np.uint32)},         # an empty layer
               {"nlayers": 0}, {"ninputs": 0}):
        rc, h = new(**kw)
        assert rc == ZK_EINVAL and h.value is None, kw         # (*out is cleared, no handle is made)
    rc, h = new(nlayers=257, gates=np.ones(257, np.uint32), ops=np.zeros(257, np.uint8),
                left=np.zeros(257, np.uint32), right=np.zeros(257, np.uint32), ninputs=1)
    assert rc == ZK_EUNSUPPORTED and h.value is None
    with pytest.raises(ZkError) as e:
        WiredCircuit([[(0, 0, 0)]] * 257, 1)
    assert e.value.code == ZK_EUNSUPPORTED
    for bad in ([[(0, 0, 3)]], [[(2, 0, 1)]], [[(0, 0, 1)], []], []):
        with pytest.raises(ValueError):
            WiredCircuit(bad, 3)

    # a handle made on another context
    circ = WiredCircuit([[(0, 0, 1), (1, 1, 2)], [(1, 0, 1)]], 3)
    other = zk_amd.Context(0)
    try:
        with pytest.raises(ValueError, match="another context"):
            prove(circ.device(other), [1, 2, 3], ctx)
        assert prove(circ.device(other), [1, 2, 3]).output_poly == [(1 + 2) * (2 * 3), 0]
    finally:
        circ.close()
        other.close()

    # a failing proof (an input that is no field element) leaves every output as it was
    hd = circ.device(ctx)
    x = np.zeros((3, 4), np.uint64)
    x[1] = np.uint64((1 << 64) - 1)
    outs = [np.full((n, 4), 7, np.uint64) for n in (2, 3 * 8, 8, 2, 2)]
    nco = np.full(8, 7, np.uint8)
    rc = L.zk_gkr_wired_prove(hd.h, 0, 0, x.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data, nco.ctypes.data,
                              outs[2].ctypes.data, outs[3].ctypes.data, outs[4].ctypes.data)
    assert rc == ZK_EINVAL
    assert all((o == 7).all() for o in outs) and (nco == 7).all()
    with pytest.raises(ValueError):
        prove(circ, [1, 2], ctx)  # the wrong number of inputs
    assert prove(circ, [1, 2, 3], ctx).output_poly == [18, 0]
    circ.close()

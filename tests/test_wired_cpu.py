"""Wired GKR circuits on the CPU: the dense model
(tests/gkr_wired_oracle.py) equals the reference restatement
(oracle/gkr_oracle.py) on tree circuits, and the library's host verifier
(zk_gkr_wired_verify, no device) accepts the dense model's proofs on any
wiring and rejects every tampering."""
from __future__ import annotations

import random

import pytest

import gkr_oracle as go
import gkr_wired_oracle as wo

from zk_amd import UnivariatePoly
from zk_amd._lib import ZK_EUNSUPPORTED, ZkError
from zk_amd.gkr import Circuit, GkrCircuitProof, Operation, WiredCircuit, verify

A, M = go.ADD, go.MUL


def to_lib(field: int, proof: dict) -> GkrCircuitProof:
    polys = [[UnivariatePoly(list(p), field) for p in layer] for layer in proof["proof_polynomials"]]
    return GkrCircuitProof(list(proof["output_poly"]), polys, [tuple(c) for c in proof["claimed_evaluations"]],
                           tuple(proof["input_evaluations"]), [])


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("out_gates", [1, 2])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_dense_model_equals_reference_on_trees(field, out_gates, depth):
    rng = random.Random(100 * depth + 10 * out_gates + field)
    structure = [[rng.choice((A, M)) for _ in range(out_gates << (depth - 1 - i))] for i in range(depth)]
    inputs = [rng.randrange(go.MODULI[field]) for _ in range(2 * len(structure[0]))]
    layers, ninputs = wo.tree_layers(structure)
    assert wo.prove(field, layers, ninputs, inputs) == go.prove(field, structure, inputs)
    circ = Circuit([[Operation.Mul if o == M else Operation.Add for o in ops] for ops in structure], field)
    wired = WiredCircuit.from_tree(circ)
    assert [list(zip(o.tolist(), a.tolist(), b.tolist())) for o, a, b in wired.layers] == layers
    assert wired.evaluate(inputs) == circ.evaluate(inputs)


SHAPES = [(6, [5, 3, 1]), (4, [16, 4]), (8, [8, 8, 3]), (2, [1]), (1, [1, 1]), (5, [7, 2])]


def _case(field: int, ninputs: int, gates: list[int]):
    rng = random.Random(f"{field}-{ninputs}-{gates}")
    layers = wo.random_layers(rng, ninputs, gates)
    inputs = [rng.randrange(go.MODULI[field]) for _ in range(ninputs)]
    return layers, inputs


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("ninputs,gates", SHAPES)
def test_host_verifier_accepts_dense_model(field, ninputs, gates):
    layers, inputs = _case(field, ninputs, gates)
    proof = to_lib(field, wo.prove(field, layers, ninputs, inputs))
    circ = WiredCircuit(layers, ninputs, field)
    assert circ.rounds() == [len(layer) for layer in proof.proof_polynomials]
    assert len(proof.output_poly) == 1 << circ.output_vars
    assert verify(proof, circ, inputs)
    assert verify(proof, circ)  # without the inputs: the sum-check chain alone
    assert circ.evaluate(inputs) == wo.circuit_evaluate(go.MODULI[field], layers, inputs)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_host_verifier_rejects_tampering(field):
    ninputs, gates = 6, [5, 4, 3]
    layers, inputs = _case(field, ninputs, gates)
    # gate 0 of the first layer: an Add over two distinct wires whose values differ
    layers[0][0] = (0, 1, 4)
    # gates 1, 2 of the first layer: a Mul-free pair reading (0, 2) and (3, 5)
    layers[0][1], layers[0][2] = (0, 0, 2), (0, 3, 5)
    p = go.MODULI[field]
    dense = wo.prove(field, layers, ninputs, inputs)
    circ = WiredCircuit(layers, ninputs, field)
    assert verify(to_lib(field, dense), circ, inputs)
    t = to_lib(field, dense)  # a round coefficient
    t.proof_polynomials[-1][0].coefficient[0] = (t.proof_polynomials[-1][0].coefficient[0] + 1) % p
    assert not verify(t, circ, inputs)
    t = to_lib(field, dense)  # a claimed evaluation
    o1, o2 = t.claimed_evaluations[0]
    t.claimed_evaluations[0] = (o1, (o2 + 1) % p)
    assert not verify(t, circ, inputs)
    t = to_lib(field, dense)  # an input evaluation
    t.input_evaluations = ((t.input_evaluations[0] + 1) % p, t.input_evaluations[1])
    assert not verify(t, circ, inputs)
    assert not verify(t, circ)
    bad = list(inputs)  # an input
    bad[3] = (bad[3] + 1) % p
    assert not verify(to_lib(field, dense), circ, bad)
    t = to_lib(field, dense)  # the output polynomial's padding is part of the statement
    t.output_poly[3] = 1
    assert not verify(t, circ, inputs)
    # the right wires of the Mul-free pair swapped: gates 1, 2 now add (0, 5) and (3, 2) — another circuit
    swapped = [list(layer) for layer in layers]
    swapped[0][1], swapped[0][2] = (0, 0, 5), (0, 3, 2)
    assert wo.circuit_evaluate(p, swapped, inputs) != wo.circuit_evaluate(p, layers, inputs)
    assert not verify(to_lib(field, dense), WiredCircuit(swapped, ninputs, field), inputs)
    # left and right of one Add gate swapped: the same function, another wiring predicate
    mirrored = [list(layer) for layer in layers]
    mirrored[0][0] = (0, 4, 1)
    assert not verify(to_lib(field, dense), WiredCircuit(mirrored, ninputs, field), inputs)
    flipped = [list(layer) for layer in layers]  # an op
    flipped[1][2] = (1 - flipped[1][2][0],) + flipped[1][2][1:]
    assert not verify(to_lib(field, dense), WiredCircuit(flipped, ninputs, field), inputs)


def test_special_wirings_verify():
    """A constant wire, left == right everywhere, one pair under an Add and two
    Muls, and a layer that leaves half its wires unused."""
    field, p = 0, go.MODULI[0]
    rng = random.Random(77)
    ninputs = 8
    layers = [
        [(rng.randrange(2), 0, rng.randrange(8)) for _ in range(8)],   # every gate reads wire 0 on the left
        [(rng.randrange(2), g % 8, g % 8) for g in range(6)],          # left == right
        [(0, 2, 5), (1, 2, 5), (1, 2, 5), (0, 1, 1)],                  # one pair, three gates
        [(rng.randrange(2), rng.randrange(2), rng.randrange(2)) for _ in range(3)],  # wires 2, 3 unused
    ]
    inputs = [rng.randrange(p) for _ in range(ninputs)]
    proof = to_lib(field, wo.prove(field, layers, ninputs, inputs))
    circ = WiredCircuit(layers, ninputs, field)
    assert verify(proof, circ, inputs)


def test_shape_and_wiring_errors():
    ok = [[(0, 0, 1), (1, 1, 1)], [(0, 0, 1)]]
    WiredCircuit(ok, 2)
    with pytest.raises(ValueError, match="wire"):
        WiredCircuit([[(0, 0, 2)]], 2)  # an index >= n_below
    with pytest.raises(ValueError, match="wire"):
        WiredCircuit([[(0, 0, 1)], [(0, 0, 1)]], 2)  # ... of a later layer
    with pytest.raises(ValueError, match="op"):
        WiredCircuit([[(2, 0, 1)]], 2)
    with pytest.raises(ValueError, match="no gates"):
        WiredCircuit([[(0, 0, 1)], []], 2)
    with pytest.raises(ValueError, match="at least one layer"):
        WiredCircuit([], 2)
    with pytest.raises(ValueError, match="at least one input"):
        WiredCircuit([[(0, 0, 0)]], 0)
    with pytest.raises(ZkError) as e:  # over the caps: a valid request this build does not implement
        WiredCircuit([[(0, 0, 0)]] * 257, 1)
    assert e.value.code == ZK_EUNSUPPORTED


def test_c_verifier_validates_wiring():
    """zk_gkr_wired_verify checks the wiring itself (the Python class checks first)."""
    import ctypes as C

    import numpy as np

    from zk_amd._lib import ZK_EINVAL, lib

    gates = np.array([1], np.uint32)
    z = np.zeros((4, 4), np.uint64)
    nco = np.zeros(2, np.uint8)
    ok = C.c_int(7)

    def call(ops, left, right, nlayers=1):
        return lib().zk_gkr_wired_verify(0, 0, nlayers, gates.ctypes.data, np.array(ops, np.uint8).ctypes.data,
                                         np.array(left, np.uint32).ctypes.data, np.array(right, np.uint32).ctypes.data,
                                         2, None, z.ctypes.data, z.ctypes.data, nco.ctypes.data, z.ctypes.data,
                                         z.ctypes.data, C.byref(ok))

    assert call([0], [0], [2]) == ZK_EINVAL
    assert call([2], [0], [1]) == ZK_EINVAL
    assert call([0], [0], [1], nlayers=0) == ZK_EINVAL
    assert ok.value == 7  # nothing written on failure
    assert call([0], [0], [1]) == 0 and ok.value in (0, 1)

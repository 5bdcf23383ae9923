"""The linear-time circuit model (tests/gkr_circuit_model.py) against the dense
reference restatement (oracle/gkr_oracle.py) wherever the latter can run, the
library's host verifier against the model at the 2^14-input limit, and the
named cases of the GPU edge tests shown to be what they are meant to be.
CPU only."""
from __future__ import annotations

import pytest

import extreme_tables as xt
import gkr_circuit_model as gm
import gkr_oracle as go

from zk_amd import UnivariatePoly
from zk_amd.gkr import Circuit, GkrCircuitProof, Operation, verify

OPS = {go.ADD: Operation.Add, go.MUL: Operation.Mul}
FIELDS = (0, 1, 2)
DENSE_KEYS = ("output_poly", "proof_polynomials", "claimed_evaluations", "input_evaluations", "final_rb", "final_rc")
IN_KINDS = ("random", "zeros", "ones", "pm1", "last")


def _same_as_dense(field, depth, out_gates, ops, kind):
    structure = gm.circuit(depth, out_gates, ops, seed=7)
    ins = gm.inputs(field, 2 * len(structure[0]), kind, seed=3)
    got = gm.prove(field, structure, ins)
    want = go.prove(field, [list(layer) for layer in structure], list(ins))
    tag = (field, depth, out_gates, ops, kind)
    for key in DENSE_KEYS:
        a, b = got[key], want[key]
        if key == "proof_polynomials":
            a, b = [[list(q) for q in layer] for layer in a], [[list(q) for q in layer] for layer in b]
        elif key == "claimed_evaluations":
            a, b = [tuple(c) for c in a], [tuple(c) for c in b]
        else:
            a, b = list(a), list(b)
        assert a == b, (key, tag)
    assert sorted(got) == sorted(DENSE_KEYS + ("challenges",))
    nv = [2 * (2 * len(layer)).bit_length() - 2 for layer in reversed(structure)]
    assert len(got["challenges"]) == sum(nv), tag
    assert got["challenges"][-nv[-1]:] == list(want["final_rb"]) + list(want["final_rc"]), tag


# up to 16 inputs the dense oracle takes milliseconds: every op pattern with every input pattern
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("depth,out_gates", [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2)])
def test_model_equals_dense_oracle_small(field, depth, out_gates):
    for ops in gm.OP_KINDS:
        for kind in IN_KINDS:
            _same_as_dense(field, depth, out_gates, ops, kind)


# 32 .. 128 inputs (0.05 s .. 2.4 s of dense oracle each): every shape in every
# field, and over each shape's rows every op pattern and every input pattern
LARGER = [(5, 1), (4, 2), (6, 1), (5, 2), (7, 1), (6, 2)]
PAIRS = [("random", "random"), ("add", "ones"), ("mul", "last"), ("mul_ends", "pm1"), ("random", "zeros"),
         ("mul", "random"), ("add", "pm1"), ("mul_ends", "last")]


def _larger_cases():
    out = []
    for s, (depth, out_gates) in enumerate(LARGER):
        per_field = 3 if depth + out_gates <= 6 else 1  # 32 inputs: three pairs per field; above: one
        k = 0
        for field in FIELDS:
            for _ in range(per_field):
                ops, kind = PAIRS[(3 * s + k) % len(PAIRS)]
                k += 1
                out.append(pytest.param(field, depth, out_gates, ops, kind, id=f"f{field}-d{depth}x{out_gates}-{ops}-{kind}"))
    return out


@pytest.mark.parametrize("field,depth,out_gates,ops,kind", _larger_cases())
def test_model_equals_dense_oracle_larger(field, depth, out_gates, ops, kind):
    _same_as_dense(field, depth, out_gates, ops, kind)


def test_larger_cases_cover_every_pattern():
    seen_ops, seen_kinds = set(), set()
    for c in _larger_cases():
        seen_ops.add(c.values[3])
        seen_kinds.add(c.values[4])
    assert seen_ops == set(gm.OP_KINDS) and seen_kinds == set(IN_KINDS)


# ---------------------------------------------------------------------------
# the library's host verifier against the model at the documented limit
# ---------------------------------------------------------------------------
def _to_lib(field: int, proof: dict) -> GkrCircuitProof:
    polys = [[UnivariatePoly(list(q), field) for q in layer] for layer in proof["proof_polynomials"]]
    return GkrCircuitProof(list(proof["output_poly"]), polys, [tuple(c) for c in proof["claimed_evaluations"]],
                           tuple(proof["input_evaluations"]), [])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["C14", "C13x2"])
def test_host_verifier_accepts_model_and_rejects_tampering(name, field):
    p = go.MODULI[field]
    structure = gm.named_circuit(name)
    ins = gm.inputs(field, 1 << 14, "random")
    assert 2 * len(structure[0]) == 1 << 14
    model = gm.proof(field, structure, ins)
    circ = Circuit([[OPS[o] for o in layer] for layer in structure], field)
    assert verify(_to_lib(field, model), circ, list(ins))
    assert verify(_to_lib(field, model), circ)
    mid = len(structure) // 2  # (in processing order; its polynomials are not trimmed: random inputs)
    t = _to_lib(field, model)  # one round coefficient
    c = t.proof_polynomials[mid][3].coefficient
    c[1] = (c[1] + 1) % p
    assert not verify(t, circ, list(ins)) and not verify(t, circ)
    t = _to_lib(field, model)  # one claim
    o1, o2 = t.claimed_evaluations[mid]
    t.claimed_evaluations[mid] = (o1, (o2 + 1) % p)
    assert not verify(t, circ, list(ins)) and not verify(t, circ)
    t = _to_lib(field, model)  # one input evaluation
    t.input_evaluations = (t.input_evaluations[0], (t.input_evaluations[1] + 1) % p)
    assert not verify(t, circ, list(ins)) and not verify(t, circ)
    flipped = [list(layer) for layer in circ.layers]  # one gate's op, in a layer of 2^7 (C13x2: 2^8) gates
    g = len(flipped[6]) - 3
    flipped[6][g] = Operation.Mul if flipped[6][g] == Operation.Add else Operation.Add
    assert not verify(_to_lib(field, model), Circuit(flipped, field), list(ins))
    assert not verify(_to_lib(field, model), Circuit(flipped, field))


# ---------------------------------------------------------------------------
# the named cases are what they are for
# ---------------------------------------------------------------------------
def test_named_circuits_have_their_shapes():
    for name, (depth, out_gates) in gm.CIRCUITS.items():
        s = gm.named_circuit(name)
        assert [len(layer) for layer in s] == [out_gates << (depth - 1 - i) for i in range(depth)]
        assert {op for layer in s[:-1] for op in layer} == {go.ADD, go.MUL}
    for layer in gm.circuit(12, 1, "mul_ends"):
        G = len(layer)
        assert [g for g in range(G) if layer[g] == go.MUL] == sorted({0, G - 1})
    assert {op for layer in gm.circuit(12, 1, "add") for op in layer} == {go.ADD}
    assert {op for layer in gm.circuit(12, 1, "mul") for op in layer} == {go.MUL}
    assert gm.named_circuit("C12") is gm.named_circuit("C12")  # built once


@pytest.mark.parametrize("field", [0, 2])
def test_zero_inputs_trim_every_round_to_empty(field):
    model = gm.proof(field, gm.named_circuit("C12"), gm.inputs(field, 1 << 12, "zeros"))
    assert [len(layer) for layer in model["proof_polynomials"]] == [2 * (k + 1) for k in range(12)]
    assert all(list(q) == [] for layer in model["proof_polynomials"] for q in layer)
    assert model["output_poly"] == [0, 0] and model["input_evaluations"] == (0, 0)


@pytest.mark.parametrize("field", [0, 2])
def test_all_mul_with_one_zero_input_kills_one_path(field):
    """One zero among nonzero inputs under Mul gates only: a product of
    nonzero field elements is nonzero, so in every layer exactly the gate above
    the zero is 0 (index ONE_ZERO_AT >> (l + 1)), up to the output."""
    p = go.MODULI[field]
    structure = gm.circuit(12, 1, "mul")
    ins = gm.inputs(field, 1 << 12, "one_zero")
    assert [i for i, v in enumerate(ins) if v == 0] == [gm.ONE_ZERO_AT]
    values = go.circuit_evaluate(p, [list(layer) for layer in structure], list(ins))
    for l, layer in enumerate(values):
        assert [g for g, v in enumerate(layer) if v == 0] == [gm.ONE_ZERO_AT >> (l + 1)], l
    model = gm.proof(field, structure, ins)
    assert model["output_poly"] == [0, 0]
    assert any(list(q) for layer in model["proof_polynomials"] for q in layer)  # (the proof itself is not trivial)


@pytest.mark.parametrize("field", FIELDS)
def test_special_inputs_are_the_saturating_words(field):
    p = go.MODULI[field]
    n = 1 << 12
    words = gm.special_words(field, n)
    s = xt.specials(field)
    assert set(words) == {0, 1, p - 1, s["sat+"], s["sat-"]} and all(w < p for w in words)
    assert list(words[:7]) == xt.special_list(field)
    ins = gm.inputs(field, n, "special")
    assert list(ins) == [xt.canonical(field, w) for w in words]
    assert all(xt.montgomery(field, v) == w for v, w in zip(ins[:14], words[:14]))
    # every pair of neighbours (a gate's two inputs) occurs: 7 is odd, so the pairs (2g, 2g+1) cycle through all 7 offsets
    assert {(words[2 * g], words[2 * g + 1]) for g in range(n // 2)} == {(words[i], words[i + 1]) for i in range(7)}

"""The tree verifier (zk_gkr_circuit_verify) and the wired verifier
(zk_gkr_wired_verify) are one layer loop over two wirings (csrc/gkr_layers.hpp),
and every sum-check verifier checks its rounds through one function
(csrc/composed_plan.hpp verify_rounds). On the model's proofs of tree circuits
(tests/gkr_circuit_model.py) both verifiers give the same answer: accept, reject
each tampering of test_wired_cpu.py::test_host_verifier_rejects_tampering (a
round coefficient, a claimed evaluation where the circuit has an inner layer, an
input evaluation, an input), raise ZK_EINVAL at a round with four coefficients
that they reach, and plainly reject when an earlier round fails first — as
zk_gkr_sumcheck_verify does. No device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gkr_circuit_model as gm
import gkr_oracle as go

from zk_amd import Transcript, UnivariatePoly
from zk_amd._lib import ZK_EINVAL, ZK_OK, lib
from zk_amd.context import REPR_CANONICAL
from zk_amd.elems import as_limbs, ptr
from zk_amd.gkr import Circuit, GkrCircuitProof, Operation, WiredCircuit, verify

TOO_LONG = "round polynomial has more than 3 coefficients"
CASES = [(depth, out_gates) for depth in (1, 2, 5) for out_gates in (1, 2)]


def _case(field: int, depth: int, out_gates: int):
    structure = gm.circuit(depth, out_gates, "random", depth)
    ins = gm.inputs(field, 2 * len(structure[0]))
    tree = Circuit([[Operation.Mul if o == go.MUL else Operation.Add for o in ops] for ops in structure], field)
    return tree, WiredCircuit.from_tree(tree), list(ins), gm.proof(field, structure, ins)


def to_lib(field: int, proof: dict) -> GkrCircuitProof:
    polys = [[UnivariatePoly(list(p), field) for p in layer] for layer in proof["proof_polynomials"]]
    return GkrCircuitProof(list(proof["output_poly"]), polys, [tuple(c) for c in proof["claimed_evaluations"]],
                           tuple(proof["input_evaluations"]), [])


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("depth,out_gates", CASES)
def test_both_verifiers_accept_and_reject_alike(field, depth, out_gates):
    tree, wired, ins, model = _case(field, depth, out_gates)
    p = go.MODULI[field]
    for circ in (tree, wired):
        assert verify(to_lib(field, model), circ, ins)
        assert verify(to_lib(field, model), circ)
        t = to_lib(field, model)  # a round coefficient
        t.proof_polynomials[-1][0].coefficient[0] = (t.proof_polynomials[-1][0].coefficient[0] + 1) % p
        assert not verify(t, circ, ins)
        if depth > 1:  # a claimed evaluation (a one-layer circuit has none)
            t = to_lib(field, model)
            o1, o2 = t.claimed_evaluations[0]
            t.claimed_evaluations[0] = (o1, (o2 + 1) % p)
            assert not verify(t, circ, ins)
        t = to_lib(field, model)  # an input evaluation
        t.input_evaluations = ((t.input_evaluations[0] + 1) % p, t.input_evaluations[1])
        assert not verify(t, circ, ins)
        assert not verify(t, circ)
        bad = list(ins)  # an input
        bad[-1] = (bad[-1] + 1) % p
        assert not verify(to_lib(field, model), circ, bad)


def _proof_arrays(model: dict):
    flat = [list(q) for layer in model["proof_polynomials"] for q in layer]
    coeffs = np.zeros((len(flat), 3, 4), np.uint64)
    nco = np.zeros(len(flat), np.uint8)
    for k, q in enumerate(flat):
        nco[k] = len(q)
        if q:
            coeffs[k, : len(q)] = as_limbs(q)
    cl = [v for pair in model["claimed_evaluations"] for v in pair]
    claims = as_limbs(cl) if cl else np.zeros((1, 4), np.uint64)
    return coeffs, nco, claims, as_limbs(list(model["output_poly"])), as_limbs(list(model["input_evaluations"]))


def _answer(rc: int, ok: C.c_int):
    return rc, ok.value, lib().zk_last_error().decode() if rc != ZK_OK else ""


def _tree_verify(tree, ins, coeffs, nco, claims, outp, inev):
    gates, ops = tree._abi()
    ok = C.c_int(-1)
    rc = lib().zk_gkr_circuit_verify(int(tree.field), REPR_CANONICAL, len(gates), ptr(gates), ptr(ops),
                                     ptr(as_limbs(ins)), len(ins), ptr(outp), ptr(coeffs), ptr(nco), ptr(claims),
                                     ptr(inev), C.byref(ok))
    return _answer(rc, ok)


def _wired_verify(wired, ins, coeffs, nco, claims, outp, inev):
    ok = C.c_int(-1)
    rc = lib().zk_gkr_wired_verify(int(wired.field), REPR_CANONICAL, len(wired.gates), ptr(wired.gates),
                                   ptr(wired.ops), ptr(wired.left), ptr(wired.right), wired.ninputs,
                                   ptr(as_limbs(ins)), ptr(outp), ptr(coeffs), ptr(nco), ptr(claims), ptr(inev),
                                   C.byref(ok))
    return _answer(rc, ok)


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("depth,out_gates", CASES)
def test_four_coefficients_in_a_layer_round(field, depth, out_gates):
    """Coefficients are validated round by round: the last round claiming four
    coefficients is ZK_EINVAL once every round before it has passed, and is
    never looked at once round 0 has failed (verified = 0, ZK_OK)."""
    tree, wired, ins, model = _case(field, depth, out_gates)
    for call, circ in ((_tree_verify, tree), (_wired_verify, wired)):
        coeffs, nco, claims, outp, inev = _proof_arrays(model)
        assert call(circ, ins, coeffs, nco, claims, outp, inev) == (ZK_OK, 1, "")
        nco[-1] = 4
        assert call(circ, ins, coeffs, nco, claims, outp, inev) == (ZK_EINVAL, -1, TOO_LONG)
        coeffs[0, 0, 0] ^= np.uint64(1)  # round 0 no longer sums to the claim
        assert call(circ, ins, coeffs, nco, claims, outp, inev) == (ZK_OK, 0, "")


@pytest.mark.parametrize("field", [0, 1, 2])
def test_four_coefficients_in_a_sumcheck_round(field):
    """zk_gkr_sumcheck_verify on two rounds: s_0 = 3 + 4x against the claim
    s_0(0) + s_0(1) = 10, then a round claiming four coefficients."""
    coeffs = np.zeros((2, 3, 4), np.uint64)
    coeffs[0, :2] = as_limbs([3, 4])
    nco = np.array([2, 4], np.uint8)

    def call(claim: int):
        ok = C.c_int(-1)
        fin = np.full((1, 4), 7, np.uint64)
        ch = np.full((2, 4), 7, np.uint64)
        t = Transcript(field)
        rc = lib().zk_gkr_sumcheck_verify(field, REPR_CANONICAL, ptr(coeffs), ptr(nco), 2, ptr(as_limbs([claim])),
                                          t.h, C.byref(ok), ptr(fin), ptr(ch))
        return _answer(rc, ok), fin, ch

    assert call(10)[0] == (ZK_EINVAL, -1, TOO_LONG)
    ans, fin, ch = call(11)  # round 0 fails first: a plain rejection, zero final claim and one zero challenge
    assert ans == (ZK_OK, 0, "")
    assert not fin.any() and not ch[0].any()

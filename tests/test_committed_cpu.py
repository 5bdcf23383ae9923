"""The committed sum-check without a GPU: the library's host-only
verifiers, zk_kzg_batch_verify and zk_committed_sumcheck_verify, on proofs the
Python model (tests/committed_oracle.py) makes — accepted for every shape of the
issue at n = 1, 2, 3, rejected for every kind of damage — zk_mle_eq_eval against
the model on all fields, and every error path with nothing written."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import committed_cases as cc
import committed_oracle as mo
import kzg_oracle as ko
import pyoracle as po

import zk_amd
from zk_amd import _lib
from zk_amd._lib import ZK_EINVAL, ZK_EUNSUPPORTED, ZK_OK
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import KZG, _g1_array, _g2_array

R = mo.R


def test_model_accepts_its_own_proof_and_rejects_a_changed_evaluation():
    """the one pairing check in pure Python (slow): n = 1, the zero-check"""
    proof, factors, claim = cc.model_proof("zero_check", 1)
    g2 = cc.setup(1)[1]
    ok, chal = mo.verify(proof, factors, claim, g2, mo.Transcript(2))
    assert ok and chal == proof["challenges"]
    idx = mo.committed_indices(proof["mask"], 6)
    vals = [proof["table_evals"][i] for i in idx]
    vals[0] = (vals[0] + 1) % R
    assert not mo.batch_verify(proof["commitments"], proof["rho"], vals, proof["opening"], proof["challenges"], g2)


@pytest.mark.parametrize("nvars", [1, 2, 3])
@pytest.mark.parametrize("name", cc.SHAPES)
def test_verifiers_accept_model_proofs(name, nvars):
    proof, factors, claim = cc.model_proof(name, nvars)
    g2 = cc.setup(nvars)[1]
    idx = mo.committed_indices(proof["mask"], len(proof["table_evals"]))
    if name == "three_zero":
        assert proof["commitments"][2] is None  # the all-zero table commits to infinity
    if name == "same_pointer":
        assert proof["commitments"][0] == proof["commitments"][1]
    assert KZG.batch_verify(proof["commitments"], proof["rho"], [proof["table_evals"][i] for i in idx],
                            proof["opening"], proof["challenges"], g2)
    rc, ok, chal, _ = cc.verify_raw(proof, factors, claim, g2)
    assert (rc, ok) == (ZK_OK, 1) and chal == proof["challenges"]


def test_batch_verify_of_one_table_is_verify_whatever_rho():
    proof, _, _ = cc.model_proof("one", 2)
    g2 = cc.setup(2)[1]
    v = proof["table_evals"][:1]
    assert KZG.verify(proof["commitments"][0], v[0], proof["opening"], proof["challenges"], g2)
    for rho in (0, 1, 12345, R - 1):
        assert KZG.batch_verify(proof["commitments"], rho, v, proof["opening"], proof["challenges"], g2)


@pytest.mark.parametrize("damage", sorted(cc.TAMPERINGS))
@pytest.mark.parametrize("name,nvars", [("three_zero", 2), ("zero_check", 3)])
def test_damaged_proofs_are_rejected(name, nvars, damage):
    proof, factors, claim = cc.model_proof(name, nvars)
    g2 = cc.setup(nvars)[1]
    cc.TAMPERINGS[damage](proof)
    rc, ok, _, _ = cc.verify_raw(proof, factors, claim, g2)
    assert (rc, ok) == (ZK_OK, 0), damage


@pytest.mark.parametrize("name,nvars", [("three_zero", 2), ("zero_check", 3)])
def test_a_transcript_that_absorbed_other_bytes_first_rejects(name, nvars):
    proof, factors, claim = cc.model_proof(name, nvars)
    g2 = cc.setup(nvars)[1]
    assert cc.verify_raw(proof, factors, claim, g2)[:2] == (ZK_OK, 1)
    assert cc.verify_raw(proof, factors, claim, g2, pre=cc.PRE_BYTES)[:2] == (ZK_OK, 0)


def test_wrong_setup_and_wrong_claim_reject():
    proof, factors, claim = cc.model_proof("zero_check", 2)
    assert claim == 0
    assert cc.verify_raw(proof, factors, 1, cc.setup(2)[1])[:2] == (ZK_OK, 0)
    other = list(reversed(cc.setup(2)[1]))
    assert cc.verify_raw(proof, factors, claim, other)[:2] == (ZK_OK, 0)


def test_batch_verify_rejects_damage():
    proof, _, _ = cc.model_proof("three_zero", 2)
    g2 = cc.setup(2)[1]
    cm, rho, vals, op, pt = proof["commitments"], proof["rho"], proof["table_evals"], proof["opening"], proof["challenges"]
    assert KZG.batch_verify(cm, rho, vals, op, pt, g2)
    assert not KZG.batch_verify([cc.another_point(cm[0])] + cm[1:], rho, vals, op, pt, g2)
    assert not KZG.batch_verify([cm[1], cm[0], cm[2]], rho, vals, op, pt, g2)
    assert not KZG.batch_verify(cm, (rho + 1) % R, vals, op, pt, g2)
    assert not KZG.batch_verify(cm, rho, [vals[0], (vals[1] + 1) % R, vals[2]], op, pt, g2)
    assert not KZG.batch_verify(cm, rho, vals, [op[0], cc.another_point(op[1])], pt, g2)
    assert not KZG.batch_verify(cm, rho, vals, op, [pt[0], (pt[1] + 1) % R], g2)


# ---- zk_mle_eq_eval ------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 1, 2])
def test_eq_eval_matches_the_model(field):
    p = po.MODULI[field]
    rng = random.Random(60 + field)
    assert zk_amd.MultilinearPoly.eq_eval([], [], field) == 1
    for n in range(1, 7):
        a = [rng.randrange(p) for _ in range(n)]
        b = [rng.randrange(p) for _ in range(n)]
        assert zk_amd.MultilinearPoly.eq_eval(a, b, field) == mo.eq_eval(p, a, b)
    a = [0, 1, p - 1, rng.randrange(p)]
    table = mo.eq_table(p, a)
    for j in range(16):  # at a hypercube point it is the table's entry, MSB first
        bits = [(j >> (3 - k)) & 1 for k in range(4)]
        assert zk_amd.MultilinearPoly.eq_eval(a, bits, field) == table[j]
    assert table == [po.evaluate(p, [int(i == j) for i in range(16)], a) for j in range(16)]


def test_model_lincomb_and_eq_table():
    p = po.MODULI[0]
    assert mo.lincomb(p, [[1, 2], [3, 4]], [p - 1, 2], 5) == [(5 - 1 + 6) % p, (5 - 2 + 8) % p]
    assert mo.eq_table(p, []) == [1]
    assert sum(mo.eq_table(p, [3, 5, 7])) % p == 1


# ---- error paths: the code, and nothing written --------------------------------
def _eq_eval_raw(field, repr_, a, b, n, null=()):
    out = np.full((1, 4), cc.SENTINEL, np.uint64)
    args = {"a": ptr(as_limbs(a)), "b": ptr(as_limbs(b)), "out": ptr(out)}
    for name in null:
        args[name] = None
    rc = _lib.lib().zk_mle_eq_eval(field, repr_, args["a"], args["b"], n, args["out"])
    return rc, bool((out == cc.SENTINEL).all())


def test_eq_eval_error_paths_write_nothing():
    p = po.MODULI[0]
    assert _eq_eval_raw(0, 0, [1, 2], [3, 4], 2) == (ZK_OK, False)
    assert _eq_eval_raw(0, 0, [1, 2], [3, 4], 0, null=("a", "b")) == (ZK_OK, False)
    for null in ("a", "b", "out"):
        assert _eq_eval_raw(0, 0, [1, 2], [3, 4], 2, null=(null,)) == (ZK_EINVAL, True), null
    assert _eq_eval_raw(3, 0, [1, 2], [3, 4], 2) == (ZK_EINVAL, True)
    assert _eq_eval_raw(0, 2, [1, 2], [3, 4], 2) == (ZK_EINVAL, True)
    assert _eq_eval_raw(0, 0, [1, p], [3, 4], 2) == (ZK_EINVAL, True)
    assert _eq_eval_raw(0, 0, [1, 2], [p, 4], 2) == (ZK_EINVAL, True)


def _batch_verify_raw(proof, g2, repr_=0, ntables=None, rho=None, nproof=None, npoint=None, commitments=None, null=()):
    ok = C.c_int(77)
    idx = mo.committed_indices(proof["mask"], len(proof["table_evals"]))
    cm = proof["commitments"] if commitments is None else commitments
    args = {"cm": ptr(cm if isinstance(cm, np.ndarray) else _g1_array(cm)),
            "rho": ptr(as_limbs([proof["rho"] if rho is None else rho])),
            "vals": ptr(as_limbs([proof["table_evals"][i] for i in idx])), "proof": ptr(_g1_array(proof["opening"])),
            "point": ptr(as_limbs(proof["challenges"])), "g2": ptr(_g2_array(list(g2))), "ok": C.byref(ok)}
    for name in null:
        args[name] = None
    n = len(proof["challenges"])
    rc = _lib.lib().zk_kzg_batch_verify(repr_, args["cm"], len(idx) if ntables is None else ntables, args["rho"],
                                        args["vals"], args["proof"], n if nproof is None else nproof, args["point"],
                                        n if npoint is None else npoint, args["g2"], args["ok"])
    return rc, ok.value == 77


def test_batch_verify_error_paths_write_nothing():
    proof, _, _ = cc.model_proof("three_zero", 2)
    g2 = cc.setup(2)[1]
    assert _batch_verify_raw(proof, g2) == (ZK_OK, False)
    for null in ("cm", "rho", "vals", "proof", "point", "g2", "ok"):
        assert _batch_verify_raw(proof, g2, null=(null,)) == (ZK_EINVAL, True), null
    assert _batch_verify_raw(proof, g2, ntables=0) == (ZK_EINVAL, True)
    assert _batch_verify_raw(proof, g2, ntables=17) == (ZK_EUNSUPPORTED, True)
    assert _batch_verify_raw(proof, g2, nproof=1) == (ZK_EINVAL, True)   # nproof != npoint
    assert _batch_verify_raw(proof, g2, repr_=2) == (ZK_EINVAL, True)
    assert _batch_verify_raw(proof, g2, rho=R) == (ZK_EINVAL, True)      # rho >= p
    off = _g1_array(proof["commitments"])
    off[0, 6] ^= np.uint64(1)                                             # y changed: not on the curve
    assert _batch_verify_raw(proof, g2, commitments=off) == (ZK_EINVAL, True)


def test_committed_verify_error_paths_write_nothing():
    proof, factors, claim = cc.model_proof("zero_check", 2)
    g2 = cc.setup(2)[1]
    assert cc.verify_raw(proof, factors, claim, g2)[:2] == (ZK_OK, 1)

    def code(**kw):
        rc, _, _, untouched = cc.verify_raw(proof, factors, claim, g2, **kw)
        return rc, untouched

    for null in ("coeffs", "ncoeffs", "claim", "factors", "evals", "commitments", "opening", "g2", "t", "ok", "ch"):
        assert code(null=(null,)) == (ZK_EINVAL, True), null
    assert code(mask=0) == (ZK_EINVAL, True)                 # nothing committed
    assert code(mask=proof["mask"] | 1 << 6) == (ZK_EINVAL, True)  # a bit at ntables
    assert code(mask=1 << 31) == (ZK_EINVAL, True)
    assert code(nrounds=0) == (ZK_EINVAL, True)              # KZG needs a variable
    assert code(repr_=2) == (ZK_EINVAL, True)
    assert code(ntables=17) == (ZK_EUNSUPPORTED, True)       # the composed caps, unchanged
    assert code(ntables=2) == (ZK_EINVAL, True)              # a factor names a table >= ntables
    bad = dict(proof, table_evals=[R] + proof["table_evals"][1:])
    assert cc.verify_raw(bad, factors, claim, g2)[0::3] == (ZK_EINVAL, True)   # an evaluation >= p
    bad = dict(proof, commitments=[(proof["commitments"][0][0], 1)] + proof["commitments"][1:])
    assert cc.verify_raw(bad, factors, claim, g2)[0::3] == (ZK_EINVAL, True)   # a commitment off the curve
    bad = dict(proof, opening=[proof["opening"][0], (5, 5)])
    assert cc.verify_raw(bad, factors, claim, g2)[0::3] == (ZK_EINVAL, True)   # a quotient off the curve
    assert cc.verify_raw(proof, factors, R, g2)[0::3] == (ZK_EINVAL, True)     # claimed sum >= p


def test_python_surface():
    assert zk_amd.committed_prove and zk_amd.committed_verify and zk_amd.CommittedProof
    for name in ("commit_batch", "batch_open", "batch_open_device", "batch_verify"):
        assert hasattr(KZG, name)
    assert hasattr(zk_amd.DeviceTable, "lincomb") and hasattr(zk_amd.MultilinearPoly, "eq")
    assert ko.on_curve(cc.another_point(ko.G1))

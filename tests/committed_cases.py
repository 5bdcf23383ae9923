"""Shapes, model proofs and raw C-ABI calls the committed sum-check's CPU and GPU
tests share (test helper, not a test module). Model proofs are made once per
(shape, nvars) and never changed: a test that damages one works on a copy."""
from __future__ import annotations

import copy
import ctypes as C
import functools

import numpy as np

import committed_oracle as mo
import composed_oracle as cm
import kzg_oracle as ko
import pairing_oracle as pg

from zk_amd import _lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import _g1_array, _g2_array, _points

R = mo.R
SENTINEL = 0xA5A5A5A5A5A5A5A5


def taus(nvars: int) -> list[int]:
    return [5, 2, 3, 11, 7, 13, 17, 19, 23, 29, 31, 37, 41, 43][:nvars]


@functools.lru_cache(maxsize=None)
def setup(nvars: int):
    """(Lagrange basis in G1, G2 taus) of the model's setup"""
    return ko.get_lagrange_basis(taus(nvars)), pg.g2_taus(taus(nvars))


def shape(name: str, nvars: int):
    """-> (tables, factors, committed mask, same-pointer groups): the shapes of the issue"""
    N = 1 << nvars
    if name == "one":  # one committed table
        return cm.random_tables(2, 1, nvars, 11 + nvars), [[0]], 0b1
    if name == "three_zero":  # three committed tables, the last all zero: its commitment is infinity
        a, b = cm.random_tables(2, 2, nvars, 21 + nvars)
        return [a, b, [0] * N], [[0, 1], [1, 2], [2, 0]], 0b111
    if name == "zero_check":  # eq a b + neq c one, a b c committed
        tabs, _ = mo.zero_check_tables(nvars, 31 + nvars)
        return tabs, mo.ZERO_CHECK_FACTORS, mo.ZERO_CHECK_MASK
    if name == "same_pointer":  # tables 0 and 1 are one table, both committed; table 2 public
        a, b = cm.random_tables(2, 2, nvars, 41 + nvars)
        return [a, a, b], [[0, 1], [2, 2]], 0b011
    raise KeyError(name)


SHAPES = ("one", "three_zero", "zero_check", "same_pointer")


@functools.lru_cache(maxsize=None)
def _model_proof(name: str, nvars: int):
    tables, factors, mask = shape(name, nvars)
    claim = cm.true_sum(R, tables, factors)
    return mo.prove(tables, factors, mask, claim, setup(nvars)[0], mo.Transcript(2)), claim


def model_proof(name: str, nvars: int):
    """-> (proof dict (a fresh copy), factors, claimed sum)"""
    proof, claim = _model_proof(name, nvars)
    return copy.deepcopy(proof), shape(name, nvars)[1], claim


def verify_raw(proof: dict, factors, claimed_sum: int, g2_taus, pre: bytes = b"", repr_: int = 0, null=(), mask=None,
               nrounds=None, ntables=None):
    """zk_committed_sumcheck_verify on a model-shaped proof -> (rc, verified,
    challenges, outputs untouched). `pre`: bytes the verifier's transcript
    absorbed beforehand."""
    L = _lib.lib()
    degree = len(factors[0])
    n = len(proof["polys"]) if nrounds is None else nrounds
    coeffs = np.zeros((max(n, 1), degree + 1, 4), np.uint64)
    nco = np.zeros(max(n, 1), np.uint8)
    for k, q in enumerate(proof["polys"][:n]):
        nco[k] = len(q)
        if q:
            coeffs[k, : len(q)] = as_limbs(list(q))
    t = L.zk_transcript_new()
    if pre:
        L.zk_transcript_append(t, (C.c_uint8 * len(pre)).from_buffer_copy(pre), len(pre))
    ok = C.c_int(77)
    ch = np.full((max(n, 1), 4), SENTINEL, np.uint64)
    fac = np.array(factors, np.uint8).reshape(-1)
    args = {"coeffs": ptr(coeffs), "ncoeffs": ptr(nco), "claim": ptr(as_limbs([claimed_sum])), "factors": ptr(fac),
            "evals": ptr(as_limbs(list(proof["table_evals"]))), "commitments": ptr(_g1_array(proof["commitments"])),
            "opening": ptr(_g1_array(proof["opening"])), "g2": ptr(_g2_array(list(g2_taus))), "t": t,
            "ok": C.byref(ok), "ch": ptr(ch)}
    for name in null:
        args[name] = None
    rc = L.zk_committed_sumcheck_verify(repr_, degree, args["coeffs"], args["ncoeffs"], n, args["claim"],
                                        args["factors"], len(factors),
                                        len(proof["table_evals"]) if ntables is None else ntables, args["evals"],
                                        proof["mask"] if mask is None else mask, args["commitments"], args["opening"],
                                        args["g2"], args["t"], args["ok"], args["ch"])
    L.zk_transcript_free(t)
    untouched = ok.value == 77 and bool((ch == SENTINEL).all())
    return rc, ok.value, (to_ints(ch[:n]) if rc == 0 and ok.value == 1 else None), untouched


def another_point(P):
    """a valid G1 point different from P"""
    return ko.add(P, ko.G1)


# Every way the issue lists of damaging a proof: name -> (proof -> None, in place)
def _change_commitment(p):
    p["commitments"][0] = another_point(p["commitments"][0])


def _swap_commitments(p):
    c = p["commitments"]
    j = next(j for j in range(1, len(c)) if c[j] != c[0])
    c[0], c[j] = c[j], c[0]


def _change_eval(p):
    i = mo.committed_indices(p["mask"], len(p["table_evals"]))[-1]
    p["table_evals"][i] = (p["table_evals"][i] + 1) % R


def _change_quotient(p):
    p["opening"][-1] = another_point(p["opening"][-1])


def _change_coefficient(p):
    q = p["polys"][0]
    if q:
        q[0] = (q[0] + 1) % R
    else:
        q.append(1)


TAMPERINGS = {"commitment": _change_commitment, "swap": _swap_commitments, "eval": _change_eval,
              "quotient": _change_quotient, "coefficient": _change_coefficient}
PRE_BYTES = b"other bytes absorbed first"


def points_from(arr: np.ndarray) -> list:
    return _points(arr)

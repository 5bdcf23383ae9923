"""Sum-check over KZG-committed tables with one batched opening:
composed_prove / composed_verify with the committed tables' evaluations tied to
their commitments (zk_committed_sumcheck_prove / _verify). BLS12-381 Fr."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import lib
from .api import Field, MultilinearPoly, SumPoly, Transcript, UnivariatePoly, _call, _factor_array, default_context
from .context import REPR_CANONICAL, Context
from .elems import as_limbs, one, ptr, to_ints
from .kzg import KZG, _g1_array, _g2_array, _points

FIELD = Field.BLS12_381_FR


@dataclass
class CommittedProof:
    proof_polynomials: list[UnivariatePoly]
    claimed_sum: int
    random_challenges: list[int]
    table_evals: list[int]  # every distinct table at the challenge point (SumPoly.composed_tables order)
    committed_mask: int     # bit i: table i is committed
    commitments: list       # the committed tables' commitments, table-index order
    opening: list           # one batched opening: nvars quotient commitments


@dataclass
class CommittedVerify:
    verified: bool
    random_challenges: list[int]


def _mask(committed, tables: list, sum_poly: SumPoly) -> int:
    """`committed`: an integer mask, or the committed tables as indices into
    SumPoly.composed_tables() or as the MultilinearPoly objects themselves."""
    if isinstance(committed, int):
        return committed
    index = {}
    for pp in sum_poly.polys:
        for mle in pp.evaluation:
            index.setdefault(id(mle), len(index))
    mask = 0
    for item in committed:
        i = index[id(item)] if isinstance(item, MultilinearPoly) else int(item)
        if not 0 <= i < len(tables):
            raise ValueError("a committed table is not one of the polynomial's tables")
        mask |= 1 << i
    return mask


def committed_prove(claimed_sum: int, sum_poly: SumPoly, transcript: Transcript, kzg: KZG, committed,
                    commitments: list | None = None, ctx: Context | None = None) -> CommittedProof:
    """composed_prove over `sum_poly` with the tables named by `committed`
    committed under `kzg` and opened, all at once, at the challenge point.
    `commitments` (table-index order) reuses commitments made earlier."""
    if int(sum_poly.field) != int(FIELD):
        raise ValueError("committed tables are BLS12-381 Fr")
    tables, factors = sum_poly.composed_tables()
    fac, nterms, degree = _factor_array(factors)
    mask = _mask(committed, tables, sum_poly)
    nc = bin(mask).count("1")
    if commitments is not None and len(commitments) != nc:
        raise ValueError("one commitment per committed table")
    ctx = ctx or kzg.ctx or default_context()
    n = tables[0].shape[0].bit_length() - 1
    arr = (C.c_void_p * len(tables))(*[t.ctypes.data for t in tables])
    coeffs = np.zeros((max(n, 1), degree + 1, 4), np.uint64)
    nco = np.zeros(max(n, 1), np.uint8)
    ch = np.zeros((max(n, 1), 4), np.uint64)
    ev = np.zeros((len(tables), 4), np.uint64)
    cs = np.zeros((1, 4), np.uint64)
    cm = np.zeros((max(nc, 1), 12), np.uint64)
    op = np.zeros((max(n, 1), 12), np.uint64)
    cin = ptr(_g1_array(list(commitments))) if commitments is not None else None
    _call(lib().zk_committed_sumcheck_prove(ctx.h, kzg.h, REPR_CANONICAL, arr, len(tables), n, ptr(fac), nterms, degree,
                                            mask, cin, ptr(one(claimed_sum)), transcript.h, ptr(coeffs), ptr(nco),
                                            ptr(ch), ptr(ev), ptr(cs), ptr(cm), ptr(op)))
    polys = [UnivariatePoly(to_ints(coeffs[k, : nco[k]]), sum_poly.field) for k in range(n)]
    return CommittedProof(polys, to_ints(cs)[0], to_ints(ch[:n]), to_ints(ev), mask, _points(cm)[:nc], _points(op)[:n])


def committed_verify(proof: CommittedProof, claimed_sum: int, transcript: Transcript, factors, g2_taus: list,
                     public_tables: dict | None = None, ctx: Context | None = None) -> CommittedVerify:
    """zk_committed_sumcheck_verify, then the part it leaves to the caller: every
    public table's entry of table_evals is checked against the table itself,
    public_tables = {index: evaluations}, at the returned challenges
    (zk_mle_evaluate). Every table is either committed or in public_tables;
    g2_taus come from a setup the verifier trusts."""
    fac, nterms, degree = _factor_array(factors)
    public_tables = public_tables or {}
    ntables = len(proof.table_evals)
    for i in range(ntables):
        if not (proof.committed_mask >> i) & 1 and i not in public_tables:
            raise ValueError(f"table {i} is neither committed nor public")
    n = len(proof.proof_polynomials)
    coeffs = np.zeros((max(n, 1), degree + 1, 4), np.uint64)
    nco = np.zeros(max(n, 1), np.uint8)
    for k, rp in enumerate(proof.proof_polynomials):
        c = rp.coefficient if isinstance(rp, UnivariatePoly) else list(rp)
        nco[k] = min(len(c), 255)
        keep = c[: degree + 1]
        if keep:
            coeffs[k, : len(keep)] = as_limbs(keep)
    ok = C.c_int(0)
    ch = np.zeros((max(n, 1), 4), np.uint64)
    _call(lib().zk_committed_sumcheck_verify(REPR_CANONICAL, degree, ptr(coeffs), ptr(nco), n, ptr(one(claimed_sum)),
                                             ptr(fac), nterms, ntables, ptr(as_limbs(list(proof.table_evals))),
                                             proof.committed_mask, ptr(_g1_array(list(proof.commitments))),
                                             ptr(_g1_array(list(proof.opening))), ptr(_g2_array(list(g2_taus)[:n])),
                                             transcript.h, C.byref(ok), ptr(ch)))
    if not ok.value:
        return CommittedVerify(False, [0])
    chal = to_ints(ch[:n])
    for i, evals in public_tables.items():
        if MultilinearPoly(evals, FIELD, ctx).evaluate(chal) != proof.table_evals[i]:
            return CommittedVerify(False, chal)
    return CommittedVerify(True, chal)

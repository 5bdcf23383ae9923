"""Model of the committed sum-check in Python integers, composed
of oracle/kzg_oracle.py, oracle/pairing_oracle.py, pyoracle.Transcript and
tests/composed_oracle.py.

TEST INFRASTRUCTURE ONLY. Tables are BLS12-381 Fr. The transcript: for each
committed table in index order the 96 bytes of its commitment (x then y, 48
bytes little-endian each, infinity all zero); the composed sum-check; the bytes
of every table's evaluation, then rho; committed table j (index order) weighted
by rho^j and one get_proof of the combination at the challenges. Pairing checks
(batch_verify, verify) are slow in Python: keep them at n <= 3.
"""
from __future__ import annotations

import composed_oracle as cm
import kzg_oracle as ko
import pairing_oracle as pg
from pyoracle import MODULI, Transcript, fq_vec_to_bytes

FIELD = 2
R = MODULI[FIELD]


def eq_table(p: int, point: list[int]) -> list[int]:
    """entry j = eq(point, bits of j), bit n-1-k of j against point[k] (MSB first)"""
    t = [1]
    for r in point:
        t = [v for x in t for v in ((x - x * r) % p, x * r % p)]
    return t


def eq_eval(p: int, a: list[int], b: list[int]) -> int:
    e = 1
    for x, y in zip(a, b):
        e = e * (x * y + (1 - x) * (1 - y)) % p
    return e


def lincomb(p: int, tables, coeffs, constant: int = 0) -> list[int]:
    return [(sum(c * tb[j] for c, tb in zip(coeffs, tables)) + constant) % p for j in range(len(tables[0]))]


def g1_bytes(P) -> bytes:
    x, y = (0, 0) if P is None else P
    return x.to_bytes(48, "little") + y.to_bytes(48, "little")


def committed_indices(mask: int, ntables: int) -> list[int]:
    return [i for i in range(ntables) if (mask >> i) & 1]


def batch_open(tables, rho: int, values, point, basis) -> list:
    """get_proof(v, point, g): g = sum_j rho^j tables[j], v = sum_j rho^j values[j]"""
    pows = [pow(rho, j, R) for j in range(len(tables))]
    g = lincomb(R, tables, pows)
    v = sum(w * x for w, x in zip(pows, values)) % R
    return ko.get_proof(g, v, list(point), basis)


def batch_verify(commitments, rho: int, values, proof, point, g2_taus) -> bool:
    C = None
    v = 0
    for j, (cj, vj) in enumerate(zip(commitments, values)):
        w = pow(rho, j, R)
        C = ko.add(C, ko.mul(w, cj))
        v = (v + w * vj) % R
    return pg.verify(C, v, list(proof), list(point), list(g2_taus))


def prove(tables, factors, mask: int, claimed_sum: int, basis, t: Transcript, commitments=None) -> dict:
    idx = committed_indices(mask, len(tables))
    cms = list(commitments) if commitments is not None else [ko.commit(tables[i], basis) for i in idx]
    for c in cms:
        t.append(g1_bytes(c))
    polys, cs, chal, evals = cm.prove(FIELD, claimed_sum, tables, factors, t)
    t.append(fq_vec_to_bytes(evals))
    rho = t.get_random_challenge()
    opening = batch_open([tables[i] for i in idx], rho, [evals[i] for i in idx], chal, basis)
    return {"polys": polys, "claimed_sum": cs, "challenges": chal, "table_evals": evals, "mask": mask,
            "commitments": cms, "opening": opening, "rho": rho}


def verify(proof: dict, factors, claimed_sum: int, g2_taus, t: Transcript):
    """-> (verified, challenges); the public tables' evaluations are the caller's to check"""
    idx = committed_indices(proof["mask"], len(proof["table_evals"]))
    for c in proof["commitments"]:
        t.append(g1_bytes(c))
    ok, fin, chal = cm.verify(FIELD, proof["polys"], claimed_sum, t, len(factors[0]))
    if not ok or fin != cm.combine(R, proof["table_evals"], factors):
        return False, [0]
    t.append(fq_vec_to_bytes(proof["table_evals"]))
    rho = t.get_random_challenge()
    if not batch_verify(proof["commitments"], rho, [proof["table_evals"][i] for i in idx], proof["opening"], chal,
                        g2_taus):
        return False, [0]
    return True, chal


# The zero-check eq (a b - c) = 0 as a sum of products of one degree:
# eq a b + neq c one with neq = -eq. Tables: 0 eq, 1 a, 2 b, 3 neq, 4 c, 5 one;
# a, b and c are committed, the rest public.
ZERO_CHECK_FACTORS = [[0, 1, 2], [3, 4, 5]]
ZERO_CHECK_MASK = 0b010110
ZERO_CHECK_PUBLIC = (0, 3, 5)


def zero_check_tables(nvars: int, seed: int, point=None):
    """a, b random, c = a b, eq at `point` (default: a fixed pseudo-random one)"""
    a, b = cm.random_tables(FIELD, 2, nvars, seed)
    c = [x * y % R for x, y in zip(a, b)]
    pt = list(point) if point is not None else [pow(7 + seed, 3 + k, R) for k in range(nvars)]
    eq = eq_table(R, pt)
    return [eq, a, b, [(-x) % R for x in eq], c, [1] * (1 << nvars)], pt

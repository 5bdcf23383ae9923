"""Dense model of the composed sum-check, in Python integers on
the pieces of oracle/pyoracle.py.

TEST INFRASTRUCTURE ONLY. It restates pyoracle.gkr_prove (sum_check_protocol.rs:
86-166) with SumPoly::reduce done in full: the polynomial is
f = sum_t prod_d tables[factors[t][d]]; round k takes y_i = sum_j f_k(i, j) for
i = 0..degree with variable 0 bound to i by partial_evaluate(0, i), interpolates
through (i, y_i), trims, absorbs the coefficient bytes, draws r_k and folds
every table by it. Verify is pyoracle.gkr_verify with a degree bound; combine is
f at the tables' evaluations.
"""
from __future__ import annotations

import random

from pyoracle import MODULI, Transcript, fq_vec_to_bytes, interpolate, partial_evaluate, uni_evaluate


def round_poly(p: int, tables, factors) -> list[int]:
    degree = len(factors[0])
    ys = []
    for i in range(degree + 1):
        part = [partial_evaluate(p, tb, 0, i) for tb in tables]
        total = 0
        for term in factors:
            for j in range(len(part[0])):
                prod = 1
                for f in term:
                    prod = prod * part[f][j] % p
                total += prod
        ys.append(total % p)
    return interpolate(p, list(range(degree + 1)), ys)  # (trimmed)


def prove(field: int, claimed_sum: int, tables, factors, t: Transcript):
    """-> (round polynomials, claimed_sum, challenges, table_evals)"""
    p = MODULI[field]
    n = len(tables[0]).bit_length() - 1
    cur = [list(tb) for tb in tables]
    polys, chal = [], []
    for _ in range(n):
        rp = round_poly(p, cur, factors)
        t.append(fq_vec_to_bytes(rp))
        polys.append(rp)
        r = t.get_random_challenge()
        chal.append(r)
        cur = [partial_evaluate(p, tb, 0, r) for tb in cur]
    return polys, claimed_sum, chal, [tb[0] for tb in cur]


def verify(field: int, round_polys, claimed_sum: int, t: Transcript, degree: int):
    """-> (verified, final claim, challenges); a rejection is (False, 0, [0])"""
    p = MODULI[field]
    chal = []
    for rp in round_polys:
        if len(rp) > degree + 1:
            return False, 0, [0]
        if (uni_evaluate(p, rp, 0) + uni_evaluate(p, rp, 1)) % p != claimed_sum:
            return False, 0, [0]
        t.append(fq_vec_to_bytes(rp))
        r = t.get_random_challenge()
        chal.append(r)
        claimed_sum = uni_evaluate(p, rp, r)
    return True, claimed_sum, chal


def combine(p: int, table_evals, factors) -> int:
    total = 0
    for term in factors:
        prod = 1
        for f in term:
            prod = prod * table_evals[f] % p
        total += prod
    return total % p


def true_sum(p: int, tables, factors) -> int:
    total = 0
    for term in factors:
        for j in range(len(tables[0])):
            prod = 1
            for f in term:
                prod = prod * tables[f][j] % p
            total += prod
    return total % p


# The shapes the tests share: name -> (ntables, factors)
SHAPES = {
    "gkr4": (4, [[0, 1], [2, 3]]),                # SumPoly[ProductPoly[A, S], ProductPoly[M, P]]
    "deg1": (3, [[0], [1], [2]]),                 # a sum of three MLEs
    "deg2": (3, [[0, 1], [1, 2], [2, 0]]),
    "deg3": (3, [[0, 1, 2]]),                     # eq * a * b
    "deg3_shared": (4, [[0, 1, 2], [0, 3, 3]]),   # table 0 in both terms, table 3 twice in one
    "deg4": (5, [[0, 1, 2, 3], [4, 4, 0, 1]]),
    "repeat": (2, [[0, 0, 1]]),                   # a factor repeated within a term
    "unused1": (5, [[0, 2]]),                     # tables 1, 3 and 4 are in no term
    "unused15": (16, [[7]] * 16),                 # degree 1, 15 unused tables: the unused list is full
    "caps": (16, [[(t + d) % 16 for d in range(4)] for t in range(16)]),  # 16 tables, 16 terms, degree 4
    "caps_one_table": (16, [[3, 3, 3, 3]] * 16),  # the caps with one table named 64 times, 15 unused
}


def random_tables(field: int, ntables: int, nvars: int, seed: int):
    rng = random.Random(seed)
    p = MODULI[field]
    return [[rng.randrange(p) for _ in range(1 << nvars)] for _ in range(ntables)]

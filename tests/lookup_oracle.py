"""Model of the lookup argument in Python integers, composed of
tests/composed_oracle.py, tests/committed_oracle.py, pyoracle.Transcript and
oracle/kzg_oracle.py.

TEST INFRASTRUCTURE ONLY. f is a column of 2^n elements, t a public table of T
<= 2^n, t_pad[j] = t[min(j, T - 1)], m_j the number of column entries equal to
t_j at the first index holding that value. The transcript: the table's digest,
n, the commitments of f and m; alpha; the commitments of h_f = 1 / (alpha - f)
and h_t = m / (alpha - t_pad); tau_0 .. tau_(n-1), lambda; the committed
sum-check of claimed sum 0 over TABLES / FACTORS with the four columns
committed. 1 / 0 is 0, as the library's inversion has it. Proving and verifying
are BLS12-381 Fr; the hash, the counts and the table's evaluation take any
field. Pairing checks at n <= 3.
"""
from __future__ import annotations

import committed_oracle as mo
import kzg_oracle as ko
from pyoracle import MODULI, Transcript, evaluate, keccak256

FIELD = 2
R = MODULI[FIELD]
EMPTY = 0xFFFFFFFF
HASH_MUL = 0x9E3779B1
NTABLES = 11
HF, HT, F, M, TPAD, ONE, NEG, E0 = range(8)
MASK = 0b1111
FACTORS = [[0, 5, 5], [1, 6, 5], [7, 0, 5], [8, 0, 2], [8, 5, 5], [9, 1, 5], [10, 1, 4], [10, 3, 5]]


def slot_log(T: int) -> int:
    lg = 1
    while (1 << lg) < 2 * T:
        lg += 1
    return lg


def home(value: int, lg: int) -> int:
    """the home slot of a canonical value: a multiplicative mix of its low 32 bits"""
    return (((value & 0xFFFFFFFF) * HASH_MUL) & 0xFFFFFFFF) >> (32 - lg)


def hash_slots(table) -> list[int]:
    """linear probing in index order; a slot holds the first index of its value"""
    lg = slot_log(len(table))
    slots = [EMPTY] * (1 << lg)
    for j, v in enumerate(table):
        s = home(v, lg)
        while slots[s] != EMPTY and table[slots[s]] != v:
            s = (s + 1) & ((1 << lg) - 1)
        if slots[s] == EMPTY:
            slots[s] = j
    return slots


def multiplicities(table, f, n: int):
    """-> (m over 2^n slots, missing)"""
    first = {}
    for j, v in enumerate(table):
        first.setdefault(v, j)
    m = [0] * (1 << n)
    missing = 0
    for x in f:
        if x in first:
            m[first[x]] += 1
        else:
            missing += 1
    return m, missing


def pad(table, n: int) -> list[int]:
    return [table[min(j, len(table) - 1)] for j in range(1 << n)]


def table_eval(p: int, table, point) -> int:
    return evaluate(p, pad(table, len(point)), list(point))


def digest(field: int, table) -> bytes:
    out = b"zk-lookup-v1" + int(field).to_bytes(4, "little") + len(table).to_bytes(4, "little")
    return keccak256(out + b"".join(int(v).to_bytes(32, "little") for v in table))


def inv0(p: int, x: int) -> int:
    return pow(x, p - 2, p)  # 0 -> 0


def begin(t: Transcript, table, n: int, cm_f, cm_m) -> int:
    t.append(digest(FIELD, table))
    t.append(int(n).to_bytes(4, "little"))
    t.append(mo.g1_bytes(cm_f))
    t.append(mo.g1_bytes(cm_m))
    return t.get_random_challenge()


def draw(t: Transcript, n: int, cm_hf, cm_ht):
    t.append(mo.g1_bytes(cm_hf))
    t.append(mo.g1_bytes(cm_ht))
    tau = [t.get_random_challenge() for _ in range(n)]
    return tau, t.get_random_challenge()


def eq_scalars(alpha: int, lam: int) -> list[int]:
    return [alpha * lam % R, (-lam) % R, alpha * lam * lam % R, (-lam * lam) % R]


def tables_of(table, f, n: int, alpha: int, lam: int, tau) -> list[list[int]]:
    N = 1 << n
    m, _ = multiplicities(table, f, n)
    tp = pad(table, n)
    hf = [inv0(R, (alpha - x) % R) for x in f]
    ht = [c * inv0(R, (alpha - x) % R) % R for c, x in zip(m, tp)]
    eq = mo.eq_table(R, list(tau))
    return [hf, ht, list(f), m, tp, [1] * N, [R - 1] * N] + [[w * e % R for e in eq] for w in eq_scalars(alpha, lam)]


def prove(table, f, basis, t: Transcript, commitment=None) -> dict:
    n = len(f).bit_length() - 1
    assert len(f) == 1 << n and 1 <= len(table) <= len(f)
    m, missing = multiplicities(table, f, n)
    cm_f = commitment if commitment is not None else ko.commit(list(f), basis)
    cm_m = ko.commit(m, basis)
    alpha = begin(t, table, n, cm_f, cm_m)
    tp = pad(table, n)
    hf = [inv0(R, (alpha - x) % R) for x in f]
    ht = [c * inv0(R, (alpha - x) % R) % R for c, x in zip(m, tp)]
    cm_hf, cm_ht = ko.commit(hf, basis), ko.commit(ht, basis)
    tau, lam = draw(t, n, cm_hf, cm_ht)
    tabs = tables_of(table, f, n, alpha, lam, tau)
    inner = mo.prove(tabs, FACTORS, MASK, 0, basis, t, commitments=[cm_hf, cm_ht, cm_f, cm_m])
    return {"n": n, "polys": inner["polys"], "table_evals": inner["table_evals"], "commitments": inner["commitments"],
            "opening": inner["opening"], "missing": missing, "point": inner["challenges"], "alpha": alpha, "tau": tau,
            "lambda": lam}


def verify(table, proof: dict, g2_taus, t: Transcript):
    """-> (verified, point)"""
    n = proof["n"]
    cm_hf, cm_ht, cm_f, cm_m = proof["commitments"]
    alpha = begin(t, table, n, cm_f, cm_m)
    tau, lam = draw(t, n, cm_hf, cm_ht)
    inner = {"polys": proof["polys"], "table_evals": proof["table_evals"], "mask": MASK,
             "commitments": proof["commitments"], "opening": proof["opening"]}
    ok, point = mo.verify(inner, FACTORS, 0, g2_taus, t)
    if not ok:
        return False, []
    ev = proof["table_evals"]
    e = mo.eq_eval(R, tau, point)
    if ev[ONE] != 1 or ev[NEG] != R - 1 or ev[TPAD] != table_eval(R, table, point):
        return False, []
    if any(ev[E0 + i] != w * e % R for i, w in enumerate(eq_scalars(alpha, lam))):
        return False, []
    return True, point

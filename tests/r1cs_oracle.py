"""Model of the R1CS prover in Python integers, composed of
tests/composed_oracle.py, pyoracle.Transcript, oracle/kzg_oracle.py and
oracle/pairing_oracle.py.

TEST INFRASTRUCTURE ONLY. An instance is (A z) o (B z) = C z over z of 2^sy
entries, the first half the witness, the second half (1, io, 0 ..); A, B, C are
lists of (row, col, value) in any order, duplicates adding up. The transcript:
the digest of the instance, io, (committed) the 96 bytes of the witness'
commitment; tau; the zero-check eq(tau,.) (Az Bz - Cz) as the composed sum-check
[eq, Az, Bz, -eq, Cz, 1] / {0,1,2},{3,4,5}; (va, vb, vc), rho; M = sum_x eq(rx, x)
(A + rho B + rho^2 C)(x, .); the composed sum-check [M, z] / {0,1} with claim
va + rho vb + rho^2 vc; vw = w~(ry[1:]); (committed) get_proof(w, vw, ry[1:]).
Dense and slow: small instances only; pairing checks at sy <= 3.
"""
from __future__ import annotations

from dataclasses import dataclass

import committed_oracle as mo
import composed_oracle as cm
import kzg_oracle as ko
import pairing_oracle as pg
from pyoracle import MODULI, Transcript, evaluate, fq_vec_to_bytes, keccak256

SC1_FACTORS = [[0, 1, 2], [3, 4, 5]]
SC2_FACTORS = [[0, 1]]


@dataclass
class Instance:
    field: int
    nrows: int
    sy: int
    npub: int
    A: list
    B: list
    C: list

    @property
    def p(self) -> int:
        return MODULI[self.field]

    @property
    def sx(self) -> int:
        return max(1, (self.nrows - 1).bit_length())

    @property
    def matrices(self):
        return (self.A, self.B, self.C)


def _u32(x: int) -> bytes:
    return int(x).to_bytes(4, "little")


def digest(inst: Instance) -> bytes:
    out = b"zk-r1cs-v1" + b"".join(_u32(x) for x in (inst.field, inst.nrows, inst.sx, inst.sy, inst.npub))
    for m in inst.matrices:
        out += _u32(len(m))
        for r, c, v in m:
            out += _u32(r) + _u32(c) + int(v).to_bytes(32, "little")
    return keccak256(out)


def z_of(inst: Instance, w, io) -> list[int]:
    half = 1 << (inst.sy - 1)
    assert len(w) == half and len(io) == inst.npub and inst.npub + 1 <= half
    return list(w) + [1] + list(io) + [0] * (half - 1 - inst.npub)


def mul(inst: Instance, z) -> list[list[int]]:
    """-> [Az, Bz, Cz], 2^sx entries each"""
    p = inst.p
    out = []
    for m in inst.matrices:
        t = [0] * (1 << inst.sx)
        for r, c, v in m:
            t[r] = (t[r] + v * z[c]) % p
        out.append(t)
    return out


def is_satisfied(inst: Instance, w, io) -> bool:
    a, b, c = mul(inst, z_of(inst, w, io))
    return all(x * y % inst.p == v for x, y, v in zip(a, b, c))


def mul_t(inst: Instance, x) -> list[list[int]]:
    """-> [A^T x, B^T x, C^T x], 2^sy entries each"""
    p = inst.p
    out = []
    for m in inst.matrices:
        t = [0] * (1 << inst.sy)
        for r, c, v in m:
            t[c] = (t[c] + v * x[r]) % p
        out.append(t)
    return out


def bound_columns(inst: Instance, rx) -> list[list[int]]:
    """per matrix, its column table sum_x eq(rx, x) M(x, .) of 2^sy entries"""
    p = inst.p
    ex = mo.eq_table(p, list(rx))
    out = []
    for m in inst.matrices:
        t = [0] * (1 << inst.sy)
        for r, c, v in m:
            t[c] = (t[c] + v * ex[r]) % p
        out.append(t)
    return out


def matrix_evals(inst: Instance, rx, ry) -> list[int]:
    p = inst.p
    ey = mo.eq_table(p, list(ry))
    return [sum(x * e for x, e in zip(t, ey)) % p for t in bound_columns(inst, rx)]


def public_eval(inst: Instance, io, pt) -> int:
    half = 1 << (inst.sy - 1)
    return evaluate(inst.p, [1] + list(io) + [0] * (half - 1 - inst.npub), list(pt)) if pt else 1


def prove(inst: Instance, w, io, t: Transcript, basis=None, commitment=None) -> dict:
    p = inst.p
    z = z_of(inst, w, io)
    committed = basis is not None
    cmt = None
    if committed:
        cmt = commitment if commitment is not None else ko.commit(list(w), basis)
    t.append(digest(inst))
    t.append(fq_vec_to_bytes(io))
    if committed:
        t.append(mo.g1_bytes(cmt))
    tau = [t.get_random_challenge() for _ in range(inst.sx)]
    az, bz, cz = mul(inst, z)
    eq = mo.eq_table(p, tau)
    tabs = [eq, az, bz, [(-x) % p for x in eq], cz, [1] * len(eq)]
    polys1, _, rx, ev = cm.prove(inst.field, 0, tabs, SC1_FACTORS, t)
    va, vb, vc = ev[1], ev[2], ev[4]
    t.append(fq_vec_to_bytes([va, vb, vc]))
    rho = t.get_random_challenge()
    cols = bound_columns(inst, rx)
    M = [(a + rho * b + rho * rho * c) % p for a, b, c in zip(*cols)]
    claim = (va + rho * vb + rho * rho * vc) % p
    polys2, _, ry, ev2 = cm.prove(inst.field, claim, [M, z], SC2_FACTORS, t)
    vw = evaluate(p, list(w), ry[1:]) if inst.sy > 1 else w[0]
    t.append(fq_vec_to_bytes([vw]))
    opening = ko.get_proof(list(w), vw, ry[1:], basis) if committed else []
    return {"polys1": polys1, "polys2": polys2, "va": va, "vb": vb, "vc": vc, "vw": vw, "committed": committed,
            "commitment": cmt, "opening": opening, "tau": tau, "rx": rx, "ry": ry, "rho": rho, "M": M,
            "sc2_evals": ev2}


def verify(inst: Instance, proof: dict, io, t: Transcript, g2_taus=None):
    """-> (verified, rx, ry)"""
    p = inst.p
    t.append(digest(inst))
    t.append(fq_vec_to_bytes(io))
    if proof["committed"]:
        t.append(mo.g1_bytes(proof["commitment"]))
    tau = [t.get_random_challenge() for _ in range(inst.sx)]
    if len(proof["polys1"]) != inst.sx or len(proof["polys2"]) != inst.sy:
        return False, [], []
    ok, fin1, rx = cm.verify(inst.field, proof["polys1"], 0, t, 3)
    va, vb, vc, vw = proof["va"], proof["vb"], proof["vc"], proof["vw"]
    if not ok or fin1 != mo.eq_eval(p, tau, rx) * (va * vb - vc) % p:
        return False, [], []
    t.append(fq_vec_to_bytes([va, vb, vc]))
    rho = t.get_random_challenge()
    ok, fin2, ry = cm.verify(inst.field, proof["polys2"], (va + rho * vb + rho * rho * vc) % p, t, 2)
    if not ok:
        return False, [], []
    t.append(fq_vec_to_bytes([vw]))
    ma, mb, mc = matrix_evals(inst, rx, ry)
    vz = ((1 - ry[0]) * vw + ry[0] * public_eval(inst, io, ry[1:])) % p
    if fin2 != (ma + rho * mb + rho * rho * mc) * vz % p:
        return False, [], []
    if proof["committed"]:
        if g2_taus is None or not pg.verify(proof["commitment"], vw, list(proof["opening"]), ry[1:], list(g2_taus)):
            return False, [], []
    return True, rx, ry

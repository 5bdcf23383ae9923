"""R1CS satisfiability by two sum-checks over a committed witness:
(A z) o (B z) = C z with sparse A, B, C, z = (w | 1, io, 0 ..), proved by the
Spartan reduction on the composed sum-check and closed on the witness with KZG
(zk_r1cs_* in include/zk_sumcheck.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field as _dc_field

import numpy as np

from ._lib import lib
from .api import Field, Transcript, UnivariatePoly, _call, modulus
from .context import REPR_CANONICAL, Context, DeviceTable
from .elems import as_limbs, ptr, to_ints
from .kzg import KZG, _g1_array, _g2_array, _points


@dataclass
class R1csProof:
    round_polys_1: list[UnivariatePoly]  # the zero-check eq (Az Bz - Cz): sx rounds, degree 3
    round_polys_2: list[UnivariatePoly]  # M z: sy rounds, degree 2
    va: int                              # Az, Bz, Cz at rx
    vb: int
    vc: int
    vw: int                              # the witness at ry[1..]
    commitment: object = None            # of the witness (None: infinity, or no KZG setup; see `committed`)
    opening: list = _dc_field(default_factory=list)  # sy - 1 quotient commitments
    committed: bool = False
    rx: list[int] = _dc_field(default_factory=list)  # the prover's challenges (not part of the proof)
    ry: list[int] = _dc_field(default_factory=list)


@dataclass
class R1csVerify:
    verified: bool
    rx: list[int]
    ry: list[int]  # uncommitted: the caller checks w~(ry[1:]) == proof.vw


def _coeff_arrays(polys, n: int, slots: int):
    coeffs = np.zeros((max(n, 1), slots, 4), np.uint64)
    nco = np.zeros(max(n, 1), np.uint8)
    for k, rp in enumerate(polys[:n]):
        c = rp.coefficient if isinstance(rp, UnivariatePoly) else list(rp)
        nco[k] = min(len(c), 255)
        keep = c[:slots]
        if keep:
            coeffs[k, : len(keep)] = as_limbs(keep)
    return coeffs, nco


def _matrix_arrays(m):
    """(row, col, value) triples, or (rows uint32[n], cols uint32[n], values uint64[n, 4]) -> the three arrays"""
    if isinstance(m, tuple) and len(m) == 3 and all(isinstance(a, np.ndarray) for a in m):
        rows, cols, vals = m
        if not len(rows) == len(cols) == len(vals):
            raise ValueError("a matrix' rows, cols and values differ in length")
        return (np.ascontiguousarray(rows, np.uint32), np.ascontiguousarray(cols, np.uint32),
                as_limbs(vals) if len(vals) else np.zeros((0, 4), np.uint64))
    ent = list(m)
    return (np.array([e[0] for e in ent], np.uint32), np.array([e[1] for e in ent], np.uint32),
            as_limbs([int(e[2]) for e in ent]) if ent else np.zeros((0, 4), np.uint64))


class R1CS:
    """An R1CS instance: `nrows` constraints over z of 2**sy entries, the first
    half the witness, the second half (1, io_0 .. io_(npub-1), 0 ..). A, B, C are
    lists of (row, col, value) in any order, or array triples (rows, cols,
    values as uint64[n, 4] limbs); duplicates add up. With a Context
    the groupings and values live on the device and the instance can prove;
    with ctx=None the handle is host-only: it multiplies and verifies on the
    host. Use it only while its context lives."""

    def __init__(self, field, nrows: int, sy: int, npub: int, A, B, C_, ctx: Context | None = None):
        self.field = Field(int(field))
        self.ctx = ctx
        self.nrows, self.sy, self.npub = int(nrows), int(sy), int(npub)
        mats = [_matrix_arrays(m) for m in (A, B, C_)]
        nnz = np.array([len(m[0]) for m in mats], np.uint32)
        rows = np.ascontiguousarray(np.concatenate([m[0] for m in mats]))
        cols = np.ascontiguousarray(np.concatenate([m[1] for m in mats]))
        vals = np.ascontiguousarray(np.concatenate([m[2] for m in mats]))
        ent = len(rows) > 0
        h = C.c_void_p()
        _call(lib().zk_r1cs_new(ctx.h if ctx is not None else None, int(self.field), REPR_CANONICAL, self.nrows, self.sy,
                                self.npub, ptr(nnz), ptr(rows) if ent else None, ptr(cols) if ent else None,
                                ptr(vals) if ent else None, C.byref(h)))
        self.h = h
        sx, sy_, r1, r2 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        dg = (C.c_uint8 * 32)()
        _call(lib().zk_r1cs_shape(self.h, C.byref(sx), C.byref(sy_), C.byref(r1), C.byref(r2), dg))
        self.sx = sx.value
        self.digest = bytes(dg)

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().zk_r1cs_free(self.h)  # (does not read the context: safe after the context is closed)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the statement ----
    def z(self, witness, io) -> list[int]:
        half = 1 << (self.sy - 1)
        w, io = [int(x) for x in witness], [int(x) for x in io]
        if len(w) != half or len(io) != self.npub:
            raise ValueError("the witness has 2**(sy-1) entries and io has npub")
        return w + [1] + io + [0] * (half - 1 - self.npub)

    def mul(self, z):
        """-> (Az, Bz, Cz), each 2**sx entries (zero in the padded rows)"""
        z = [int(x) for x in z]
        if len(z) != 1 << self.sy:
            raise ValueError("z has 2**sy entries")
        out = [np.zeros((1 << self.sx, 4), np.uint64) for _ in range(3)]
        _call(lib().zk_r1cs_mul(self.h, REPR_CANONICAL, ptr(as_limbs(z)), ptr(out[0]), ptr(out[1]), ptr(out[2])))
        return tuple(to_ints(o) for o in out)

    def is_satisfied(self, witness, io) -> bool:
        p = modulus(self.field)
        az, bz, cz = self.mul(self.z(witness, io))
        return all(a * b % p == c for a, b, c in zip(az, bz, cz))

    def matrix_evals(self, rx, ry):
        """the multilinear extensions of A, B, C at (rx, ry)"""
        if len(rx) != self.sx or len(ry) != self.sy:
            raise ValueError("rx has sx coordinates and ry has sy")
        out = np.zeros((3, 4), np.uint64)
        _call(lib().zk_r1cs_matrix_evals(self.h, REPR_CANONICAL, ptr(as_limbs([int(x) for x in rx])),
                                         ptr(as_limbs([int(x) for x in ry])), ptr(out)))
        return to_ints(out)

    # ---- prove / verify ----
    def prove(self, witness, io, transcript: Transcript, kzg: KZG | None = None, commitment=None) -> R1csProof:
        """`witness`: 2**(sy-1) ints, or a DeviceTable of them. With `kzg` (a
        setup of sy - 1 variables, BLS12-381 Fr) the witness is committed and
        opened; `commitment` reuses one made earlier."""
        io = [int(x) for x in io]
        if len(io) != self.npub:
            raise ValueError("io has npub entries")
        sx, sy = self.sx, self.sy
        c1 = np.zeros((sx, 4, 4), np.uint64)
        n1 = np.zeros(sx, np.uint8)
        c2 = np.zeros((sy, 3, 4), np.uint64)
        n2 = np.zeros(sy, np.uint8)
        ev = np.zeros((4, 4), np.uint64)
        rx = np.zeros((sx, 4), np.uint64)
        ry = np.zeros((sy, 4), np.uint64)
        cm = np.zeros((1, 12), np.uint64)
        op = np.zeros((max(sy - 1, 1), 12), np.uint64)
        iop = ptr(as_limbs(io)) if io else None
        cin = ptr(_g1_array([commitment])) if (kzg is not None and commitment is not None) else None
        kh = kzg.h if kzg is not None else None
        tail = (iop, kh, cin, transcript.h, ptr(c1), ptr(n1), ptr(c2), ptr(n2), ptr(ev), ptr(rx), ptr(ry), ptr(cm), ptr(op))
        if isinstance(witness, DeviceTable):
            if witness.count != 1 << (sy - 1):
                raise ValueError("the witness has 2**(sy-1) entries")
            _call(lib().zk_dev_r1cs_prove(self.h, REPR_CANONICAL, witness.ptr, *tail))
        else:
            w = [int(x) for x in witness]
            if len(w) != 1 << (sy - 1):
                raise ValueError("the witness has 2**(sy-1) entries")
            _call(lib().zk_r1cs_prove(self.h, REPR_CANONICAL, ptr(as_limbs(w)), *tail))
        p1 = [UnivariatePoly(to_ints(c1[k, : n1[k]]), self.field) for k in range(sx)]
        p2 = [UnivariatePoly(to_ints(c2[k, : n2[k]]), self.field) for k in range(sy)]
        e = to_ints(ev)
        return R1csProof(p1, p2, e[0], e[1], e[2], e[3], _points(cm)[0] if kzg is not None else None,
                         _points(op)[: sy - 1] if kzg is not None else [], kzg is not None, to_ints(rx), to_ints(ry))

    def verify(self, proof: R1csProof, io, transcript: Transcript, g2_taus: list | None = None) -> R1csVerify:
        """With `g2_taus` (from a setup the verifier trusts) the proof's
        commitment and opening are checked; without, the claim
        w~(ry[1:]) == proof.vw is the caller's to check."""
        io = [int(x) for x in io]
        if len(io) != self.npub:
            raise ValueError("io has npub entries")
        sx, sy = self.sx, self.sy
        if len(proof.round_polys_1) != sx or len(proof.round_polys_2) != sy:
            return R1csVerify(False, [], [])
        c1, n1 = _coeff_arrays(proof.round_polys_1, sx, 4)
        c2, n2 = _coeff_arrays(proof.round_polys_2, sy, 3)
        committed = g2_taus is not None
        if proof.committed and not committed:
            raise ValueError("a committed proof is verified against g2_taus")
        if committed and (not proof.committed or len(proof.opening) != sy - 1 or len(g2_taus) < sy - 1):
            return R1csVerify(False, [], [])
        ok = C.c_int(0)
        rx = np.zeros((sx, 4), np.uint64)
        ry = np.zeros((sy, 4), np.uint64)
        _call(lib().zk_r1cs_verify(self.h, REPR_CANONICAL, ptr(as_limbs(io)) if io else None, ptr(c1), ptr(n1), ptr(c2),
                                   ptr(n2), ptr(as_limbs([proof.va, proof.vb, proof.vc, proof.vw])),
                                   ptr(_g1_array([proof.commitment])) if committed else None,
                                   ptr(_g1_array(list(proof.opening))) if committed else None,
                                   ptr(_g2_array(list(g2_taus)[: sy - 1])) if committed else None, transcript.h,
                                   C.byref(ok), ptr(rx), ptr(ry)))
        if not ok.value:
            return R1csVerify(False, [], [])
        return R1csVerify(True, to_ints(rx), to_ints(ry))

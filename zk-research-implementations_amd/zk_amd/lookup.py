"""Lookups (LogUp) over committed columns: every entry of a
committed column of 2**n elements lies in a public table, proved by one
committed sum-check over the column, its multiplicities and two helper columns
of inverses (zk_lookup_* and zk_fe_batch_inverse in include/zk_sumcheck.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field as _dc_field

import numpy as np

from ._lib import lib
from .api import Field, Transcript, UnivariatePoly, _call
from .context import REPR_CANONICAL, Context, DeviceTable
from .elems import as_limbs, ptr, to_ints
from .kzg import KZG, _g1_array, _g2_array, _points

NTABLES = 11  # h_f, h_t, f, m, t_pad, ones, -ones and four multiples of eq(tau, .)


def batch_inverse(values, field, ctx: Context | None = None):
    """x -> 1/x for every entry, 0 -> 0. A list of ints is inverted on the host,
    or on the device when `ctx` is given; a DeviceTable is inverted on the
    device into a new DeviceTable."""
    if isinstance(values, DeviceTable):
        out = DeviceTable(values.ctx, values.field, values.count)
        _call(lib().zk_dev_fe_batch_inverse(values.ctx.h, int(values.field), values.ptr, values.count, out.ptr))
        return out
    vals = [int(x) for x in values]
    if not vals:
        raise ValueError("batch_inverse needs at least one value")
    if ctx is not None:
        t = ctx.upload(int(field), vals)
        try:
            _call(lib().zk_dev_fe_batch_inverse(ctx.h, int(field), t.ptr, t.count, t.ptr))
            return t.to_ints()
        finally:
            t.free()
    out = np.zeros((len(vals), 4), np.uint64)
    _call(lib().zk_fe_batch_inverse(int(field), REPR_CANONICAL, ptr(as_limbs(vals)), len(vals), ptr(out)))
    return to_ints(out)


@dataclass
class LookupProof:
    n: int
    round_polys: list[UnivariatePoly]  # n rounds, degree 3
    table_evals: list[int]             # the eleven tables at the sum-check's point
    commitments: list                  # h_f, h_t, f, m
    opening: list                      # n quotient commitments
    missing: int = 0                   # column entries found nowhere in the table (not part of the proof)
    point: list[int] = _dc_field(default_factory=list)  # the prover's challenges (not part of the proof)


@dataclass
class LookupVerify:
    verified: bool
    point: list[int]


class Lookup:
    """A public table of T field elements, duplicates allowed. With a Context
    its hash lives on the device and the handle can count and prove; with
    ctx=None the handle is host-only: it counts, evaluates and verifies on the
    host. Use it only while its context lives."""

    def __init__(self, table, ctx: Context | None = None, field=Field.BLS12_381_FR):
        self.field = Field(int(field))
        self.ctx = ctx
        tb = [int(x) for x in table]
        self.T = len(tb)
        h = C.c_void_p()
        _call(lib().zk_lookup_new(ctx.h if ctx is not None else None, int(self.field), REPR_CANONICAL,
                                  ptr(as_limbs(tb)) if tb else None, self.T, C.byref(h)))
        self.h = h
        T, ns = C.c_uint32(), C.c_uint32()
        dg = (C.c_uint8 * 32)()
        _call(lib().zk_lookup_info(self.h, C.byref(T), C.byref(ns), dg, None))
        self.nslots = ns.value
        self.digest = bytes(dg)

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().zk_lookup_free(self.h)  # (does not read the context: safe after the context is closed)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slots(self) -> list[int]:
        """the open-addressing table: per slot the first index of its value, or 0xFFFFFFFF"""
        out = np.zeros(self.nslots, np.uint32)
        _call(lib().zk_lookup_info(self.h, None, None, None, ptr(out)))
        return [int(x) for x in out]

    def min_vars(self) -> int:
        return max(1, (self.T - 1).bit_length())

    def multiplicities(self, f, n: int | None = None):
        """-> (m, missing): m over 2**n slots (default: the smallest n holding
        the column and the table), missing = entries found nowhere. `f`: ints,
        or a DeviceTable (then m is a DeviceTable too)."""
        count = f.count if isinstance(f, DeviceTable) else len(f)
        if n is None:
            n = max(self.min_vars(), (count - 1).bit_length(), 1)
        missing = C.c_uint64(0)
        if isinstance(f, DeviceTable):
            m = DeviceTable(f.ctx, f.field, 1 << n)
            _call(lib().zk_dev_lookup_multiplicities(self.h, f.ptr, count, m.ptr, n, C.byref(missing)))
            return m, missing.value
        out = np.zeros((1 << n, 4), np.uint64)
        vals = [int(x) for x in f]
        _call(lib().zk_lookup_multiplicities(self.h, REPR_CANONICAL, ptr(as_limbs(vals)) if vals else None, count, n,
                                             ptr(out), C.byref(missing)))
        return to_ints(out), missing.value

    def table_eval(self, point) -> int:
        """the padded table's multilinear extension at `point` (MSB first)"""
        pt = [int(x) for x in point]
        out = np.zeros((1, 4), np.uint64)
        _call(lib().zk_lookup_table_eval(self.h, REPR_CANONICAL, ptr(as_limbs(pt)) if pt else None, len(pt), ptr(out)))
        return to_ints(out)[0]

    def prove(self, f, transcript: Transcript, kzg: KZG, commitment=None) -> LookupProof:
        """`f`: 2**n ints, or a DeviceTable of them; `kzg`: a setup of n
        variables; `commitment` reuses a commitment of f made earlier. A column
        with non-members is proved all the same: `missing` counts them and the
        proof is rejected."""
        count = f.count if isinstance(f, DeviceTable) else len(f)
        n = max(count - 1, 0).bit_length()
        if count != 1 << n:
            raise ValueError("the column has 2**n entries")
        r = max(n, 1)
        coeffs = np.zeros((r, 4, 4), np.uint64)
        nco = np.zeros(r, np.uint8)
        ev = np.zeros((NTABLES, 4), np.uint64)
        pt = np.zeros((r, 4), np.uint64)
        cm = np.zeros((4, 12), np.uint64)
        op = np.zeros((r, 12), np.uint64)
        missing = C.c_uint64(0)
        cin = ptr(_g1_array([commitment])) if commitment is not None else None
        tail = (n, kzg.h if kzg is not None else None, cin, transcript.h, ptr(coeffs), ptr(nco), ptr(ev), ptr(pt),
                ptr(cm), ptr(op), C.byref(missing))
        if isinstance(f, DeviceTable):
            _call(lib().zk_dev_lookup_prove(self.h, REPR_CANONICAL, f.ptr, *tail))
        else:
            _call(lib().zk_lookup_prove(self.h, REPR_CANONICAL, ptr(as_limbs([int(x) for x in f])), *tail))
        polys = [UnivariatePoly(to_ints(coeffs[k, : nco[k]]), self.field) for k in range(n)]
        return LookupProof(n, polys, to_ints(ev), _points(cm), _points(op)[:n], missing.value, to_ints(pt[:n]))

    def verify(self, proof: LookupProof, transcript: Transcript, g2_taus: list) -> LookupVerify:
        """`g2_taus` come from a setup the verifier trusts."""
        n = int(proof.n)
        if (len(proof.round_polys) != n or len(proof.table_evals) != NTABLES or len(proof.commitments) != 4
                or len(proof.opening) != n or len(g2_taus) < n):
            return LookupVerify(False, [])
        r = max(n, 1)
        coeffs = np.zeros((r, 4, 4), np.uint64)
        nco = np.zeros(r, np.uint8)
        for k, rp in enumerate(proof.round_polys):
            c = rp.coefficient if isinstance(rp, UnivariatePoly) else list(rp)
            nco[k] = min(len(c), 255)
            if c[:4]:
                coeffs[k, : len(c[:4])] = as_limbs(c[:4])
        ok = C.c_int(0)
        pt = np.zeros((r, 4), np.uint64)
        _call(lib().zk_lookup_verify(self.h, REPR_CANONICAL, n, ptr(coeffs), ptr(nco),
                                     ptr(as_limbs([int(x) for x in proof.table_evals])),
                                     ptr(_g1_array(list(proof.commitments))),
                                     ptr(_g1_array(list(proof.opening))) if n else None,
                                     ptr(_g2_array(list(g2_taus)[:n])) if n else None, transcript.h, C.byref(ok),
                                     ptr(pt)))
        if not ok.value:
            return LookupVerify(False, [])
        return LookupVerify(True, to_ints(pt[:n]))

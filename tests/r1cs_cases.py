"""Instances, model proofs and raw C-ABI calls the R1CS tests share (test helper,
not a test module). Model proofs are made once per case and never changed: a
test that damages one works on a copy.

Column layout of every builder: witness entry j is column j; the constant 1 is
column H = 2^(sy-1); io_k is column H + 1 + k."""
from __future__ import annotations

import copy
import ctypes as C
import functools
import random

import numpy as np

import kzg_oracle as ko
import pairing_oracle as pg
import r1cs_oracle as ro
from pyoracle import MODULI

from zk_amd import _lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import _g1_array, _g2_array

SENTINEL = 0xA5A5A5A5A5A5A5A5
PRE_BYTES = b"other bytes absorbed first"


def taus(nvars: int) -> list[int]:
    return [5, 2, 3, 11, 7, 13, 17, 19, 23, 29, 31, 37, 41, 43][:nvars]


@functools.lru_cache(maxsize=None)
def setup(nvars: int):
    """(Lagrange basis in G1, G2 taus) of the model's setup"""
    return ko.get_lagrange_basis(taus(nvars)), pg.g2_taus(taus(nvars))


@functools.lru_cache(maxsize=None)
def other_g2(nvars: int):
    """the G2 taus of another setup"""
    return pg.g2_taus([t + 1 for t in taus(nvars)])


# ---- instance builders: -> (Instance, witness, io) ------------------------------
def cubic(field: int, x: int = 3):
    """x^3 + x + 5 = y: x x = v1, v1 x = v2, (v2 + x + 5) 1 = y; w = (x, v1, v2, 0), io = (y,)"""
    p = MODULI[field]
    H, one, y_col = 4, 4, 5
    v1, v2 = x * x % p, x * x * x % p
    y = (v2 + x + 5) % p
    A = [(0, 0, 1), (1, 1, 1), (2, 2, 1), (2, 0, 1), (2, one, 5)]
    B = [(0, 0, 1), (1, 0, 1), (2, one, 1)]
    C_ = [(0, 1, 1), (1, 2, 1), (2, y_col, 1)]
    return ro.Instance(field, 3, 3, 1, A, B, C_), [x % p, v1, v2, 0], [y]


def chain(field: int, nrows: int, sy: int | None = None, c: int = 7, v0: int = 2):
    """The squaring chain v_(i+1) = v_i^2 + c in nrows constraints: v_i v_i =
    v_(i+1) - c 1 for i < nrows - 1, then v_last 1 = io_0. Every constraint reads
    the constant-1 column (the skew that splits a column)."""
    p = MODULI[field]
    n = nrows - 1  # squarings
    if sy is None:  # the smallest witness half that holds v_0 .. v_n and, beside it, (1, io_0)
        sy = (max(n + 1, 2) - 1).bit_length() + 1
    H = 1 << (sy - 1)
    assert n + 1 <= H and 2 <= H
    v = [v0 % p]
    for _ in range(n):
        v.append((v[-1] * v[-1] + c) % p)
    A = [(i, i, 1) for i in range(n)] + [(n, n, 1)]
    B = [(i, i, 1) for i in range(n)] + [(n, H, 1)]
    C_ = [e for i in range(n) for e in ((i, i + 1, 1), (i, H, (-c) % p))] + [(n, H + 1, 1)]
    return ro.Instance(field, nrows, sy, 1, A, B, C_), v + [0] * (H - n - 1), [v[-1]]


def random_instance(field: int, nrows: int, sy: int, npub: int, per_row: int, seed: int, satisfied: bool = True):
    """Random A, B and a witness; C = one entry per row on the constant column
    carrying (Az)_i (Bz)_i, so the instance is satisfied by construction."""
    p = MODULI[field]
    rng = random.Random(seed)
    H = 1 << (sy - 1)
    w = [rng.randrange(p) for _ in range(H)]
    io = [rng.randrange(p) for _ in range(npub)]
    inst = ro.Instance(field, nrows, sy, npub, [], [], [])
    for m in (inst.A, inst.B):
        for r in range(nrows):
            for _ in range(per_row):
                m.append((r, rng.randrange(1 << sy), rng.randrange(p)))
        rng.shuffle(m)
    az, bz, _ = ro.mul(inst, ro.z_of(inst, w, io))
    inst.C.extend((r, H, az[r] * bz[r] % p) for r in range(nrows))
    if not satisfied:
        inst.C[0] = (0, H, (inst.C[0][2] + 1) % p)
    return inst, w, io


# The (sx, sy) cases of the issue: name -> builder
CASES = {
    "1_1": lambda f: random_instance(f, 2, 1, 0, 2, 101),      # sx = sy = 1: the witness is one value
    "1_2": lambda f: random_instance(f, 1, 2, 1, 2, 102),      # one constraint, sx still 1
    "2_2": lambda f: random_instance(f, 3, 2, 1, 2, 103),
    "3_2": lambda f: random_instance(f, 7, 2, 0, 3, 104),
    "3_4": lambda f: random_instance(f, 5, 4, 3, 3, 105),
    "cubic": lambda f: cubic(f),
    "chain5": lambda f: chain(f, 5),
}


@functools.lru_cache(maxsize=None)
def case(name: str, field: int):
    return CASES[name](field)


@functools.lru_cache(maxsize=None)
def _model_proof(name: str, field: int, committed: bool):
    inst, w, io = case(name, field)
    basis = setup(inst.sy - 1)[0] if committed else None
    return ro.prove(inst, w, io, ro.Transcript(field), basis)


def model_proof(name: str, field: int, committed: bool = False) -> dict:
    return copy.deepcopy(_model_proof(name, field, committed))


# ---- raw calls -------------------------------------------------------------------
def new_raw(inst, ctx=None, repr_=0, null=(), nnz=None, field=None, nrows=None, sy=None, npub=None):
    """zk_r1cs_new -> (rc, handle or None)"""
    L = _lib.lib()
    ent = [e for m in inst.matrices for e in m]
    n3 = np.array([len(m) for m in inst.matrices] if nnz is None else nnz, np.uint32)
    rows = np.array([e[0] for e in ent] or [0], np.uint32)
    cols = np.array([e[1] for e in ent] or [0], np.uint32)
    vals = as_limbs([e[2] for e in ent] or [0])
    h = C.c_void_p(SENTINEL)
    args = {"nnz": ptr(n3), "rows": ptr(rows), "cols": ptr(cols), "vals": ptr(vals), "out": C.byref(h)}
    for k in null:
        args[k] = None
    rc = L.zk_r1cs_new(ctx.h if ctx is not None else None, inst.field if field is None else field, repr_,
                       inst.nrows if nrows is None else nrows, inst.sy if sy is None else sy,
                       inst.npub if npub is None else npub, args["nnz"], args["rows"], args["cols"], args["vals"],
                       args["out"])
    if rc != 0:
        assert h.value == SENTINEL, "the handle was written on failure"
        return rc, None
    return rc, h


def handle(inst, ctx=None):
    rc, h = new_raw(inst, ctx)
    assert rc == 0, _lib.lib().zk_last_error()
    return h


def proof_arrays(inst, proof: dict):
    sx, sy = inst.sx, inst.sy
    c1 = np.zeros((sx, 4, 4), np.uint64)
    n1 = np.zeros(sx, np.uint8)
    c2 = np.zeros((sy, 3, 4), np.uint64)
    n2 = np.zeros(sy, np.uint8)
    for arr, nco, polys, slots in ((c1, n1, proof["polys1"], 4), (c2, n2, proof["polys2"], 3)):
        for k, q in enumerate(polys[: len(nco)]):
            nco[k] = len(q)
            if q:
                arr[k, : min(len(q), slots)] = as_limbs(list(q)[:slots])
    return c1, n1, c2, n2


def verify_raw(h, inst, proof: dict, io, g2_taus=None, pre: bytes = b"", repr_: int = 0, null=()):
    """zk_r1cs_verify on a model-shaped proof -> (rc, verified, rx, ry, outputs and
    transcript untouched)."""
    L = _lib.lib()
    c1, n1, c2, n2 = proof_arrays(inst, proof)
    t = L.zk_transcript_new()
    if pre:
        L.zk_transcript_append(t, (C.c_uint8 * len(pre)).from_buffer_copy(pre), len(pre))
    before = transcript_bytes(t)
    ok = C.c_int(77)
    rx = np.full((inst.sx, 4), SENTINEL, np.uint64)
    ry = np.full((inst.sy, 4), SENTINEL, np.uint64)
    committed = g2_taus is not None
    args = {"io": ptr(as_limbs(list(io))) if io else None, "c1": ptr(c1), "n1": ptr(n1), "c2": ptr(c2), "n2": ptr(n2),
            "ev": ptr(as_limbs([proof["va"], proof["vb"], proof["vc"], proof["vw"]])),
            "cm": ptr(_g1_array([proof["commitment"]])) if committed else None,
            "op": ptr(_g1_array(list(proof["opening"]))) if committed else None,
            "g2": ptr(_g2_array(list(g2_taus))) if committed else None, "t": t, "ok": C.byref(ok), "rx": ptr(rx),
            "ry": ptr(ry)}
    for k in null:
        args[k] = None
    rc = L.zk_r1cs_verify(h, repr_, args["io"], args["c1"], args["n1"], args["c2"], args["n2"], args["ev"], args["cm"],
                          args["op"], args["g2"], args["t"], args["ok"], args["rx"], args["ry"])
    same_t = transcript_bytes(t) == before
    L.zk_transcript_free(t)
    accepted = rc == 0 and ok.value == 1
    untouched = bool((rx == SENTINEL).all() and (ry == SENTINEL).all()) and same_t and (rc == 0 or ok.value == 77)
    return rc, ok.value, (to_ints(rx) if accepted else None), (to_ints(ry) if accepted else None), untouched


def transcript_bytes(t) -> bytes:
    L = _lib.lib()
    n = C.c_size_t(0)
    L.zk_transcript_serialize(t, None, 0, C.byref(n))
    buf = (C.c_uint8 * n.value)()
    assert L.zk_transcript_serialize(t, buf, n.value, C.byref(n)) == 0
    return bytes(buf)


def another_point(P):
    """a valid G1 point different from P"""
    return ko.add(P, ko.G1)


# Every way of damaging a proof: name -> (proof -> None, in place)
def _bump_poly(key):
    def f(p):
        q = p[key][-1]
        if q:
            q[0] = (q[0] + 1) % p["_p"]
        else:
            q.append(1)
    return f


def _bump(key):
    def f(p):
        p[key] = (p[key] + 1) % p["_p"]
    return f


def _change_commitment(p):
    p["commitment"] = another_point(p["commitment"])


def _change_quotient(p):
    p["opening"][-1] = another_point(p["opening"][-1])


TAMPERINGS = {"coefficient1": _bump_poly("polys1"), "coefficient2": _bump_poly("polys2"), "va": _bump("va"),
              "vb": _bump("vb"), "vc": _bump("vc"), "vw": _bump("vw")}
TAMPERINGS_COMMITTED = {"commitment": _change_commitment, "quotient": _change_quotient}


def damaged(proof: dict, field: int, how: str) -> dict:
    q = copy.deepcopy(proof)
    q["_p"] = MODULI[field]
    {**TAMPERINGS, **TAMPERINGS_COMMITTED}[how](q)
    return q

"""Instances, model proofs and raw C-ABI calls the lookup tests share (test
helper, not a test module). Model proofs are made once per case and never
changed: a test that damages one works on a copy."""
from __future__ import annotations

import copy
import ctypes as C
import functools
import random

import numpy as np

import kzg_oracle as ko
import lookup_oracle as lo
from pyoracle import MODULI, Transcript
from r1cs_cases import PRE_BYTES, SENTINEL, other_g2, setup, transcript_bytes  # noqa: F401

from zk_amd import _lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.kzg import _g1_array, _g2_array

# lookup_plan.hpp's constants of the batched inversion
RUN, WAVE, BLOCK = 64, 64, 256


# ---- tables and columns: name -> (table, column, n) --------------------------------
def _low_words_with_home(slot: int, lg: int, count: int, start: int = 1) -> list[int]:
    """`count` distinct 32-bit words whose home slot is `slot` among 2^lg"""
    out, x = [], start
    while len(out) < count:
        if lo.home(x, lg) == slot:
            out.append(x)
        x += 1
    return out


def collision_chain(field: int, length: int = 9):
    """`length` >= 8 keys equal mod 2^32 (one home slot, one chain), then three free keys"""
    keys = [0x1234 + (i << 32) + (i << 200) for i in range(length)] + [7, 8, 9]
    return keys


def wrapping_chain(field: int):
    """T = 8, 16 slots: four keys at home 15 and 14 fill slots 14, 15 and wrap to 0, 1, 2"""
    lg = lo.slot_log(8)
    last = (1 << lg) - 1
    a = _low_words_with_home(last, lg, 3)
    b = _low_words_with_home(last - 1, lg, 2)
    keys = [b[0], a[0], a[1] + (1 << 64), b[1], a[2] + (5 << 128), 3, 4, 5]
    assert len(set(keys)) == 8
    return keys


def case(name: str, field: int, seed: int = 1):
    p = MODULI[field]
    rng = random.Random(seed * 1000 + field)
    if name == "one_value":  # T = 1, every entry equal: 2^12 adds to one counter
        v = rng.randrange(p)
        return [v], [v] * (1 << 12), 12
    if name == "permutation":  # T = 2^n, every value once
        n = 6
        table = rng.sample(range(1, 1 << 20), 1 << n)
        return table, rng.sample(table, len(table)), n
    if name == "duplicates":  # values repeated in the table: the first index counts
        n = 5
        table = [5, 9, 5, p - 1, 9, 5, 0, p - 1, 11]
        return table, [rng.choice(table) for _ in range(1 << n)], n
    if name == "collisions":
        n = 5
        table = collision_chain(field)
        return table, [rng.choice(table) for _ in range(1 << n)], n
    if name == "wrap":
        n = 5
        table = wrapping_chain(field)
        return table, [rng.choice(table) for _ in range(1 << n)], n
    if name == "odd_T":  # T not a power of two, n = 5
        n = 5
        table = [rng.randrange(p) for _ in range(19)]
        return table, [rng.choice(table) for _ in range(1 << n)], n
    if name == "one_missing":
        table, f, n = case("odd_T", field, seed)
        f = list(f)
        f[7] = next(x for x in range(p) if x not in table)
        return table, f, n
    if name == "wrap_missing":  # a non-member whose probe walks the wrapping chain to its end
        table, f, n = case("wrap", field, seed)
        lg = lo.slot_log(len(table))
        f = list(f)
        f[3] = _low_words_with_home((1 << lg) - 1, lg, 1, start=1 << 20)[0] + (9 << 96)
        assert f[3] not in table
        return table, f, n
    if name == "all_missing":
        table, f, n = case("odd_T", field, seed)
        return table, [(x + 1) % p if (x + 1) % p not in table else (x + 2) % p for x in f], n
    raise KeyError(name)


COUNT_CASES = ["one_value", "permutation", "duplicates", "collisions", "wrap", "odd_T", "one_missing", "wrap_missing",
               "all_missing"]


def small(n: int, missing: bool = False):
    """the instance of the model proofs at n = 1, 2, 3 (BLS12-381 Fr): T = 2^n - 1 or 1, a duplicate from n = 2 on"""
    rng = random.Random(40 + n)
    table = [rng.randrange(lo.R) for _ in range(max(1, (1 << n) - 1))]
    if n >= 2:
        table[-1] = table[0]
    f = [rng.choice(table) for _ in range(1 << n)]
    if missing:
        f[-1] = next(x for x in range(lo.R) if x not in table)
    return table, f


@functools.lru_cache(maxsize=None)
def _model_proof(n: int, missing: bool, pre: bytes):
    table, f = small(n, missing)
    t = Transcript(lo.FIELD)
    if pre:
        t.append(pre)
    proof = lo.prove(table, f, setup(n)[0], t)
    proof["end_state"] = t.get_random_challenge()
    return proof


def model_proof(n: int, missing: bool = False, pre: bytes = b"") -> dict:
    return copy.deepcopy(_model_proof(n, missing, pre))


# ---- raw calls -------------------------------------------------------------------
def new_raw(table, field: int = lo.FIELD, ctx=None, repr_: int = 0, null=(), T=None):
    """zk_lookup_new -> (rc, handle or None)"""
    L = _lib.lib()
    tb = as_limbs([int(x) for x in table] or [0])
    h = C.c_void_p(SENTINEL)
    args = {"table": ptr(tb), "out": C.byref(h)}
    for k in null:
        args[k] = None
    rc = L.zk_lookup_new(ctx.h if ctx is not None else None, field, repr_, args["table"],
                         len(table) if T is None else T, args["out"])
    if rc != 0:
        assert h.value == SENTINEL, "the handle was written on failure"
        return rc, None
    return rc, h


def handle(table, field: int = lo.FIELD, ctx=None):
    rc, h = new_raw(table, field, ctx)
    assert rc == 0, _lib.lib().zk_last_error()
    return h


def info(h):
    """-> (T, slots, digest)"""
    L = _lib.lib()
    T, ns = C.c_uint32(), C.c_uint32()
    dg = (C.c_uint8 * 32)()
    assert L.zk_lookup_info(h, C.byref(T), C.byref(ns), dg, None) == 0
    slots = np.zeros(ns.value, np.uint32)
    assert L.zk_lookup_info(h, None, None, None, ptr(slots)) == 0
    return T.value, [int(x) for x in slots], bytes(dg)


def proof_arrays(proof: dict):
    n = proof["n"]
    cf = np.zeros((n, 4, 4), np.uint64)
    nco = np.zeros(n, np.uint8)
    for k, q in enumerate(proof["polys"][:n]):
        nco[k] = len(q)
        if q:
            cf[k, : min(len(q), 4)] = as_limbs(list(q)[:4])
    return cf, nco


def verify_raw(h, proof: dict, g2_taus, pre: bytes = b"", repr_: int = 0, null=(), n=None):
    """zk_lookup_verify on a model-shaped proof -> (rc, verified, point, end state,
    outputs and transcript untouched)."""
    L = _lib.lib()
    cf, nco = proof_arrays(proof)
    t = L.zk_transcript_new()
    if pre:
        L.zk_transcript_append(t, (C.c_uint8 * len(pre)).from_buffer_copy(pre), len(pre))
    before = transcript_bytes(t)
    ok = C.c_int(77)
    pt = np.full((proof["n"], 4), SENTINEL, np.uint64)
    args = {"cf": ptr(cf), "nco": ptr(nco), "ev": ptr(as_limbs(list(proof["table_evals"]))),
            "cm": ptr(_g1_array(list(proof["commitments"]))), "op": ptr(_g1_array(list(proof["opening"]))),
            "g2": ptr(_g2_array(list(g2_taus))), "t": t, "ok": C.byref(ok), "pt": ptr(pt)}
    for k in null:
        args[k] = None
    rc = L.zk_lookup_verify(h, repr_, proof["n"] if n is None else n, args["cf"], args["nco"], args["ev"], args["cm"],
                            args["op"], args["g2"], args["t"], args["ok"], args["pt"])
    same_t = transcript_bytes(t) == before
    accepted = rc == 0 and ok.value == 1
    end = None
    if accepted:
        c = np.zeros((1, 4), np.uint64)
        assert L.zk_transcript_get_random_challenge(t, lo.FIELD, 0, ptr(c)) == 0
        end = to_ints(c)[0]
    L.zk_transcript_free(t)
    untouched = bool((pt == SENTINEL).all()) and same_t and (rc == 0 or ok.value == 77)
    return rc, ok.value, (to_ints(pt) if accepted else None), end, untouched


def another_point(P):
    """a valid G1 point different from P"""
    return ko.add(P, ko.G1)


# Every way of damaging a proof: name -> (proof -> None, in place)
def _bump_poly(p):
    q = p["polys"][-1]
    if q:
        q[0] = (q[0] + 1) % lo.R
    else:
        q.append(1)


def _bump_eval(i):
    def f(p):
        p["table_evals"][i] = (p["table_evals"][i] + 1) % lo.R
    return f


def _change_commitment(i):
    def f(p):
        p["commitments"][i] = another_point(p["commitments"][i])
    return f


def _change_quotient(p):
    p["opening"][-1] = another_point(p["opening"][-1])


TAMPERINGS = {"coefficient": _bump_poly, "quotient": _change_quotient,
              **{f"table_eval{i}": _bump_eval(i) for i in range(lo.NTABLES)},
              **{f"commitment{i}": _change_commitment(i) for i in range(4)}}


def damaged(proof: dict, how: str) -> dict:
    q = copy.deepcopy(proof)
    TAMPERINGS[how](q)
    return q

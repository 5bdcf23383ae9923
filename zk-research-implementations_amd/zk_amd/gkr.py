"""Mirror of the reference `gkr` crate (gkr/src/gkr_circuit.rs,
gkr/src/gkr_protocol.rs) over the C ABI: a layered circuit, `prove` (circuit
evaluation, per-layer tables and sum-checks on the GPU) and `verify` (host).

Differences from the reference:
* the input layer's KZG step (gkr_protocol.rs:92-118) runs over BLS12-381 Fr
  (the reference's KZG field, kzg.rs:3), as the reference always runs it: by
  default (`taus="entropy"`) the taus are drawn from the OS entropy source like
  the reference's `StdRng::from_entropy()` (:94-103) — a fresh, unreproducible
  setup per proof — and caller-given taus make the proof reproducible (tests).
  The proof then carries `input_proof` (commitment, both get_proofs, the opened
  values, the G2 taus) and `verify` checks it with two KZG::verify pairings
  (:155-175). `taus=None` skips the KZG step (a library extension, and the only
  mode over BN254, whose reference `gkr::prove` cannot instantiate the
  BLS12-381 KZG): the proof then carries only the two input-MLE evaluations
  KZG::open would return, and `verify` recomputes them from the inputs when
  they are given;
* `Circuit` accepts only the shape for which the reference's table sizes
  agree (binary tree, powers of two, 1- or 2-gate output layer); anything
  else raises ValueError (the reference panics or mis-sizes);
* `WiredCircuit` (not in the reference) carries its wiring explicitly — any
  (op, left, right) per gate, any widths — and is proved and verified by the
  same `prove` / `verify`, without the KZG step.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from enum import IntEnum

import numpy as np

from ._lib import lib
from .api import Field, UnivariatePoly, _call, default_context, modulus
from .context import REPR_CANONICAL, Context
from .elems import as_limbs, ptr, to_ints


class Operation(IntEnum):  # multilinear_polynomial_evaluation.rs:4-17
    Add = 0
    Mul = 1

    def apply(self, a: int, b: int, p: int) -> int:
        return (a + b) % p if self is Operation.Add else (a * b) % p


class Circuit:  # gkr_circuit.rs:107-144
    def __init__(self, structure: list[list[Operation]], field: int = Field.BN254_FR):
        # immutable, like the reference's Circuit after Circuit::new (gkr_circuit.rs:114-125)
        self.layers = tuple(tuple(Operation(op) for op in layer) for layer in structure)
        self.field = Field(field)

    def evaluate(self, inputs: list[int]) -> list[list[int]]:  # :127-143 (host; O(#gates))
        p = modulus(self.field)
        out, cur = [], [int(x) % p for x in inputs]
        for ops in self.layers:
            vals = [op.apply(0, 0, p) for op in ops]
            for i, op in enumerate(ops):
                if 2 * i + 1 < len(cur):
                    vals[i] = op.apply(cur[2 * i], cur[2 * i + 1], p)
            out.append(vals)
            cur = vals
        return out

    def _abi(self):
        # the C arrays of the structure, built once (the layers are tuples;
        # assigning a new `layers` rebuilds them)
        if getattr(self, "_abi_src", None) is not self.layers:  # (holds the source: no id reuse)
            gates = np.array([len(layer) for layer in self.layers], np.uint32)
            ops = np.fromiter((op for layer in self.layers for op in layer), np.uint8, int(gates.sum()))
            self._abi_cache, self._abi_src = (gates, ops), self.layers
        return self._abi_cache


def _index_array(values, dtype, what: str) -> np.ndarray:
    """values as a C-contiguous array of `dtype` (a numpy array of that dtype
    is taken as it is); ValueError if one does not fit."""
    a = np.asarray(values)
    if a.dtype != dtype:
        if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > np.iinfo(dtype).max):
            raise ValueError(f"{what} must be integers in [0, {np.iinfo(dtype).max}]")
        a = a.astype(dtype)
    return np.ascontiguousarray(a.reshape(-1))


class WiredCircuit:
    """A layered circuit with explicit wiring, layers input ->
    output. Each layer is a tuple of three arrays `(ops, left, right)` — numpy
    arrays (uint8, uint32, uint32) are used as they are, with no per-gate
    Python work — or a list of `(op, left, right)` gate tuples: gate g computes
    `below[left] op below[right]` over the layer below (the `ninputs` inputs
    for the first layer). Counts need not be powers of two; wires may be
    shared, repeated (`left == right`) or unused; a layer may be wider than the
    one below. The wiring and its gate groupings are sent to the device once
    per context, at the first proof there, and freed by `close()` or with the
    context."""

    def __init__(self, layers, ninputs: int, field: int = Field.BN254_FR):
        self.field = Field(field)
        self.ninputs = int(ninputs)
        if not 0 <= self.ninputs < 1 << 32:
            raise ValueError("ninputs out of range")
        per = []
        for layer in layers:
            if isinstance(layer, tuple) and len(layer) == 3 and all(np.ndim(a) == 1 for a in layer):
                ops, left, right = layer
            else:
                g = np.asarray(list(layer), dtype=np.int64).reshape(-1, 3)
                ops, left, right = g[:, 0], g[:, 1], g[:, 2]
            ops, left, right = (_index_array(ops, np.uint8, "gate ops"), _index_array(left, np.uint32, "wire indices"),
                                _index_array(right, np.uint32, "wire indices"))
            if not len(ops) == len(left) == len(right):
                raise ValueError("a layer's ops, left and right differ in length")
            per.append((ops, left, right))
        self.layers = tuple(per)
        self.gates = np.array([len(x[0]) for x in per], np.uint32)
        cat = lambda i, dt: np.ascontiguousarray(np.concatenate([x[i] for x in per]) if per else np.zeros(0, dt))  # noqa: E731
        self.ops, self.left, self.right = cat(0, np.uint8), cat(1, np.uint32), cat(2, np.uint32)
        tot, v = C.c_uint32(0), C.c_uint32(0)
        _call(lib().zk_gkr_wired_shape(len(per), ptr(self.gates), self.ninputs, C.byref(tot), C.byref(v)))
        self.total_rounds, self.output_vars = tot.value, v.value
        below = self.ninputs
        for ops, left, right in per:  # (the library checks again: this fails at construction, before any device work)
            if int(ops.max()) > 1:
                raise ValueError("gate op must be 0 (add) or 1 (mul)")
            if int(max(left.max(), right.max())) >= below:
                raise ValueError("a gate reads a wire the layer below does not have")
            below = len(ops)
        self._handles: dict[int, WiredHandle] = {}

    @classmethod
    def from_tree(cls, circuit: Circuit) -> "WiredCircuit":
        """The tree circuit's wiring made explicit: gate g reads (2g, 2g + 1)."""
        layers = []
        for ops in circuit.layers:
            g = np.arange(len(ops), dtype=np.uint32)
            layers.append((np.array([int(o) for o in ops], np.uint8), 2 * g, 2 * g + 1))
        return cls(layers, 2 * len(circuit.layers[0]), circuit.field)

    def rounds(self) -> list[int]:
        """Sum-check rounds per layer, output layer first: 2 kb(l)."""
        below = [self.ninputs] + [int(g) for g in self.gates[:-1]]
        return [2 * max(1, (n - 1).bit_length()) for n in reversed(below)]

    def evaluate(self, inputs) -> list[list[int]]:
        """Every layer's values (host; O(gates) Python integer operations)."""
        p = modulus(self.field)
        cur = [int(x) % p for x in (to_ints(inputs) if isinstance(inputs, np.ndarray) else inputs)]
        if len(cur) != self.ninputs:
            raise ValueError(f"need {self.ninputs} inputs")
        out = []
        for ops, left, right in self.layers:
            cur = [(cur[a] * cur[b] if o else cur[a] + cur[b]) % p
                   for o, a, b in zip(ops.tolist(), left.tolist(), right.tolist())]
            out.append(cur)
        return out

    def device(self, ctx: Context | None = None) -> "WiredHandle":
        """This circuit on `ctx`'s device: made at the first call per context."""
        ctx = ctx or default_context()
        h = self._handles.get(id(ctx))
        if h is None or h.ctx is not ctx or not h.h:
            h = self._handles[id(ctx)] = WiredHandle(self, ctx)
        return h

    def close(self) -> None:
        for h in self._handles.values():
            h.close()
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WiredHandle:
    """A WiredCircuit resident on one context's device (zk_wired_circuit)."""

    def __init__(self, circuit: WiredCircuit, ctx: Context):
        self.circuit, self.ctx, self.h = circuit, ctx, None
        h = C.c_void_p()
        _call(lib().zk_gkr_wired_new(ctx.h, len(circuit.gates), ptr(circuit.gates), ptr(circuit.ops),
                                     ptr(circuit.left), ptr(circuit.right), circuit.ninputs, C.byref(h)))
        self.h, self._ctx_h = h, ctx.h

    def close(self) -> None:
        if self.h:
            if self.ctx.h and self.ctx.h is self._ctx_h:  # (a destroyed context has already released it)
                lib().zk_gkr_wired_free(self.h)
            self.h = None


@dataclass
class KzgProof:  # gkr_protocol.rs:15-21
    commitment: tuple | None              # G1 affine (x, y), None = infinity
    proof: tuple[list, list]              # get_proof at r_b, at r_c (nvars G1 points each)
    opened_evals: tuple[int, int]         # KZG::open at r_b, r_c
    g2_taus: list                         # kzg_setup.g2_taus


@dataclass
class GkrCircuitProof:  # gkr_protocol.rs:23-29
    output_poly: list[int]
    proof_polynomials: list[list[UnivariatePoly]]  # per layer, output layer first
    claimed_evaluations: list[tuple[int, int]]
    input_evaluations: tuple[int, int]
    random_challenges: list[list[int]]
    input_proof: KzgProof | None = None


def _rounds(gates: np.ndarray) -> int:
    n = C.c_uint32(0)
    _call(lib().zk_gkr_circuit_rounds(len(gates), ptr(gates), C.byref(n)))
    return n.value


def _tree_rounds(gates) -> list[int]:
    """Rounds per layer of a tree circuit, output layer first."""
    return [2 * (2 * int(g)).bit_length() - 2 for g in reversed(gates)]


def _layer_rounds(rounds, coeffs, nco, ch, field):
    """Per layer (output first, `rounds` of them each): its round polynomials
    (trimmed) and challenges, from the C arrays in one conversion each."""
    flat, chs, cnt = to_ints(coeffs.reshape(-1, 4)), to_ints(ch), nco.tolist()
    polys, chal, k0 = [], [], 0
    for nv in rounds:
        polys.append([UnivariatePoly(flat[3 * k: 3 * k + cnt[k]], field) for k in range(k0, k0 + nv)])
        chal.append(chs[k0: k0 + nv])
        k0 += nv
    return polys, chal


ENTROPY = "entropy"


def entropy_taus(nvars: int, field: int = Field.BLS12_381_FR) -> list[int]:
    """nvars field elements from the OS entropy source (the reference's
    F::rand(StdRng::from_entropy()), gkr_protocol.rs:94-101): 512 random bits
    reduced mod p each (bias < 2^-256)."""
    p = modulus(field)
    return [int.from_bytes(os.urandom(64), "little") % p for _ in range(nvars)]


def prove(circuit: Circuit, inputs: list[int] | np.ndarray, ctx: Context | None = None,
          taus: list[int] | str | None = ENTROPY) -> GkrCircuitProof:  # :31-126
    """gkr::prove. inputs: canonical ints, or a uint64[n, 4] array of them
    (little-endian limbs, the C ABI layout) which skips their conversion.
    taus: "entropy" (default; BLS12-381 Fr circuits run the input layer's KZG
    step over a fresh setup drawn from os.urandom, like the reference, and
    other fields skip it: the reference's KZG is BLS12-381-only), a list of
    one tau per input variable (reproducible; BLS12-381 Fr only), or None (no
    KZG step).
    A WiredCircuit (or its WiredHandle on `ctx`) is proved by the wired prover:
    `output_poly` then has 2^v entries, there is no KZG step (`input_proof` is
    None; the input evaluations and final points compose with zk_amd.kzg) and
    a list of taus is an error."""
    if isinstance(circuit, (WiredCircuit, WiredHandle)):
        if taus is not None and not isinstance(taus, str):
            raise ValueError("the wired prover has no KZG step: open the input evaluations with zk_amd.kzg")
        return _prove_wired(circuit, inputs, ctx)
    ctx = ctx or default_context()
    if isinstance(taus, str):
        if taus != ENTROPY:
            raise ValueError(f'taus must be a list, None or "{ENTROPY}"')
        taus = entropy_taus(len(inputs).bit_length() - 1) if circuit.field == Field.BLS12_381_FR else None
    if taus is not None:
        return _prove_kzg(circuit, inputs, ctx, taus)
    gates, ops = circuit._abi()
    total = _rounds(gates)
    L = len(gates)
    outp = np.zeros((2, 4), np.uint64)
    coeffs = np.zeros((total, 3, 4), np.uint64)
    nco = np.zeros(total, np.uint8)
    ch = np.zeros((total, 4), np.uint64)
    claims = np.zeros((max(2 * (L - 1), 1), 4), np.uint64)
    ins = np.zeros((2, 4), np.uint64)
    x = as_limbs(inputs)
    _call(lib().zk_gkr_circuit_prove(ctx.h, int(circuit.field), REPR_CANONICAL, L, ptr(gates), ptr(ops), ptr(x),
                                     len(inputs), ptr(outp), ptr(coeffs), ptr(nco), ptr(ch), ptr(claims), ptr(ins)))
    polys, chal = _layer_rounds(_tree_rounds(gates), coeffs, nco, ch, circuit.field)
    cl = to_ints(claims[: 2 * (L - 1)])
    return GkrCircuitProof(to_ints(outp), polys, [(cl[2 * i], cl[2 * i + 1]) for i in range(L - 1)],
                           tuple(to_ints(ins)), chal)


def _prove_wired(circuit, inputs, ctx: Context | None) -> GkrCircuitProof:
    if isinstance(circuit, WiredHandle):
        handle, circuit = circuit, circuit.circuit
        if ctx is not None and ctx is not handle.ctx:
            raise ValueError("the circuit handle belongs to another context")
        if not handle.h or not handle.ctx.h:
            raise ValueError("the circuit handle has been closed")
    else:
        handle = circuit.device(ctx)
    x = as_limbs(inputs)
    if x.shape[0] != circuit.ninputs:
        raise ValueError(f"need {circuit.ninputs} inputs")
    total, L = circuit.total_rounds, len(circuit.gates)
    outp = np.zeros((1 << circuit.output_vars, 4), np.uint64)
    coeffs = np.zeros((total, 3, 4), np.uint64)
    nco = np.zeros(total, np.uint8)
    ch = np.zeros((total, 4), np.uint64)
    claims = np.zeros((max(2 * (L - 1), 1), 4), np.uint64)
    ins = np.zeros((2, 4), np.uint64)
    _call(lib().zk_gkr_wired_prove(handle.h, int(circuit.field), REPR_CANONICAL, ptr(x), ptr(outp), ptr(coeffs),
                                   ptr(nco), ptr(ch), ptr(claims), ptr(ins)))
    polys, chal = _layer_rounds(circuit.rounds(), coeffs, nco, ch, circuit.field)
    cl = to_ints(claims[: 2 * (L - 1)])
    return GkrCircuitProof(to_ints(outp), polys, [(cl[2 * i], cl[2 * i + 1]) for i in range(L - 1)],
                           tuple(to_ints(ins)), chal)


def _prove_kzg(circuit: Circuit, inputs: list[int], ctx: Context, taus: list[int]) -> GkrCircuitProof:
    from .kzg import _g2_points, _points

    if circuit.field != Field.BLS12_381_FR:
        raise ValueError("the input layer's KZG commitment is over BLS12-381 (kzg.rs:3): use Field.BLS12_381_FR")
    gates, ops = circuit._abi()
    total = _rounds(gates)
    L = len(gates)
    nin = len(inputs).bit_length() - 1
    if len(taus) != nin:
        raise ValueError(f"need {nin} taus (one per input variable)")
    outp = np.zeros((2, 4), np.uint64)
    coeffs = np.zeros((total, 3, 4), np.uint64)
    nco = np.zeros(total, np.uint8)
    ch = np.zeros((total, 4), np.uint64)
    claims = np.zeros((max(2 * (L - 1), 1), 4), np.uint64)
    ins = np.zeros((2, 4), np.uint64)
    com = np.zeros((1, 12), np.uint64)
    prf = np.zeros((max(2 * nin, 1), 12), np.uint64)
    g2 = np.zeros((max(nin, 1), 24), np.uint64)
    x = as_limbs(inputs)  # Python ints or the C ABI layout uint64[n, 4], as on the plain path
    _call(lib().zk_gkr_circuit_prove_kzg(ctx.h, REPR_CANONICAL, L, ptr(gates), ptr(ops), ptr(x), len(inputs),
                                         ptr(as_limbs([int(t) for t in taus])), ptr(outp), ptr(coeffs), ptr(nco),
                                         ptr(ch), ptr(claims), ptr(ins), ptr(com), ptr(prf), ptr(g2)))
    polys, chal = _layer_rounds(_tree_rounds(gates), coeffs, nco, ch, circuit.field)
    cl = to_ints(claims[: 2 * (L - 1)])
    opened = tuple(to_ints(ins))
    pts = _points(prf[: 2 * nin])
    kp = KzgProof(_points(com)[0], (pts[:nin], pts[nin:]), opened, _g2_points(g2[:nin]))
    return GkrCircuitProof(to_ints(outp), polys, [(cl[2 * i], cl[2 * i + 1]) for i in range(L - 1)], opened, chal, kp)


def _verify_kzg(proof: GkrCircuitProof, circuit: Circuit, gates, ops, coeffs, nco, claims) -> bool:
    from .kzg import _g1_array, _g2_array

    kp = proof.input_proof
    nin = (2 * int(gates[0])).bit_length() - 1
    if circuit.field != Field.BLS12_381_FR or len(kp.proof) != 2 or any(len(q) != nin for q in kp.proof) \
            or len(kp.g2_taus) != nin:
        return False
    ok = C.c_int(0)
    _call(lib().zk_gkr_circuit_verify_kzg(REPR_CANONICAL, len(gates), ptr(gates), ptr(ops),
                                          ptr(as_limbs(proof.output_poly)), ptr(coeffs), ptr(nco), ptr(claims),
                                          ptr(as_limbs(list(kp.opened_evals))), ptr(_g1_array([kp.commitment])),
                                          ptr(_g1_array(list(kp.proof[0]) + list(kp.proof[1]))),
                                          ptr(_g2_array(kp.g2_taus)), C.byref(ok)))
    return bool(ok.value)


def verify(proof: GkrCircuitProof, circuit: Circuit, inputs: list[int] | None = None) -> bool:  # :128-227
    """gkr::verify. With an input-layer KZG proof (BLS12-381 Fr) the two
    pairing checks use proof.input_proof.g2_taus, as the reference does
    (gkr_protocol.rs:167,175): that setup must come from a trusted source the
    verifier holds. Taken from an untrusted prover it makes the check unsound
    (a prover who picks its own setup can satisfy both pairings). Inputs, when
    given, are checked as well: their MLE evaluations at the final points must
    equal the opened values (without a KZG proof they are the only check of
    the input layer).
    For a WiredCircuit (zk_gkr_wired_verify, host only) the proof carries no
    KZG step: without the inputs only the sum-check chain down to the claimed
    input evaluations is checked."""
    wired = isinstance(circuit, WiredCircuit)
    if wired:
        gates, ops, total = circuit.gates, circuit.ops, circuit.total_rounds
        if proof.input_proof is not None or len(proof.output_poly) != 1 << circuit.output_vars:
            return False
        if inputs is not None and len(inputs) != circuit.ninputs:
            return False
    else:
        gates, ops = circuit._abi()
        total = _rounds(gates)
    flat = [p for layer in proof.proof_polynomials for p in layer]
    if len(flat) != total:
        return False
    coeffs = np.zeros((max(total, 1), 3, 4), np.uint64)
    nco = np.zeros(max(total, 1), np.uint8)
    for k, poly in enumerate(flat):
        c = poly.coefficient
        if len(c) > 3:
            return False
        nco[k] = len(c)
        if c:
            coeffs[k, : len(c)] = as_limbs(c)
    L = len(gates)
    cl = [v for pair in proof.claimed_evaluations for v in pair]
    if len(cl) != 2 * (L - 1):
        return False
    claims = as_limbs(cl) if cl else np.zeros((1, 4), np.uint64)
    if proof.input_proof is not None:  # the reference's verifier: KZG checks, no inputs needed
        if not _verify_kzg(proof, circuit, gates, ops, coeffs, nco, claims):
            return False
        if inputs is None:
            return True
        if tuple(proof.input_evaluations) != tuple(proof.input_proof.opened_evals):
            return False
    if inputs is None:
        x = None
    else:
        x = as_limbs(inputs if isinstance(inputs, np.ndarray) else [int(v) for v in inputs])
    ok = C.c_int(0)
    if wired:
        _call(lib().zk_gkr_wired_verify(int(circuit.field), REPR_CANONICAL, L, ptr(gates), ptr(ops), ptr(circuit.left),
                                        ptr(circuit.right), circuit.ninputs, ptr(x) if x is not None else None,
                                        ptr(as_limbs(proof.output_poly)), ptr(coeffs), ptr(nco), ptr(claims),
                                        ptr(as_limbs(list(proof.input_evaluations))), C.byref(ok)))
        return bool(ok.value)
    _call(lib().zk_gkr_circuit_verify(int(circuit.field), REPR_CANONICAL, L, ptr(gates), ptr(ops),
                                      ptr(x) if x is not None else None, len(inputs) if inputs is not None else
                                      2 * int(gates[0]), ptr(as_limbs(proof.output_poly)), ptr(coeffs), ptr(nco),
                                      ptr(claims), ptr(as_limbs(list(proof.input_evaluations))), C.byref(ok)))
    return bool(ok.value)

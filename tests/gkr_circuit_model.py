"""Linear-time model of the layered-circuit GKR prover (test helper, not a test
module).

oracle/gkr_oracle.py builds the wiring predicates densely, 2^(3g+2) entries per
layer, so it stops at a few dozen gates. This model proves the same protocol
(gkr_protocol.rs:31-126) from tables of L = 2G entries per layer, in two phases
as the comment above k_phase1_tables (csrc/kernels.hpp) derives them, and so
reaches the documented limit of 2^14 inputs in about a second. It is written
from that derivation and the reference's protocol, not from the library's host
route (host_layer), and uses only pyoracle's sum-check pieces plus
gkr_oracle.circuit_evaluate / initiate_protocol.
tests/test_gkr_circuit_model_cpu.py checks it against gkr_oracle.prove, key by
key, wherever the dense oracle can still run.

For a layer with inputs w (L values), gate weights wt (G values) and gate g
reading (2g, 2g + 1), the layer's sum over (b, c) of A S + M P is

  phase 1 (b):  tables [W, U, V, 1] with W = w, U[2g] = wt_g (Add) or
                wt_g w[2g+1] (Mul), V[2g] = wt_g w[2g+1] (Add), zero elsewhere;
  phase 2 (c):  tables [A, S, M, P] with A[2g+1] (Add) or M[2g+1] (Mul)
                = wt_g eq(r_b, 2g), S = w(r_b) + w, P = w(r_b) w,

both on one transcript and one claim (gkr_prove never reads the claim: it is
passed through). wt_g = eq([r0], g) for the output layer, else
alpha eq(r_b', g) + beta eq(r_c', g) over the previous layer's challenge halves.
eq is MSB-first: variable 0 is the top index bit, as `evaluate` folds.

The named circuits and input patterns of the circuit tests live here as well,
each built once and handed out as tuples.
"""
from __future__ import annotations

import functools
import random

import extreme_tables as xt
import gkr_oracle as go
from pyoracle import MODULI, Transcript, evaluate, fq_vec_to_bytes, gkr_prove

ADD, MUL = go.ADD, go.MUL


def eq_table(p: int, point) -> list[int]:
    """eq(point, x) for every x in [0, 2^len(point)), point[0] the top bit of x."""
    tab = [1]
    for r in point:
        nxt = []
        for t in tab:
            hi = t * r % p
            nxt.append((t - hi) % p)
            nxt.append(hi)
        tab = nxt
    return tab


def prove(field: int, structure, inputs) -> dict:
    """The keys of gkr_oracle.prove plus "challenges": every round's challenge
    in processing order (output layer first, b rounds then c rounds)."""
    p = MODULI[field]
    t = Transcript(field)
    values = go.circuit_evaluate(p, [list(layer) for layer in structure], list(inputs))
    w0 = list(values[-1])
    if len(w0) == 1:
        w0.append(0)
    claim, r0 = go.initiate_protocol(p, t, w0)
    nlayers = len(structure)
    polys, claims, challenges = [], [], []
    rb = rc = []
    alpha = beta = 0
    input_evals = None
    for idx in range(nlayers):
        l = nlayers - 1 - idx
        ops = structure[l]
        G = len(ops)
        L = 2 * G
        w = list(inputs) if l == 0 else list(values[l - 1])
        assert len(w) == L
        if idx == 0:
            wt = eq_table(p, [r0])[:G]
        else:
            eb, ec = eq_table(p, rb), eq_table(p, rc)
            assert len(eb) == len(ec) == G
            wt = [(alpha * eb[g] + beta * ec[g]) % p for g in range(G)]
        # phase 1: sum over c done in closed form, b left
        U, V = [0] * L, [0] * L
        for g, op in enumerate(ops):
            right = wt[g] * w[2 * g + 1] % p
            if op == MUL:
                U[2 * g] = right
            else:
                U[2 * g] = wt[g]
                V[2 * g] = right
        rp1, claim, rb = gkr_prove(field, claim, [w, U, V, [1] * L], t)
        o1 = evaluate(p, w, rb)
        # phase 2: b bound to r_b, c left
        eqb = eq_table(p, rb)
        A, M = [0] * L, [0] * L
        for g, op in enumerate(ops):
            (M if op == MUL else A)[2 * g + 1] = wt[g] * eqb[2 * g] % p
        S = [(o1 + x) % p for x in w]
        P = [o1 * x % p for x in w]
        rp2, claim, rc = gkr_prove(field, claim, [A, S, M, P], t)
        o2 = evaluate(p, w, rc)
        polys.append(rp1 + rp2)
        challenges += list(rb) + list(rc)
        if idx < nlayers - 1:
            t.append(fq_vec_to_bytes([o1]))
            alpha = t.get_random_challenge()
            t.append(fq_vec_to_bytes([o2]))
            beta = t.get_random_challenge()
            claim = (alpha * o1 + beta * o2) % p
            claims.append((o1, o2))
        else:
            input_evals = (o1, o2)
    return {"output_poly": w0, "proof_polynomials": polys, "claimed_evaluations": claims,
            "input_evaluations": input_evals, "final_rb": rb, "final_rc": rc, "challenges": challenges}


# ---------------------------------------------------------------------------
# Named circuits (layers input -> output, tuples of go.ADD / go.MUL) and inputs
# ---------------------------------------------------------------------------
OP_KINDS = ("random", "add", "mul", "mul_ends")


@functools.lru_cache(maxsize=None)
def circuit(depth: int, out_gates: int = 1, ops: str = "random", seed: int = 0) -> tuple:
    """A binary tree of `depth` layers over out_gates * 2^depth inputs.
    ops: "random"; "add" / "mul" (every gate the same: one wiring table is
    identically zero); "mul_ends" (Mul at gates 0 and G - 1 of every layer, Add
    between them)."""
    assert ops in OP_KINDS
    rng = random.Random(f"circuit-{depth}-{out_gates}-{seed}")
    layers = []
    for i in range(depth):
        G = out_gates << (depth - 1 - i)
        if ops == "random":
            layer = [rng.choice((ADD, MUL)) for _ in range(G)]
        elif ops == "mul_ends":
            layer = [MUL if g in (0, G - 1) else ADD for g in range(G)]
        else:
            layer = [ADD if ops == "add" else MUL] * G
        layers.append(tuple(layer))
    return tuple(layers)


CIRCUITS = {  # name -> (depth, output gates); all with random ops, seed = depth
    "C14": (14, 1),    # 2^14 inputs, the documented limit: every table size lgL = 1 .. 14
    "C13x2": (13, 2),  # 2^14 inputs under a 2-gate output layer: lgL = 2 .. 14
    "C12": (12, 1),
    "C11": (11, 1),
    "C4": (4, 1),
}


def named_circuit(name: str) -> tuple:
    depth, out_gates = CIRCUITS[name]
    return circuit(depth, out_gates, "random", depth)


INPUT_KINDS = ("random", "zeros", "ones", "pm1", "last", "one_zero", "special")
ONE_ZERO_AT = 5  # the index of the zero in "one_zero" (any n >= 8)


def special_words(field: int, n: int) -> tuple:
    """The in-memory (Montgomery) words of the "special" inputs: 0, 1, p - 1,
    sat+, sat- (extreme_tables.special_list, whose last two repeat sat-, sat+)
    in turn."""
    sp = xt.special_list(field)
    return tuple(sp[i % len(sp)] for i in range(n))


@functools.lru_cache(maxsize=None)
def inputs(field: int, n: int, kind: str = "random", seed: int = 0) -> tuple:
    """n canonical inputs.
    zeros / ones / pm1: that value everywhere; last: zero but for one random
    nonzero value at index n - 1; one_zero: random nonzero values with a zero at
    ONE_ZERO_AT; special: the values whose Montgomery words are special_words."""
    assert kind in INPUT_KINDS
    p = MODULI[field]
    rng = random.Random(f"inputs-{field}-{n}-{kind}-{seed}")
    if kind == "random":
        return tuple(rng.randrange(p) for _ in range(n))
    if kind == "zeros":
        return (0,) * n
    if kind == "ones":
        return (1,) * n
    if kind == "pm1":
        return (p - 1,) * n
    if kind == "last":
        return (0,) * (n - 1) + (rng.randrange(1, p),)
    if kind == "one_zero":
        return tuple(0 if i == ONE_ZERO_AT % n else rng.randrange(1, p) for i in range(n))
    return tuple(xt.canonical(field, w) for w in special_words(field, n))


@functools.lru_cache(maxsize=None)
def proof(field: int, structure: tuple, ins: tuple) -> dict:
    """prove(), once per (field, circuit, inputs). Shared: do not change it."""
    return prove(field, structure, ins)

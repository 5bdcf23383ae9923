"""Dense model of the wired GKR protocol, from the pieces of
oracle/pyoracle.py and oracle/gkr_oracle.py.

TEST INFRASTRUCTURE ONLY. It restates gkr_oracle.prove (gkr_protocol.rs:31-126)
with the wiring made explicit: add_i / mul_i are full tables of 2^(ka + 2 kb)
entries with a one at (g, left_g, right_g), folded over the gate index by
multi_partial_evaluate; the layer polynomial is the dense SumPoly
[add_i' * (w + w), mul_i' * (w * w)] over 2 kb variables, proved by gkr_prove.
The only generalisations are the ones the shape forces: every width is padded
to its own power of two (at least one variable), and an output layer of 2^v
padded values draws v challenges. Meant for widths <= 16.

A circuit is a list of layers (input -> output), each a list of
(op, left, right) with op 0 = Add, 1 = Mul, plus the number of inputs.
"""
from __future__ import annotations

import random

from gkr_oracle import multi_partial_evaluate
from pyoracle import MODULI, Transcript, evaluate, fq_vec_to_bytes, gkr_prove, tensor_add_mul


def nvars(n: int) -> int:
    """max(1, ceil log2 n)"""
    return max(1, (n - 1).bit_length())


def circuit_evaluate(p: int, layers, inputs: list[int]) -> list[list[int]]:
    out, cur = [], [x % p for x in inputs]
    for layer in layers:
        cur = [(cur[a] * cur[b] if op else cur[a] + cur[b]) % p for op, a, b in layer]
        out.append(cur)
    return out


def padded(values: list[int], k: int) -> list[int]:
    return list(values) + [0] * ((1 << k) - len(values))


def wiring_table(layer, n_below: int, op: int) -> list[int]:
    """add_i (op 0) or mul_i (op 1): 2^(ka + 2 kb) entries, index g | left | right, MSB first."""
    ka, kb = nvars(len(layer)), nvars(n_below)
    t = [0] * (1 << (ka + 2 * kb))
    for g, (o, a, b) in enumerate(layer):
        assert a < n_below and b < n_below and o in (0, 1)
        if o == op:
            t[(g << (2 * kb)) | (a << kb) | b] = 1
    return t


def prove(field: int, layers, ninputs: int, inputs: list[int]) -> dict:
    p = MODULI[field]
    assert len(inputs) == ninputs
    t = Transcript(field)
    vals = circuit_evaluate(p, layers, inputs)
    v = nvars(len(layers[-1]))
    w0 = padded(vals[-1], v)
    t.append(fq_vec_to_bytes(w0))
    r0 = [t.get_random_challenge() for _ in range(v)]
    claimed = evaluate(p, w0, r0)
    t.append(fq_vec_to_bytes([claimed]))
    n = len(layers)
    polys, claims = [], []
    rb, rc = r0, []
    alpha = beta = 0
    for idx in range(n):
        l = n - 1 - idx
        below = list(inputs) if l == 0 else vals[l - 1]
        w = padded(below, nvars(len(below)))
        tabs = []
        for op in (0, 1):
            full = wiring_table(layers[l], len(below), op)
            if idx == 0:
                tabs.append(multi_partial_evaluate(p, full, rb))
            else:
                a, c = multi_partial_evaluate(p, full, rb), multi_partial_evaluate(p, full, rc)
                tabs.append([(alpha * x + beta * y) % p for x, y in zip(a, c)])
        tabs = [tabs[0], tensor_add_mul(p, w, w, "add"), tabs[1], tensor_add_mul(p, w, w, "mul")]
        rp, _, chal = gkr_prove(field, claimed, tabs, t)
        polys.append(rp)
        mid = len(chal) // 2
        rb, rc = chal[:mid], chal[mid:]
        o1, o2 = evaluate(p, w, rb), evaluate(p, w, rc)
        if idx < n - 1:
            t.append(fq_vec_to_bytes([o1]))
            alpha = t.get_random_challenge()
            t.append(fq_vec_to_bytes([o2]))
            beta = t.get_random_challenge()
            claimed = (alpha * o1 + beta * o2) % p
            claims.append((o1, o2))
        else:
            input_evals = (o1, o2)
    return {"output_poly": w0, "proof_polynomials": polys, "claimed_evaluations": claims,
            "input_evaluations": input_evals, "final_rb": rb, "final_rc": rc}


def tree_layers(structure) -> tuple[list, int]:
    """gkr_oracle's structure (lists of "add" / "mul") as a wired circuit."""
    layers = [[(1 if op == "mul" else 0, 2 * g, 2 * g + 1) for g, op in enumerate(ops)] for ops in structure]
    return layers, 2 * len(structure[0])


def random_layers(rng: random.Random, ninputs: int, gates: list[int]) -> list:
    layers, below = [], ninputs
    for g in gates:
        layers.append([(rng.randrange(2), rng.randrange(below), rng.randrange(below)) for _ in range(g)])
        below = g
    return layers

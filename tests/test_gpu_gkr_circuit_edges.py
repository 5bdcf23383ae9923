"""The layered-circuit GKR prover (zk_gkr_circuit_prove, csrc/gkr_circuit.hip;
kernels k_circuit_layer, k_gate_weights, k_layer_tables, k_phase1_tables,
k_phase2_tables, k_mle_eval2) against the linear-time model
(tests/gkr_circuit_model.py, itself checked against the dense oracle on the
CPU) up to the documented limit of 2^14 inputs, on every route a layer can
take, at boundary inputs and op patterns, and through the raw C ABI.

Every proof is compared whole: output poly, every trimmed round polynomial,
every challenge, every claim, both input evaluations; and the host verifier
must accept it. Which route ran is read off the "layer" launch counter: per
layer one k_circuit_layer, and on the device one k_gate_weights plus
  two-phase: k_phase1_tables, k_phase2_tables, and one k_mle_eval2 per phase
             that did not end in host rounds (both with ZK_HOST_ROUNDS=0);
  dense:     k_layer_tables and one k_mle_eval2.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import extreme_tables as xt
import gkr_circuit_model as gm
import gkr_oracle as go

from zk_amd._lib import ZK_EINVAL, ZK_OK, lib
from zk_amd.context import REPR_CANONICAL, REPR_MONTGOMERY
from zk_amd.elems import ptr, to_ints
from zk_amd.gkr import Circuit, Operation, prove, verify

pytestmark = pytest.mark.gpu
OPS = {go.ADD: Operation.Add, go.MUL: Operation.Mul}
KNOBS = ("ZK_CIRCUIT_HOST_LGL", "ZK_HOST_ROUNDS", "ZK_CIRCUIT_DENSE", "ZK_GRID_CAP", "ZK_DEVICE_FS")
DEVICE = {"ZK_CIRCUIT_HOST_LGL": "0"}  # every layer on the device


@functools.lru_cache(maxsize=None)
def _circ(structure: tuple, field: int) -> Circuit:
    return Circuit([[OPS[o] for o in layer] for layer in structure], field)


@functools.lru_cache(maxsize=None)
def _limbs(ins: tuple) -> np.ndarray:
    a = xt.limbs(ins)
    a.setflags(write=False)
    return a


def _context(monkeypatch, env: dict):
    import zk_amd

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return zk_amd.Context(0)


def _assert_is_model(got, model):
    assert got.output_poly == list(model["output_poly"])
    assert [[list(q.coefficient) for q in layer] for layer in got.proof_polynomials] == \
        [[list(q) for q in layer] for layer in model["proof_polynomials"]]
    assert [r for layer in got.random_challenges for r in layer] == list(model["challenges"])
    assert got.claimed_evaluations == [tuple(c) for c in model["claimed_evaluations"]]
    assert tuple(got.input_evaluations) == tuple(model["input_evaluations"])


def _prove_on_route(monkeypatch, env: dict, field: int, structure: tuple, ins: tuple, stats: dict | None = None) -> int:
    """Prove under `env`, compare with the model, verify; returns the "layer"
    launches (and the context's whole counters in `stats`)."""
    model = gm.proof(field, structure, ins)
    circ, x = _circ(structure, field), _limbs(ins)
    ctx = _context(monkeypatch, env)
    try:
        ctx.reset_stats()
        got = prove(circ, x, ctx, taus=None)
        st = ctx.stats()
        launches = st["kernels"]["layer"]["launches"]
        if stats is not None:
            stats.update(st)
    finally:
        ctx.close()
    _assert_is_model(got, model)
    assert verify(got, circ, x) and verify(got, circ)
    return launches


def _named(name: str, field: int):
    s = gm.named_circuit(name)
    return s, gm.inputs(field, 2 * len(s[0]), "random")


# ---------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 1, 2])
def test_default_knobs(monkeypatch, field):
    """Layers of <= 2^9 entries on the host; lgL = 10 .. 14 in two phases on
    the device, ending in host rounds."""
    s, ins = _named("C14", field)
    n = _prove_on_route(monkeypatch, {}, field, s, ins)
    assert len(s) < n < 6 * len(s)


@pytest.mark.parametrize("name,field", [("C14", 0), ("C14", 1), ("C14", 2), ("C13x2", 2)])
def test_every_layer_on_the_device(monkeypatch, name, field):
    s, ins = _named(name, field)
    n = _prove_on_route(monkeypatch, DEVICE, field, s, ins)
    assert 4 * len(s) <= n <= 6 * len(s)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_no_host_rounds_evaluates_with_mle_eval2(monkeypatch, field):
    """No phase ends on the host, so w(r_b) and w(r_c) of every layer come from
    k_mle_eval2, n = 1 .. 14 (at 14 its 128-entry half tables and LayerPts::r are full)."""
    s, ins = _named("C14", field)
    n = _prove_on_route(monkeypatch, {**DEVICE, "ZK_HOST_ROUNDS": "0"}, field, s, ins)
    assert n == 6 * len(s)


def test_every_layer_on_the_host(monkeypatch):
    s, ins = _named("C14", 0)
    n = _prove_on_route(monkeypatch, {"ZK_CIRCUIT_HOST_LGL": "14"}, 0, s, ins)
    assert n == len(s)


@pytest.mark.parametrize("field", [0, 2])
def test_dense_tables_grid_stride(monkeypatch, field):
    """ZK_CIRCUIT_DENSE=1: the input layer's four tables have 2^22 entries each,
    more threads than one resident grid, so k_layer_tables strides."""
    s, ins = _named("C11", field)
    n = _prove_on_route(monkeypatch, {**DEVICE, "ZK_CIRCUIT_DENSE": "1"}, field, s, ins)
    assert n == 4 * len(s)


def test_grid_cap_one(monkeypatch):
    """ZK_GRID_CAP=1: the matrix-core steps of lgL = 11, 12 take several chunks per block."""
    s, ins = _named("C12", 0)
    n = _prove_on_route(monkeypatch, {**DEVICE, "ZK_GRID_CAP": "1"}, 0, s, ins)
    assert 4 * len(s) <= n <= 6 * len(s)


# ---------------------------------------------------------------------------
# boundary inputs and op patterns on 2^12 inputs (lgL = 11, 12 on the matrix cores)
# ---------------------------------------------------------------------------
EDGE_CASES = {  # name -> (op pattern, input pattern)
    "zeros": ("random", "zeros"),            # every round polynomial trims to empty: nothing absorbed
    "pm1": ("random", "pm1"),
    "ones_all_add": ("add", "ones"),         # M identically zero
    "random_all_mul": ("mul", "random"),     # A identically zero
    "all_mul_one_zero": ("mul", "one_zero"),
    "mul_at_ends": ("mul_ends", "random"),   # Mul at gates 0 and G - 1 only
    "last_input_only": ("random", "last"),
}
ROUTES = {"default": {}, "device": DEVICE}


def _edge(case: str, field: int):
    ops, kind = EDGE_CASES[case]
    s = gm.circuit(12, 1, ops, seed=12)
    return s, gm.inputs(field, 1 << 12, kind)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("field", [0, 2])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_inputs_and_ops(monkeypatch, case, field, route):
    s, ins = _edge(case, field)
    n = _prove_on_route(monkeypatch, ROUTES[route], field, s, ins)
    if route == "default":
        assert len(s) < n < 6 * len(s)  # (lgL = 10, 11, 12 on the device)
    else:
        assert 4 * len(s) <= n <= 6 * len(s)


# ---------------------------------------------------------------------------
# the raw C ABI
# ---------------------------------------------------------------------------
SENT64, SENT8, GUARD = 0xA5A5A5A5A5A5A5A5, 0xA5, 8
OUT_NAMES = ("output_poly", "coeffs", "ncoeffs", "challenges", "claims", "input_evals")


class _Outputs:
    """The six output arrays, filled with a sentinel, GUARD elements longer than
    the call may write."""

    def __init__(self, total: int, nlayers: int):
        self.n = {"output_poly": 2, "coeffs": 3 * total, "ncoeffs": total, "challenges": total,
                  "claims": 2 * (nlayers - 1), "input_evals": 2}
        self.a = {k: np.full(n + GUARD, SENT8, np.uint8) if k == "ncoeffs" else np.full((n + GUARD, 4), SENT64, np.uint64)
                  for k, n in self.n.items()}

    def ptrs(self, null=()) -> list:
        return [None if k in null else ptr(self.a[k]) for k in OUT_NAMES]

    def guards_intact(self) -> bool:
        return all(bool((self.a[k][self.n[k]:] == (SENT8 if k == "ncoeffs" else SENT64)).all()) for k in OUT_NAMES)

    def untouched(self) -> bool:
        return all(bool((self.a[k] == (SENT8 if k == "ncoeffs" else SENT64)).all()) for k in OUT_NAMES)

    def get(self, k: str) -> np.ndarray:
        return self.a[k][: self.n[k]]


def _abi(structure) -> tuple:
    gates = np.array([len(layer) for layer in structure], np.uint32)
    ops = np.fromiter((1 if op == go.MUL else 0 for layer in structure for op in layer), np.uint8, int(gates.sum()))
    return gates, ops


def _total_rounds(gates) -> int:
    n = C.c_uint32(0)
    assert lib().zk_gkr_circuit_rounds(len(gates), ptr(gates), C.byref(n)) == ZK_OK
    return n.value


def _raw_prove(ctx, field, repr_, gates, ops, x, out: _Outputs, *, nlayers=None, ninputs=None, null=()):
    return lib().zk_gkr_circuit_prove(
        None if "ctx" in null else ctx.h, field, repr_, len(gates) if nlayers is None else nlayers,
        None if "gates" in null else ptr(gates), None if "ops" in null else ptr(ops),
        None if "inputs" in null else ptr(x), x.shape[0] if ninputs is None else ninputs, *out.ptrs(null))


def _proof_ints(ctx, field, repr_, out: _Outputs) -> dict:
    """The outputs as canonical ints; Montgomery words go back through the device."""
    conv = to_ints if repr_ == REPR_CANONICAL else (lambda a: ctx.upload(field, np.ascontiguousarray(a), REPR_MONTGOMERY).to_ints())
    nco = out.get("ncoeffs").tolist()
    cf = conv(out.get("coeffs"))
    cl = conv(out.get("claims")) if out.n["claims"] else []
    return {"output_poly": conv(out.get("output_poly")), "ncoeffs": nco,
            "coeffs": [cf[3 * k: 3 * k + 3] for k in range(len(nco))], "challenges": conv(out.get("challenges")),
            "claims": cl, "input_evals": conv(out.get("input_evals"))}


def _model_ints(model: dict) -> dict:
    flat = [list(q) for layer in model["proof_polynomials"] for q in layer]
    return {"output_poly": list(model["output_poly"]), "ncoeffs": [len(q) for q in flat],
            "coeffs": [q + [0] * (3 - len(q)) for q in flat],  # (a trimmed coefficient is a zero one)
            "challenges": list(model["challenges"]), "claims": [v for c in model["claimed_evaluations"] for v in c],
            "input_evals": list(model["input_evaluations"])}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name,field", [("C4", 0), ("C4", 1), ("C4", 2), ("C12", 0), ("C12", 2)])
def test_raw_abi_montgomery_in_and_out(monkeypatch, name, field, route):
    s, ins = _named(name, field)
    want = _model_ints(gm.proof(field, s, ins))
    gates, ops = _abi(s)
    total = _total_rounds(gates)
    assert total == len(want["challenges"])
    ctx = _context(monkeypatch, ROUTES[route])
    try:
        canon = _limbs(ins)
        mont = ctx.upload(field, canon).download(REPR_MONTGOMERY)
        assert to_ints(mont[:4]) == [xt.montgomery(field, v) for v in ins[:4]]
        got = {}
        for repr_, x in ((REPR_CANONICAL, canon), (REPR_MONTGOMERY, mont)):
            out = _Outputs(total, len(gates))
            assert _raw_prove(ctx, field, repr_, gates, ops, x, out) == ZK_OK
            assert out.guards_intact(), repr_
            got[repr_] = _proof_ints(ctx, field, repr_, out)
        assert got[REPR_CANONICAL] == want
        assert got[REPR_MONTGOMERY] == want
    finally:
        ctx.close()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("field", [0, 2])
def test_saturating_montgomery_words_as_inputs(monkeypatch, field, route):
    """Inputs whose in-memory words cycle through 0, 1, p - 1, sat+ and sat-
    (tests/extreme_tables.py): they reach the device tables unchanged only
    through ZK_REPR_MONTGOMERY. Random ops, 2^12 inputs."""
    s = gm.named_circuit("C12")
    n = 1 << 12
    ins = gm.inputs(field, n, "special")
    want = _model_ints(gm.proof(field, s, ins))
    gates, ops = _abi(s)
    words = xt.limbs(gm.special_words(field, n))
    out = _Outputs(_total_rounds(gates), len(gates))
    ctx = _context(monkeypatch, ROUTES[route])
    try:
        assert _raw_prove(ctx, field, REPR_MONTGOMERY, gates, ops, words, out) == ZK_OK
        assert out.guards_intact()
        assert _proof_ints(ctx, field, REPR_MONTGOMERY, out) == want
    finally:
        ctx.close()


@pytest.mark.parametrize("out_gates", [1, 2])
def test_one_layer_needs_no_claims_array(ctx, out_gates):
    s = gm.circuit(1, out_gates, "random", seed=out_gates)
    ins = gm.inputs(2, 2 * out_gates, "random", seed=1)
    gates, ops = _abi(s)
    out = _Outputs(_total_rounds(gates), 1)
    assert out.n["claims"] == 0
    assert _raw_prove(ctx, 2, REPR_CANONICAL, gates, ops, _limbs(ins), out, null=("claims",)) == ZK_OK
    assert out.guards_intact()
    assert _proof_ints(ctx, 2, REPR_CANONICAL, out) == _model_ints(gm.proof(2, s, ins))


def _bad_calls(field: int):
    """(label, keyword changes to a valid depth-4 call) that must each be ZK_EINVAL."""
    p = go.MODULI[field]
    s, ins = _named("C4", field)
    gates, ops = _abi(s)
    x = _limbs(ins)
    u32 = lambda v: np.array(v, np.uint32)  # noqa: E731
    bad = [(f"{k} NULL", {"null": (k,)}) for k in ("ctx", "gates", "ops", "inputs") + OUT_NAMES]
    bad += [
        ("nlayers 0", {"nlayers": 0}),
        ("nlayers 25", {"gates": u32([1 << (24 - i) for i in range(25)])}),
        ("6 gates", {"gates": u32([6, 3, 2, 1]), "ninputs": 12}),
        ("12 gates over 8", {"gates": u32([12, 8, 4, 2]), "ninputs": 24}),
        ("no halving", {"gates": u32([8, 2, 1])}),
        ("doubling", {"gates": u32([8, 4, 2, 4])}),
        ("4 output gates", {"gates": u32([8, 4])}),
        ("ninputs 8", {"ninputs": 8}),
        ("ninputs 32", {"ninputs": 32}),
        ("op 2 first", {"ops": np.concatenate([[2], ops[1:]]).astype(np.uint8)}),
        ("op 2 last", {"ops": np.concatenate([ops[:-1], [2]]).astype(np.uint8)}),
        ("op 255", {"ops": np.concatenate([ops[:7], [255], ops[8:]]).astype(np.uint8)}),
        ("field 3", {"field": 3}),
        ("repr 2", {"repr_": 2}),
    ]
    for at in (0, 15):
        for label, repr_, v in (("p canonical", REPR_CANONICAL, p), ("p montgomery", REPR_MONTGOMERY, p),
                                ("2^256 - 1 montgomery", REPR_MONTGOMERY, (1 << 256) - 1)):
            y = x.copy()
            y[at] = xt.limbs([v])[0]
            bad.append((f"input {at} = {label}", {"x": y, "repr_": repr_}))
    return gates, ops, x, bad


@pytest.mark.parametrize("field", [0, 2])
def test_bad_arguments_are_einval_and_write_nothing(ctx, field):
    gates, ops, x, bad = _bad_calls(field)
    total = _total_rounds(gates)
    for label, kw in bad:
        out = _Outputs(total, len(gates))
        kw = dict(kw)
        code = _raw_prove(ctx, kw.pop("field", field), kw.pop("repr_", REPR_CANONICAL), kw.pop("gates", gates),
                          kw.pop("ops", ops), kw.pop("x", x), out, **kw)
        assert code == ZK_EINVAL, label
        assert out.untouched(), label
    # the 2^15-input circuit: one layer past the limit
    big = np.array([1 << (14 - i) for i in range(15)], np.uint32)
    out = _Outputs(2 * sum(range(1, 16)), 15)
    assert _raw_prove(ctx, field, REPR_CANONICAL, big, np.zeros(int(big.sum()), np.uint8),
                      np.zeros((1 << 15, 4), np.uint64), out) == ZK_EINVAL
    assert out.untouched()
    # and the context still proves
    s, ins = _named("C4", field)
    out = _Outputs(total, len(gates))
    assert _raw_prove(ctx, field, REPR_CANONICAL, gates, ops, x, out) == ZK_OK
    assert _proof_ints(ctx, field, REPR_CANONICAL, out) == _model_ints(gm.proof(field, s, ins))


def test_kzg_entry_point_checks_its_arguments_first(ctx):
    """zk_gkr_circuit_prove_kzg: a NULL taus and a bad shape are refused before
    anything runs (what a later KZG failure leaves in the circuit outputs is
    not specified)."""
    s, ins = _named("C4", 2)
    gates, ops = _abi(s)
    x = _limbs(ins)
    taus = xt.limbs([5, 2, 3, 7])
    total = _total_rounds(gates)
    com = np.full((1 + GUARD, 12), SENT64, np.uint64)
    prf = np.full((8 + GUARD, 12), SENT64, np.uint64)
    g2 = np.full((4 + GUARD, 24), SENT64, np.uint64)

    def call(gates_, taus_):
        out = _Outputs(total, len(gates))
        code = lib().zk_gkr_circuit_prove_kzg(ctx.h, REPR_CANONICAL, len(gates_), ptr(gates_), ptr(ops), ptr(x), x.shape[0],
                                              None if taus_ is None else ptr(taus_), *out.ptrs(), ptr(com), ptr(prf), ptr(g2))
        return code, out

    for gates_, taus_ in ((gates, None), (np.array([8, 2, 1], np.uint32), taus), (np.array([8, 4], np.uint32), taus)):
        code, out = call(gates_, taus_)
        assert code == ZK_EINVAL
        assert out.untouched() and all(bool((a == SENT64).all()) for a in (com, prf, g2))
    code, out = call(gates, taus)  # the valid call, for contrast: the circuit part is the model's
    assert code == ZK_OK and out.guards_intact()
    assert all(bool((a[n:] == SENT64).all()) for a, n in ((com, 1), (prf, 8), (g2, 4)))
    assert _proof_ints(ctx, 2, REPR_CANONICAL, out) == _model_ints(gm.proof(2, s, ins))


# ---------------------------------------------------------------------------
# device-resident Fiat-Shamir: kept last in the file
# ---------------------------------------------------------------------------
def test_device_fiat_shamir(monkeypatch):
    """ZK_DEVICE_FS=1: the persistent tail draws the challenges of phases that
    start at round offset lgL (phase 2 of every device layer). With the last
    rounds on the host (default), and with none there (ZK_HOST_ROUNDS=0), where
    a 12-round phase is known to draw on the device (tests/test_gpu_device_fs.py)."""
    s, ins = _named("C12", 0)
    n = _prove_on_route(monkeypatch, {**DEVICE, "ZK_DEVICE_FS": "1"}, 0, s, ins)
    assert 4 * len(s) <= n <= 6 * len(s)
    st = {}
    n = _prove_on_route(monkeypatch, {**DEVICE, "ZK_DEVICE_FS": "1", "ZK_HOST_ROUNDS": "0"}, 0, s, ins, st)
    assert n == 6 * len(s)
    assert st["device_fs_rounds"] > 0, "the device drew no challenge"

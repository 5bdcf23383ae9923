"""The composed sum-check's round kernels (csrc/composed.hpp)
where tests/test_gpu_composed.py does not reach them. Every case runs all its
rounds on the device (ZK_COMPOSED_HOST_LG=0, checked from the launch counts),
and every comparison is an equality with the dense model
(tests/composed_oracle.py) on the canonical values: round polynomials,
challenges, table_evals and the carried claimed sum.

(a) shapes: tables that no term names (the `nunused` fold loop of
    composed_pair: a wrong loop leaves the round polynomials right and the
    table_evals of exactly those tables wrong), a factor repeated inside a
    term on the device, and the documented caps (16 tables, 16 terms, degree 4:
    85 limb-sum columns, a 360-byte argument struct, 16 stores per pair);
(b) every degree 1..4 on every field;
(c) boundary tables (tests/extreme_tables.py composed_family) in place of
    random ones: the kernel's hi - lo borrow, its v += diff chain across the
    points 0..D and its unreduced accumulators at p - 1, 0 and words whose
    sums ripple carries through every limb.

What (c) reaches and what it does not: an accumulator (field.hpp Wide) holds
544 bits and one product of two words below p < 2^255 is below 2^510, so it
takes 2^34 products to overflow one; a round at the caps has 16 terms x 2^25
pairs = 2^29 products for all its threads together. No shape within the caps
can overflow an accumulator, and none here tries: the target is
the carries and borrows inside one sum, at the largest magnitudes (all p - 1,
128 products per accumulator with one block under ZK_GRID_CAP=1). Constant
tables collapse every round polynomial to one coefficient, so they are kept for
the magnitudes only; for the three varying families the MODEL's output must
have degree + 1 coefficients in every round, or the comparison would be of
trimmed polynomials. checker_pm1 cannot meet that on two of the shapes, for
any seed. Its tables stay two-valued under every fold, L(X) in the pairs of
one parity and c - L(X) in the others, with odd-numbered tables the
complement. A term of a even-numbered and b odd-numbered factors then sums to
L^a (c - L)^b + (c - L)^a L^b over the two parities, whose top coefficient
(-1)^b + (-1)^a is zero when a + b is odd (deg3_shared, every degree-3 shape),
and deg4's two terms, L^2 (c - L)^2 and L^3 (c - L), cancel at the top as
well. The checker runs on deg2, caps_one_table and caps instead, which the
model shows at full degree in every round.
"""
from __future__ import annotations

import numpy as np
import pytest

import composed_oracle as cm
import extreme_tables as xt
import pyoracle as po
from test_gpu_composed import _composed, _context

from zk_amd._lib import ZK_OK
from zk_amd.context import REPR_MONTGOMERY
from zk_amd.elems import as_limbs, to_ints

pytestmark = pytest.mark.gpu
FIELDS = (0, 1, 2)
CLAIM = 7
_models: dict = {}


def _model(key, field, tables, factors):
    """composed_oracle.prove, once per case: (polys, challenges, table_evals)."""
    if key not in _models:
        polys, _, chal, evals = cm.prove(field, CLAIM, tables, factors, po.Transcript(field))
        _models[key] = (polys, chal, evals)
    return _models[key]


def _prove_and_compare(ctx, field, dts, factors, nvars, want, what):
    """One device-resident proof over the uploaded tables `dts` against the model's output."""
    polys, chal, evals = want
    ctx.reset_stats()
    got = _composed(ctx, field, dts, factors, CLAIM, dev=True)
    assert got.rc == ZK_OK, what
    assert got.polys() == polys, what
    assert to_ints(got.ch) == chal and to_ints(got.ev) == evals and to_ints(got.cs) == [CLAIM], what
    st = ctx.stats()["kernels"]
    assert st["gkr_round0"]["launches"] == 1 and st["gkr_round"]["launches"] == nvars - 1, what


# ---- (a) unused tables, repeated factors, the caps --------------------------------
# nvars 1: the first-round kernel alone; 2, 3: the fused kernel at h = 1, 2; 9: one block; 10: two blocks;
# 12 with ZK_GRID_CAP=2: every thread loops four times. All three fields at 9, one field elsewhere, rotated.
SIZES = [(1, {}), (2, {}), (3, {}), (9, {}), (10, {}), (12, {"ZK_GRID_CAP": 2})]
EDGE_SHAPES = ["unused1", "unused15", "repeat", "caps", "caps_one_table"]


def _fields_of(shape, nvars):
    return FIELDS if nvars == 9 else ((EDGE_SHAPES.index(shape) + nvars) % 3,)


@pytest.mark.parametrize("nvars,knobs", SIZES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_shapes_equal_the_dense_model(monkeypatch, shape, nvars, knobs):
    ntables, factors = cm.SHAPES[shape]
    named = {f for term in factors for f in term}
    ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=0, **knobs)
    try:
        for field in _fields_of(shape, nvars):
            p = po.MODULI[field]
            ints = cm.random_tables(field, ntables, nvars, 7000 + 10 * nvars + field)
            want = _model(("shape", shape, field, nvars), field, ints, factors)
            limbs = [as_limbs(tb) for tb in ints]
            dts = [ctx.upload(field, a) for a in limbs]
            before = [d.download(REPR_MONTGOMERY) for d in dts]
            _prove_and_compare(ctx, field, dts, factors, nvars, want, (shape, field, nvars))
            _, chal, evals = want
            if shape.startswith("unused"):
                assert len(named) < ntables
                for i in range(ntables):  # (independent of the model's folds: the unused tables' evaluations above all)
                    assert evals[i] == po.evaluate(p, ints[i], chal), (shape, field, nvars, i)
            for d, b, a in zip(dts, before, limbs):  # every input, unused ones included, is read-only
                assert np.array_equal(d.download(REPR_MONTGOMERY), b) and np.array_equal(d.download(), a)
                d.free()
    finally:
        ctx.close()


# ---- (b) every degree on every field -----------------------------------------------
@pytest.mark.parametrize("nvars", [9, 10])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("shape", ["deg1", "deg2", "deg3", "deg4"])
def test_every_degree_on_every_field(monkeypatch, shape, field, nvars):
    ntables, factors = cm.SHAPES[shape]
    ints = cm.random_tables(field, ntables, nvars, 7500 + nvars)
    want = _model(("degree", shape, field, nvars), field, ints, factors)
    assert all(len(q) == len(factors[0]) + 1 for q in want[0])
    ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=0)
    try:
        dts = [ctx.upload(field, as_limbs(tb)) for tb in ints]
        _prove_and_compare(ctx, field, dts, factors, nvars, want, (shape, field, nvars))
        for d in dts:
            d.free()
    finally:
        ctx.close()


# ---- (c) boundary tables -------------------------------------------------------------
VARYING = ("sprinkled", "palette_cycle", "checker_pm1")


def boundary_cases(name):
    """(shape, nvars, knobs) of family `name`; the last one is the single-block case:
    each thread loops 8 times over 16 terms, 128 products into each accumulator."""
    shapes = ("deg2", "caps_one_table", "caps") if name == "checker_pm1" else ("deg3_shared", "deg4", "caps")
    return [(s, n, {}) for s in shapes for n in (3, 9, 10)] + [("caps", 12, {"ZK_GRID_CAP": 1})]


def boundary_model(name, field, shape, nvars):
    """-> (the family's tables, the model's proof of them); shared with nothing that changes it."""
    ntables, factors = cm.SHAPES[shape]
    tabs = xt.composed_family(name, field, ntables, nvars)
    want = _model(("boundary", name, field, shape, nvars), field, [t.canon_ints() for t in tabs], factors)
    if name in VARYING:  # or the comparison would be of trimmed polynomials
        assert [len(q) for q in want[0]] == [len(factors[0]) + 1] * nvars, (name, field, shape, nvars)
    return tabs, want


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", xt.COMPOSED_FAMILIES)
def test_boundary_tables_equal_the_dense_model(monkeypatch, name, field):
    cases = boundary_cases(name)
    for knobs in ({}, {"ZK_GRID_CAP": 1}):
        ctx = _context(monkeypatch, ZK_COMPOSED_HOST_LG=0, **knobs)
        try:
            for shape, nvars, k in cases:
                if k != knobs:
                    continue
                tabs, want = boundary_model(name, field, shape, nvars)
                dts = [ctx.upload(field, t.words, REPR_MONTGOMERY) for t in tabs]
                _prove_and_compare(ctx, field, dts, cm.SHAPES[shape][1], nvars, want, (name, field, shape, nvars, knobs))
                for d, t in zip(dts, tabs):
                    assert np.array_equal(d.download(REPR_MONTGOMERY), t.words)
                    d.free()
        finally:
            ctx.close()

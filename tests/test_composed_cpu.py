"""The composed sum-check without a GPU: the dense model
(tests/composed_oracle.py) against pyoracle.gkr_prove on the four-table shape,
and the library's host-only entry points, zk_composed_sumcheck_verify and
zk_composed_combine, on proofs the model makes — accepted for every degree,
rejected for every kind of damage, trimmed shapes, and every error path with
nothing written."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import composed_oracle as cm
import pyoracle as po

import zk_amd
from zk_amd import _lib
from zk_amd._lib import ZK_EINVAL, ZK_EUNSUPPORTED, ZK_OK
from zk_amd.elems import as_limbs, ptr, to_ints

CAP = 4  # ZK_COMPOSED_MAX_DEGREE


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("nvars", [1, 4])
def test_model_equals_gkr_prove_on_the_four_table_shape(field, nvars):
    tabs = cm.random_tables(field, 4, nvars, 100 + 10 * field + nvars)
    polys, cs, chal, evals = cm.prove(field, 12345, tabs, cm.SHAPES["gkr4"][1], po.Transcript(field))
    want = po.gkr_prove(field, 12345, tabs, po.Transcript(field))
    assert (polys, cs, chal) == want
    assert evals == [po.evaluate(po.MODULI[field], tb, chal) for tb in tabs]


def _model_proof(shape, field, nvars, seed, tables=None):
    ntables, factors = cm.SHAPES[shape]
    tabs = tables if tables is not None else cm.random_tables(field, ntables, nvars, seed)
    claim = cm.true_sum(po.MODULI[field], tabs, factors)
    polys, _, chal, evals = cm.prove(field, claim, tabs, factors, po.Transcript(field))
    return factors, claim, polys, chal, evals


def _accepts(field, factors, claim, polys, chal, evals):
    degree = len(factors[0])
    res = zk_amd.composed_verify([zk_amd.UnivariatePoly(list(q), field) for q in polys], claim,
                                 zk_amd.Transcript(field), degree)
    if not res.verified:
        assert res.final_claimed_sum == 0 and res.random_challenges == [0]
        return False
    assert res.random_challenges == chal
    assert (res.verified, res.final_claimed_sum, res.random_challenges) == \
        cm.verify(field, polys, claim, po.Transcript(field), degree)
    return res.final_claimed_sum == zk_amd.composed_combine(evals, factors, field)


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("shape", ["deg1", "deg3_shared", "deg4", "repeat", "deg2", "deg3"])
def test_verify_and_combine_accept_model_proofs(field, shape):
    factors, claim, polys, chal, evals = _model_proof(shape, field, 4, 7 + field)
    p = po.MODULI[field]
    assert zk_amd.composed_combine(evals, factors, field) == cm.combine(p, evals, factors)
    assert _accepts(field, factors, claim, polys, chal, evals)


@pytest.mark.parametrize("shape", ["deg1", "deg3_shared", "deg4"])
def test_damaged_proofs_are_rejected(shape):
    field = 0
    p = po.MODULI[field]
    factors, claim, polys, chal, evals = _model_proof(shape, field, 3, 31)
    degree = len(factors[0])
    assert _accepts(field, factors, claim, polys, chal, evals)
    for k in (0, len(polys) - 1):  # a changed coefficient, first and last round
        bad = [list(q) for q in polys]
        bad[k][0] = (bad[k][0] + 1) % p
        assert not _accepts(field, factors, claim, bad, chal, evals)
    assert not _accepts(field, factors, (claim + 1) % p, polys, chal, evals)  # a wrong claimed sum
    for i in range(len(evals)):  # a changed table evaluation: only combine can see it
        worse = list(evals)
        worse[i] = (worse[i] + 1) % p
        assert not _accepts(field, factors, claim, polys, chal, worse)
    long = [list(q) for q in polys]  # a round with degree + 2 coefficients (zero s(0) + s(1) change: x^(d+1) - x^d)
    long[1] = long[1] + [0] * (degree + 2 - len(long[1]))
    long[1][degree + 1] = 1
    long[1][degree] = (long[1][degree] - 1) % p
    res = zk_amd.composed_verify([zk_amd.UnivariatePoly(q, field) for q in long], claim, zk_amd.Transcript(field), degree)
    assert (res.verified, res.final_claimed_sum, res.random_challenges) == (False, 0, [0])
    assert cm.verify(field, long, claim, po.Transcript(field), degree) == (False, 0, [0])


def test_a_constant_table_trims_the_top_coefficient():
    field, nvars = 2, 3
    tabs = cm.random_tables(field, 3, nvars, 77)
    tabs[1] = [5] * (1 << nvars)  # constant in every variable: every round polynomial has degree <= 2
    factors, claim, polys, chal, evals = _model_proof("deg3", field, nvars, 0, tables=tabs)
    assert all(len(q) == 3 for q in polys)
    assert _accepts(field, factors, claim, polys, chal, evals)


def test_all_zero_tables_give_empty_round_polynomials():
    field, nvars = 0, 3
    tabs = [[0] * (1 << nvars) for _ in range(3)]
    factors, claim, polys, chal, evals = _model_proof("deg3", field, nvars, 0, tables=tabs)
    assert claim == 0 and polys == [[]] * nvars and evals == [0, 0, 0]
    assert _accepts(field, factors, claim, polys, chal, evals)


# ---- error paths: the code, and nothing written -------------------------------
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _verify_raw(field, repr_, degree, coeffs, nco, nrounds, claim, null=()):
    L = _lib.lib()
    t = L.zk_transcript_new()
    ok = C.c_int(77)
    fin = np.full((1, 4), SENTINEL, np.uint64)
    ch = np.full((max(nrounds, 1), 4), SENTINEL, np.uint64)
    args = {"coeffs": ptr(coeffs), "ncoeffs": ptr(nco), "claim": ptr(claim), "t": t, "ok": C.byref(ok), "fin": ptr(fin),
            "ch": ptr(ch)}
    for name in null:
        args[name] = None
    rc = L.zk_composed_sumcheck_verify(field, repr_, degree, args["coeffs"], args["ncoeffs"], nrounds, args["claim"],
                                       args["t"], args["ok"], args["fin"], args["ch"])
    L.zk_transcript_free(t)
    untouched = ok.value == 77 and (fin == SENTINEL).all() and (ch == SENTINEL).all()
    return rc, untouched


def test_verify_error_paths_write_nothing():
    p = po.MODULI[0]
    coeffs = as_limbs([1, 2, 3, 4, 5, 6, 7, 8])
    nco = np.array([4, 4], np.uint8)
    claim = as_limbs([9])
    assert _verify_raw(0, 0, 3, coeffs, nco, 2, claim)[0] == ZK_OK
    for null in ("coeffs", "ncoeffs", "claim", "t", "ok", "fin", "ch"):
        assert _verify_raw(0, 0, 3, coeffs, nco, 2, claim, null=(null,)) == (ZK_EINVAL, True), null
    assert _verify_raw(0, 0, 0, coeffs, nco, 2, claim) == (ZK_EINVAL, True)           # degree 0
    assert _verify_raw(0, 0, CAP + 1, coeffs, nco, 1, claim) == (ZK_EUNSUPPORTED, True)  # degree above the cap
    assert _verify_raw(3, 0, 3, coeffs, nco, 2, claim) == (ZK_EINVAL, True)           # unknown field
    assert _verify_raw(0, 2, 3, coeffs, nco, 2, claim) == (ZK_EINVAL, True)           # unknown repr
    assert _verify_raw(0, 0, 3, coeffs, nco, 2, as_limbs([p])) == (ZK_EINVAL, True)   # claimed sum >= p
    big = coeffs.copy()
    big[5] = as_limbs([p])[0]
    assert _verify_raw(0, 0, 3, big, nco, 2, claim) == (ZK_EINVAL, True)              # a coefficient >= p
    assert _verify_raw(0, 0, 3, coeffs, nco, 0, claim, null=("coeffs", "ncoeffs"))[0] == ZK_OK  # no rounds: nothing to read


def _combine_raw(field, repr_, evals, ntables, factors, nterms, degree, null=()):
    out = np.full((1, 4), SENTINEL, np.uint64)
    fac = np.array(factors, np.uint8)
    args = {"evals": ptr(evals), "factors": ptr(fac), "out": ptr(out)}
    for name in null:
        args[name] = None
    rc = _lib.lib().zk_composed_combine(field, repr_, args["evals"], ntables, args["factors"], nterms, degree, args["out"])
    return rc, bool((out == SENTINEL).all())


def test_combine_error_paths_write_nothing():
    p = po.MODULI[0]
    ev = as_limbs(list(range(1, 18)))
    assert _combine_raw(0, 0, ev, 3, [0, 1, 2, 2], 2, 2) == (ZK_OK, False)
    for null in ("evals", "factors", "out"):
        assert _combine_raw(0, 0, ev, 3, [0, 1, 2, 2], 2, 2, null=(null,)) == (ZK_EINVAL, True), null
    assert _combine_raw(0, 0, ev, 0, [0, 0], 1, 2) == (ZK_EINVAL, True)       # ntables = 0
    assert _combine_raw(0, 0, ev, 3, [0, 0], 0, 2) == (ZK_EINVAL, True)       # nterms = 0
    assert _combine_raw(0, 0, ev, 3, [0, 0], 2, 0) == (ZK_EINVAL, True)       # degree = 0
    assert _combine_raw(0, 0, ev, 3, [0, 1, 2, 3], 2, 2) == (ZK_EINVAL, True)  # a factor index >= ntables
    assert _combine_raw(3, 0, ev, 3, [0, 1], 1, 2) == (ZK_EINVAL, True)       # unknown field
    assert _combine_raw(0, 5, ev, 3, [0, 1], 1, 2) == (ZK_EINVAL, True)       # unknown repr
    bad = ev.copy()
    bad[1] = as_limbs([p])[0]
    assert _combine_raw(0, 0, bad, 3, [0, 1], 1, 2) == (ZK_EINVAL, True)      # a value >= p
    assert _combine_raw(0, 0, ev, 17, [0, 16], 1, 2) == (ZK_EUNSUPPORTED, True)          # ntables > 16
    assert _combine_raw(0, 0, ev, 3, [0] * 17, 17, 1) == (ZK_EUNSUPPORTED, True)         # nterms > 16
    assert _combine_raw(0, 0, ev, 3, [0] * (CAP + 1), 1, CAP + 1) == (ZK_EUNSUPPORTED, True)  # degree above the cap
    assert _combine_raw(0, 0, ev, 16, list(range(16)) * CAP, 16, CAP)[0] == ZK_OK        # every cap reached


def test_the_header_states_the_cap():
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "include", "zk_sumcheck.h")).read()
    assert int(re.search(r"#define ZK_COMPOSED_MAX_DEGREE (\d+)", src).group(1)) == CAP >= 4


def test_python_shapes():
    a, b, e = (zk_amd.MultilinearPoly(cm.random_tables(0, 1, 2, s)[0], 0) for s in (1, 2, 3))
    sp = zk_amd.SumPoly([zk_amd.ProductPoly.from_polys([e, a, b]), zk_amd.ProductPoly.from_polys([e, b, b])])
    tables, factors = sp.composed_tables()
    assert factors == [[0, 1, 2], [0, 2, 2]] and len(tables) == 3
    assert [to_ints(t) for t in tables] == [e.evaluation, a.evaluation, b.evaluation]
    assert sp.get_degree() == 3 and len(sp.gkr_tables()) == 4  # the old view is unchanged
    # equal values in distinct objects stay distinct tables
    sp2 = zk_amd.SumPoly([zk_amd.ProductPoly([a.evaluation, a.evaluation], 0)])
    assert sp2.composed_tables()[1] == [[0, 1]]
    with pytest.raises(ValueError):
        zk_amd.ProductPoly.from_polys([])
    with pytest.raises(ValueError):
        zk_amd.ProductPoly.from_polys([a, zk_amd.MultilinearPoly([1, 2], 0)])

"""Univariate polynomials over arbitrary points on the GPU through the C ABI:
`UnivariatePoly::evaluate` at many points at once and
`UnivariatePoly::interpolate` (univariate_polynomial_dense.rs :20-26, :48-74).
Any of the three fields; no evaluation domain is involved, so BN254 Fq works
like the scalar fields.

Field elements are canonical Python ints. Where the reference panics (two
points with the same x: its division by zero at :62-64) or a value is >= p,
these raise ValueError; a request above the library's caps (more than 2^16
points to interpolate, more than 2^28 coefficients or points or 2^40 of their
product to evaluate) raises ZkError with code ZK_EUNSUPPORTED.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib
from .api import Field, UnivariatePoly, _call, default_context
from .context import REPR_CANONICAL, Context, DeviceTable
from .elems import as_limbs, ptr, to_ints

INTERPOLATE_MAX = 1 << 16


def _limbs(values) -> np.ndarray:
    if isinstance(values, np.ndarray):
        return as_limbs(values)
    values = [int(v) for v in values]
    return as_limbs(values) if values else np.zeros((0, 4), np.uint64)


def evaluate_many(coeffs, xs, field: int = Field.BN254_FR, ctx: Context | None = None) -> list[int]:
    """evaluate :20-26 at every x of `xs` in one call; no coefficients: 0 everywhere."""
    ctx = ctx or default_context()
    c, x = _limbs(coeffs), _limbs(xs)
    m = x.shape[0]
    if m == 0:
        return []
    out = np.zeros((m, 4), np.uint64)
    _call(lib().zk_poly_evaluate(ctx.h, int(field), REPR_CANONICAL, ptr(c) if c.shape[0] else None, c.shape[0], ptr(x), m,
                                 ptr(out)))
    return to_ints(out)


def dev_evaluate(coeffs: DeviceTable, xs: DeviceTable, out: DeviceTable | None = None) -> DeviceTable:
    """The polynomial whose coefficients are the table `coeffs`, at every point
    of the table `xs`, without leaving the device: into `out` (same context,
    field and count as `xs`; `xs` itself for in place), else into a new table."""
    if not coeffs.ptr or not xs.ptr:
        raise ValueError("the device table has been freed")
    if coeffs.ctx is not xs.ctx:
        raise ValueError("the tables belong to different contexts")
    if int(coeffs.field) != int(xs.field):
        raise ValueError("the tables hold elements of different fields")
    if out is None:
        out = DeviceTable(xs.ctx, xs.field, xs.count)
    else:
        if not out.ptr:
            raise ValueError("the output table has been freed")
        if out.ctx is not xs.ctx:
            raise ValueError("the output table belongs to another context")
        if int(out.field) != int(xs.field):
            raise ValueError("the output table holds elements of another field")
        if out.count != xs.count:
            raise ValueError("the output table has another length")
    _call(lib().zk_dev_poly_evaluate(xs.ctx.h, int(xs.field), coeffs.ptr, coeffs.count, xs.ptr, xs.count, out.ptr))
    return out


def eval_plan(ncoeffs: int, npoints: int, ctx: Context | None = None) -> tuple[int, int]:
    """(chunks, chunk_len): how an evaluation of that shape runs on the context's
    device. chunks > 1: the coefficients are split over the grid's second
    dimension and a second kernel combines the cells."""
    ctx = ctx or default_context()
    chunks, length = C.c_uint32(0), C.c_uint64(0)
    _call(lib().zk_poly_eval_plan(ctx.h, int(ncoeffs), int(npoints), C.byref(chunks), C.byref(length)))
    return chunks.value, length.value


def interpolate(points, field: int = Field.BN254_FR, ctx: Context | None = None) -> UnivariatePoly:
    """interpolate :48-74: the polynomial of degree < n through the n points
    (x, y), trimmed of trailing zeros (no points, or every y = 0: no
    coefficients). Two points with the same x raise ValueError."""
    ctx = ctx or default_context()
    pts = [(int(x), int(y)) for x, y in points]
    n = len(pts)
    if n == 0:
        return UnivariatePoly([], Field(field))
    xs, ys = as_limbs([x for x, _ in pts]), as_limbs([y for _, y in pts])
    out = np.zeros((min(n, INTERPOLATE_MAX), 4), np.uint64)
    cnt = C.c_uint64(0)
    # cap is the buffer's real length; above 2^16 points the library answers ZK_EUNSUPPORTED before it looks at cap
    _call(lib().zk_poly_interpolate(ctx.h, int(field), REPR_CANONICAL, ptr(xs), ptr(ys), n, ptr(out), out.shape[0],
                                    C.byref(cnt)))
    return UnivariatePoly(to_ints(out[: cnt.value]), Field(field))

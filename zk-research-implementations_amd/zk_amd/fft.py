"""Mirror of the reference `fft` crate (fft/src/fft.rs) and of the polynomial
product (univariate_polynomial_dense.rs impl Mul) on the GPU through the C ABI:
the radix-2 number-theoretic transform between the coefficient and the
evaluation form, in natural order on both sides.

Field elements are canonical Python ints. Where the reference panics (a length
that is no power of two, a length the field has no root of unity for, a value
>= p, the zero polynomial as a factor) these raise ValueError; a request
outside what the build runs (more than 2^28 points) raises ZkError with code
ZK_EUNSUPPORTED.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib
from .api import Field, UnivariatePoly, _call, default_context
from .context import REPR_CANONICAL, Context, DeviceTable
from .elems import as_limbs, ptr, to_ints


def get_root_of_unity(n: int, field: int = Field.BN254_FR) -> int:
    """F::get_root_of_unity(n) for a power of two n (fft.rs :38)."""
    n = int(n)
    if n < 0 or n >= 1 << 64:
        raise ValueError("Length must be a power of 2")
    out = np.zeros((1, 4), np.uint64)
    _call(lib().zk_fft_root_of_unity(int(field), REPR_CANONICAL, n, ptr(out)))
    return to_ints(out)[0]


def get_interpolation_roots(n: int, field: int = Field.BN254_FR) -> list[int]:
    """get_interpolation_roots :70-78: w_N^(-k) / N for k < n, N = n rounded up to a power of two."""
    n = int(n)
    if n < 1 or n > 1 << 28:  # (the library's own bound, checked here before n values are allocated)
        raise ValueError("no evaluation domain of this size")
    get_root_of_unity(1 << (n - 1).bit_length(), field)  # the field and its two-adicity, likewise
    out = np.zeros((n, 4), np.uint64)
    _call(lib().zk_fft_interpolation_roots(int(field), REPR_CANONICAL, n, ptr(out)))
    return to_ints(out)


def split_poly(values) -> tuple[list[int], list[int]]:
    """split_poly :62-68: the even- and the odd-indexed coefficients."""
    values = list(values)
    return values[0::2], values[1::2]


def _transform(fn, values, field: int, ctx: Context | None) -> list[int]:
    ctx = ctx or default_context()
    a = as_limbs(values if isinstance(values, np.ndarray) else [int(v) for v in values])
    n = a.shape[0]
    if n == 0:
        raise ValueError("Length must be a power of 2")
    out = np.zeros((n, 4), np.uint64)
    _call(fn(ctx.h, int(field), REPR_CANONICAL, ptr(a), n, ptr(out)))
    return to_ints(out)


def fft_evaluate(poly, ctx: Context | None = None, field: int | None = None) -> list[int]:
    """fft_evaluate :31-41: the polynomial (a UnivariatePoly, or its coefficients
    with `field`) at w^0 .. w^(n-1), n = the number of coefficients."""
    if isinstance(poly, UnivariatePoly):
        coeffs, field = poly.coefficient, poly.field if field is None else field
    else:
        coeffs, field = poly, Field.BN254_FR if field is None else field
    return _transform(lib().zk_fft_evaluate, coeffs, field, ctx)


def fft_interpolate(evals, field: int = Field.BN254_FR, ctx: Context | None = None) -> UnivariatePoly:
    """fft_interpolate :43-60: all n coefficients, untrimmed (UnivariatePoly::new :59)."""
    return UnivariatePoly(_transform(lib().zk_fft_interpolate, evals, field, ctx), Field(field))


def dev_fft(table: DeviceTable, inverse: bool = False, out: DeviceTable | None = None) -> DeviceTable:
    """The transform of a device-resident table (Montgomery elements) without
    leaving the device: into `out` (same context, field and count; `table`
    itself for in place), else into a new table. `table` is only read."""
    if not table.ptr:
        raise ValueError("the device table has been freed")
    if out is None:
        out = DeviceTable(table.ctx, table.field, table.count)
    else:
        if not out.ptr:
            raise ValueError("the output table has been freed")
        if out.ctx is not table.ctx:
            raise ValueError("the output table belongs to another context")
        if int(out.field) != int(table.field):
            raise ValueError("the output table holds elements of another field")
        if out.count != table.count:
            raise ValueError("the output table has another length")
    _call(lib().zk_dev_fft(table.ctx.h, int(table.field), table.ptr, table.count, 1 if inverse else 0, out.ptr))
    return out


def poly_mul(a: UnivariatePoly, b: UnivariatePoly, ctx: Context | None = None) -> UnivariatePoly:
    """impl Mul :95-109 as two transforms, a pointwise product and an inverse
    transform on the device; trailing zeros of the operands do not count."""
    if int(a.field) != int(b.field):
        raise ValueError("the factors are over different fields")
    ctx = ctx or default_context()
    x = as_limbs([int(v) for v in a.coefficient]) if a.coefficient else np.zeros((1, 4), np.uint64)
    y = as_limbs([int(v) for v in b.coefficient]) if b.coefficient else np.zeros((1, 4), np.uint64)
    cap = x.shape[0] + y.shape[0] - 1
    out = np.zeros((cap, 4), np.uint64)
    n = C.c_uint64(0)
    _call(lib().zk_poly_mul(ctx.h, int(a.field), REPR_CANONICAL, ptr(x), x.shape[0], ptr(y), y.shape[0], ptr(out), cap,
                            C.byref(n)))
    return UnivariatePoly(to_ints(out[: n.value]), Field(a.field))

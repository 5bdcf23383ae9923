"""Pure-Python restatement of the reference fft crate (fft/src/fft.rs) over
pyoracle.MODULI, the checker of the GPU transform: the recursive dft :6-29 with
its per-level split, fft_evaluate :31-41, fft_interpolate :43-60,
get_interpolation_roots :70-78, and the schoolbook product of
univariate_polynomial_dense.rs :95-109. Field elements are canonical ints.

root_of_unity is ark-ff's FftField::get_root_of_unity for a power of two n:
TWO_ADIC_ROOT_OF_UNITY = g^((p - 1) / 2^s), squared s - log2 n times, with the
fields' public generators and two-adicities (BN254 Fr: g = 5, s = 28;
BLS12-381 Fr: g = 7, s = 32; BN254 Fq: s = 1, the root is -1).
"""
from __future__ import annotations

import pyoracle as po

GENERATOR = {0: 5, 1: 3, 2: 7}
TWO_ADICITY = {0: 28, 1: 1, 2: 32}


def two_adic_root(field: int) -> int:
    p = po.MODULI[field]
    s = TWO_ADICITY[field]
    assert (p - 1) % (1 << s) == 0 and ((p - 1) >> s) % 2 == 1
    return pow(GENERATOR[field], (p - 1) >> s, p)


def root_of_unity(field: int, n: int) -> int:
    if n < 1 or n & (n - 1):
        raise ValueError("Length must be a power of 2")
    k = n.bit_length() - 1
    if k > TWO_ADICITY[field]:
        raise ValueError("no root of unity of this order")
    p = po.MODULI[field]
    w = two_adic_root(field)
    for _ in range(TWO_ADICITY[field] - k):
        w = w * w % p
    return w


def split_poly(values):  # :62-68
    return list(values[0::2]), list(values[1::2])


def dft(values, root: int, p: int) -> list[int]:  # :6-29
    n = len(values)
    if n == 1:
        return list(values)
    even, odd = split_poly(values)
    root_sq = root * root % p
    y_even, y_odd = dft(even, root_sq, p), dft(odd, root_sq, p)
    y = [0] * n
    tw = 1  # root.pow([j])
    for j in range(n // 2):
        t = tw * y_odd[j] % p
        y[j] = (y_even[j] + t) % p
        y[j + n // 2] = (y_even[j] - t) % p
        tw = tw * root % p
    return y


def fft_evaluate(field: int, coeffs) -> list[int]:  # :31-41
    return dft(list(coeffs), root_of_unity(field, len(coeffs)), po.MODULI[field])


def fft_interpolate(field: int, evals) -> list[int]:  # :43-60 (untrimmed)
    p = po.MODULI[field]
    n = len(evals)
    omega_inv = pow(root_of_unity(field, n), p - 2, p)
    inv_n = pow(n, p - 2, p)
    return [c * inv_n % p for c in dft(list(evals), omega_inv, p)]


def interpolation_roots(field: int, n: int) -> list[int]:  # :70-78
    if n < 1:
        raise ValueError("no evaluation domain of this size")
    p = po.MODULI[field]
    size = 1 << (n - 1).bit_length()  # GeneralEvaluationDomain::new rounds up
    omega_inv = pow(root_of_unity(field, size), p - 2, p)
    inv_n = pow(size, p - 2, p)
    return [pow(omega_inv, k, p) * inv_n % p for k in range(n)]


def poly_mul(field: int, a, b) -> list[int]:  # impl Mul :95-109
    p = po.MODULI[field]
    a, b = list(a), list(b)
    while a and a[-1] == 0:  # degree() trims :28-32
        a.pop()
    while b and b[-1] == 0:
        b.pop()
    if not a or not b:
        raise ValueError("attempt to subtract with overflow")
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def naive_dft(field: int, values, root: int) -> list[int]:
    """The definition y[k] = sum_j c[j] root^(jk), O(n^2)."""
    p = po.MODULI[field]
    n = len(values)
    return [sum(c * pow(root, j * k, p) for j, c in enumerate(values)) % p for k in range(n)]


def table_bytes(values) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)

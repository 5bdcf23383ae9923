"""Pure-Python restatement of the reference's univariate polynomial over
arbitrary points (univariate_polynomial/src/univariate_polynomial_dense.rs) and
of its shamir_secret_sharing crate, statement by statement, plus an independent
O(n^2) interpolation for sizes the reference's O(n^3) loop is too slow for.

Polynomials are lists of canonical ints, lowest coefficient first. Where the
reference panics these raise: ZeroDivisionError for the division at :62-64
(two equal x), IndexError-like ValueError for degree() of the zero polynomial
(:28-32), ValueError for the two panics of the Shamir crate."""
from __future__ import annotations

import hashlib

import pyoracle as po

FQ = 1  # the crate's field, BN254 Fq


# --- univariate_polynomial_dense.rs --------------------------------------------------
def trim(c):  # :14-18
    c = list(c)
    while c and c[-1] == 0:
        c.pop()
    return c


def evaluate(p: int, coeffs, x: int) -> int:  # :20-26
    return sum(c * pow(x, i, p) for i, c in enumerate(coeffs)) % p


def degree(c) -> int:  # :28-32 (on the trimmed copy the caller keeps)
    c = trim(c)
    if not c:
        raise ValueError("attempt to subtract with overflow")
    return len(c) - 1


def scalar_mul(p: int, c, s: int):  # :34-46
    return trim([v * s % p for v in c])


def add(p: int, a, b):  # impl Add :77-93
    out = [0] * max(len(a), len(b))
    for i, v in enumerate(a):
        out[i] = (out[i] + v) % p
    for i, v in enumerate(b):
        out[i] = (out[i] + v) % p
    return out


def mul(p: int, a, b):  # impl Mul :95-109
    a, b = trim(a), trim(b)
    out = [0] * (degree(a) + degree(b) + 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return out


def interpolate(p: int, points):  # :48-74
    n = len(points)
    result = [0]
    for i in range(n):
        x_i, y_i = points[i]
        l_i = [1]
        for j in range(n):
            if i != j:
                x_j, _ = points[j]
                numerator = [(-x_j) % p, 1]
                denominator = (x_i - x_j) % p
                if denominator == 0:
                    raise ZeroDivisionError("attempt to divide by zero")  # F::one() / 0 panics
                l_i = mul(p, l_i, scalar_mul(p, numerator, pow(denominator, -1, p)))
        result = add(p, result, scalar_mul(p, l_i, y_i % p))
    return trim(result)


# --- an independent O(n^2) interpolation ---------------------------------------------
def interpolate_fast(p: int, points):
    """The same polynomial by another route: the master polynomial A = prod (x -
    x_j), each A / (x - x_i) by synthetic division, weights 1 / A'(x_i)."""
    n = len(points)
    xs = [x % p for x, _ in points]
    if len(set(xs)) != n:
        raise ZeroDivisionError("attempt to divide by zero")
    A = [1]
    for xj in xs:
        A = [((A[k - 1] if k > 0 else 0) - xj * (A[k] if k < len(A) else 0)) % p for k in range(len(A) + 1)]
    out = [0] * n
    for (xi, yi) in ((x % p, y % p) for x, y in points):
        q = [0] * n
        carry = 0
        for k in range(n, 0, -1):
            carry = (A[k] + xi * carry) % p
            q[k - 1] = carry
        d = 0
        for k in range(n - 1, -1, -1):  # q(x_i) = A'(x_i)
            d = (d * xi + q[k]) % p
        s = yi * pow(d, -1, p) % p
        for k in range(n):
            out[k] = (out[k] + s * q[k]) % p
    return trim(out)


def horner(p: int, coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def is_interpolant(p: int, coeffs, points) -> bool:
    """The definition: at most n coefficients, trimmed, and the value y_i at
    every x_i. With distinct x this pins the polynomial."""
    return len(coeffs) <= len(points) and (not coeffs or coeffs[-1] != 0) and all(
        horner(p, coeffs, x) == y % p for x, y in points)


def digest(values) -> str:
    """SHA-256 of the canonical little-endian 32-byte images, in order."""
    return hashlib.sha256(b"".join(int(v).to_bytes(32, "little") for v in values)).hexdigest()


# --- shamir_secret_sharing.rs (field: BN254 Fq) ---------------------------------------
def create_polynomial(threshold: int, secret_value: int, secret_point: int, random_points):  # :6-24
    p = po.MODULI[FQ]
    points = [(secret_point % p, secret_value % p)]
    rnd = iter(random_points)
    for _ in range(1, threshold):
        points.append(next(rnd))
    return interpolate(p, points)


def recover_polynomial(points, threshold: int):  # :26-38
    if len(points) < threshold:
        raise ValueError("Not enough points to recreate polynomial")
    selected = points[0:4] if len(points) > 3 else list(points)
    return interpolate(po.MODULI[FQ], selected)


def get_secret(poly, x_point: int) -> int:  # :40-44
    return evaluate(po.MODULI[FQ], poly, x_point)


def share_points(num_of_shares: int, threshold: int, poly, random_xs):  # :46-68
    if num_of_shares < threshold:
        raise ValueError("Num of shares too low")
    p = po.MODULI[FQ]
    rnd = iter(random_xs)
    shares = []
    for _ in range(num_of_shares):
        x = next(rnd)
        shares.append((x, evaluate(p, poly, x)))
    return shares

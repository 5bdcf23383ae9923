"""Mirror of the reference `shamir_secret_sharing` crate
(shamir_secret_sharing/src/shamir_secret_sharing.rs), function by function, on
`UnivariatePoly.interpolate` and `UnivariatePoly.evaluate_many` (zk_amd.poly).

The reference draws its random points from `StdRng::from_entropy()`, so no
two runs of it agree. Here every function that draws takes the values as an
optional argument (tests pass them in) and draws them from `secrets` otherwise.
Where the reference panics (:27-29, :51-53) these raise ValueError. The
default field is the crate's, BN254 Fq.
"""
from __future__ import annotations

import secrets

from .api import Field, UnivariatePoly, modulus
from .context import Context


def _draw(field: int) -> int:
    return secrets.randbelow(modulus(field))


def create_polynomial(threshold: int, secret_value: int, secret_point: int, random_points=None,
                      field: int = Field.BN254_FQ, ctx: Context | None = None) -> UnivariatePoly:
    """create_polynomia :6-24: the polynomial through (secret_point, secret_value)
    and threshold - 1 random points, `random_points` as (x, y) pairs when given."""
    threshold = int(threshold)
    if random_points is None:
        random_points = [(_draw(field), _draw(field)) for _ in range(1, threshold)]
    random_points = [(int(x), int(y)) for x, y in random_points]
    if len(random_points) != max(threshold - 1, 0):
        raise ValueError("create_polynomial draws threshold - 1 random points")
    return UnivariatePoly.interpolate([(int(secret_point), int(secret_value))] + random_points, field, ctx)


def recover_polynomial(points, threshold: int, field: int = Field.BN254_FQ, ctx: Context | None = None) -> UnivariatePoly:
    """recover_polynomial :26-38, with the reference's rule at :31-35: given more
    than three points it interpolates the first four only."""
    points = list(points)
    if len(points) < threshold:
        raise ValueError("Not enough points to recreate polynomial")
    selected = points[0:4] if len(points) > 3 else points
    return UnivariatePoly.interpolate(selected, field, ctx)


def recover_polynomial_all(points, threshold: int, field: int = Field.BN254_FQ,
                           ctx: Context | None = None) -> UnivariatePoly:
    """recover_polynomial through every point given.

    This departs from the reference, whose recover_polynomial never looks past
    the fourth point (:31-35) and so cannot recover a polynomial of a threshold
    above four."""
    points = list(points)
    if len(points) < threshold:
        raise ValueError("Not enough points to recreate polynomial")
    return UnivariatePoly.interpolate(points, field, ctx)


def get_secret(poly: UnivariatePoly, x_point: int) -> int:
    """get_secret :40-44."""
    return poly.evaluate(int(x_point))


def share_points(num_of_shares: int, threshold: int, poly: UnivariatePoly, random_xs=None,
                 ctx: Context | None = None) -> list[tuple[int, int]]:
    """share_points :46-68: num_of_shares points (x, poly(x)) at random x
    (`random_xs` when given), all evaluated in one call."""
    if num_of_shares < threshold:
        raise ValueError("Num of shares too low")
    if random_xs is None:
        random_xs = [_draw(poly.field) for _ in range(num_of_shares)]
    xs = [int(x) for x in random_xs]
    if len(xs) != num_of_shares:
        raise ValueError("share_points draws one x per share")
    return list(zip(xs, poly.evaluate_many(xs, ctx)))

"""GPU parity of zk_amd.shamir with shamir_secret_sharing.rs as restated in
tests/poly_oracle.py, with the randomness passed in: the crate's end-to-end
test, many shares in one evaluation call, recovery at a threshold the
reference's first-four rule cannot reach, and that rule itself. Exact equality
throughout; BN254 Fq, the crate's field."""
from __future__ import annotations

import os

import pytest

import coracle as co
import poly_oracle as O
import pyoracle as po

import zk_amd
from zk_amd import shamir
from zk_amd.api import UnivariatePoly

pytestmark = pytest.mark.gpu

FQ = 1
P = po.MODULI[FQ]
SEED = 29


def _rand(table: int, n: int) -> list:
    return co.from_limbs(co.synth(FQ, SEED, table, 0, n))


@pytest.fixture(scope="module")
def dev():
    old = os.environ.get("ZK_POLY_HOST_MAX")
    os.environ["ZK_POLY_HOST_MAX"] = "0"
    try:
        c = zk_amd.Context(0)
    finally:
        if old is None:
            os.environ.pop("ZK_POLY_HOST_MAX", None)
        else:
            os.environ["ZK_POLY_HOST_MAX"] = old
    yield c
    c.close()


@pytest.mark.parametrize("which", ["device", "default"])
def test_it_all_works_properly(dev, ctx, which):  # :153-169
    c = dev if which == "device" else ctx
    secret_point, secret_data = 0, P - 5
    rnd = list(zip(_rand(0, 2), _rand(1, 2)))
    secret_poly = shamir.create_polynomial(3, secret_data, secret_point, rnd, ctx=c)
    assert secret_poly.coefficient == O.create_polynomial(3, secret_data, secret_point, rnd)
    xs = _rand(2, 10)
    shares = shamir.share_points(10, 3, secret_poly, xs, ctx=c)
    assert shares == O.share_points(10, 3, secret_poly.coefficient, xs) and len(shares) == 10
    recreated = shamir.recover_polynomial(shares[2:6], 3, ctx=c)
    assert recreated.coefficient == secret_poly.coefficient == O.recover_polynomial(shares[2:6], 3)
    assert shamir.get_secret(recreated, secret_point) == secret_data


def test_it_creates_a_correct_polynomial(dev):  # :77-89
    f = shamir.create_polynomial(4, 40, 6, list(zip(_rand(3, 3), _rand(4, 3))), ctx=dev)
    assert f.evaluate(6) == 40 and f.degree() == 3


def test_many_shares_in_one_call(dev):
    f = shamir.create_polynomial(4, 1234567, 0, list(zip(_rand(5, 3), _rand(6, 3))), ctx=dev)
    xs = _rand(7, 4096)
    shares = shamir.share_points(4096, 4, f, xs, ctx=dev)
    assert [x for x, _ in shares] == xs
    assert [y for _, y in shares] == [O.horner(P, f.coefficient, x) for x in xs]
    back = shamir.recover_polynomial(shares[1000:1004], 4, ctx=dev)
    assert back.coefficient == f.coefficient and shamir.get_secret(back, 0) == 1234567


def test_recover_all_at_threshold_40(dev):
    f = shamir.create_polynomial(40, 99, 0, list(zip(_rand(8, 39), _rand(9, 39))), ctx=dev)
    assert f.degree() == 39
    shares = shamir.share_points(200, 40, f, _rand(10, 200), ctx=dev)
    back = shamir.recover_polynomial_all(shares[100:140], 40, ctx=dev)
    assert back.coefficient == f.coefficient and shamir.get_secret(back, 0) == 99
    with pytest.raises(ValueError):
        shamir.recover_polynomial_all(shares[:39], 40, ctx=dev)


def test_first_four_rule(dev):
    """recover_polynomial :31-35 never looks past the fourth point: at threshold
    5 it returns the cubic through the first four shares, as the oracle does."""
    f = shamir.create_polynomial(5, 7, 0, list(zip(_rand(11, 4), _rand(12, 4))), ctx=dev)
    shares = shamir.share_points(8, 5, f, _rand(13, 8), ctx=dev)
    got = shamir.recover_polynomial(shares, 5, ctx=dev)
    assert got.coefficient == O.recover_polynomial(shares, 5) == O.interpolate(P, shares[:4])
    assert got.coefficient != f.coefficient and len(got.coefficient) == 4
    assert shamir.recover_polynomial_all(shares, 5, ctx=dev).coefficient == f.coefficient
    assert shamir.recover_polynomial(shares[:3], 3, ctx=dev).coefficient == O.interpolate(P, shares[:3])


def test_panics_are_value_errors(dev):  # :27-29, :51-53
    with pytest.raises(ValueError):
        shamir.recover_polynomial([(1, P - 1), (2, 5)], 3, ctx=dev)
    with pytest.raises(ValueError):
        shamir.share_points(2, 3, UnivariatePoly([P - 5, 3, 1], FQ), [1, 2], ctx=dev)

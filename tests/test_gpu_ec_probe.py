"""csrc/ec.hpp as hipcc generates it for gfx950: the device legs of the ec.hpp
probe (tests/native/ec_probe.hip, zk_amd/_lib/libzkecprobe.so) on the cases of
tests/ec_cases.py, one launch per op, against Python integers.

The device compilation of fq_mul is the 12 x 32-bit CIOS (288 mad64) that every
MSM, setup and proof runs and that the host never compiles; here it gets all
56 x 56 pairs of the 381-bit boundary palette, and through it every Fq op and
every G1 / XYZZ group-law branch (equal points under different Z, P + (-P),
infinity as Z = 0 over garbage, the order-3 point (0, 2), g1_mul_small at 0 and
2^32 - 1). tests/test_ec_cases_cpu.py runs the same cases through the host leg
(fqh::mul): a failure here and none there puts the fault in the 32-bit path or
in its generated code. A missing probe library is a failure: build() makes it."""
from __future__ import annotations

import pytest

import ec_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(ctx):  # (ctx: the session's device is initialised and current)
    return ec.Probe()  # OSError, a failure, where the library was not built


@pytest.mark.parametrize("op", ec.FQ_OPS)
def test_fq_device_leg_equals_python_integers(probe, op):
    bad = ec.fq_failures(probe, op, 1)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("op", ec.G1_OPS)
def test_g1_device_leg_equals_the_python_group_law(probe, op):
    bad = ec.g1_failures(probe, op, 1)
    assert not bad, (len(bad), bad[:5])


def test_device_and_host_legs_agree_word_for_word(probe):
    """Beyond equal group elements: the same output words from both compilations
    (the formulas are deterministic, so Z, ZZ and ZZZ agree too)."""
    for op in ("g1_add", "g1x_add_mixed", "g1_mul_small"):
        _, a, b, _ = ec.g1_cases(op)
        assert probe.g1(op, 1, a, b) == probe.g1(op, 0, a, b), op

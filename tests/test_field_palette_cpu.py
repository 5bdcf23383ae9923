"""csrc/field.hpp on the CPU, on the boundary palette (tests/extreme_tables.py):
builds tests/native/field_palette_check.cpp with hipcc (host code only) and
compares it with Python integers. Per field: all 42 x 42 pairs under fe_add,
fe_sub and fe_mul, fe_inv of every word, wide_mac of every word with itself
summed 1 to 1000 times into one accumulator, and wide_redc of 8 extreme and
2000 random 544-bit values; 22 656 cases in all.

The kernels compile the same source for gfx950, and
tests/test_gpu_field_palette.py runs the same pairs there: a failure there and
none here puts the fault in the generated code, not in the source. fe_inv and
wide_redc have no device entry of their own and are pinned here."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

import extreme_tables as xt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
R = xt.R
MAC_COUNTS = (1, 2, 17, 256, 1000)
WIDE = 1 << 544


def wide_values(field: int) -> list[int]:
    p = xt.modulus(field)
    extreme = [0, 1, WIDE - 1, 1 << 543, WIDE - R, R - 1, R, (p - 1) * (p - 1) * 1000]
    rng = random.Random(544 + field)
    return extreme + [rng.randrange(WIDE) for _ in range(2000)]


def cases(field: int):
    """-> [(input line, expected word)]"""
    p = xt.modulus(field)
    rinv = pow(R, -1, p)
    pal = xt.palette(field)
    out = []
    for a in pal:
        for b in pal:
            out.append((f"{field} add {a:x} {b:x}", (a + b) % p))
            out.append((f"{field} sub {a:x} {b:x}", (a - b) % p))
            out.append((f"{field} mul {a:x} {b:x}", a * b * rinv % p))
        out.append((f"{field} inv {a:x}", pow(a * rinv, p - 2, p) * R % p))  # (0 maps to 0)
        out += [(f"{field} mac {a:x} {a:x} {n}", n * a * a * rinv % p) for n in MAC_COUNTS]
    out += [(f"{field} redc {v:x}", v * rinv % p) for v in wide_values(field)]
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("fpc") / "field_palette_check")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-x", "c++",
                    "-I", os.path.join(ROOT, "zk-research-implementations_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "field_palette_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@pytest.mark.parametrize("field", xt.FIELDS)
def test_field_hpp_equals_python_integers_on_the_palette(checker, field):
    cs = cases(field)
    assert len(cs) == 42 * 42 * 3 + 42 + 42 * len(MAC_COUNTS) + 2008 == 7552
    r = subprocess.run([checker], input="".join(line + "\n" for line, _ in cs), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split()
    assert len(got) == len(cs)
    wrong = [(line, f"{want:064x}", g) for (line, want), g in zip(cs, got) if int(g, 16) != want]
    assert not wrong, (len(wrong), wrong[:5])


def test_a_malformed_line_is_an_error(checker):
    r = subprocess.run([checker], input="0 add 1\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == ""

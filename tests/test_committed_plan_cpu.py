"""The host-only part of the committed sum-check (csrc/committed_plan.hpp), run
on the CPU: tests/native/committed_plan_check.cpp is a stand-alone program
compiled with the ROCm clang (host code only, no GPU, no library) under ASan +
UBSan. Its self check covers the mask validation and its errors, the powers of
rho and the combined value on the boundary scalars, and the 96-byte point
encoding with infinity; the powers, the encoding and the whole transcript
(commitments absorbed, composed sum-check, rho) are compared with vectors the
Python model (tests/committed_oracle.py) makes."""
from __future__ import annotations

import os
import random
import subprocess

import pytest

import committed_cases as cc
import committed_oracle as mo
import kzg_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "committed_plan_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
R = mo.R


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    exe = str(tmp_path_factory.mktemp("cmpc") / "committed_plan_check")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "zk-research-implementations_amd", "csrc"),
                    SRC, "-o", exe], check=True)
    return exe


def _run(checker, args, values):
    out = subprocess.run([checker] + [str(a) for a in args], input=" ".join(f"{v:x}" for v in values) + "\n",
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout


def test_self_check(checker):
    assert _run(checker, ["self"], []) == "ok cap=16\n"


def test_rho_powers_and_combined_value_match_the_model(checker):
    rng = random.Random(5)
    for rho in (0, 1, R - 1, 2, rng.randrange(R)):
        for k in (1, 2, 3, 16):
            for vals in ([0] * k, [1] * k, [R - 1] * k, [rng.randrange(R) for _ in range(k)]):
                lines = _run(checker, ["rho", k], [rho] + vals).splitlines()
                pows = [pow(rho, j, R) for j in range(k)]
                assert [int(x, 16) for x in lines[0].split()] == pows
                assert int(lines[1], 16) == sum(w * v for w, v in zip(pows, vals)) % R


def test_point_encoding_matches_the_model(checker):
    pts = [None, ko.G1, ko.mul(42, ko.G1), (ko.Q - 1, 1), (1, ko.Q - 1)]  # (the last two: byte order only, not curve points)
    for P in pts:
        x, y = (0, 0) if P is None else P
        assert bytes.fromhex(_run(checker, ["bytes"], [x, y]).strip()) == mo.g1_bytes(P)
    assert mo.g1_bytes(None) == bytes(96)
    assert mo.g1_bytes((1, 2)) == b"\x01" + bytes(47) + b"\x02" + bytes(47)


@pytest.mark.parametrize("nvars", [1, 2, 3])
@pytest.mark.parametrize("name", cc.SHAPES)
def test_transcript_matches_the_model(checker, name, nvars):
    """the byte stream is right if and only if every challenge and rho are the model's"""
    tables, factors, mask = cc.shape(name, nvars)
    proof, _, _ = cc.model_proof(name, nvars)
    args = ["transcript", nvars, len(tables), len(factors), len(factors[0]), mask] + [f for t in factors for f in t]
    vals = [c for P in proof["commitments"] for c in ((0, 0) if P is None else P)] + [v for tb in tables for v in tb]
    lines = dict(ln.split(" ", 1) for ln in _run(checker, args, vals).splitlines())
    assert [int(x, 16) for x in lines["chal"].split()] == proof["challenges"]
    assert [int(x, 16) for x in lines["evals"].split()] == proof["table_evals"]
    assert int(lines["rho"], 16) == proof["rho"]
    idx = mo.committed_indices(mask, len(tables))
    pows = [pow(proof["rho"], j, R) for j in range(len(idx))]
    assert [int(x, 16) for x in lines["pows"].split()] == pows
    assert int(lines["v"], 16) == sum(w * proof["table_evals"][i] for w, i in zip(pows, idx)) % R


def test_a_different_commitment_changes_every_challenge(checker):
    tables, factors, mask = cc.shape("zero_check", 2)
    proof, _, _ = cc.model_proof("zero_check", 2)
    args = ["transcript", 2, len(tables), len(factors), len(factors[0]), mask] + [f for t in factors for f in t]
    cms = [cc.another_point(proof["commitments"][0])] + proof["commitments"][1:]
    vals = [c for P in cms for c in P] + [v for tb in tables for v in tb]
    lines = dict(ln.split(" ", 1) for ln in _run(checker, args, vals).splitlines())
    assert all(int(a, 16) != b for a, b in zip(lines["chal"].split(), proof["challenges"]))
    want = mo.prove(tables, factors, mask, 0, cc.setup(2)[0], mo.Transcript(2), commitments=cms)
    assert int(lines["rho"], 16) == want["rho"] != proof["rho"]


def test_mask_errors(checker):
    base = ["transcript", 2, 3, 1, 2]
    assert _run(checker, base + [0, 0, 1], []).startswith("error=1 ")        # nothing committed
    assert _run(checker, base + [8, 0, 1], []).startswith("error=1 ")        # a bit at ntables
    assert _run(checker, base + [1, 0, 3], []).startswith("error=1 ")        # a factor index >= ntables
    assert _run(checker, ["transcript", 2, 17, 1, 1, 1, 0], []).startswith("error=5 ")  # the composed caps stay

"""The host-only plan of a wired GKR circuit (csrc/wired_plan.hpp), run on the
CPU: tests/native/wired_plan_check.cpp is a stand-alone program compiled with
the ROCm clang (host code only, no GPU, no library) under ASan + UBSan. Its
self check covers the validation errors and caps, the derived widths and round
counts, both gate groupings (permutations, grouped correctly) and the chunking
(every chunk <= T, a row's chunks tile it exactly, rows of fan-out 0, 1, T,
T + 1 and all gates); the shapes it derives are compared with the dense model's."""
from __future__ import annotations

import os
import subprocess

import pytest

import gkr_wired_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "wired_plan_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    exe = str(tmp_path_factory.mktemp("wpc") / "wired_plan_check")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "zk-research-implementations_amd", "csrc"),
                    SRC, "-o", exe], check=True)
    return exe


def test_self_check(checker):
    out = subprocess.run([checker, "self"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("ok ") and "T=256" in out.stdout, out.stdout


@pytest.mark.parametrize("ninputs,gates", [(6, [5, 3, 1]), (4, [16, 4]), (8, [8, 8, 3]), (2, [1]), (1, [1, 1]),
                                           (4096, [4096, 4096, 64, 8]), (1 << 20, [1 << 20, 2]), (3, [1 << 24, 9])])
def test_shape_matches_dense_model(checker, ninputs, gates):
    out = subprocess.run([checker, "shape", str(ninputs)] + [str(g) for g in gates], capture_output=True, text=True,
                         check=True).stdout.split()
    f = dict(kv.split("=") for kv in out)
    below = [ninputs] + gates[:-1]
    assert [int(x) for x in f["kb"].rstrip(",").split(",")] == [wo.nvars(n) for n in below]
    assert [int(x) for x in f["ka"].rstrip(",").split(",")] == [wo.nvars(g) for g in gates]
    assert int(f["total"]) == sum(2 * wo.nvars(n) for n in below)
    assert int(f["v"]) == wo.nvars(gates[-1])


def test_shape_errors(checker):
    run = lambda *a: subprocess.run([checker, "shape", *a], capture_output=True, text=True, check=True).stdout  # noqa: E731
    assert run("4", "3", "0").startswith("error=1 ")       # a zero-gate layer: ZK_EINVAL
    assert run("0", "3").startswith("error=1 ")            # no inputs
    assert run(str((1 << 24) + 1), "3").startswith("error=5 ")  # over a cap: ZK_EUNSUPPORTED
    assert run("3", str((1 << 24) + 1)).startswith("error=5 ")

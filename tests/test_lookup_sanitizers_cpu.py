"""Host sanitizers for the lookup argument's host side (in the manner of
test_r1cs_sanitizers_cpu.py): the product library's host side compiled with
ASan + UBSan (`-Xarch_host -fsanitize=...`: device code is never sanitised) and
linked into the stand-alone tests/native/lookup_asan_check.cpp, which reads a
table, a column and a proof of the Python model from a file this test writes
and drives a host-only handle on it: the proof accepted as given, rejected with
any word changed, the host counts, the table's evaluation and the host
inversion, an error for every hostile argument, and the prover entries without
a device. Any sanitizer report aborts the checker (-fno-sanitize-recover=all).
No Python process loads the sanitised code."""
from __future__ import annotations

import os
import subprocess

import pytest

import lookup_cases as lc
from conftest import ROOT

PKG = os.path.join(ROOT, "zk-research-implementations_amd")


def _gpu_present() -> bool:
    return os.path.exists("/dev/kfd")


def _words(n: int) -> list[int]:
    table, f = lc.small(n)
    proof = lc.model_proof(n)
    out = [n, len(table)] + list(table) + list(f)
    for q in proof["polys"]:
        out += [len(q)] + list(q) + [0] * (4 - len(q))
    out += list(proof["table_evals"])
    for P in list(proof["commitments"]) + list(proof["opening"]):
        out += [0, 0] if P is None else list(P)
    for (x0, x1), (y0, y1) in lc.setup(n)[1]:
        out += [x0, x1, y0, y1]
    return out


@pytest.fixture(scope="module")
def checker():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    if _gpu_present():
        pytest.skip("sanitised code is not run on a machine with a GPU")
    # the sanitised objects are the ones `make asan` builds; make is a no-op when they are up to date
    jobs = os.environ.get("MAX_JOBS", "8")
    subprocess.run(["make", "-s", "-j", jobs, "-C", PKG, "asan-lookup"], check=True, timeout=1800)
    return os.path.join(PKG, "build", "asan", "lookup_asan_check")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_lookup_host_side_under_asan_ubsan(checker, tmp_path, n):
    path = tmp_path / "proof.txt"
    path.write_text(" ".join(f"{v:x}" for v in _words(n)) + "\n")
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "lookup_asan_check ok" in r.stdout

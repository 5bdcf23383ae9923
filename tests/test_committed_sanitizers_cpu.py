"""Host sanitizers for the committed sum-check's verifiers (in the manner of
test_merkle_sanitizers_cpu.py): the product library's host side compiled with
ASan + UBSan (`-Xarch_host -fsanitize=...`: device code is never sanitised) and
linked into the stand-alone tests/native/committed_asan_check.cpp, which reads a
proof of the Python model and drives zk_committed_sumcheck_verify,
zk_kzg_batch_verify and zk_mle_eq_eval on it: accepted as given, rejected with
any word changed, an error for every hostile argument (values >= p, points off
the curve, masks and counts out of range, null pointers), and the device entry
points without a device. Any sanitizer report aborts the checker
(-fno-sanitize-recover=all). No Python process loads the sanitised code."""
from __future__ import annotations

import os
import subprocess

import pytest

import committed_cases as cc
from conftest import ROOT

PKG = os.path.join(ROOT, "zk-research-implementations_amd")


def _gpu_present() -> bool:
    return os.path.exists("/dev/kfd")


def _words(name: str, nvars: int) -> list[int]:
    proof, factors, claim = cc.model_proof(name, nvars)
    degree = len(factors[0])
    out = [nvars, len(proof["table_evals"]), len(factors), degree, proof["mask"]] + [f for t in factors for f in t]
    out.append(claim)
    for q in proof["polys"]:
        out += [len(q)] + list(q) + [0] * (degree + 1 - len(q))
    out += proof["table_evals"] + [proof["rho"]]
    for P in proof["commitments"] + proof["opening"]:
        out += [0, 0] if P is None else list(P)
    for (x0, x1), (y0, y1) in cc.setup(nvars)[1]:
        out += [x0, x1, y0, y1]
    return out


@pytest.fixture(scope="module")
def checker():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    if _gpu_present():
        pytest.skip("the checker expects zk_ctx_create to fail without a GPU")
    # the sanitised objects are the ones `make asan` builds; make is a no-op when they are up to date
    jobs = os.environ.get("MAX_JOBS", "8")
    subprocess.run(["make", "-s", "-j", jobs, "-C", PKG, "asan-committed"], check=True, timeout=1800)
    return os.path.join(PKG, "build", "asan", "committed_asan_check")


@pytest.mark.parametrize("name,nvars", [("zero_check", 3), ("three_zero", 2), ("same_pointer", 2), ("one", 1)])
def test_committed_verifiers_under_asan_ubsan(checker, name, nvars):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker], input=" ".join(f"{v:x}" for v in _words(name, nvars)) + "\n", capture_output=True,
                       text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "committed_asan_check ok" in r.stdout

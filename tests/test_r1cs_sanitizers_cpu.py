"""Host sanitizers for the R1CS prover's host side (in the manner of
test_committed_sanitizers_cpu.py): the product library's host side compiled with
ASan + UBSan (`-Xarch_host -fsanitize=...`: device code is never sanitised) and
linked into the stand-alone tests/native/r1cs_asan_check.cpp, which reads an
instance and a proof of the Python model from a file this test writes and
drives a host-only handle on it: the proof accepted as given, rejected with any
word changed, the host multiplication and matrix evaluation, an error for every
out-of-range input, and the prover entries without a device. Any sanitizer
report aborts the checker (-fno-sanitize-recover=all). No Python process loads
the sanitised code."""
from __future__ import annotations

import os
import subprocess

import pytest

import r1cs_cases as rc
from conftest import ROOT

PKG = os.path.join(ROOT, "zk-research-implementations_amd")


def _gpu_present() -> bool:
    return os.path.exists("/dev/kfd")


def _words(name: str, field: int, committed: bool) -> list[int]:
    inst, _, io = rc.case(name, field)
    proof = rc.model_proof(name, field, committed)
    out = [field, inst.nrows, inst.sy, inst.npub] + [len(m) for m in inst.matrices]
    out += [x for m in inst.matrices for e in m for x in e]
    out += list(io) + [int(committed)]
    for polys, slots in ((proof["polys1"], 4), (proof["polys2"], 3)):
        for q in polys:
            out += [len(q)] + list(q) + [0] * (slots - len(q))
    out += [proof["va"], proof["vb"], proof["vc"], proof["vw"]]
    if committed:
        for P in [proof["commitment"]] + proof["opening"]:
            out += [0, 0] if P is None else list(P)
        for (x0, x1), (y0, y1) in rc.setup(inst.sy - 1)[1]:
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
    subprocess.run(["make", "-s", "-j", jobs, "-C", PKG, "asan-r1cs"], check=True, timeout=1800)
    return os.path.join(PKG, "build", "asan", "r1cs_asan_check")


@pytest.mark.parametrize("name,field,committed", [("3_4", 0, False), ("1_1", 1, False), ("chain5", 2, False),
                                                  ("cubic", 2, True), ("2_2", 2, True)])
def test_r1cs_host_side_under_asan_ubsan(checker, tmp_path, name, field, committed):
    path = tmp_path / "proof.txt"
    path.write_text(" ".join(f"{v:x}" for v in _words(name, field, committed)) + "\n")
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "r1cs_asan_check ok" in r.stdout

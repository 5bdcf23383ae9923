"""Host sanitizers for the univariate polynomial entry points (in the manner of
test_fft_sanitizers_cpu.py): the product library's host side compiled with
ASan + UBSan (`-Xarch_host -fsanitize=...`: device code is never sanitised) and
linked into the stand-alone tests/native/poly_asan_check.cpp, which drives
zk_poly_evaluate / zk_dev_poly_evaluate / zk_poly_eval_plan /
zk_poly_interpolate without a device on valid and hostile arguments (sizes
beyond the caps, n = 2^63 + 1, cap = 0, null buffers, an unknown field, values
>= p) and the host path of csrc/poly_host.hpp, compiled into the checker under
the same sanitizers, on real inputs in exactly-sized heap buffers. Any
sanitizer report aborts the checker (-fno-sanitize-recover=all). No Python
process loads the sanitised code."""
from __future__ import annotations

import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "zk-research-implementations_amd")


def _gpu_present() -> bool:
    return os.path.exists("/dev/kfd")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not present")
@pytest.mark.skipif(_gpu_present(), reason="the checker expects zk_ctx_create to fail without a GPU")
def test_poly_host_side_under_asan_ubsan():
    # the sanitised objects are the ones `make asan` builds; make is a no-op when they are up to date
    jobs = os.environ.get("MAX_JOBS", "8")
    subprocess.run(["make", "-s", "-j", jobs, "-C", PKG, "asan-poly"], check=True, timeout=1800)
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "build", "asan", "poly_asan_check")], capture_output=True, text=True, env=e,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "poly_asan_check ok" in r.stdout

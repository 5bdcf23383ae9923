"""bench.py's arguments and --dump-outputs files, on the CPU (no GPU is touched)."""
from __future__ import annotations

import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_side_legs_and_full_turns_them_on(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 2, None)
    a = _parse(monkeypatch, "--full", "--no-config4", "--dump-outputs", "somewhere")
    assert a.full and not a.config4 and a.dump_outputs == "somewhere"
    assert not (a.no_serving or a.no_e2e or a.no_fold or a.no_circuit or a.no_config5 or a.no_plain or a.no_cpu_baseline)


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_that_cannot_be_timed_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_round_trips_every_limb(tmp_path):
    rng = np.random.default_rng(7)
    n = 5
    coeffs = rng.integers(0, 1 << 64, size=(n, 3, 4), dtype=np.uint64)
    coeffs[0, 0, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)  # no float64 holds this u64; its 32-bit words are exact
    nco = np.array([3, 3, 2, 3, 1], np.uint8)
    ch = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    out = tmp_path / "deep" / "dir"
    bench.dump_outputs(str(out), coeffs, nco, ch)
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["challenges.npy", "round_poly_coeffs.npy", "round_poly_ncoeffs.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["round_poly_coeffs.npy"].shape == (n, 3, 8) and got["challenges.npy"].shape == (n, 8)
    back = got["round_poly_coeffs.npy"].astype("<u4").view("<u8").reshape(n, 3, 4)
    assert np.array_equal(back, coeffs)
    assert np.array_equal(got["challenges.npy"].astype("<u4").view("<u8").reshape(n, 4), ch)
    assert np.array_equal(got["round_poly_ncoeffs.npy"], nco.astype(np.float64))

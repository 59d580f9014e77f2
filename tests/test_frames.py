"""The frame selection and the tile cover of the history analyses (csrc/gdyn_frames.hpp) on the CPU: tests/native/test_frames.cpp holds
gd::frames_fit, gd::frames_served and gd::tile_cover to brute-force loops at their edges (one frame, selections past the history, exactly
one frame that fits, 2^32 - 1 without wrap-around; rectangles inside a tile, across a boundary, above their columns, with and without
diagonal tiles, the last partial tile), gd::lag_windows to a search over small budgets and at the two real ones (160 KiB of float32 and
float64 rows, and budgets that hold fewer than two rows), and gd::sort_lags on a few lists."""
import os
import subprocess

import pytest
from conftest import ROOT

PKG_DIR = "2022a-genome-dynamics_amd"


def _compile(exe, *flags):
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, PKG_DIR, "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "native", "test_frames.cpp")]


def test_frames_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_frames")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "frames: ok" in out.stdout, out.stdout + out.stderr


def test_frames_against_brute_force_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan (CPU build), where the compiler offers them."""
    sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.call(["g++", *sanitize, "-o", str(tmp_path / "probe"), str(probe)], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this compiler has no sanitizer runtime: the plain build covers the arithmetic")
    exe = str(tmp_path / "test_frames_asan")
    subprocess.check_call(_compile(exe, *sanitize))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "frames: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_frames_header_needs_no_hip_runtime_or_error_reporting():
    """The header is plain C++: no HIP call, no handle, no fail()."""
    import re
    src = open(os.path.join(ROOT, PKG_DIR, "csrc", "gdyn_frames.hpp")).read()
    assert not re.search(r"hip[A-Z_]|HIPCHK|fail\(|gdyn_analysis", src)

"""The option scanner of the analysis programs (host/gd_cli_args.hpp) on the CPU: tests/native/test_cli_args.cpp drives it with
three tables (long options only, long plus short options with attached values, one flag only) over argv arrays of exactly argc
pointers, and checks the three messages it owns, the tokens at the edge of the option syntax and that no key matches by prefix."""
import os
import re
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")


def _compile(exe, *flags):
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "test_cli_args.cpp")]


def test_scanner(tmp_path):
    exe = str(tmp_path / "test_cli_args")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "cli args: ok" in out.stdout, out.stdout + out.stderr


def test_scanner_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan, where the compiler offers them: nothing past argv[argc - 1] is read."""
    exe = str(tmp_path / "test_cli_args_asan")
    if subprocess.call(_compile(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), stderr=subprocess.DEVNULL) != 0:
        return      # (no sanitizer runtime: the plain build above covers the answers)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "cli args: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_scanner_header_stands_alone():
    """The scanner is the standard library's: no HDF5, no libgdyn, and it includes no header of the project."""
    src = open(os.path.join(HOST, "gd_cli_args.hpp")).read()
    assert not re.search(r'hdf5|gdyn\.h|H5[A-Z]|#include "', src)

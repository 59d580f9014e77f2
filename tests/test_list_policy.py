"""The list policy of libgdyn (csrc/gdyn_policy.hpp) on the CPU: tests/native/test_list_policy.cpp drives gd::ListPolicy with synthetic
build reports and accepted chunks and checks the decisions of its rules (tile class, dense states, row width, single-class lists,
memory guard, width by tile class, interval adaptation, the auto_skin sweep)."""
import os
import subprocess

from conftest import ROOT

PKG_DIR = "2022a-genome-dynamics_amd"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compile(exe, *flags):
    # gdyn_types.h needs the HIP vector types only: the HIP headers, no HIP runtime
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
            "-I", os.path.join(ROOT, PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "test_list_policy.cpp")]


def test_list_policy_decisions(tmp_path):
    exe = str(tmp_path / "test_list_policy")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "policy: ok" in out.stdout, out.stdout + out.stderr


def test_list_policy_decisions_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan (CPU build), where the compiler offers them."""
    exe = str(tmp_path / "test_list_policy_asan")
    if subprocess.call(_compile(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), stderr=subprocess.DEVNULL) != 0:
        return      # (no sanitizer runtime: the plain build above covers the decisions)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "policy: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_list_policy_header_needs_no_hip_runtime_or_environment():
    """The policy is plain C++: no HIP API call, no handle, no environment variable."""
    import re
    src = open(os.path.join(ROOT, PKG_DIR, "csrc", "gdyn_policy.hpp")).read()
    assert not re.search(r"hip[A-Z]|getenv|dev_env|gd_system", src)

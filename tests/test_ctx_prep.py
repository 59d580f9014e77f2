"""The prepared-context rule of the grouped step launches (csrc/gdyn_policy.hpp: gd::ctx_prepared) on the CPU:
tests/native/test_ctx_prep.cpp pins the table of its decisions (only in spans that run in two groups, the three group modes, the
threshold, the developer override); the entry points of include/gdyn_prep.h are libgdyn.so's alone."""
import os
import re
import subprocess

from conftest import ROOT

PKG_DIR = "2022a-genome-dynamics_amd"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compile(exe, *flags):
    # gdyn_types.h needs the HIP vector types only: the HIP headers, no HIP runtime
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
            "-I", os.path.join(ROOT, PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "test_ctx_prep.cpp")]


def test_ctx_prep_rule(tmp_path):
    exe = str(tmp_path / "test_ctx_prep")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ctx prep: ok" in out.stdout, out.stdout + out.stderr


def test_ctx_prep_rule_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan (CPU build, a stand-alone program), where the compiler offers them."""
    exe = str(tmp_path / "test_ctx_prep_asan")
    if subprocess.call(_compile(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), stderr=subprocess.DEVNULL) != 0:
        return      # (no sanitizer runtime: the plain build above covers the decisions)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "ctx prep: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_prep_header_is_outside_the_core_abi():
    """include/gdyn_prep.h has its own version; include/gdyn.h and include/gdyn_groups.h declare none of its symbols, the library
    exports both of them, and none is in ABI_SYMBOLS."""
    import importlib
    gdyn = importlib.import_module(PKG_DIR)
    inc = os.path.join(ROOT, "include")
    hdr = open(os.path.join(inc, "gdyn_prep.h")).read()
    names = re.findall(r"^int\s+(gd_\w+)\(", hdr, flags=re.M)
    assert set(names) == {"gd_prep_abi_version", "gd_get_ctx_prepared"}
    assert re.search(r"^#define GD_PREP_ABI_VERSION 1$", hdr, flags=re.M)
    for other in ("gdyn.h", "gdyn_groups.h"):
        text = open(os.path.join(inc, other)).read()
        assert not any(n in text for n in names), other
    assert not set(names) & set(gdyn.ABI_SYMBOLS)
    groups = re.findall(r"^int\s+(gd_\w+)\(", open(os.path.join(inc, "gdyn_groups.h")).read(), flags=re.M)
    assert set(groups) == {"gd_groups_abi_version", "gd_set_step_groups", "gd_get_step_groups"}      # (as it was)
    if not os.path.exists(gdyn.LIBGDYN_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(gdyn.LIBGDYN_PATH)])
    exported = subprocess.check_output(["nm", "-D", "--defined-only", gdyn.LIBGDYN_PATH], text=True)
    for n in names:
        assert re.search(rf"\bT {n}\b", exported), n
    pol = open(os.path.join(ROOT, PKG_DIR, "csrc", "gdyn_policy.hpp")).read()
    assert re.search(r"CTX_PREP_NEVER = 0, CTX_PREP_RULE = 1, CTX_PREP_ALWAYS = 2", pol)

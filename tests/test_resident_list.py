"""The resident list of a handle (csrc/gdyn_list.hpp) on the CPU: tests/native/test_resident_list.cpp drives gd::ResidentList alone
through every event that changes it (the transition table of DESIGN.md) and checks its queries -- row-width prediction, freshness for an
observation, pair searches, the list fields of gd_context.  Two source checks hold the handle's host files to calling the transitions."""
import glob
import os
import re
import subprocess

from conftest import ROOT

PKG_DIR = "2022a-genome-dynamics_amd"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CSRC = os.path.join(ROOT, PKG_DIR, "csrc")


def _compile(exe, *flags):
    # gdyn_types.h (through gdyn_policy.hpp) needs the HIP vector types only: the HIP headers, no HIP runtime
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
            "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "test_resident_list.cpp")]


def test_resident_list_transitions(tmp_path):
    exe = str(tmp_path / "test_resident_list")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "resident list: ok" in out.stdout, out.stdout + out.stderr


def test_resident_list_transitions_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan (CPU build), where the compiler offers them."""
    exe = str(tmp_path / "test_resident_list_asan")
    if subprocess.call(_compile(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), stderr=subprocess.DEVNULL) != 0:
        return      # (no sanitizer runtime: the plain build above covers the transitions)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "resident list: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_resident_list_header_needs_no_hip_runtime_or_environment():
    """The list state is plain C++: no HIP API call, no handle, no environment variable."""
    src = open(os.path.join(CSRC, "gdyn_list.hpp")).read()
    assert not re.search(r"hip[A-Z]|getenv|dev_env|gd_system", src)


def _members():
    """Data members of gd::ResidentList, from its declaration (up to the first transition)."""
    src = open(os.path.join(CSRC, "gdyn_list.hpp")).read()
    body = src[src.index("struct ResidentList {"):src.index("// ---- transitions")]
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for decl in re.findall(r"\b(?:bool|int|float|uint32_t|uint64_t)\s+([^;]+);", body):
        names += [re.match(r"\s*(\w+)", part).group(1) for part in decl.split(",")]
    return names


def test_capi_assigns_no_member_of_the_resident_list():
    """The handle's host files (gdyn_capi.hip, the gdyn_capi_*.hip of the features) and the header that declares the handle
    (gdyn_system.hpp) change the list state through the named transitions only: the handle has one ResidentList, none of the loose
    members it replaced, and no statement assigns, increments or takes a reference to a member of it."""
    members = _members()
    assert set(members) >= {"valid", "tiled", "W", "tile_cap", "rv", "rn", "steps_since_build", "search_list", "verified_serial", "w_packed",
                            "bbox_cur", "bbox_valid", "need_valid", "need_rv", "need_all_near", "order_valid", "pool_used", "repairs"}, members
    files = sorted(glob.glob(os.path.join(CSRC, "gdyn_capi*.hip")))
    assert len(files) == 4, files
    src = "\n".join(open(f).read() for f in files + [os.path.join(CSRC, "gdyn_system.hpp")])
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
    assert len(re.findall(r"\bgd::ResidentList\s+\w+\s*;", code)) == 1
    alt = "|".join(members)
    # s->list.member followed by an assignment operator (not ==, <=, >=, !=), ++ / --, or preceded by ++ / -- / & (a reference handed on)
    writes = re.findall(r"(?:(?:\+\+|--|&)\s*)?\b\w+(?:->|\.)list\.(?:%s)\b\s*(?:=(?!=)|[-+*/%%^|&]=|<<=|>>=|\+\+|--)" % alt, code)
    writes += re.findall(r"(?:\+\+|--|[^&]&)\s*\w+(?:->|\.)list\.(?:%s)\b" % alt, code)
    assert not writes, writes
    assert not re.search(r"(?:->|\.)list\s*=(?!=)", code)                      # ... nor replaces the whole struct
    old = r"s->(?:list_valid|list_tiled|list_W|list_tile_cap|rv|rn|steps_since_build|search_list|verified_serial|w_packed|bbox_cur|bbox_valid|" \
          r"need_valid|need_rv|need_all_near|pool_used|repairs)\b"
    assert not re.search(old, code)

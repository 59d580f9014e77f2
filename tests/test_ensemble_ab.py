"""Per-replica A/B tables without a GPU: the host logic (csrc/gdyn_ensemble.hpp) driven alone by tests/native/test_ensemble_ab.cpp --
classes by first appearance, tables set back, a column left out, one value fp16 does not hold, N = 1 -- in a plain build and under
AddressSanitizer + UBSan (a stand-alone program); the symbols of include/gdyn_ensemble.h against the binding and the library; what
gd_interphase does with files whose A/B factors differ where the library has no per-replica tables, and with an --ensemble-matrix
output that lacks {model}; gd_randomize.py against outputs recorded from the reference's module."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

PKG_DIR = "2022a-genome-dynamics_amd"
CSRC = os.path.join(ROOT, PKG_DIR, "csrc")
HOST = os.path.join(ROOT, PKG_DIR, "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


# ---------------------------------------------------------------------------------------------- the host logic alone

def _compile(exe, *flags):
    return ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", exe,
            os.path.join(ROOT, "tests", "native", "test_ensemble_ab.cpp")]


def test_ensemble_tables(tmp_path):
    exe = str(tmp_path / "test_ensemble_ab")
    subprocess.check_call(_compile(exe))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ensemble ab: ok" in out.stdout, out.stdout + out.stderr


def test_ensemble_tables_under_sanitizers(tmp_path):
    """The same under AddressSanitizer + UBSan (CPU build), where the compiler offers them."""
    exe = str(tmp_path / "test_ensemble_ab_asan")
    if subprocess.call(_compile(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), stderr=subprocess.DEVNULL) != 0:
        return      # (no sanitizer runtime: the plain build above covers the logic)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "ensemble ab: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_ensemble_header_needs_no_hip_runtime_or_environment():
    src = open(os.path.join(CSRC, "gdyn_ensemble.hpp")).read()
    assert not re.search(r"hip[A-Z_/]|getenv|dev_env|gd_system", src)


def test_ensemble_header_is_outside_the_gdyn_abi():
    """include/gdyn_ensemble.h has its own version; gdyn.h and gdyn_replica.h declare none of its symbols; libgdyn exports exactly them."""
    inc = os.path.join(ROOT, "include")
    for other in ("gdyn.h", "gdyn_replica.h"):
        assert "gd_ensemble" not in open(os.path.join(inc, other)).read(), other
    hdr = open(os.path.join(inc, "gdyn_ensemble.h")).read()
    names = re.findall(r"^int (gd_ensemble_\w+)\(", hdr, flags=re.M)
    assert names == ["gd_ensemble_abi_version", "gd_ensemble_set_ab", "gd_ensemble_get_ab", "gd_ensemble_classes"]
    assert re.search(r"#define GD_ENSEMBLE_ABI_VERSION 1\b", hdr)
    gdyn = importlib.import_module(PKG_DIR)
    ensemble = importlib.import_module(PKG_DIR + ".ensemble")
    assert names == ensemble.ENSEMBLE_SYMBOLS and ensemble.ENSEMBLE_ABI_VERSION == 1
    assert not set(names) & set(gdyn.ABI_SYMBOLS)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", gdyn.LIBGDYN_PATH], text=True)
    assert set(re.findall(r"\bT (gd_ensemble_\w+)", exported)) == set(names)
    oracle = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "oracle", "liboracle.so")], text=True)
    assert "gd_ensemble" not in oracle


# ---------------------------------------------------------------------------------------------- gd_interphase

def permute_ab(d, seed):
    """Rewrites <d>/traj.h5, as test_host_driver._inputs left it, with its A/B columns under a seeded permutation of the beads;
    everything else -- config, chromosome table, initial structure -- stays.  Returns the permuted (a, b)."""
    ab = np.fromfile(d / "ab.f64", dtype="<f8").reshape(-1, 2)
    ab = ab[np.random.default_rng(seed).permutation(len(ab))]
    ab.astype("<f8").tofile(d / "ab.f64")
    os.remove(d / "traj.h5")
    subprocess.check_call([os.path.join(HOST, "gd_h5tool"), "make-input", str(d / "traj.h5"), str(d / "config.json"),
                           str(d / "chroms.tsv"), str(d / "ab.f64"), str(d / "pos.f64")])
    return ab[:, 0].copy(), ab[:, 1].copy()


def _two_models(tmp):
    """Two prepared files that differ in ab.f64 alone"""
    from test_host_driver import _inputs
    files = []
    for k in range(2):
        d = tmp / f"run{k}"
        d.mkdir()
        _inputs(d)
        if k == 1:
            permute_ab(d, 3)
        files.append(d / "traj.h5")
    assert files[0].read_bytes() != files[1].read_bytes()
    return files


@needs_h5
def test_library_without_tables_refuses_differing_models(tmp_path, oracle):
    """The oracle exports gdyn.h alone: the driver linked against it still builds (the gd_ensemble_* symbols are weak references) and
    refuses the batch with the message it always had."""
    from test_host_driver import _env, _make_oracle
    drv = _make_oracle("gd_interphase", tmp_path)
    files = _two_models(tmp_path)
    r = subprocess.run([str(drv), *map(str, files)], capture_output=True, text=True, env=_env(os.path.join(ROOT, "oracle")))
    assert r.returncode == 1 and "A/B factors differ" in r.stderr and "[model" not in r.stderr, (r.returncode, r.stderr)


@needs_h5
def test_ensemble_matrix_of_several_models_needs_the_placeholder(tmp_path):
    """The device-linked program, before it touches a device or a file: two models and an output without {model}."""
    from test_host_driver import _make
    drv = _make("gd_interphase", ".", "../csrc", "gdyn")
    files = _two_models(tmp_path)
    before = [f.read_bytes() for f in files]
    out = tmp_path / "out.h5"
    r = subprocess.run([str(drv), "--ensemble-matrix", "4", str(out), *map(str, files)], capture_output=True, text=True)
    assert r.returncode == 1 and "{model}" in r.stderr and "2 models" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists() and [f.read_bytes() for f in files] == before
    assert not [p for p in os.listdir(tmp_path) if p.endswith(".h5")]


# ---------------------------------------------------------------------------------------------- gd_randomize.py

RANDOMIZE = os.path.join(HOST, "gd_randomize.py")
MODES = {"default": [], "preserve": ["--preserve-structure"], "random": ["--completely-random"]}
FIXTURE_SEED = 20220101      # tests/golden/make_randomize_fixtures.py


def _golden(name):
    with open(os.path.join(GOLDEN, f"randomize_{name}.tsv"), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("mode", list(MODES))
def test_randomize_equals_the_reference(tmp_path, mode):
    """Byte for byte what the reference's module wrote for the same table, seed and mode: on stdout and through -o."""
    genome = os.path.join(GOLDEN, "randomize_genome.tsv")
    r = subprocess.run([sys.executable, RANDOMIZE, "--seed", str(FIXTURE_SEED), *MODES[mode], genome], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == _golden(mode)
    assert f"seed {FIXTURE_SEED}" in r.stderr.decode()      # the seed is echoed, beside the table
    out = tmp_path / "control.tsv"
    r = subprocess.run([sys.executable, RANDOMIZE, "--seed", str(FIXTURE_SEED), *MODES[mode], "-o", str(out), genome], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == _golden(mode)


def test_randomize_fixtures_are_controls_of_their_model():
    """What the batching rests on: in every mode chain, start, end stay on their rows and so do the structural tags; the modes differ
    from the model and from each other."""
    rows = {name: [ln.split("\t") for ln in _golden(name).decode().splitlines()] for name in ("genome", *MODES)}
    for mode in MODES:
        assert len(rows[mode]) == len(rows["genome"]) and rows[mode][0] == rows["genome"][0]
        for got, want in zip(rows[mode][1:], rows["genome"][1:]):
            assert got[:3] == want[:3]
            assert [t for t in got[5].split(",") if t not in "ABu"] == [t for t in want[5].split(",") if t not in "ABu"]
        assert [r[3:5] for r in rows[mode]] != [r[3:5] for r in rows["genome"]]
    structural = [any(s in r[5] for s in ("cen", "anor", "bnor")) for r in rows["genome"]]
    assert any(structural)
    for got, want, keep in zip(rows["preserve"], rows["genome"], structural):
        assert not keep or got[3:5] == want[3:5]
    assert all(r[3:5] in (["1.0", "0.0"], ["0.0", "1.0"]) for r in rows["random"][1:])


def test_randomize_unseeded_run_names_its_seed_and_repeats():
    genome = os.path.join(GOLDEN, "randomize_genome.tsv")
    r = subprocess.run([sys.executable, RANDOMIZE, genome], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    seed = re.search(r"seed (\d+)", r.stderr).group(1)
    again = subprocess.run([sys.executable, RANDOMIZE, "--seed", seed, genome], capture_output=True, text=True)
    assert again.returncode == 0 and again.stdout == r.stdout


def test_randomize_refuses_both_modes_together(tmp_path):
    out = tmp_path / "control.tsv"
    r = subprocess.run([sys.executable, RANDOMIZE, "--preserve-structure", "--completely-random", "-o", str(out),
                        os.path.join(GOLDEN, "randomize_genome.tsv")], capture_output=True, text=True)
    assert r.returncode != 0 and "can not both be specified" in r.stderr and not out.exists()

"""Host side of the lamina analysis (no GPU): the restatement (tests/lamina_restatement.py) and lamina.distance_from_surface
against the reference's own outputs (tests/golden/lamina_fixtures.npz, made by make_lamina_fixtures.py), the gd_lamina_*
symbols of libgdyn against include/gdyn_lamina.h, and the command line of gd_analyze_lamina."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import lamina_restatement as R
from conftest import ROOT

PKG = "2022a-genome-dynamics_amd"
lamina = importlib.import_module(PKG + ".lamina")
HOST = os.path.join(ROOT, PKG, "host")
Z = np.load(os.path.join(ROOT, "tests", "golden", "lamina_fixtures.npz"))
SETS = range(int(Z["n_sets"]))
HISTS = range(int(Z["n_hist"]))
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


def test_fixtures_cover_the_cases():
    assert len(SETS) >= 3
    semis = [Z[f"semi{k}"] for k in SETS]
    assert any(s[0] == s[1] == s[2] for s in semis) and any(s.max() / s.min() > 4 for s in semis)      # a sphere, a strongly oblate wall
    assert sum(int(np.isnan(Z[f"dist{k}"]).sum()) for k in SETS) > 0
    for k in SETS:
        x, d, s = Z[f"points{k}"], Z[f"dist{k}"], Z[f"semi{k}"]
        assert x.dtype == np.float32 and d.dtype == np.float64 and Z[f"points64_{k}"].dtype == np.float64
        origin = np.flatnonzero(~x.any(axis=1))
        assert len(origin) and (d[origin] == 0).all()                       # a = b = 0: distance 0
        level = ((x.astype(np.float64) / s) ** 2).sum(axis=1)
        assert (level < 0.8).any() and (np.abs(level - 1) < 1e-6).any() and (level > 1.2).any()
    assert any((np.diff(Z[f"hist_semi{t}"], axis=0) != 0).all() for t in HISTS)      # semiaxes of their own in every frame


@pytest.mark.parametrize("k", SETS)
def test_restatement_equals_the_reference(k):
    s = Z[f"semi{k}"]
    for x, d in [(Z[f"points{k}"], Z[f"dist{k}"]), (Z[f"points64_{k}"], Z[f"dist64_{k}"])]:
        assert R.same(R.distances(x, s), d)
        assert R.same(lamina.distance_from_surface(x, s), d)
        assert R.same(np.array([R.distance_scalar(p, s) for p in x]), d)


@pytest.mark.parametrize("t", HISTS)
def test_history_restatement_equals_the_reference(t):
    x, s, d = Z[f"hist_points{t}"], Z[f"hist_semi{t}"], Z[f"hist_dist{t}"]
    assert R.same(R.history(x, s), d)
    assert R.same(np.stack([lamina.distance_from_surface(x[f], s[f]) for f in range(len(x))]), d)


def test_contact_restatement_equals_the_fixtures():
    stored = [Z[f"hist_dist{t}"].astype(np.float32) for t in HISTS]
    for j, D in enumerate(Z["thresholds"]):
        cs = [R.contacts(d, D) for d in stored]
        for t in HISTS:
            assert np.array_equal(cs[t], Z[f"contact{j}_{t}"])
            assert not cs[t][np.isnan(stored[t])].any()                      # NaN is never a contact
        avg = R.average(cs)
        assert avg.dtype == np.float32 and np.array_equal(avg, Z[f"average{j}"])
        count = np.sum(cs, axis=0)
        assert np.array_equal(avg, (count.astype(np.float64) / len(cs)).astype(np.float32))
    # a threshold at a stored value excludes that value (strict <), the next float up includes it
    D = float(Z["thresholds"][2])
    at = np.flatnonzero(stored[1].ravel() == np.float32(D))
    assert len(at) and not R.contacts(stored[1], D).ravel()[at].any() and R.contacts(stored[1], np.nextafter(D, 1)).ravel()[at].all()


def test_library_exports_lamina_symbols(gdyn):
    d = C.CDLL(gdyn.LIBGDYN_PATH)
    for name in lamina.LAMINA_SYMBOLS:
        assert hasattr(d, name), name
    d.gd_lamina_abi_version.restype = C.c_int
    assert d.gd_lamina_abi_version() == lamina.LAMINA_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "gdyn_lamina.h")).read()
    assert set(re.findall(r"^int\s+(gd_lamina_\w+)\(", hdr, flags=re.M)) == set(lamina.LAMINA_SYMBOLS)
    assert f"#define GD_LAMINA_ABI_VERSION {lamina.LAMINA_ABI_VERSION}" in hdr
    exported = subprocess.check_output(["nm", "-D", "--defined-only", gdyn.LIBGDYN_PATH], text=True)
    assert set(re.findall(r"\bT (gd_lamina_\w+)", exported)) == set(lamina.LAMINA_SYMBOLS)
    lamina.load_lamina_library()


@pytest.fixture(scope="module")
def program():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_analyze_lamina"])
    return os.path.join(HOST, "gd_analyze_lamina")


def _run(program, *args):
    return subprocess.run([program, *map(str, args)], capture_output=True, text=True)


@needs_h5
def test_command_line_errors(program, tmp_path):
    out = tmp_path / "out.h5"
    cases = [([], "command"), (["plot", out], "invalid choice: 'plot'"), (["distance"], "outfile, trajfiles"), (["distance", out], "outfile, trajfiles"),
             (["contact", "--contact-distance", "0.3"], "outfile"), (["contact", "--contact-distance", "x", out], "invalid float value: 'x'"),
             (["contact", "--contact-distance"], "expected one argument"), (["contact", "--contact-distance=0.3", out, "extra"], "unrecognized arguments: extra"),
             (["distance", "--name", "n", out, "t.h5"], "unrecognized arguments: --name"), (["contact", "--bogus=1", "--contact-distance=1", out], "--bogus")]
    for args, what in cases:
        r = _run(program, *args)
        assert r.returncode == 2 and r.stderr.startswith("usage: gd_analyze_lamina") and what in r.stderr, (args, r.stderr)
        assert "gd_analyze_lamina: error:" in r.stderr
    assert not out.exists()


@needs_h5
def test_contact_distance_is_required(program, tmp_path):
    """The documented deviation: the reference's default None fails inside numpy after the file was opened."""
    r = _run(program, "contact", tmp_path / "out.h5")
    assert r.returncode == 2 and "the following arguments are required: --contact-distance" in r.stderr
    r = _run(program, "contact", "--dry-run", tmp_path / "out.h5")
    assert r.returncode == 2
    assert not (tmp_path / "out.h5").exists()


@needs_h5
def test_dry_run(program, tmp_path):
    out = tmp_path / "out.h5"
    r = _run(program, "distance", "--dry-run", out, "runs/a.h5", "b.trajectory.h5")
    assert r.returncode == 0, r.stderr
    lines = [l.split("\t") for l in r.stdout.splitlines()]
    assert ["read", "runs/a.h5", "/metadata/{config,particle_types,chromosome_ranges}"] in lines
    assert ["read", "b.trajectory.h5", "/snapshots/interphase/<step>/{positions,context}"] in lines
    assert [l[2] for l in lines if l[0] == "write"] == ["/metadata/{simulation_config,particle_types,chromosome_ranges,chromosome_names}",
                                                        "/distance/a", "/distance/b.trajectory"]
    for args, name in [(["--contact-distance", "0.25"], "uniform"), (["--name=near", "--contact-distance=0.25"], "near")]:
        r = _run(program, "contact", *args, "--dry-run", out)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == ["contact_distance\t0.25", f"read\t{out}\t/distance/<key>", f"write\t{out}\t/contact/{name}/<key>",
                                         f"write\t{out}\t/average_contact/{name}"]
    assert not out.exists()


@needs_h5
def test_runtime_errors_exit_1(program, tmp_path):
    """Without a device, or with a device and an unreadable input, the program says `error: <what>` and exits 1."""
    r = _run(program, "distance", tmp_path / "out.h5", tmp_path / "missing.h5")
    assert r.returncode == 1 and r.stderr.startswith("error: "), r.stderr

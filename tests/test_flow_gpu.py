"""The flow analyses on the device (include/gdyn_flow.h, csrc/gdyn_flow.hip) against the reference's own outputs
(tests/golden/flow_fixtures.npz, made by make_flow_fixtures.py), a cKDTree restatement at the 62 178-bead scale, and
run-to-run / batch-size determinism."""
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.spatial

from conftest import ROOT

pytestmark = pytest.mark.gpu
flow = importlib.import_module("2022a-genome-dynamics_amd.flow")

GOLDEN = os.path.join(ROOT, "tests", "golden")
Z = np.load(os.path.join(GOLDEN, "flow_fixtures.npz"))
META = json.load(open(os.path.join(GOLDEN, "flow_fixtures.json")))
HIST = Z["history"]
XMAX = float(np.abs(HIST).max())
SMOOTH = {"raw": 0, "s4": 4}


@pytest.fixture(scope="module")
def fl():
    f = flow.Flow(0)
    yield f
    f.close()


def _close_nan(a, b, tol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN masks differ", int(np.isnan(a).sum()), int(np.isnan(b).sum()))
    d = np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))) if not np.isnan(b).all() else 0.0
    assert d <= tol, (what, d, tol)


def _flow_tol(vel):
    vmax = float(np.nanmax(np.abs(vel))) if not np.isnan(vel).all() else 0.0
    return 1e-6 * XMAX + 1e-5 * vmax


@pytest.mark.parametrize("w", META["smoothings"])
def test_smoothing(fl, w):
    pos, _ = fl.velocities(HIST.astype(np.float64), w, 1)
    _close_nan(pos, Z[f"smooth64_w{w}"], 1e-12 * XMAX, f"smoothing {w}, float64 input")
    pos, _ = fl.velocities(HIST, w, 1)       # the reference's FFT runs in float32 for float32 input
    _close_nan(pos, Z[f"smooth_w{w}"], 1e-6 * XMAX, f"smoothing {w}, float32 input")


@pytest.mark.parametrize("src", ["raw", "s4"])
@pytest.mark.parametrize("d", META["delays"])
def test_velocities(fl, src, d):
    pos, vel = fl.velocities(HIST, SMOOTH[src], d)
    if src == "raw":
        assert np.array_equal(pos, HIST.astype(np.float64))
    _close_nan(vel, Z[f"vel_{src}_d{d}"], 1e-6 * XMAX, f"velocities {src} delay {d}")
    if d <= 1:
        assert np.isnan(vel[0]).all()        # a one-frame window: 0 * (1/0) in the reference
    if d == 0:
        assert np.isnan(vel).all()


@pytest.mark.parametrize("case", META["cases"]["particle"], ids=lambda c: c["key"])
def test_particle_flow(fl, case):
    fl.velocities(HIST, SMOOTH[case["source"]], case["delay"])
    got = fl.particle(case["radius"])
    ref = Z[case["key"]]
    assert got.dtype == np.float32
    _close_nan(got, ref, _flow_tol(Z[f"vel_{case['source']}_d{case['delay']}"]), case["key"])


@pytest.mark.parametrize("case", META["cases"]["grid"], ids=lambda c: c["key"])
def test_grid_flow(fl, case):
    fl.velocities(HIST, SMOOTH[case["source"]], case["delay"])
    flows, cov = fl.grid(case["radius"], Z[f"{case['grid']}_points"])
    assert np.array_equal(cov, Z[case["key"].replace("gflow", "gcov")])
    _close_nan(flows, Z[case["key"]], _flow_tol(Z[f"vel_{case['source']}_d{case['delay']}"]), case["key"])


def test_ties(fl):
    """Coincident beads and exact dyadic ties at r = 0.5 are inside (cKDTree's <=): bead 0's flow includes beads 1 and 2."""
    _, vel = fl.velocities(HIST, 0, 2)
    got = fl.particle(0.5)
    assert np.array_equal(got, fl.particle(0.5))
    cov = fl.grid(0.5, Z["tiegrid_points"])[1]
    assert np.array_equal(cov, Z["gcov_raw_d2_r0.5_tiegrid"])
    tied = np.flatnonzero((np.abs(Z["tiegrid_points"] - [0.0, 0.0, 0.0]).sum(1) == 0))[0]
    assert (cov[:, tied] >= 1).all()          # bead 3 sits exactly 0.5 away


def test_bad_arguments(fl):
    fl.velocities(HIST, 0, 1)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(flow.GdynError, match="GD_EINVAL"):
            fl.particle(r)
        with pytest.raises(flow.GdynError, match="GD_EINVAL"):
            fl.grid(r, Z["grid_points"])
    bad = HIST.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(flow.GdynError, match="GD_EINVAL"):
        fl.velocities(bad, 0, 1)
    with pytest.raises(flow.GdynError, match="GD_ESTATE"):
        flow.Flow(0).particle(0.6)


# ---- scale: the 62 178-bead model's density (a random walk inside a sphere of radius 8)

SCALE_N, SCALE_F, SCALE_R = 62178, 16, 0.6


def _walk(n, frames, radius, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x = u * radius * rng.uniform(size=(n, 1)) ** (1 / 3)
    out = np.empty((frames, n, 3))
    for f in range(frames):
        x = x + rng.normal(scale=0.05, size=x.shape)
        nr = np.linalg.norm(x, axis=1)
        x[nr > radius] *= (radius / nr[nr > radius])[:, None]
        out[f] = x
    return (np.round(out * 65536) / 65536).astype(np.float32)


@pytest.fixture(scope="module")
def scale():
    hist = _walk(SCALE_N, SCALE_F, 8.0, 5)
    points, _, _ = flow.make_grid((-8.5, 8.5), (-8.5, 8.5), (-8.5, 8.5), 0.3)
    return hist, points


def test_scale_against_kdtree(scale):
    hist, points = scale
    with flow.Flow(0) as f:
        pos, vel = f.velocities(hist, 0, 1)
        pflows = f.particle(SCALE_R)
        gflows, gcov = f.grid(SCALE_R, points)
    tol = 1e-6 * float(np.abs(hist).max()) + 1e-5 * float(np.nanmax(np.abs(vel)))
    gtree = scipy.spatial.cKDTree(points)
    for fr in range(SCALE_F):
        x, v = pos[fr], vel[fr]
        tree = scipy.spatial.cKDTree(x)
        p = tree.query_pairs(SCALE_R, output_type="ndarray")
        s, n = v.copy(), np.ones(len(x))
        np.add.at(s, p[:, 0], v[p[:, 1]])
        np.add.at(s, p[:, 1], v[p[:, 0]])
        np.add.at(n, p[:, 0], 1)
        np.add.at(n, p[:, 1], 1)
        _close_nan(pflows[fr], s / n[:, None], tol, f"particle frame {fr}")
        m = gtree.sparse_distance_matrix(tree, SCALE_R, output_type="ndarray")
        cov = np.bincount(m["i"], minlength=len(points))
        assert np.array_equal(gcov[fr], cov), f"coverage frame {fr}"
        g = np.stack([np.bincount(m["i"], weights=v[m["j"], a], minlength=len(points)) for a in range(3)], axis=1)
        _close_nan(gflows[fr], g / np.maximum(cov, 1)[:, None], tol, f"grid frame {fr}")


def test_determinism(scale):
    hist, points = scale
    hist, points = hist[:7], points[::7]
    results = []
    for batch in (0, 0, 1, 3):
        with flow.Flow(0, max_frames_per_launch=batch) as f:
            pos, vel = f.velocities(hist, 4, 2)
            results.append((pos, vel, f.particle(SCALE_R), *f.grid(SCALE_R, points)))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert a.tobytes() == b.tobytes()


# ---- the programs gd_particle_flow / gd_grid_flow end to end (HDF5 in, HDF5 out)

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5DUMP = "/opt/conda/bin/h5dump"
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


@pytest.fixture(scope="module")
def progs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_particle_flow", "gd_grid_flow"])
    return {k: os.path.join(HOST, k) for k in ("gd_h5tool", "gd_particle_flow", "gd_grid_flow")}


def _traj(progs, path, hist):
    for f, x in enumerate(hist):
        raw = path.with_suffix(".f64")
        x.astype("<f8").tofile(raw)
        subprocess.check_call([progs["gd_h5tool"], "put-positions", str(path), "interphase", str(100 * f), str(raw)])
    return path


def _dataset(progs, tmp, h5, path):
    out = subprocess.check_output([progs["gd_h5tool"], "dataset", str(h5), path, str(tmp / "ds.f64")], text=True)
    shape = tuple(int(s) for s in out.split())
    return np.fromfile(tmp / "ds.f64", dtype="<f8").reshape(shape)


def _samples(h5, path):
    out = subprocess.check_output([H5DUMP, "-d", path, str(h5)], text=True)
    return re.findall(r'"([^"]*)"', out.split("DATA {", 1)[1])


def _header(h5, path):
    return subprocess.check_output([H5DUMP, "-H", "-p", "-d", path, str(h5)], text=True)


@needs_h5
def test_programs_end_to_end(progs, tmp_path):
    a = _traj(progs, tmp_path / "traj_a.h5", HIST)
    b = _traj(progs, tmp_path / "traj_b.h5", HIST[::-1])
    out = tmp_path / "flow.h5"
    # particle mode, raw history, delay 1 (frame 0 NaN)
    subprocess.run([progs["gd_particle_flow"], "--scan-radius", "0.6", str(out), str(a)], check=True, capture_output=True)
    name = flow.config_name(flow.config_json(None, 1, 0.6))
    root = f"/particle_flow/{name}"
    got = _dataset(progs, tmp_path, out, f"{root}/traj_a/velocity")
    _close_nan(got, Z["pflow_raw_d1_r0.6"].astype(np.float64), _flow_tol(Z["vel_raw_d1"]), "particle program")
    assert np.array_equal(_dataset(progs, tmp_path, out, f"{root}/traj_a/position"), HIST.astype(np.float64))
    cfg = subprocess.check_output([progs["gd_h5tool"], "strings", str(out), f"{root}/.config"], text=True).strip()
    assert cfg == flow.config_json(None, 1, 0.6)
    h = _header(out, f"{root}/traj_a/position")
    assert "H5T_IEEE_F32LE" in h and "SHUFFLE" in h and "LEVEL 1" in h
    # smoothed: position is float64
    subprocess.run([progs["gd_particle_flow"], "--name", "s4", "--smoothing", "4", "--velocity-delay", "2", "--scan-radius", "0.6",
                    str(out), str(a)], check=True, capture_output=True)
    assert "H5T_IEEE_F64LE" in _header(out, "/particle_flow/s4/traj_a/position")
    _close_nan(_dataset(progs, tmp_path, out, "/particle_flow/s4/traj_a/position"), Z["smooth_w4"], 1e-6 * XMAX, "smoothed position")
    _close_nan(_dataset(progs, tmp_path, out, "/particle_flow/s4/traj_a/velocity"), Z["pflow_s4_d2_r0.6"].astype(np.float64),
               _flow_tol(Z["vel_s4_d2"]), "smoothed particle program")
    # particle mode replaces .samples with this run's
    assert _samples(out, f"{root}/.samples") == ["traj_a"]
    subprocess.run([progs["gd_particle_flow"], "--scan-radius", "0.6", str(out), str(b)], check=True, capture_output=True)
    assert _samples(out, f"{root}/.samples") == ["traj_b"]
    h = _header(out, f"{root}/.samples")
    assert "STRSIZE 6" in h and "H5T_STR_NULLPAD" in h and "H5T_CSET_ASCII" in h

    # grid mode
    case = next(c for c in META["cases"]["grid"] if c["key"] == "gflow_s4_d2_r0.35_grid")
    g = META["grids"]["grid"]
    args = ["--smoothing", "4", "--velocity-delay", "2", "--scan-radius", "0.35", "--grid-interval", str(g["interval"])]
    args += [f"--{ax}-range={lo!r},{hi!r}" for ax, (lo, hi) in zip("xyz", (g["x_range"], g["y_range"], g["z_range"]))]
    subprocess.run([progs["gd_grid_flow"], *args, str(out), str(a)], check=True, capture_output=True)
    gname = flow.config_name(flow.config_json(4, 2, 0.35, g["interval"], *(tuple(map(float, g[k])) for k in ("x_range", "y_range", "z_range"))))
    groot = f"/grid_flow/{gname}"
    assert np.array_equal(_dataset(progs, tmp_path, out, f"{groot}/.grid/points"), Z["grid_points"])
    assert np.array_equal(_dataset(progs, tmp_path, out, f"{groot}/.grid/indices"), Z["grid_indices"])
    assert np.array_equal(_dataset(progs, tmp_path, out, f"{groot}/.grid/shape"), Z["grid_shape"])
    assert np.array_equal(_dataset(progs, tmp_path, out, f"{groot}/traj_a/coverages"), Z["gcov_s4_d2_r0.35_grid"])
    factor = case["scaleoffset"]
    _close_nan(_dataset(progs, tmp_path, out, f"{groot}/traj_a/flows"), Z[case["key"]].astype(np.float64),
               _flow_tol(Z["vel_s4_d2"]) + 0.5 * 10.0 ** -factor, "grid program")
    h = _header(out, f"{groot}/traj_a/flows")      # (h5dump -p names the scale type, not the factor)
    assert "H5T_IEEE_F32LE" in h and "SCALEOFFSET" in h and "SHUFFLE" in h and "LEVEL 1" in h, h
    h = _header(out, f"{groot}/traj_a/coverages")
    assert "H5T_STD_I32LE" in h and "SCALEOFFSET" in h and "SHUFFLE" in h and "LEVEL 1" in h, h
    for ds, typ in [(".grid/shape", "H5T_STD_I64LE"), (".grid/points", "H5T_IEEE_F64LE"), (".grid/indices", "H5T_STD_I64LE")]:
        assert typ in _header(out, f"{groot}/{ds}")
    # a second grid (exact ties, scale-offset factor 5): stored flows within half a unit of the factor's last digit
    tie = next(c for c in META["cases"]["grid"] if c["grid"] == "tiegrid")
    t = META["grids"]["tiegrid"]
    targs = ["--name", "tie", "--velocity-delay", "2", "--scan-radius", "0.5", "--grid-interval", str(t["interval"])]
    targs += [f"--{ax}-range={lo!r},{hi!r}" for ax, (lo, hi) in zip("xyz", (t["x_range"], t["y_range"], t["z_range"]))]
    subprocess.run([progs["gd_grid_flow"], *targs, str(out), str(a)], check=True, capture_output=True)
    stored = _dataset(progs, tmp_path, out, "/grid_flow/tie/traj_a/flows")
    assert np.array_equal(_dataset(progs, tmp_path, out, "/grid_flow/tie/traj_a/coverages"), Z["gcov_raw_d2_r0.5_tiegrid"])
    f = tie["scaleoffset"]
    assert f == 5
    _close_nan(stored, Z[tie["key"]].astype(np.float64), _flow_tol(Z["vel_raw_d2"]) + 0.5 * 10.0 ** -f, "tie grid program")
    # grid mode merges .samples, keeping the last occurrence of a duplicate
    subprocess.run([progs["gd_grid_flow"], *args, str(out), str(b), str(a)], check=True, capture_output=True)
    assert _samples(out, f"{groot}/.samples") == ["traj_b", "traj_a"]


@needs_h5
def test_particle_flow_of_a_real_trajectory(progs, tmp_path):
    """A short gd_interphase run (as test_host_driver.py makes it), then gd_particle_flow on its file."""
    from test_host_driver import _env, _inputs
    subprocess.check_call(["make", "-s", "-C", HOST, "gd_interphase"])
    _inputs(tmp_path)
    subprocess.run([os.path.join(HOST, "gd_interphase"), str(tmp_path / "traj.h5")], check=True, capture_output=True,
                   env=_env(os.path.join(ROOT, "2022a-genome-dynamics_amd", "csrc")))
    steps = subprocess.check_output([progs["gd_h5tool"], "steps", str(tmp_path / "traj.h5"), "interphase"], text=True).split()
    assert len(steps) >= 2
    out = tmp_path / "flow.h5"
    subprocess.run([progs["gd_particle_flow"], "--name", "run", "--scan-radius", "0.6", str(out), str(tmp_path / "traj.h5")],
                   check=True, capture_output=True)
    v = _dataset(progs, tmp_path, out, "/particle_flow/run/traj/velocity")
    x = _dataset(progs, tmp_path, out, "/particle_flow/run/traj/position")
    assert v.shape == x.shape == (len(steps), x.shape[1], 3)
    assert np.isnan(v[0]).all() and np.isfinite(v[1:]).all()
    assert _samples(out, "/particle_flow/run/.samples") == ["traj"]

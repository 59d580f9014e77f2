"""The lamina analysis on the device (include/gdyn_lamina.h, csrc/gdyn_lamina.hip) against the reference's own outputs
(tests/golden/lamina_fixtures.npz, made by make_lamina_fixtures.py) bit for bit, against the restatement
(tests/lamina_restatement.py) at the 62 178-bead scale, run-to-run / batch-size determinism, and gd_analyze_lamina end to end
on trajectories gd_interphase writes."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import lamina_restatement as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
lamina = importlib.import_module("2022a-genome-dynamics_amd.lamina")

Z = np.load(os.path.join(ROOT, "tests", "golden", "lamina_fixtures.npz"))
SETS = range(int(Z["n_sets"]))
HISTS = range(int(Z["n_hist"]))


@pytest.fixture(scope="module")
def lam():
    with lamina.Lamina(0) as l:
        yield l


def _report(what, got, want):
    """Prints the largest difference in ulps of the float64 reference before the caller asserts."""
    both = np.isfinite(got) & np.isfinite(want)
    ulps = np.abs(got[both].astype(np.float64) - want[both].astype(np.float64)) / np.spacing(np.abs(want[both]).astype(want.dtype)) if both.any() else np.zeros(1)
    print(f"{what}: {int(both.sum())} finite, {int(np.isnan(want).sum())} NaN, max |diff| {ulps.max():.3g} ulp, {int((ulps > 0).sum())} differ")


# ---- the reference's outputs, bit for bit

@pytest.mark.parametrize("k", SETS)
@pytest.mark.parametrize("src", ["float32", "float64"])
def test_distances_equal_the_reference(lam, k, src):
    x, want = (Z[f"points{k}"], Z[f"dist{k}"]) if src == "float32" else (Z[f"points64_{k}"], Z[f"dist64_{k}"])
    got = lam.distances(x, Z[f"semi{k}"])
    assert got.dtype == np.float64 and got.shape == (1, len(x))
    _report(f"set {k} {src} -> float64", got[0], want)
    assert np.array_equal(np.isnan(got[0]), np.isnan(want))
    assert R.same(got[0], want)
    got32 = lam.distances(x, Z[f"semi{k}"], dtype=np.float32)
    assert got32.dtype == np.float32
    assert R.same(got32[0], want.astype(np.float32))


@pytest.mark.parametrize("t", HISTS)
def test_histories_equal_the_reference(lam, t):
    """analyze_distances_history's output: semiaxes of their own in every frame."""
    x, s, want = Z[f"hist_points{t}"], Z[f"hist_semi{t}"], Z[f"hist_dist{t}"]
    for batch in (0, 1, 4):
        with lamina.Lamina(0, max_frames_per_launch=batch) as l:
            got = l.distances(x, s)
            _report(f"history {t} batch {batch}", got, want)
            assert R.same(got, want)
            assert R.same(l.distances(x.astype(np.float64), s, dtype=np.float32), want.astype(np.float32))


# ---- scale: the 62 178-bead model, 64 frames, every frame with semiaxes of its own

SCALE_N, SCALE_F = 62178, 64


@pytest.fixture(scope="module")
def scale():
    from test_flow_gpu import _walk
    hist = _walk(SCALE_N, SCALE_F, 8.0, 5)
    f = np.arange(SCALE_F, dtype=np.float64)
    semi = np.stack([8.6 - 0.004 * f, 8.2 + 0.003 * f, 8.05 + 0.001 * f * f / SCALE_F], axis=1)
    return hist, semi


def test_scale_against_the_restatement(scale):
    hist, semi = scale
    want = R.history(hist, semi)
    assert np.isfinite(want).all()
    results = []
    for batch in (0, 0, 1, 3):
        with lamina.Lamina(0, max_frames_per_launch=batch) as l:
            results.append((l.distances(hist, semi), l.distances(hist, semi, dtype=np.float32)))
    _report("62 178 x 64", results[0][0], want)
    assert R.same(results[0][0], want)
    assert R.same(results[0][1], want.astype(np.float32))
    for d64, d32 in results[1:]:
        assert d64.tobytes() == results[0][0].tobytes() and d32.tobytes() == results[0][1].tobytes()


# ---- contacts and averages

def test_contacts_and_averages_equal_the_fixtures():
    stored = [Z[f"hist_dist{t}"].astype(np.float32) for t in HISTS]
    for batch in (0, 1, 3):          # 50 beads per frame: batches of 1 and 3 frames start off the 16-byte grid of the sum
        with lamina.Lamina(0, max_frames_per_launch=batch) as l:
            for j, D in enumerate(Z["thresholds"]):
                l.reset()
                for t in HISTS:
                    c = l.contacts(stored[t], D)
                    assert c.dtype == np.bool_ and np.array_equal(c, Z[f"contact{j}_{t}"]), (batch, j, t)
                avg = l.average()
                assert avg.dtype == np.float32 and np.array_equal(avg, Z[f"average{j}"]), (batch, j)


def test_contacts_against_numpy():
    rng = np.random.default_rng(11)
    F, N, K = 37, 1001, 5
    hists = [rng.uniform(0, 2, size=(F, N)).astype(np.float32) for _ in range(K)]
    for h in hists:
        h[rng.integers(F, size=200), rng.integers(N, size=200)] = np.nan
    D = float(hists[2][5, 7])                                   # at a stored value
    for thr in (np.nextafter(D, 0), D, np.nextafter(D, 4), -1.0, 0.0, 5.0, float("inf"), 0.1 + 0.2):
        want = [R.contacts(h, thr) for h in hists]
        outs = []
        for batch in (0, 1, 3, 4):
            with lamina.Lamina(0, max_frames_per_launch=batch) as l:
                got = [l.contacts(h, thr) for h in hists]
                avg = l.average()
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (thr, batch)
            assert np.array_equal(avg, R.average(want)), (thr, batch)
            outs.append(avg.tobytes())
        assert len(set(outs)) == 1
    at = (5, 7)
    assert not R.contacts(hists[2], D)[at] and R.contacts(hists[2], np.nextafter(D, 4))[at]


def test_shape_change_is_einval(lam):
    lam.reset()
    lam.contacts(np.zeros((3, 10), np.float32), 0.5)
    for shape in [(3, 11), (4, 10), (10, 3), (0, 10)]:
        with pytest.raises(lamina.GdynError, match="GD_EINVAL"):
            lam.contacts(np.zeros(shape, np.float32), 0.5)
    assert np.array_equal(lam.average(), np.ones((3, 10), np.float32))      # the failed calls did not count
    lam.reset()
    assert lam.contacts(np.zeros((4, 10), np.float32), 0.5).all()
    lam.reset()


def test_bad_arguments(lam):
    x = Z["points0"]
    for bad in [(0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)]:
        with pytest.raises(lamina.GdynError, match="GD_EINVAL"):
            lam.distances(x, bad)
    with pytest.raises(lamina.GdynError, match="GD_EINVAL"):
        lam.distances(np.stack([x, x]), [(1.0, 1.0, 1.0), (1.0, 0.0, 1.0)])      # the second frame's
    with pytest.raises(lamina.GdynError, match="GD_EINVAL"):
        lam.contacts(np.zeros((2, 2), np.float32), float("nan"))
    # empty inputs give empty results
    assert lam.distances(np.zeros((0, 5, 3), np.float32), np.zeros((0, 3))).shape == (0, 5)
    assert lam.distances(np.zeros((4, 0, 3), np.float32), (1.0, 2.0, 3.0)).shape == (4, 0)
    lam.reset()
    assert lam.contacts(np.zeros((4, 0), np.float32), 1.0).shape == (4, 0) and lam.average().shape == (4, 0)
    lam.reset()
    with pytest.raises(lamina.GdynError, match="GD_ESTATE"):
        lam.average()
    # null pointers through the C-ABI
    d, h = lam.dll, lam._h
    semi = (C.c_double * 3)(1.0, 1.0, 1.0)
    buf = (C.c_float * 12)()
    EINVAL = d.gd_lamina_distances(None, buf, 0, 1, 4, semi, buf, 0)
    assert "GD_EINVAL" in str(lamina.GdynError(EINVAL, ""))
    assert d.gd_lamina_distances(h, None, 0, 1, 4, semi, buf, 0) == EINVAL
    assert d.gd_lamina_distances(h, buf, 0, 1, 4, None, buf, 0) == EINVAL
    assert d.gd_lamina_distances(h, buf, 0, 1, 4, semi, None, 0) == EINVAL
    assert d.gd_lamina_contacts(h, None, 1, 4, 1.0, buf) == EINVAL
    assert d.gd_lamina_contacts(h, buf, 1, 4, 1.0, None) == EINVAL
    assert d.gd_lamina_contacts(None, buf, 1, 4, 1.0, buf) == EINVAL
    assert d.gd_lamina_average(None, buf) == EINVAL and d.gd_lamina_reset(None) == EINVAL
    assert b"gd_lamina_reset" in d.gd_last_error()
    with pytest.raises(lamina.GdynError, match="GD_ESTATE"):
        lam.average()                                            # none of the failed calls fixed a shape


# ---- gd_analyze_lamina end to end on trajectories gd_interphase writes (HDF5 in, HDF5 out)

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5DUMP = "/opt/conda/bin/h5dump"
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


@pytest.fixture(scope="module")
def progs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_interphase", "gd_analyze_lamina"])
    return {k: os.path.join(HOST, k) for k in ("gd_h5tool", "gd_interphase", "gd_analyze_lamina")}


def _trajectory(progs, tmp, name, seed, env, interphase_steps=None):
    """A short gd_interphase run on an input with /metadata/particle_types, as `prepare` writes it (test_host_driver's inputs
    through gd_h5tool make-metadata).  Returns the file, the stored float32 positions (F, N, 3) and the stored semiaxes (F, 3)."""
    import json
    from test_host_driver import N, _inputs
    work = tmp / f"in_{name}"
    work.mkdir()
    cfg, a, b, _, _, _ = _inputs(work, seed=seed, walk_seed=seed)
    if interphase_steps is not None:
        cfg["interphase_steps"] = interphase_steps
        (work / "config.json").write_text(json.dumps(cfg))
    np.stack([a, b], axis=1).astype("<f4").tofile(work / "ab.f32")
    np.where(a > b, 1, 2).astype("i1").tofile(work / "types.i8")
    (work / "chromosomes.tsv").write_text((work / "chroms.tsv").read_text())
    (work / "nucleoli.tsv").write_text("")
    (work / "nucleolus_bonds.i32").write_bytes(b"")
    traj = tmp / f"{name}.h5"
    subprocess.check_call([progs["gd_h5tool"], "make-metadata", str(traj), str(work)])
    subprocess.check_call([progs["gd_h5tool"], "put-positions", str(traj), "relaxation", "0", str(work / "pos.f64")])
    subprocess.run([progs["gd_interphase"], str(traj)], check=True, capture_output=True, env=env)
    steps = subprocess.check_output([progs["gd_h5tool"], "steps", str(traj), "interphase"], text=True).split()
    assert len(steps) >= 2
    frames, semis = [], []
    for s in steps:
        subprocess.check_call([progs["gd_h5tool"], "positions", str(traj), "interphase", s, str(tmp / "x.f64")])
        frames.append(np.fromfile(tmp / "x.f64", dtype="<f8").reshape(N, 3).astype(np.float32))      # stored as float32: exact
        semis.append(json.loads(subprocess.check_output([progs["gd_h5tool"], "context", str(traj), "interphase", s], text=True))["wall_semiaxes"])
    return traj, np.stack(frames), np.array(semis)


def _dataset(progs, tmp, h5, path):
    out = subprocess.check_output([progs["gd_h5tool"], "dataset", str(h5), path, str(tmp / "ds.f64")], text=True)
    shape = tuple(int(s) for s in out.split())
    return np.fromfile(tmp / "ds.f64", dtype="<f8").reshape(shape)


def _header(h5, path):
    return subprocess.check_output([H5DUMP, "-H", "-p", "-d", path, str(h5)], text=True)


def _check_output_file(progs, tmp, out, trajs, name, D):
    stored = {}
    for key, (_, frames, semis) in trajs.items():
        got = _dataset(progs, tmp, out, f"/distance/{key}")
        want = R.history(frames, semis)
        assert got.shape == want.shape and np.isfinite(want).all()
        # half a unit of the D-scale 3 grid, plus one float32 ulp for the float32 rounding of min + k / 1000
        tol = 5e-4 + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got - want)
        print(f"/distance/{key}: max |stored - restatement| {err.max():.3e}, bound {tol.min():.3e}")
        assert (err <= tol).all(), (key, float(err.max()))
        stored[key] = got.astype(np.float32)
        assert np.array_equal(stored[key].astype(np.float64), got)
        h = _header(out, f"/distance/{key}")
        assert "H5T_IEEE_F32LE" in h and "SCALEOFFSET" in h and "SHUFFLE" in h and "LEVEL 1" in h, h
    contacts = []
    for key in sorted(stored):
        c = _dataset(progs, tmp, out, f"/contact/{name}/{key}")
        want = R.contacts(stored[key], D)
        assert want.any() and not want.all()                      # D separates the beads
        assert np.array_equal(c, want.astype(np.float64)), key
        contacts.append(want)
        h = _header(out, f"/contact/{name}/{key}")
        assert "H5T_ENUM" in h and "H5T_STD_I8LE" in h and '"FALSE"' in h and '"TRUE"' in h and "SHUFFLE" in h and "LEVEL 1" in h, h
        assert "SCALEOFFSET" not in h
    avg = _dataset(progs, tmp, out, f"/average_contact/{name}")
    assert np.array_equal(avg, R.average(contacts).astype(np.float64))
    h = _header(out, f"/average_contact/{name}")
    assert "H5T_IEEE_F32LE" in h and "SHUFFLE" in h and "LEVEL 1" in h and "SCALEOFFSET" not in h, h
    return stored


@needs_h5
def test_program_end_to_end(progs, tmp_path):
    from test_host_driver import N, _env
    env = _env(os.path.join(ROOT, "2022a-genome-dynamics_amd", "csrc"))
    trajs = {"cell_a": _trajectory(progs, tmp_path, "cell_a", 101, env), "cell_b": _trajectory(progs, tmp_path, "cell_b", 202, env)}
    out = tmp_path / "lamina.h5"
    prog = progs["gd_analyze_lamina"]
    run = lambda *args: subprocess.run([prog, *map(str, args)], check=True, capture_output=True, text=True)      # noqa: E731
    run("distance", out, trajs["cell_a"][0], trajs["cell_b"][0])
    every = np.concatenate([R.history(f, s).ravel() for _, f, s in trajs.values()])
    D = float(np.median(every))
    run("contact", "--contact-distance", repr(D), out)
    stored = _check_output_file(progs, tmp_path, out, trajs, "uniform", D)
    # the metadata of the first trajectory
    tool = lambda *args: subprocess.check_output([progs["gd_h5tool"], *map(str, args)], text=True)      # noqa: E731
    assert tool("strings", out, "/metadata/simulation_config").strip() == tool("strings", trajs["cell_a"][0], "/metadata/config").strip()
    types = _dataset(progs, tmp_path, out, "/metadata/particle_types")
    assert np.array_equal(types, _dataset(progs, tmp_path, trajs["cell_a"][0], "/metadata/particle_types")) and types.shape == (N,)
    h = _header(out, "/metadata/particle_types")
    assert "H5T_ENUM" in h and '"centromere"' in h and '"nucleolus"' in h, h
    ranges = _dataset(progs, tmp_path, out, "/metadata/chromosome_ranges")
    assert np.array_equal(ranges, _dataset(progs, tmp_path, trajs["cell_a"][0], "/metadata/chromosome_ranges"))
    assert "H5T_STD_I32LE" in _header(out, "/metadata/chromosome_ranges")
    names = tool("strings", out, "/metadata/chromosome_names").split()
    assert names == [f"chr{k + 1}" for k in range(len(ranges))]
    h = _header(out, "/metadata/chromosome_names")
    assert "H5T_STR_NULLPAD" in h and "H5T_CSET_ASCII" in h, h
    # a second run replaces every dataset instead of failing; a second name lives beside the first
    run("distance", out, trajs["cell_b"][0], trajs["cell_a"][0])
    run("contact", "--contact-distance", repr(D), out)
    again = _check_output_file(progs, tmp_path, out, trajs, "uniform", D)
    assert all(np.array_equal(stored[k], again[k]) for k in stored)
    D2 = float(np.quantile(every, 0.8))
    run("contact", "--name=wide", f"--contact-distance={D2!r}", out)
    _check_output_file(progs, tmp_path, out, trajs, "wide", D2)
    _check_output_file(progs, tmp_path, out, trajs, "uniform", D)
    # histories of different shapes: contact fails as numpy's broadcast does
    c = _trajectory(progs, tmp_path, "cell_c", 303, env, interphase_steps=40)
    assert len(c[1]) != len(trajs["cell_a"][1])
    run("distance", out, c[0])
    r = subprocess.run([prog, "contact", "--contact-distance", repr(D), str(out)], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and "GD_EINVAL" not in r.stdout and "history" in r.stderr, r.stderr
    r = subprocess.run([prog, "contact", "--contact-distance", "1", str(tmp_path / "nothing.h5")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("error: "), r.stderr

"""gd_interphase --particle-flow / --grid-flow: the flow outputs of a run written from frames recorded on the device equal, dataset
for dataset, what gd_particle_flow and gd_grid_flow write from the trajectory files of that run afterwards."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_flow_gpu import _dataset, _header, _samples, needs_h5

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5LS, H5DIFF = "/opt/conda/bin/h5ls", "/opt/conda/bin/h5diff"
GRID = ["--grid-interval", "1.0", "--x-range=-2,2", "--y-range=-2,2", "--z-range=-2,2"]      # 125 points around a wall of radius 1.7


@pytest.fixture(scope="module")
def progs():
    names = ("gd_h5tool", "gd_interphase", "gd_particle_flow", "gd_grid_flow")
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", *names])
    return {k: os.path.join(HOST, k) for k in names}


def _two_files(tmp):
    """Two prepared files of one ensemble, a.h5 and b.h5 (test_host_driver._inputs: same model, their own seeds and structures)."""
    from test_host_driver import _inputs
    files = []
    for k, name in enumerate("ab"):
        d = tmp / name
        d.mkdir(parents=True)
        _inputs(d, seed=12345 + k, walk_seed=8 + k)
        files.append(shutil.move(str(d / "traj.h5"), str(tmp / f"{name}.h5")))
    return files


def _stored(tmp, files):
    """Every stored frame of the files: positions, context and contact map (test_host_driver._frames reads <dir>/traj.h5)."""
    from test_host_driver import _frames
    out = []
    for k, f in enumerate(files):
        d = tmp / f"read{k}"
        d.mkdir()
        shutil.copy(f, d / "traj.h5")
        out.append(_frames(d))
    return out


@pytest.fixture(scope="module")
def plain(progs, tmp_path_factory):
    """The run without the options."""
    tmp = tmp_path_factory.mktemp("plain")
    files = _two_files(tmp)
    r = subprocess.run([progs["gd_interphase"], *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return files, _stored(tmp, files)


def _listing(h5):
    return subprocess.check_output([H5LS, "-r", str(h5)], text=True)


def _same_file(progs, tmp, got, want, root, datasets):
    assert _listing(got) == _listing(want)      # the same groups and datasets, with their shapes
    assert set(re.findall(r"^(\S+)\s+Dataset", _listing(got), flags=re.M)) == {f"{root}/{d}" for d in datasets} | {f"{root}/.config", f"{root}/.samples"}
    for d in datasets:
        a, b = _dataset(progs, tmp, got, f"{root}/{d}"), _dataset(progs, tmp, want, f"{root}/{d}")
        assert a.shape == b.shape and a.size and np.array_equal(a, b, equal_nan=True), d
        assert _header(got, f"{root}/{d}").replace(str(got), "") == _header(want, f"{root}/{d}").replace(str(want), ""), d      # type, shape, filters
    for d in (".config", ".samples"):
        assert _header(got, f"{root}/{d}").replace(str(got), "") == _header(want, f"{root}/{d}").replace(str(want), ""), d
    config = [subprocess.check_output([progs["gd_h5tool"], "strings", str(f), f"{root}/.config"], text=True) for f in (got, want)]
    assert config[0] == config[1] and '"scan_radius": 0.6' in config[0]
    assert _samples(got, f"{root}/.samples") == _samples(want, f"{root}/.samples") == ["a", "b"]
    assert subprocess.run([H5DIFF, "-q", str(got), str(want)]).returncode == 0


@needs_h5
@pytest.mark.parametrize("smoothing", [[], ["--smoothing", "3", "--velocity-delay", "2"]], ids=["raw", "smoothed"])
def test_driver_writes_the_flows_of_its_replicas(progs, plain, tmp_path, smoothing):
    """gd_interphase --particle-flow P.h5 --grid-flow G.h5 <flow options> a.h5 b.h5, then gd_particle_flow P2.h5 ... a.h5 b.h5 and
    gd_grid_flow G2.h5 ... on the files it wrote.  The trajectory files hold what a run without the options stores: every frame,
    context and contact map is compared, and h5diff finds no difference.  (Their bytes cannot be compared: HDF5 stamps each object
    with its modification time, so two runs of the same command already differ in those bytes.)"""
    files = _two_files(tmp_path)
    P, G, P2, G2 = (tmp_path / f"{k}.h5" for k in ("P", "G", "P2", "G2"))
    opts = ["--name", "live", "--scan-radius", "0.6", *smoothing]
    r = subprocess.run([progs["gd_interphase"], "--particle-flow", str(P), "--grid-flow", str(G), *opts, *GRID, *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"[flow] recording 4 frames of 2 replicas of 600 beads on the device: {2 * 4 * 600 * 12} bytes" in r.stderr
    subprocess.run([progs["gd_particle_flow"], *opts, str(P2), *files], check=True, capture_output=True)
    subprocess.run([progs["gd_grid_flow"], *opts, *GRID, str(G2), *files], check=True, capture_output=True)
    _same_file(progs, tmp_path, P, P2, "/particle_flow/live", [f"{s}/{d}" for s in "ab" for d in ("position", "velocity")])
    _same_file(progs, tmp_path, G, G2, "/grid_flow/live",
               [".grid/shape", ".grid/points", ".grid/indices", *[f"{s}/{d}" for s in "ab" for d in ("flows", "coverages")]])
    assert ("H5T_IEEE_F64LE" if smoothing else "H5T_IEEE_F32LE") in _header(P, "/particle_flow/live/a/position")
    cov = _dataset(progs, tmp_path, G, "/grid_flow/live/a/coverages")
    assert cov.shape == (4, 125) and (cov == 0).any() and (cov > 0).any()
    # the trajectory files
    plain_files, want = plain
    got = _stored(tmp_path, files)
    for p, q, fp, fq in zip(files, plain_files, got, want):
        assert fp.keys() == fq.keys() and sum(k[0] == "interphase" for k in fp) == 4
        for key in fp:
            assert np.array_equal(fp[key][0], fq[key][0]) and fp[key][1] == fq[key][1] and fp[key][2] == fq[key][2], key
        assert subprocess.run([H5DIFF, "-q", p, q]).returncode == 0


@needs_h5
def test_driver_refuses_flow_options_it_cannot_use(progs, tmp_path):
    files = _two_files(tmp_path)
    before = [open(f, "rb").read() for f in files]
    out = tmp_path / "P.h5"
    for args, text in [(["--particle-flow", str(out)], "error: the following arguments are required: --scan-radius\n"),
                       (["--particle-flow", str(out), "--scan-radius", "0.6", *GRID], "error: unrecognized arguments: --grid-interval\n"),
                       (["--grid-flow", str(out), "--scan-radius", "0.6"],
                        "error: the following arguments are required: --grid-interval, --x-range, --y-range, --z-range\n"),
                       (["--scan-radius", "0.6"], "error: --scan-radius needs --particle-flow or --grid-flow\n"),
                       (["--particle-flow", str(out), "--scan-radius", "0.6", "--velocity-delay", "-1"],
                        "error: --velocity-delay and --smoothing must be >= 0\n")]:
        r = subprocess.run([progs["gd_interphase"], *args, *files], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr == text, (args, r.stderr)
    assert not out.exists() and [open(f, "rb").read() for f in files] == before

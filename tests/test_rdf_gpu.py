"""The radial distribution counts on the device (include/gdyn_rdf.h, csrc/gdyn_rdf.hip) against the brute-force restatement
(tests/rdf_restatement.py): exact integer counts on edge cases, determinism over batch sizes and runs, a cKDTree-backed check
at ~62 k beads, and gd_rdf_analysis / gd_rdf_analysis_hetero end to end on a trajectory gd_ab_box wrote on the GPU."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.spatial

import rdf_restatement as R
from test_ab_driver import _inputs
from test_host_driver import HOST, _make, _tool

pytestmark = pytest.mark.gpu
rdf = importlib.import_module("2022a-genome-dynamics_amd.rdf")


@pytest.fixture(scope="module")
def dev():
    r = rdf.Rdf(0)
    yield r
    r.close()


def _want(frames, box, bw, md, centers, targets=None):
    out = []
    for x in np.asarray(frames, np.float64).reshape(-1, np.asarray(frames).shape[-2], 3):
        if targets is None:
            out.append(R.counts_self(x[centers], box, bw, md))
        else:
            out.append(R.counts_cross(x[centers], x[targets], box, bw, md))
    return np.array(out, np.uint64).reshape(len(out), R.n_bins(bw, md))


def _check(dev, frames, box, bw, md, centers=None, targets=None, expect_pairs=True):
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n = frames.shape[1]
    centers = np.arange(n) if centers is None else np.asarray(centers, np.int64)
    targets = None if targets is None else np.asarray(targets, np.int64)
    b3 = np.broadcast_to(np.asarray(box, np.float64), (3,))
    got = dev.counts(frames, b3, bw, md, centers, targets)
    want = _want(frames, b3, bw, md, centers, targets)
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    if expect_pairs:
        assert want.sum() > 0
    return got


def _split(n, rng):
    perm = rng.permutation(n)
    return np.sort(perm[: n // 3]), np.sort(perm[n // 3:])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("box", [(4.0, 4.0, 4.0), (3.0, 5.0, 7.5)])
def test_uniform(dev, dtype, box):
    rng = np.random.default_rng(1)
    x = (rng.uniform(size=(3, 700, 3)) * box).astype(dtype)
    _check(dev, x, box, 0.1, 1.0)
    _check(dev, x, box, 0.1, 1.3)
    c, t = _split(700, rng)
    _check(dev, x, box, 0.1, 1.0, c, t)
    _check(dev, x, box, 0.1, 1.0, c)                    # self mode over a subset


def test_dyadic_edges_and_coincident_points(dev):
    """coordinates on a 1/8 lattice: many distances exactly on bin edges (bin_width 1/8) and exactly at max_distance (excluded),
    and coincident beads (bin 0)."""
    rng = np.random.default_rng(2)
    x = rng.integers(0, 32, size=(2, 600, 3)).astype(np.float32) / 8       # box 4
    x[:, 500:] = x[:, :1]                                                    # 100 copies of bead 0
    got = _check(dev, x, 4.0, 0.125, 1.0)
    assert got[:, 0].min() >= 100 * 101 // 2
    on_edge = R.counts_self(x[0].astype(np.float64), (4.0,) * 3, 0.125, 1.0 + 1e-9)      # md itself is a lattice distance
    assert on_edge.sum() > got[0].sum()
    c, t = _split(600, rng)
    _check(dev, x, 4.0, 0.125, 1.0, c, t)
    _check(dev, x, 4.0, 0.25, 0.5)


def test_faces_edges_corners(dev):
    """a bead near a corner of the box and its images across each of the 26 faces, edges and corners"""
    L = 5.0
    base = np.array([0.1, 0.2, 0.15])
    pts = [base]
    for off in np.array(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1])).reshape(3, -1).T:
        if off.any():
            pts.append(np.mod(base + 0.35 * off, L))                         # wraps to the far side where off < 0
    rng = np.random.default_rng(4)
    near = rng.uniform(-0.3, 0.3, size=(300, 3)) + rng.integers(0, 2, size=(300, 3)) * L       # beads around every corner
    x = np.concatenate([np.array(pts), np.mod(near, L)]).astype(np.float32)
    got = _check(dev, x, L, 0.05, 1.0)
    assert got.sum() > 1000
    _check(dev, x, L, 0.05, 1.0, np.arange(27), np.arange(27, len(x)))


def test_unwrapped_by_whole_periods(dev):
    rng = np.random.default_rng(5)
    L = np.array([4.0, 4.5, 5.0])
    x = rng.uniform(size=(800, 3)) * L
    shifted = x + rng.integers(-1000, 1001, size=x.shape) * L
    for frames in (shifted, np.stack([x, shifted]).astype(np.float32)):
        _check(dev, frames, L, 0.1, 1.0)
        _check(dev, frames, L, 0.1, 1.0, np.arange(300), np.arange(300, 800))


@pytest.mark.parametrize("box,md", [((2.0, 2.0, 2.0), 1.5), ((3.0, 3.0, 3.0), 1.4), ((2.0, 3.0, 5.0), 1.2), ((4.0, 4.0, 4.0), 2.0),
                                    ((2.0, 2.0, 2.0), 5.0)])
def test_max_distance_beyond_half_the_box(dev, box, md):
    """1-2 cells per axis: every pair once, at its minimum-image distance"""
    rng = np.random.default_rng(6)
    x = rng.uniform(size=(2, 400, 3)) * box
    _check(dev, x, box, 0.1, md)
    _check(dev, x, box, 0.1, md, np.arange(150), np.arange(150, 400))


@pytest.mark.parametrize("bw,md", [(0.3, 1.0), (0.07, 0.55), (0.1, 0.95), (0.4, 0.4)])
def test_max_distance_not_a_multiple_of_bin_width(dev, bw, md):
    rng = np.random.default_rng(7)
    x = rng.uniform(size=(2, 900, 3)) * 4.0
    _check(dev, x, 4.0, bw, md)
    _check(dev, x, 4.0, bw, md, np.arange(200), np.arange(200, 900))


@pytest.mark.parametrize("bw", [1e-4, 2.5e-4])
def test_many_bins(dev, bw):
    """1e-4: 10 000 bins > GD_RDF_LDS_BINS, the global-atomic path; 2.5e-4: 4 000 bins, one LDS copy per block"""
    assert (R.n_bins(bw, 1.0) > rdf.LDS_BINS) == (bw == 1e-4)
    rng = np.random.default_rng(8)
    x = rng.uniform(size=(2, 1500, 3)) * 4.0
    _check(dev, x, 4.0, bw, 1.0)
    _check(dev, x, 4.0, bw, 1.0, np.arange(500), np.arange(500, 1500))


def test_single_point_and_empty_selections(dev):
    x = np.random.default_rng(9).uniform(size=(2, 50, 3)) * 4.0
    _check(dev, x[:, :1], 4.0, 0.1, 1.0, expect_pairs=False)
    _check(dev, x, 4.0, 0.1, 1.0, [7], expect_pairs=False)
    _check(dev, x, 4.0, 0.1, 1.0, [], expect_pairs=False)
    _check(dev, x, 4.0, 0.1, 1.0, [], np.arange(50), expect_pairs=False)
    _check(dev, x, 4.0, 0.1, 1.0, np.arange(50), [], expect_pairs=False)
    got = _check(dev, x, 4.0, 0.1, 1.0, [3], np.arange(4, 50))
    assert got.sum() > 0


def test_bad_arguments(dev):
    x = np.zeros((1, 10, 3), np.float32)
    with pytest.raises(Exception, match="both a centre and a target"):
        dev.counts(x, 4.0, 0.1, 1.0, [1, 2], [2, 3])
    with pytest.raises(Exception, match="index 10 of 10"):
        dev.counts(x, 4.0, 0.1, 1.0, [10])
    for box, bw, md in [(0.0, 0.1, 1.0), (float("inf"), 0.1, 1.0), (4.0, 0.0, 1.0), (4.0, 0.1, -1.0), (4.0, 1e-9, 1.0)]:
        with pytest.raises(Exception):
            dev.counts(x, box, bw, md, [1, 2])


def test_determinism_over_batches_and_runs():
    rng = np.random.default_rng(10)
    x = (rng.uniform(size=(7, 3000, 3)) * 7.0 + rng.integers(-3, 4, size=(7, 3000, 3)) * 7.0).astype(np.float32)
    c, t = _split(3000, rng)
    results = {}
    for mf in (1, 3, 0):
        with rdf.Rdf(0, max_frames_per_launch=mf) as r:
            for mode, args in (("self", (c,)), ("cross", (c, t))):
                a = r.counts(x, 7.0, 0.1, 1.0, *args)
                b = r.counts(x, 7.0, 0.1, 1.0, *args)
                assert np.array_equal(a, b)
                results.setdefault(mode, []).append(a)
    for mode, rs in results.items():
        for a in rs[1:]:
            assert np.array_equal(a, rs[0]), mode
    want = _want(x[:2], (7.0,) * 3, 0.1, 1.0, c, t)
    assert np.array_equal(results["cross"][0][:2], want)


def test_scale_against_kdtree():
    """~62 k beads at the stage-4 density: candidates from cKDTree (periodic, on wrapped coordinates, radius widened by 1e-6),
    counted with the restatement's formula on the raw coordinates"""
    rng = np.random.default_rng(11)
    L, n, bw, md = 12.5, 62000, 0.1, 1.0
    x = (rng.uniform(size=(3, n, 3)) * L + rng.integers(-2, 3, size=(3, n, 3)) * L).astype(np.float32)
    is_c = np.zeros(n, bool)
    is_c[rng.permutation(n)[: n // 2]] = True
    centers, targets = np.flatnonzero(is_c), np.flatnonzero(~is_c)
    with rdf.Rdf(0) as r:
        got_self = r.counts(x, L, bw, md, np.arange(n))
        got_cross = r.counts(x, L, bw, md, centers, targets)
    for f in range(3):
        p = x[f].astype(np.float64)
        w = np.mod(p, L)
        w[w >= L] = 0.0
        pairs = scipy.spatial.cKDTree(w, boxsize=L).query_pairs(md + 1e-6, output_type="ndarray")
        assert np.array_equal(got_self[f], R.pair_counts(p, p, pairs, (L,) * 3, bw, md))
        mixed = pairs[is_c[pairs[:, 0]] != is_c[pairs[:, 1]]]
        oriented = np.where(is_c[mixed[:, :1]], mixed, mixed[:, ::-1])
        assert np.array_equal(got_cross[f], R.pair_counts(p, p, oriented, (L,) * 3, bw, md))
        assert got_self[f].sum() > 30 * n


@pytest.fixture(scope="module")
def gpu_traj(tmp_path_factory, hip):
    tmp = tmp_path_factory.mktemp("rdf_e2e")
    _inputs(tmp, "box")
    drv = _make("gd_ab_box", ".", "../csrc", "gdyn")
    subprocess.run([drv, str(tmp / "config.json"), str(tmp / "out.h5")], check=True, capture_output=True, timeout=600)
    subprocess.check_call(["make", "-s", "-C", HOST, "gd_rdf_analysis", "gd_rdf_analysis_hetero"])
    h5 = tmp / "out.h5"
    _tool("dataset", h5, "/metadata/ab_factors", tmp / "ab.f64")
    ab = np.fromfile(tmp / "ab.f64", dtype="<f8").reshape(-1, 2)
    keys = _tool("strings", h5, "/snapshots/.steps").split()
    frames = []
    for k in keys:
        _tool("dataset", h5, f"/snapshots/{k}/positions", tmp / "x.f64")
        frames.append(np.fromfile(tmp / "x.f64", dtype="<f8").reshape(-1, 3))
    box = json.loads(_tool("strings", h5, "/metadata/config"))["box_size"]
    return dict(path=h5, ab=ab, frames=frames, box=box)


@pytest.mark.parametrize("hetero,type_", [(False, "A"), (False, "B"), (False, None), (False, "X"), (True, "A"), (True, "B"),
                                          (True, None)])
@pytest.mark.parametrize("bins", [(), ("--bin-width", "0.05", "--max-distance", "0.7")])
def test_programs_end_to_end(gpu_traj, hetero, type_, bins):
    prog = os.path.join(HOST, "gd_rdf_analysis_hetero" if hetero else "gd_rdf_analysis")
    args = list(bins) + ([] if type_ is None else ["--type", type_])
    r = subprocess.run([prog, *args, str(gpu_traj["path"])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    bw = 0.05 if bins else 0.1
    md = 0.7 if bins else 1.0
    want = R.analysis_lines(gpu_traj["ab"], gpu_traj["box"], gpu_traj["frames"], bw, md, type_, hetero)
    got = r.stdout.splitlines()
    assert len(got) == len(want) == len(gpu_traj["frames"]) == 4
    for g, w in zip(got, want):
        assert g.split("\t") == w.split("\t")
        assert len(g.split("\t")) == R.n_bins(bw, md)

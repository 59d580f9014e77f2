"""The displacement correlation on the device (include/gdyn_dcorr.h, csrc/gdyn_dcorr.hip) against the numpy restatement
(tests/dcorr_restatement.py).  Every table is an integer sum, so every comparison is for equality: on both histogram paths, with
crowded and nearly empty cells, in periodic and open boxes, from run to run, for every max_frames_per_launch, between a host-fed
and a live-fed history, and between the class and the program gd_dcorr."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.spatial

import dcorr_restatement as dr
import rdf_restatement as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
g = importlib.import_module("2022a-genome-dynamics_amd")
dcorr = importlib.import_module("2022a-genome-dynamics_amd.dcorr")
live = importlib.import_module("2022a-genome-dynamics_amd.live")


def _refused(status, fn, *args, **kw):
    with pytest.raises(g.GdynError) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(status + ": "), str(e.value)


def _bytes(p):
    return [np.ascontiguousarray(a).tobytes() for a in p[:4]] + [p.scale_bits]


def _same(got, want, what=""):
    for name, a, b in zip(("count", "sum", "self_count", "self_sum"), got[:4], want[:4]):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, len(bad), bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
    assert got.scale_bits == want[4], (what, got.scale_bits, want[4])


def _device(x, label=None, K=1, chain=None, mf=0):
    d = dcorr.Dcorr(0, mf)
    d.set_history(x)
    if label is not None:
        d.set_labels(label, K)
    if chain is not None:
        d.set_chains(chain)
    return d


def _check(x, lag, bw, md, box=None, label=None, K=1, chain=None, scale=0, expect_pairs=True, **origins):
    want = dr.pairs(x, lag, bw, md, box, label, K, chain, scale, **origins)
    with _device(x, label, K, chain) as d:
        got = d.pairs(lag, bw, md, box, dcorr.SCALE_UNIT if scale == "unit" else scale,
                      origins.get("first", 0), origins.get("count", 0), origins.get("stride", 1))
    _same(got, want, (lag, bw, md, box))
    if expect_pairs:
        assert want[0].sum() > 0
    return got


def _walk(rng, F, n, extent, step, dtype):
    """F frames of n beads: uniform in the extent, then independent steps plus a common swirl (so that near pairs correlate)"""
    x0 = rng.uniform(size=(n, 3)) * extent
    steps = rng.normal(scale=step, size=(F, n, 3)) + step * np.sin(x0[None, :, ::-1] * 2.0)
    steps[0] = 0.0
    return (x0 + np.cumsum(steps, axis=0)).astype(dtype)


# ---- uniform random frames

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("box", [(4.0, 4.0, 4.0), (3.0, 5.0, 7.5), None], ids=["cube", "slab", "open"])
def test_uniform(dtype, box):
    rng = np.random.default_rng(1)
    x = _walk(rng, 4, 700, box or (4.0, 4.0, 4.0), 0.05, dtype)
    label, chain = rng.integers(-1, 3, size=700), np.arange(700) // 90
    for md in (1.0, 1.3):
        for lag in (1, 3):
            got = _check(x, lag, 0.1, md, box, label, 3)
            assert (got.sum != 0).any()
            _check(x, lag, 0.1, md, box, label, 3, chain)
    _check(x, 1, 0.1, 1.0, box)      # no labels: one class of all beads


# ---- signed sums

def test_contraction_gives_large_negative_sums():
    """beads in a ball of radius 1 move toward its centre: D_i . D_j = c^2 x_i . x_j is negative for every pair further apart than
    sqrt(|x_i|^2 + |x_j|^2), so every bin beyond sqrt(2) is negative.  A 32-bit path or an unsigned flush cannot pass."""
    rng = np.random.default_rng(2)
    v = rng.normal(size=(900, 3))
    x0 = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(size=(900, 1)) ** (1 / 3)
    x = np.stack([x0, 0.7 * x0]).astype(np.float32)
    got = _check(x, 1, 0.1, 2.0)
    assert got.scale_bits == dr.MAX_SCALE_BITS
    assert (got.sum[0, 0, 15:][got.count[0, 0, 15:] > 0] < 0).all() and (got.sum[0, 0] < 0).sum() >= 5
    assert got.sum.min() < -2 ** 32 and got.sum.max() > 2 ** 32


# ---- a dyadic lattice: distances on bin edges and at max_distance, coincident beads, integer displacements at S = 0

@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_dyadic_edges_and_coincident_points(periodic):
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 32, size=(600, 3))
    cells[500:] = cells[0]                                   # 100 copies of bead 0
    move = rng.integers(-3, 4, size=(600, 3))
    x = np.stack([cells / 8, cells / 8 + move]).astype(np.float32)      # box 4, bin width 1/8
    box = (4.0, 4.0, 4.0) if periodic else None
    got = _check(x, 1, 0.125, 1.0, box, scale="unit")
    assert got.scale_bits == 0 and got.count[0, 0, 0] >= 100 * 101 // 2
    assert np.array_equal(got.count[0, 0], R.counts_self(x[0], box or (1e6,) * 3, 0.125, 1.0))
    on_edge = R.counts_self(x[0].astype(np.float64), box or (1e6,) * 3, 0.125, 1.0 + 1e-9)      # md itself is a lattice distance
    assert on_edge.sum() > got.count.sum()
    # the closed form, in integers: distances in eighths, bin = floor(sqrt(r2)), term = move_i . move_j
    want_n, want_s = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for i in range(600):
        d = cells[i] - cells[i + 1:]
        if periodic:
            d = (d + 16) % 32 - 16
        r2 = (d * d).sum(axis=1)
        keep = r2 < 64
        b = np.array([math.isqrt(int(v)) for v in r2[keep]], np.int64)
        np.add.at(want_n, b, 1)
        np.add.at(want_s, b, (move[i + 1:][keep] * move[i]).sum(axis=1))
    assert np.array_equal(got.count[0, 0], want_n.astype(np.uint64)) and np.array_equal(got.sum[0, 0], want_s)
    assert got.self_sum[0, 0] == (move * move).sum()
    _check(x, 1, 0.25, 0.5, box, scale="unit")


# ---- a crowded cell: its partners exceed one LDS tile and its centres one block

def test_crowded_cell():
    rng = np.random.default_rng(4)
    x0 = np.concatenate([rng.uniform(size=(3000, 3)) * 2.0 + (2.0, 0.0, 2.0), rng.uniform(size=(300, 3)) * 4.0])
    x = np.stack([x0, x0 + rng.normal(scale=0.1, size=x0.shape)]).astype(np.float32)
    label = (np.arange(3300) % 2).astype(np.int32)
    for box in ((4.0, 4.0, 4.0), None):
        got = _check(x, 1, 0.1, 1.9, box, label, 2)
        assert 3000 * 2999 // 2 * 0.5 < got.count.sum() < 3300 * 3299 // 2      # most pairs of the crowded cell, each once


# ---- both histogram paths

@pytest.mark.parametrize("bins", [2730, 2731, 1], ids=["lds", "global", "one_bin"])
def test_histogram_paths(bins):
    """3 classes: 3 * 2730 = 8190 cells fit the LDS histogram (GD_DCORR_LDS_BINS = 8192), 3 * 2731 = 8193 do not"""
    rng = np.random.default_rng(5)
    bw = 1.0 / (bins - 0.5) if bins > 1 else 1.0
    assert dr.n_bins(bw, 1.0) == bins and (3 * bins > dcorr.LDS_BINS) == (bins == 2731)
    x = _walk(rng, 2, 1500, (4.0, 4.0, 4.0), 0.05, np.float32)
    label = rng.integers(0, 2, size=1500)
    got = _check(x, 1, bw, 1.0, (4.0, 4.0, 4.0), label, 2)
    assert bins == 1 or (got.sum < 0).any()
    _check(x, 1, bw, 1.0, None, label, 2)


# ---- few cells per axis, max_distance beyond half the box

@pytest.mark.parametrize("box,md", [((2.0, 2.0, 2.0), 1.5), ((3.0, 3.0, 3.0), 1.4), ((2.0, 3.0, 5.0), 1.2), ((4.0, 4.0, 4.0), 2.0),
                                    ((2.0, 2.0, 2.0), 5.0), ((9.0, 3.5, 2.0), 1.0)])
def test_fewer_than_three_cells_per_axis(box, md):
    """1-2 cells along some axis: every pair once, at its minimum-image distance"""
    rng = np.random.default_rng(6)
    x = _walk(rng, 2, 400, box, 0.05, np.float64)
    x[:, :200] += rng.integers(-3, 4, size=(1, 200, 3)) * box      # unwrapped by whole periods
    got = _check(x, 1, 0.1, md, box)
    assert np.array_equal(got.count[0, 0], R.counts_self(x[0], box, 0.1, md))


# ---- open frames whose bounding box has no extent along some axes

@pytest.mark.parametrize("flat", [(2,), (0, 1), (0, 1, 2)], ids=["plane", "line", "point"])
def test_open_frame_of_zero_extent(flat):
    rng = np.random.default_rng(7)
    x = _walk(rng, 2, 500, (6.0, 6.0, 6.0), 0.05, np.float32)
    for a in flat:
        x[0, :, a] = 1.25
    got = _check(x, 1, 0.1, 1.0)
    assert len(flat) < 3 or got.count[0, 0, 0] == 500 * 499 // 2


# ---- origins, states and errors

def test_origins_states_and_errors():
    rng = np.random.default_rng(8)
    x = _walk(rng, 7, 300, (3.0, 3.0, 3.0), 0.05, np.float32)
    label = rng.integers(-1, 2, size=300)
    args = (0.1, 1.0, (3.0, 3.0, 3.0))
    with dcorr.Dcorr(0) as d:
        _refused("GD_ESTATE", d.set_labels, label, 2)
        _refused("GD_ESTATE", d.set_chains, np.arange(300))
        _refused("GD_ESTATE", d.pairs, 1, *args)
        _refused("GD_EINVAL", d.set_history, np.zeros((0, 4, 3), np.float32))
        d.set_history(x)
        d.set_labels(label, 2)
        every = d.pairs(2, *args)
        assert every.count.shape == (5, 3, 10)
        _same(every, dr.pairs(x, 2, *args, label, 2))
        # stride 2, from origin 1; explicit origins
        _same(d.pairs(2, *args, first_origin=1, origin_stride=2), dr.pairs(x, 2, *args, label, 2, first=1, stride=2))
        some = d.pairs(2, *args, first_origin=0, n_origins=3, origin_stride=2)
        assert _bytes(some)[:4] == _bytes(dcorr.Pairs(*(t[::2] for t in every[:4]), every.scale_bits))[:4]
        _refused("GD_EINVAL", d.pairs, 2, *args, first_origin=1, n_origins=3, origin_stride=2)      # origin 5 + lag 2 = F
        _refused("GD_EINVAL", d.pairs, 2, *args, first_origin=5, n_origins=1)
        _refused("GD_EINVAL", d.pairs, 0, *args)
        _refused("GD_EINVAL", d.pairs, 1, *args, origin_stride=0)
        _refused("GD_EINVAL", d.pairs, 1, 0.0, 1.0)
        _refused("GD_EINVAL", d.pairs, 1, 0.1, 1.0, (3.0, 0.0, 3.0))
        _refused("GD_EINVAL", d.pairs, 1, *args, scale_bits=41)
        _refused("GD_EINVAL", d.set_labels, label, 1)            # label 1 >= K
        _refused("GD_EINVAL", d.set_labels, label - 1, 2)        # below -1
        _refused("GD_EINVAL", d.set_labels, label, 9)            # more than 8 labels
        for lag in (7, 9):                                       # a lag with no origin is legal and returns nothing
            none = d.pairs(lag, *args)
            assert none.count.shape == (0, 3, 10) and none.sum.shape == (0, 3, 10) and none.self_sum.shape == (0, 2)
        assert d.pairs(6, *args).count.shape == (1, 3, 10)
        assert _bytes(d.pairs(2, *args)) == _bytes(every)        # every refused call left the handle as it was
        d.set_history(x[::-1].copy())                            # the same N: labels are kept
        assert d.n_labels == 2 and d.n_classes == 3
        _same(d.pairs(2, *args), dr.pairs(x[::-1], 2, *args, label, 2))
        d.set_chains(np.arange(300) % 5)
        assert d.n_classes == 6
        d.set_history(x[:, :200].copy())                         # another N: labels and chains are dropped
        assert d.n_labels == 1 and d.n_classes == 1
        _same(d.pairs(2, *args), dr.pairs(x[:, :200], 2, *args))
        bad = x.copy()
        bad[3, 17, 2] = np.inf
        _refused("GD_EINVAL", d.set_history, bad)                # a non-finite coordinate: the handle is left without a history
        _refused("GD_ESTATE", d.pairs, 1, *args)
    _refused("GD_EINVAL", dcorr.Dcorr, 4096)


# ---- the guard

def test_guard():
    rng = np.random.default_rng(9)
    x = _walk(rng, 3, 100, (3.0, 3.0, 3.0), 0.05, np.float64)
    x[1:, 40, 0] += 1e6
    args = (0.1, 1.0, None)
    with dcorr.Dcorr(0) as d:
        d.set_history(x)
        _refused("GD_EINVAL", d.pairs, 1, *args, scale_bits=40)
        want = dr.pairs(x, 1, *args)
        assert 0 < want[4] < 20 and want[4] == dr.auto_scale(100, dr.largest_t2(x, 1))
        _same(d.pairs(1, *args), want)                           # still usable; the automatic S is the restatement's
        _refused("GD_EINVAL", d.pairs, 1, *args, scale_bits=want[4] + 1)
        _same(d.pairs(1, *args, scale_bits=want[4]), want)
        # the second lag's displacements are small again: its own, larger S
        assert d.pairs(1, *args, first_origin=1).scale_bits == dr.MAX_SCALE_BITS
        x[2, 41, 1] = 1e300                                      # t2 overflows: no scale is legal
        d.set_history(x)
        _refused("GD_EINVAL", d.pairs, 1, *args)
        assert d.pairs(1, *args, n_origins=1).scale_bits == want[4]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_automatic_scale_over_magnitudes(dtype):
    """the device's exact guard against the restatement's rational arithmetic, from displacements of 1e-9 to 1e7, and selections of
    no bead, one and two"""
    rng = np.random.default_rng(13)
    x0 = rng.uniform(size=(60, 3)) * 2.0
    u = rng.normal(size=(60, 3))
    seen = set()
    with dcorr.Dcorr(0) as d:
        for f in (0.0, 1e-9, 3e-5, 1e-2, 1.0, 37.0, 4e3, 1e5, 1e7):
            x = np.stack([x0, x0 + f * u]).astype(dtype)
            want = dr.pairs(x, 1, 0.25, 1.5)
            d.set_history(x)
            d.set_labels(None)
            got = d.pairs(1, 0.25, 1.5)
            _same(got, want, f)
            seen.add(got.scale_bits)
            if got.scale_bits < dr.MAX_SCALE_BITS:
                _refused("GD_EINVAL", d.pairs, 1, 0.25, 1.5, None, got.scale_bits + 1)
            for chosen in ([], [7], [7, 8]):      # no pair, or one: the self terms still obey the guard
                label = np.full(60, -1)
                label[chosen] = 0
                d.set_labels(label, 1)
                _same(d.pairs(1, 0.25, 1.5), dr.pairs(x, 1, 0.25, 1.5, None, label, 1), (f, chosen))
    assert len(seen) >= 4 and min(seen) < 10 and max(seen) == dr.MAX_SCALE_BITS


# ---- determinism

def test_determinism():
    rng = np.random.default_rng(10)
    x = _walk(rng, 6, 2000, (5.0, 5.0, 5.0), 0.05, np.float32)
    label, chain = rng.integers(-1, 4, size=2000), np.arange(2000) // 250
    lags = [1, 2, 4]
    first = None
    for mf in (1, 2, 0):
        for box in ((5.0, 5.0, 5.0), None):
            with _device(x, label, 4, chain, mf) as d:
                a = {lag: _bytes(d.pairs(lag, 0.1, 1.0, box)) for lag in lags}
                b = {lag: _bytes(d.pairs(lag, 0.1, 1.0, box)) for lag in lags[::-1]}      # again, the lags permuted
            assert a == b, mf
            if first is None:
                first = {}
            assert first.setdefault(box, a) == a, (mf, box)
    with _device(x, label, 4, chain) as d:
        _same(d.pairs(4, 0.1, 1.0, (5.0, 5.0, 5.0)), dr.pairs(x, 4, 0.1, 1.0, (5.0, 5.0, 5.0), label, 4, chain))


# ---- the live feed

def test_live_feed_equals_the_host_feed(hip):
    s = g.System(hip, 300, 2)
    s.set_positions(np.random.default_rng(11).normal(size=(2, 300, 3)))
    with s, live.History(s, frames_per_block=4) as hist, live.History(s, replicas=[0]) as empty, dcorr.Dcorr(0) as fed, dcorr.Dcorr(0) as dev:
        _refused("GD_ESTATE", dev.set_history_from, empty, 0)      # no frame yet
        for k in range(6):
            s.run(5, 1e-4, 1.0, seed=30 + k, noise=g.NOISE_PHILOX)
            hist.record(quantize=True)
        frames = hist.fetch(1)
        assert frames.shape == (6, 300, 3)
        fed.set_history(frames)
        dev.set_history_from(hist, 1)
        assert dev.shape == fed.shape == (6, 300)
        label, chain = np.arange(300) % 3 - 1, np.arange(300) // 150
        for d in (fed, dev):
            d.set_labels(label, 2)
            d.set_chains(chain)
        for lag in (1, 5):
            a, b = dev.pairs(lag, 0.2, 1.5), fed.pairs(lag, 0.2, 1.5)
            assert _bytes(a) == _bytes(b) and a.count.sum() > 0
        _same(dev.pairs(2, 0.2, 1.5), dr.pairs(frames, 2, 0.2, 1.5, None, label, 2, chain))
        _refused("GD_EINVAL", dev.set_history_from, empty, 1)      # a replica that is not recorded
        before = _bytes(dev.pairs(1, 0.2, 1.5))
        _refused("GD_ESTATE", dev.set_history_from, empty, 0)
        assert _bytes(dev.pairs(1, 0.2, 1.5)) == before            # a refused call leaves the handle as it was


# ---- mid size, against a cKDTree-backed evaluation of the same rules

def test_mid_size_against_kdtree():
    rng = np.random.default_rng(12)
    n, md, bw = 20000, 0.5, 0.05
    x = _walk(rng, 2, n, (10.0, 10.0, 10.0), 0.05, np.float32)
    label, chain = rng.integers(0, 4, size=n), np.arange(n) // 2500
    candidates = lambda p: scipy.spatial.cKDTree(p).query_pairs(md + 1e-6, output_type="ndarray").T
    want = dr.pairs(x, 1, bw, md, None, label, 4, chain, candidates=candidates)
    with _device(x, label, 4, chain) as d:
        got = d.pairs(1, bw, md)
        _same(got, want)
        assert got.count.sum() > 4 * n
        c = d.correlation(1, bw, md)
    assert c.dot.shape == c.normalised.shape == (20, 10) and c.r.shape == (10,)
    w = dcorr.curves(*want[:5], 4, True, bw, md)
    assert np.array_equal(c.dot, w.dot, equal_nan=True) and np.array_equal(c.normalised, w.normalised, equal_nan=True)
    assert np.nansum(c.dot[:, :4] * c.count[:, :4]) > 0      # the common swirl: near neighbours move together


# ---- the program gd_dcorr end to end (HDF5 in, HDF5 out)

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5DUMP = "/opt/conda/bin/h5dump"
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


@pytest.fixture(scope="module")
def progs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_dcorr"])
    return {k: os.path.join(HOST, k) for k in ("gd_h5tool", "gd_dcorr")}


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


def _same_as_class(progs, tmp, out, root, d, lags, bw, md, box, stride=1):
    per_lag = [d.pairs(lag, bw, md, box, origin_stride=stride) for lag in lags]
    tot = [dcorr.totals(p) for p in per_lag]
    want = {"lags": np.array(lags), "bin_edges": dcorr.bin_edges(bw, md), "scale_bits": np.array([p.scale_bits for p in per_lag]),
            "count": np.stack([t[0] for t in tot]), "sum": np.stack([t[1] for t in tot]),
            "self_count": np.stack([t[2] for t in tot]), "self_sum": np.stack([t[3] for t in tot])}
    for name, w in want.items():
        got = _dataset(progs, tmp, out, f"{root}/{name}")
        assert got.shape == w.shape and got.tobytes() == w.astype(np.float64).tobytes(), name
    assert (want["sum"] < 0).any() and (want["sum"] > 0).any()
    return per_lag


@needs_h5
def test_program_end_to_end(progs, tmp_path):
    import json
    import re
    rng = np.random.default_rng(17)
    F, N = 23, 40
    walk = np.cumsum(rng.normal(scale=0.2, size=(F, N, 3)), axis=0) + np.cumsum(rng.normal(scale=0.5, size=(1, N, 3)), axis=1)
    hist = (np.round(walk * 65536) / 65536).astype(np.float32)      # what a trajectory file stores
    a = _traj(progs, tmp_path / "traj_a.h5", hist)
    b = _traj(progs, tmp_path / "traj_b.h5", hist[::-1])
    out = tmp_path / "dcorr.h5"
    dry = subprocess.run([progs["gd_dcorr"], "--dry-run", "--log-lags", "4", "--bin-width", "0.25", "--max-distance", "2", str(out), str(a)],
                         check=True, capture_output=True, text=True)
    assert not out.exists() and "traj_a" in dry.stdout
    # no metadata: one label of all beads; two samples in one run
    subprocess.run([progs["gd_dcorr"], "--lags", "1,2,22,5", "--bin-width", "0.25", "--max-distance", "2", "--per-origin", str(out), str(a), str(b)],
                   check=True, capture_output=True)
    for sample, frames in (("traj_a", hist), ("traj_b", hist[::-1])):
        with dcorr.Dcorr(0) as d:
            d.set_history(np.ascontiguousarray(frames))
            per_lag = _same_as_class(progs, tmp_path, out, f"/dcorr/interphase/{sample}", d, [1, 2, 22, 5], 0.25, 2.0, None)
        for lag, p in zip([1, 2, 22, 5], per_lag):
            for name, w in (("count", p.count), ("sum", p.sum), ("self_count", p.self_count), ("self_sum", p.self_sum)):
                got = _dataset(progs, tmp_path, out, f"/dcorr/interphase/{sample}/per_origin/lag_{lag}/{name}")
                assert got.shape == w.shape and np.array_equal(got, w.astype(np.float64)), (lag, name)      # (values below 2^53)
        names = subprocess.check_output([H5DUMP, "-d", f"/dcorr/interphase/{sample}/class_names", str(out)], text=True)
        assert re.findall(r'"([^"]*)"', names.split("DATA {", 1)[1]) == ["all-all"]
    hdr = subprocess.check_output([H5DUMP, "-H", "-p", "-d", "/dcorr/interphase/traj_a/count", str(out)], text=True)
    assert "H5T_STD_U64LE" in hdr
    hdr = subprocess.check_output([H5DUMP, "-H", "-p", "-d", "/dcorr/interphase/traj_a/per_origin/lag_1/sum", str(out)], text=True)
    assert "H5T_STD_I64LE" in hdr
    # with metadata: labels by particle type, chains from chromosome_ranges, a periodic box, every second origin
    meta = tmp_path / "meta"
    meta.mkdir()
    types = (np.arange(N) % 3).astype("i1")
    (meta / "config.json").write_text(json.dumps({"made": "for this test"}))
    np.zeros((N, 2), "<f4").tofile(meta / "ab.f32")
    types.tofile(meta / "types.i8")
    np.zeros((0, 2), "<i4").tofile(meta / "nucleolus_bonds.i32")
    (meta / "chromosomes.tsv").write_text("chrA 0 15 3 5\nchrB 15 36 20 22\n")
    (meta / "nucleoli.tsv").write_text("")
    c = tmp_path / "traj_c.h5"
    subprocess.check_call([progs["gd_h5tool"], "make-metadata", str(c), str(meta)])
    _traj(progs, c, hist)
    subprocess.run([progs["gd_dcorr"], "--name", "interphase", "--groups", "types", "--split-chains", "--log-lags=5", "--bin-width=0.25",
                    "--max-distance", "1.5", "--origin-stride", "2", "--box", "6,7,8", str(out), str(c)], check=True, capture_output=True)
    lags = [1, 2, 5, 10, 22]      # 5 values spaced geometrically over [1, 22], rounded half up (gd_msd's --log-lags)
    with dcorr.Dcorr(0) as d:
        d.set_history(hist)
        d.set_labels(types, 3)
        d.set_chains(np.where(np.arange(N) < 15, 0, np.where(np.arange(N) < 36, 1, 2)))      # beads of no range share one more chain
        _same_as_class(progs, tmp_path, out, "/dcorr/interphase/traj_c", d, lags, 0.25, 1.5, (6.0, 7.0, 8.0), stride=2)
    names = subprocess.check_output([H5DUMP, "-d", "/dcorr/interphase/traj_c/class_names", str(out)], text=True)
    names = [n.split("\\000")[0] for n in re.findall(r'"([^"]*)"', names.split("DATA {", 1)[1])]      # (h5dump shows the padding)
    assert names[:3] == ["0-0/same", "0-0/different", "0-A/same"] and len(names) == 12 and names[0].endswith("/same") and names[1].endswith("/different")
    assert _dataset(progs, tmp_path, out, "/dcorr/interphase/traj_a/lags").tolist() == [1, 2, 22, 5]      # earlier samples stay

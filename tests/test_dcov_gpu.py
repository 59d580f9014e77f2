"""The displacement covariance maps on the device (include/gdyn_dcov.h, csrc/gdyn_dcov.hip) against the numpy restatement
(tests/dcov_restatement.py): the rows byte for byte, every cell of the map within the header's bound of the long-double product of the
device's own rows, count and the integer case exactly, and against themselves bit for bit: from run to run, for every
columns_per_stage, for a cell whatever rectangle asks for it, between M and its transpose, and between a host-fed and a live-fed
history.  Then the program gd_covariance_map end to end.

The shapes are chosen to break the kernel, not to resemble a genome: 330 beads in 83 bins, and 83 = 64 + 16 + 3 crosses a tile of 64
cells and leaves a partial 16-cell instruction tile in both directions; bins of 1, 2 and 7 beads, one of 40 beads (two pieces), two
gaps of beads in no bin; 266 frames and lag 3, so 263 origins and 789 columns: one range of 768 columns plus 21, which is no multiple
of 4.  The knobs are one group of four columns, a few, a count that divides neither 768 nor 24, and automatic.

Largest error over bound measured on one MI355X (profiles/dcov_gpu_tests.log): see the lines the bound test prints."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dcov_restatement as dc
from conftest import ROOT
from test_dcov_host import integer_walk
from test_dmap_gpu import _dataset, _strings, _traj

pytestmark = pytest.mark.gpu
g = importlib.import_module("2022a-genome-dynamics_amd")
dcov = importlib.import_module("2022a-genome-dynamics_amd.dcov")
live = importlib.import_module("2022a-genome-dynamics_amd.live")

KNOBS = [0, 4, 12, 100]
F, N, LAG = 266, 330, 3
COLUMNS = 3 * (F - LAG)
KEYS = ("sum", "count", "diag_rows", "diag_cols")


def _bins():
    """83 bins: 1, 2 and 7 beads, a gap, 40 beads (32 + 8: two pieces), a gap, then 79 bins of 3, 2, 3, ... beads; beads 268-329 in none."""
    out, at = [], 0
    for size, gap in [(1, 0), (2, 0), (7, 2), (40, 5)] + [((3, 2, 3)[k % 3], 0) for k in range(79)]:
        out.append((at, at + size))
        at += size + gap
    assert len(out) == 83 and at == 268 and out[3] == (12, 52) and out[3][1] - out[3][0] > dcov.DCOV_PIECE_BEADS
    return out


BINS = _bins()
B = len(BINS)
assert COLUMNS == 789 and COLUMNS > dcov.DCOV_COLUMN_RANGE and (COLUMNS - dcov.DCOV_COLUMN_RANGE) % 4 and B == 64 + 16 + 3

# (lag, first, stride, count, remove_drift): both modes, with and without drift removal, a strided and counted choice of each
PREPARATIONS = {"lag3": (LAG, 0, 1, 0, False), "lag3-drift": (LAG, 0, 1, 0, True), "fluct": (0, 0, 1, 0, False), "fluct-drift": (0, 0, 1, 0, True),
                "lag7-strided": (7, 5, 3, 60, True), "fluct-strided": (0, 2, 5, 40, False)}


def _refused(status, fn, *args, **kw):
    with pytest.raises(g.GdynError) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(status + ": "), str(e.value)


def _bytes(m, keys=KEYS):
    return [m[k].tobytes() for k in keys]


@pytest.fixture(scope="module")
def coils():
    """{dtype: history}; read by the tests, changed by none.  A random walk along the beads, moving a little from frame to frame."""
    rng = np.random.default_rng(2025)
    x = np.cumsum(rng.normal(scale=0.6, size=(1, N, 3)), axis=1) + np.cumsum(rng.normal(scale=0.05, size=(F, N, 3)), axis=0) + 100.0
    return {dt: x.astype(dt) for dt in (np.float32, np.float64)}


@pytest.fixture(scope="module")
def full(coils):
    """(rows, whole map) of the device for the float32 history, lag 3, automatic knob; read by the tests, changed by none"""
    with dcov.Dcov(0) as d:
        d.set_history(coils[np.float32])
        d.set_bins(BINS)
        assert d.prepare(LAG) == COLUMNS == d.columns
        return d.rows(), d.map()


# ---- stage 1

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_rows_equal_the_restatement(coils, dtype):
    x = coils[dtype]
    with dcov.Dcov(0) as d:
        d.set_history(x)
        assert d.n_bins == N and d.columns == 0
        d.set_bins(BINS)
        for what, (lag, first, stride, count, drift) in PREPARATIONS.items():
            want = dc.rows(x, BINS, lag, first, stride, count, drift)
            assert d.prepare(lag, first, stride, count, drift) == want.shape[1], what
            got = d.rows()
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), what
            assert d.rows(3, 1).tobytes() == want[3:4].tobytes() and d.rows(60, 23).tobytes() == want[60:].tobytes(), what
        d.set_bins(None)      # every bead its own bin
        want = dc.rows(x, None, 0, 1, 7, 11, True)
        assert d.prepare(0, 1, 7, 11, True) == 33 and d.rows().tobytes() == want.tobytes()


# ---- the map

@pytest.mark.skipif(not dc.LONGDOUBLE_64, reason="np.longdouble has no 64-bit significand here: no reference")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_map_within_the_bound_of_its_own_rows(coils, dtype):
    with dcov.Dcov(0) as d:
        d.set_history(coils[dtype])
        d.set_bins(BINS)
        for what, (lag, first, stride, count, drift) in PREPARATIONS.items():
            columns = d.prepare(lag, first, stride, count, drift)
            a, m = d.rows(), d.map()
            ref, mag = dc.reference(a)
            err, tol = np.abs(m["sum"].astype(np.longdouble) - ref), dc.bound(mag, columns)
            print(f"{what} {dtype.__name__}: {columns} columns, largest |device - long double| / bound:", float(np.max(err / tol)),
                  " over u sum|a||b|:", float(np.max(err / (mag * np.longdouble(dc.U)))))
            assert (tol > 0).all() and (err <= tol).all(), (what, float(np.max(err / tol)))
            assert np.array_equal(m["count"], dc.count(BINS, columns // 3)) and m["count"].dtype == np.uint64, what
            assert m["diag_rows"].tobytes() == m["diag_cols"].tobytes() == np.ascontiguousarray(np.diag(m["sum"])).tobytes(), what
            assert (m["diag_rows"] > 0).all() and m["sum"].tobytes() == np.ascontiguousarray(m["sum"].T).tobytes(), what
            # an asymmetric rectangle: its rows and columns are different bins, so a transposed result layout cannot pass
            part = d.map(rows=(2, 30), cols=(50, 33))
            assert (np.abs(part["sum"].astype(np.longdouble) - ref[2:32, 50:83]) <= tol[2:32, 50:83]).all(), what
        mean, corr = dcov.Dcov.mean(m), dcov.Dcov.correlation(m)
        assert mean[1, 3] == m["sum"][1, 3] / m["count"][1, 3] and np.array_equal(np.diag(corr), np.ones(B))
        assert np.abs(corr).max() <= 1 + 1e-12 and corr[1, 3] == m["sum"][1, 3] / np.sqrt(m["sum"][1, 1] * m["sum"][3, 3])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_integer_coordinates_are_exact(dtype):
    """Item 5: |x| < 2^10, bins of at most 64 beads, 263 origins: every entry and every sum an integer below 2^46."""
    x = integer_walk(F, N).astype(dtype)
    want_rows = dc.rows(x, BINS, LAG)
    want = dc.integer_map(want_rows)
    assert np.abs(want).max() < 2 ** 46 and len(np.unique(want)) > 1000
    for knob in (0, 12):
        with dcov.Dcov(0, knob) as d:
            d.set_history(x)
            d.set_bins(BINS)
            d.prepare(LAG)
            assert np.array_equal(d.rows(), want_rows), knob
            m = d.map()
            assert np.array_equal(m["sum"], want) and np.array_equal(m["diag_rows"], np.diag(want)), knob
            part = d.map(rows=(60, 10), cols=(0, 83))      # across the tile boundary, asymmetric
            assert np.array_equal(part["sum"], want[60:70]) and np.array_equal(part["diag_cols"], np.diag(want)), knob
            d.set_bins(None)      # bead resolution: 330 bins, 6 x 6 tiles, the last of 10 cells
            d.prepare(LAG, 0, 2, 100)
            beads = dc.rows(x, None, LAG, 0, 2, 100)
            assert np.array_equal(d.map()["sum"], dc.integer_map(beads)), knob
            assert np.array_equal(d.map(rows=(300, 30), cols=(100, 101))["sum"], dc.integer_map(beads[300:], beads[100:201])), knob


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bit_identity_from_run_to_run_and_for_every_knob(coils, full, dtype):
    first = None
    for knob in KNOBS + [0]:
        with dcov.Dcov(0, knob) as d:
            d.set_history(coils[dtype])
            d.set_bins(BINS)
            d.prepare(LAG, remove_drift=True)
            m = d.map()
            first = first or _bytes(m)
            assert _bytes(m) == first, knob      # run to run (the second knob 0) and for every knob
            assert _bytes(d.map()) == first, knob
            if dtype is np.float32:
                d.prepare(LAG)
                assert d.rows().tobytes() == full[0].tobytes() and _bytes(d.map()) == _bytes(full[1]), knob


RECTANGLES = {"one cell": ((20, 1), (4, 1)), "one cell of the long bin": ((3, 1), (3, 1)), "across bins 63|64": ((60, 8), (62, 5)),
              "above the diagonal": ((2, 8), (18, 60)), "below the diagonal": ((70, 13), (0, 12)), "across the diagonal": ((10, 60), (5, 70)),
              "a row strip": ((63, 2), (0, 83)), "the last tile": ((80, 3), (79, 4))}


@pytest.mark.parametrize("knob", [0, 4])
def test_a_cell_does_not_know_its_rectangle(coils, full, knob):
    whole = full[1]
    with dcov.Dcov(0, knob) as d:
        d.set_history(coils[np.float32])
        d.set_bins(BINS)
        d.prepare(LAG)
        for what, (rows, cols) in RECTANGLES.items():
            r, c = slice(rows[0], rows[0] + rows[1]), slice(cols[0], cols[0] + cols[1])
            m = d.map(rows=rows, cols=cols)
            assert m["sum"].shape == (rows[1], cols[1]) and m["diag_rows"].shape == (rows[1],) and m["diag_cols"].shape == (cols[1],), what
            assert _bytes(m) == [np.ascontiguousarray(whole[k][r, c]).tobytes() for k in ("sum", "count")] + \
                [whole["diag_rows"][r].tobytes(), whole["diag_cols"][c].tobytes()], what
            t = d.map(rows=cols, cols=rows)      # the transposed rectangle, a call of its own: a row strip against its column strip
            assert t["sum"].tobytes() == np.ascontiguousarray(m["sum"].T).tobytes() and t["count"].tobytes() == np.ascontiguousarray(m["count"].T).tobytes(), what
            assert t["diag_rows"].tobytes() == m["diag_cols"].tobytes() and t["diag_cols"].tobytes() == m["diag_rows"].tobytes(), what


def test_symmetry(full):
    whole = full[1]
    for k in ("sum", "count"):
        assert whole[k].tobytes() == np.ascontiguousarray(whole[k].T).tobytes(), k
    assert whole["diag_rows"].tobytes() == whole["diag_cols"].tobytes() == np.ascontiguousarray(np.diag(whole["sum"])).tobytes()
    assert (whole["diag_rows"] > 0).all() and (whole["sum"] < 0).any()


# ---- the live feed

def test_live_feed_equals_the_host_feed(hip):
    s = g.System(hip, 300, 2)
    s.set_positions(np.random.default_rng(8).normal(size=(2, 300, 3)))
    with s, live.History(s, frames_per_block=5) as hist, live.History(s, replicas=[0]) as empty, dcov.Dcov(0) as fed, dcov.Dcov(0, 8) as dev:
        _refused("GD_ESTATE", dev.set_history_from, empty, 0)      # no frame yet
        for k in range(12):
            s.run(5, 1e-4, 1.0, seed=70 + k, noise=g.NOISE_PHILOX)
            hist.record(quantize=True)
        frames = hist.fetch(1)
        assert frames.shape == (12, 300, 3) and not np.array_equal(frames, hist.fetch(0))
        fed.set_history(frames)
        dev.set_history_from(hist, 1)
        assert dev.shape == fed.shape == (12, 300) and dev.n_bins == 300
        bins = dcov.Dcov.bins_from_chains([(0, 150), (150, 300)], 11)
        for d in (fed, dev):
            d.set_bins(bins)
        for lag, drift in ((2, True), (0, False)):
            assert dev.prepare(lag, remove_drift=drift) == fed.prepare(lag, remove_drift=drift) == 3 * (12 - lag)
            assert dev.rows().tobytes() == fed.rows().tobytes() == dc.rows(frames, bins, lag, remove_drift=drift).tobytes()
            a, b = dev.map(), fed.map()
            assert _bytes(a) == _bytes(b) and a["diag_rows"].min() > 0
            assert _bytes(dev.map(rows=(3, 9), cols=(0, 28))) == _bytes(fed.map(rows=(3, 9), cols=(0, 28)))
        _refused("GD_EINVAL", dev.set_history_from, empty, 1)      # a replica that is not recorded
        _refused("GD_EINVAL", dcov.Dcov, 4096)                     # a device that does not exist
        _refused("GD_ESTATE", dev.set_history_from, empty, 0)
        assert _bytes(dev.map()) == _bytes(a)      # a refused call leaves the handle as it was


# ---- errors

def test_refusals_leave_the_handle_usable(coils, full):
    EINVAL, ESTATE = 1, 5      # gd_status of gdyn.h
    x = coils[np.float32]
    with dcov.Dcov(0) as d:
        for call in (lambda: d.map(), lambda: d.rows(0, 1), lambda: d.prepare(LAG), lambda: d.set_bins(BINS), lambda: d.set_bins(None)):      # before a history
            _refused("GD_ESTATE", call)
        _refused("GD_EINVAL", d.set_history, np.zeros((0, 4, 3), np.float32))
        d.set_history(x)
        _refused("GD_ESTATE", d.map)                                    # a history, but nothing prepared
        _refused("GD_ESTATE", d.rows)
        d.set_bins(BINS)
        d.prepare(LAG)
        good = _bytes(full[1])
        assert _bytes(d.map()) == good
        _refused("GD_EINVAL", d.prepare, F)                             # a lag that leaves no origin
        _refused("GD_EINVAL", d.prepare, F - 1, 1)
        _refused("GD_EINVAL", d.prepare, LAG, 0, 0)                     # stride 0
        _refused("GD_EINVAL", d.prepare, LAG, 0, 1, F - LAG + 1)        # an explicit origin whose partner is past the history
        _refused("GD_EINVAL", d.prepare, LAG, 200, 2, 33)
        _refused("GD_EINVAL", d.prepare, 0, F)                          # fluctuation mode without a frame
        _refused("GD_EINVAL", d.prepare, 0, 0, 1, F + 1)
        _refused("GD_EINVAL", d.map, rows=(80, 4))                      # a rectangle past B
        _refused("GD_EINVAL", d.map, cols=(B, 1))
        _refused("GD_EINVAL", d.map, rows=(0, 0))
        _refused("GD_EINVAL", d.rows, 80, 4)
        _refused("GD_EINVAL", d.rows, 0, 0)
        _refused("GD_EINVAL", d.set_bins, [(0, 60), (50, 130)])         # overlapping
        _refused("GD_EINVAL", d.set_bins, [(50, 130), (0, 50)])         # not ascending
        _refused("GD_EINVAL", d.set_bins, [(0, N + 1)])                 # beyond N
        _refused("GD_EINVAL", d.set_bins, [(0, 5), (5, 5)])             # empty
        assert d.dll.gd_dcov_rows(d._h, 0, 1, None) == EINVAL and d.dll.gd_last_error().startswith(b"gd_dcov_rows: NULL")
        assert d.dll.gd_dcov_set_history(d._h, None, 3, 3, 0) == EINVAL and d.dll.gd_dcov_set_bins(d._h, None, 3) == EINVAL
        assert d.columns == COLUMNS and _bytes(d.map()) == good         # every refused call left the handle, and its preparation, as it was
        d.prepare(LAG, 0, 1, F - LAG)                                   # the last origin that fits, asked for explicitly
        assert _bytes(d.map()) == good
        # outputs that are not asked for are not written; count alone needs no kernel
        cnt = np.zeros((B, B), np.uint64)
        assert d.dll.gd_dcov_map(d._h, 0, B, 0, B, None, cnt.ctypes.data, None, None) == 0 and cnt.tobytes() == good[1]
        # new bins drop the preparation, the same bins again too
        d.set_bins(BINS)
        assert d.columns == 0
        _refused("GD_ESTATE", d.map)
        assert d.dll.gd_dcov_map(d._h, 0, 1, 0, 1, None, cnt.ctypes.data, None, None) == ESTATE
        d.prepare(LAG)
        assert _bytes(d.map()) == good
        # a non-finite coordinate: refused, and the handle is left without a history; the bins stay for a history of the same N
        bad = x.copy()
        bad[F - 1, N - 1, 2] = np.inf
        _refused("GD_EINVAL", d.set_history, bad)
        _refused("GD_ESTATE", d.map)
        _refused("GD_ESTATE", d.prepare, LAG)
        assert d.columns == 0
        d.set_history(x)
        _refused("GD_ESTATE", d.map)                                    # a new history drops the preparation
        assert d.n_bins == B and d.prepare(LAG) == COLUMNS and _bytes(d.map()) == good
        d.set_history(x[:, :100])      # another N: the bins are dropped
        assert d.n_bins == 100 and d.prepare(1, 0, 1, 2) == 6 and d.map()["count"].shape == (100, 100) and (d.map()["count"] == 2).all()


# ---- the program gd_covariance_map end to end (HDF5 in, HDF5 out)

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


@pytest.fixture(scope="module")
def progs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_covariance_map"])
    return {k: os.path.join(HOST, k) for k in ("gd_h5tool", "gd_covariance_map")}


def _same_as_class(progs, tmp, out, root, hist, bins, selected, lag, first, stride, count, drift, with_rows):
    with dcov.Dcov(0) as d:
        d.set_history(hist)
        d.set_bins(bins)
        d.prepare(lag, first, stride, count, drift)
        m, a = d.map(), d.rows()
    sel = np.ix_(selected, selected)
    frames = dc.origins(len(hist), lag, first, stride, count)
    want = {"bins": np.asarray(bins)[selected], "sum": m["sum"][sel], "count": m["count"][sel], "lag": np.array([lag]), "origins": np.array(frames),
            "remove_drift": np.array([int(drift)])}
    if with_rows:
        want["rows"] = a[selected]
    for name, w in want.items():
        got = _dataset(progs, tmp, out, f"{root}/{name}")
        assert got.shape == w.shape and got.tobytes() == w.astype(np.float64).tobytes(), name
    assert (want["sum"] != 0).all()
    listing = subprocess.check_output(["/opt/conda/bin/h5dump", "-n", str(out)], text=True)
    assert (f"{root}/rows" in listing) == with_rows


@needs_h5
def test_program_end_to_end(progs, tmp_path):
    rng = np.random.default_rng(17)
    F_, N_ = 23, 40
    walk = np.cumsum(rng.normal(scale=0.05, size=(F_, N_, 3)), axis=0) + np.cumsum(rng.normal(scale=0.5, size=(1, N_, 3)), axis=1)
    hist = (np.round(walk * 65536) / 65536).astype(np.float32)      # what a trajectory file stores
    a = _traj(progs, tmp_path / "traj_a.h5", hist)
    b = _traj(progs, tmp_path / "traj_b.h5", hist[::-1])
    out = tmp_path / "dcov.h5"
    prog = progs["gd_covariance_map"]
    # no metadata: one chain of all beads; two samples in one run; a frame window, a stride, drift removal, the rows
    subprocess.run([prog, "--lag", "2", "--rebin-rate", "3", "--frames", "2:20", "--origin-stride", "3", "--remove-drift", "--rows", str(out), str(a), str(b)],
                   check=True, capture_output=True)
    bins = dcov.Dcov.bins_from_chains([(0, N_)], 3)
    for sample, frames in (("traj_a", hist), ("traj_b", hist[::-1])):
        _same_as_class(progs, tmp_path, out, f"/dcov/interphase/{sample}", np.ascontiguousarray(frames), bins, np.arange(len(bins)), 2, 2, 3, 6, True, True)
        assert _strings(out, f"/dcov/interphase/{sample}/chain_names") == ["all"]
    hdr = subprocess.check_output(["/opt/conda/bin/h5dump", "-H", "-p", "-d", "/dcov/interphase/traj_a/count", str(out)], text=True)
    assert "H5T_STD_U64LE" in hdr and "SHUFFLE" in hdr and "LEVEL 1" in hdr
    # fluctuation mode over all frames, by chain selection of runs: chains from chromosome_ranges; beads 36 to 39 are in no chain
    meta = tmp_path / "meta"
    meta.mkdir()
    (meta / "config.json").write_text('{"made": "for this test"}')
    np.zeros((N_, 2), "<f4").tofile(meta / "ab.f32")
    (np.arange(N_) % 3).astype("i1").tofile(meta / "types.i8")
    np.zeros((0, 2), "<i4").tofile(meta / "nucleolus_bonds.i32")
    (meta / "chromosomes.tsv").write_text("chrA 0 15 3 5\nchrB 15 30 20 22\nchrC 30 36 1 2\n")
    (meta / "nucleoli.tsv").write_text("")
    c = tmp_path / "traj_c.h5"
    subprocess.check_call([progs["gd_h5tool"], "make-metadata", str(c), str(meta)])
    _traj(progs, c, hist)
    chains = [(0, 15), (15, 30), (30, 36)]
    rate4 = dcov.Dcov.bins_from_chains(chains, 4)      # 4 + 4 + 2 bins
    for args, bins, selected, lag, drift, with_rows in (
            (["--fluctuation", "--rebin-rate", "4"], rate4, np.arange(10), 0, False, False),
            (["--lag=5", "--rebin-rate=4", "--chains", "chrA,chrC", "--rows"], rate4, np.r_[0:4, 8:10], 5, False, True),      # two runs of bins
            (["--lag", "1", "--by-chain", "--remove-drift"], chains, np.arange(3), 1, True, False)):
        subprocess.run([prog, *args, str(out), str(c)], check=True, capture_output=True)
        _same_as_class(progs, tmp_path, out, "/dcov/interphase/traj_c", hist, bins, selected, lag, 0, 1, 0, drift, with_rows)
        assert _strings(out, "/dcov/interphase/traj_c/chain_names") == ["chrA", "chrB", "chrC"]
    assert _dataset(progs, tmp_path, out, "/dcov/interphase/traj_a/lag").tolist() == [2.0]      # earlier samples stay

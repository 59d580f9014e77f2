"""The connected clusters on the device (include/gdyn_cluster.h, csrc/gdyn_cluster.hip) against the numpy restatement
(tests/cluster_restatement.py).  Every output is an integer that depends on the graph alone, so every comparison is for equality:
root, summary and histogram, on chains that wind through many cells and blocks, in one crowded cell, near the percolation threshold,
in periodic boxes with fewer than three cells along an axis, with labels and link masks, from run to run, for every
max_frames_per_launch, between a host-fed and a live-fed history, and between the class and the program gd_clusters."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cluster_restatement as cr
from conftest import ROOT

pytestmark = pytest.mark.gpu
g = importlib.import_module("2022a-genome-dynamics_amd")
cluster = importlib.import_module("2022a-genome-dynamics_amd.cluster")
live = importlib.import_module("2022a-genome-dynamics_amd.live")


def _refused(status, fn, *args, **kw):
    with pytest.raises(g.GdynError) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(status + ": "), str(e.value)


def _tables(c):
    return c.root, np.stack([c.selected, c.clusters, c.largest, c.sum_s2], axis=1), c.histogram


def _bytes(c):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in _tables(c)]


def _same(got, want, what=""):
    """got: a Components; want: (root, summary, hist) of the restatement"""
    for name, a, b in zip(("root", "summary", "hist"), _tables(got), want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, len(bad), bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def _device(x, label=None, K=1, links=None, mf=0):
    c = cluster.Clusters(0, mf)
    c.set_history(x)
    if label is not None:
        c.set_labels(label, K)
    if links is not None:
        c.set_links(links)
    return c


def _repeat(want, frames):
    return tuple(np.repeat(w, frames, axis=0) for w in want)


# ---- known answers and error paths

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", cr.known_cases(), ids=[c[0] for c in cr.known_cases()])
def test_known_answers(case, dtype):
    name, x, d, box, label, K, links, root = case
    want = cr.components(x, d, box, label, K, links, n_size_bins=3)
    assert np.array_equal(want[0][0], root)
    with _device(x[None].astype(dtype), label, K, links) as c:
        _same(c.components(d, box, size_bins=3), want, name)


def test_errors_leave_a_usable_handle():
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 3, size=(4, 200, 3)).astype(np.float32)
    label = rng.integers(-1, 2, size=200)
    want = cr.components(x, 0.4, None, label, 2, "same", n_size_bins=16)
    with cluster.Clusters(0) as c:
        assert c.n_classes == 1
        _refused("GD_ESTATE", c.components, 0.4)
        _refused("GD_ESTATE", c.set_labels, label, 2)
        _refused("GD_ESTATE", c.set_links, "all")
        c.set_history(x)
        c.set_labels(label, 2)
        c.set_links("same")
        assert c.n_classes == 3
        good = lambda: _same(c.components(0.4, size_bins=16), want)      # noqa: E731
        good()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            _refused("GD_EINVAL", c.components, bad)
            good()
        for box in ((3.0, 0.0, 3.0), (3.0, float("inf"), 3.0), (float("nan"), 3.0, 3.0)):
            _refused("GD_EINVAL", c.components, 0.4, box)
        _refused("GD_EINVAL", c.set_links, 1 << 3)      # a bit at P
        _refused("GD_EINVAL", c.set_links, 0)           # nothing may link
        good()                                          # the mask is still "same"
        for bins in (0, (1 << 20) + 1):
            _refused("GD_EINVAL", c.components, 0.4, size_bins=bins)
        _refused("GD_EINVAL", c.components, 0.4, first_frame=0, n_frames=5)
        _refused("GD_EINVAL", c.components, 0.4, first_frame=4, n_frames=1)
        _refused("GD_EINVAL", c.components, 0.4, frame_stride=0)
        _refused("GD_EINVAL", c.set_labels, np.full(200, 2), 2)
        _refused("GD_EINVAL", c.set_labels, label, 9)
        good()
        assert c.components(0.4, first_frame=4).selected.shape == (0,)      # all that fit: none
        assert c.dll.gd_cluster_frames(c._h, 1, 0, 2) == 2 and c.dll.gd_cluster_frames(c._h, 0, 0, 0) == 0
        bad = x.copy()
        bad[2, 17, 1] = np.nan
        _refused("GD_EINVAL", c.set_history, bad)
        _refused("GD_ESTATE", c.components, 0.4)         # a non-finite history leaves the handle without one
        c.set_history(x)                                  # the same N: labels and mask are kept
        good()
        c.set_labels(label, 2)                            # a new label set: the mask is "all" again
        _same(c.components(0.4, size_bins=16), cr.components(x, 0.4, None, label, 2, "all", n_size_bins=16))
        c.set_history(x[:, :150])                         # another N: one label of all beads
        assert c.n_classes == 1
        _same(c.components(0.4, size_bins=16), cr.components(x[:, :150], 0.4, n_size_bins=16))
        c.set_labels(np.full(150, -1), 1)                 # nobody takes part
        r = c.components(0.4, size_bins=5)
        assert (r.root == -1).all() and not r.selected.any() and not r.clusters.any() and not r.largest.any() and not r.sum_s2.any() and not r.histogram.any()


# ---- a snake through many cells

SNAKE_NX, SNAKE_NY, SNAKE_LAYERS, SNAKE_N = 15, 8, 32, 4096


def _snake():
    """4 096 sites of a lattice path: rows along x two lattice units apart in y, layers two units apart in z, joined by single sites,
    so that only consecutive sites are nearer than sqrt 2 units.  It ends at (0, 0, 63), one unit below the image of its start in a
    box of 64 units along z."""
    pts, x, y, z, dx, dy = [], 0, 0, 0, 1, 1
    while len(pts) < SNAKE_N:
        for _ in range(SNAKE_NX):
            pts.append((x, y, z))
            x += dx
        x -= dx
        dx = -dx
        if 0 <= y + 2 * dy <= 2 * (SNAKE_NY - 1):
            pts.append((x, y + dy, z))
            y += 2 * dy
        else:
            pts.append((x, y, z + 1))
            z += 2
            dy = -dy
    assert len(pts) == SNAKE_N == SNAKE_LAYERS * SNAKE_NY * (SNAKE_NX + 1) and pts[-1] == (0, 0, 2 * SNAKE_LAYERS - 1) and len(set(pts)) == SNAKE_N
    return np.array(pts, np.float64)


@pytest.fixture(scope="module")
def snake():
    """The path at spacing 0.9 d (d = 1), its beads in a random order: (x (N, 3) float32, position of every bead along the path)"""
    perm = np.random.default_rng(2).permutation(SNAKE_N)
    return (_snake()[perm] * 0.9).astype(np.float32), perm


SNAKE_BOX = (0.9 * (SNAKE_NX + 1), 0.9 * 2 * SNAKE_NY, 0.9 * 2 * SNAKE_LAYERS)      # every image two units from the path, but for the closure


@pytest.fixture(scope="module")
def snake_wants(snake):
    x, perm = snake
    extent = x.max(axis=0) - x.min(axis=0)
    assert (extent >= 10.0).all()      # ten cells of side d and more along every axis (the kernel's own cells are wider: it keeps 16 beads or so in each)
    cut = np.where(perm % 512 == 0, -1, 0)
    one_out = np.where(perm == 1000, -1, 0)
    whole = cr.components(x, 1.0, None)
    pieces = cr.components(x, 1.0, None, cut, 1)
    ring = cr.components(x, 1.0, SNAKE_BOX, one_out, 1)
    open_ring = cr.components(x, 1.0, None, one_out, 1)
    assert whole[1][0].tolist() == [SNAKE_N, 1, SNAKE_N, SNAKE_N ** 2] and (whole[0] == 0).all()
    assert pieces[1][0, 0] == SNAKE_N - 8 and pieces[1][0, 1] in (8, 9) and pieces[1][0, 2] == 511
    assert ring[1][0].tolist() == [SNAKE_N - 1, 1, SNAKE_N - 1, (SNAKE_N - 1) ** 2]
    assert open_ring[1][0, 1] == 2      # it is the boundary that closes the ring
    return {"whole": (None, None, whole), "pieces": (None, cut, pieces), "ring": (SNAKE_BOX, one_out, ring)}


@pytest.mark.parametrize("mf", [1, 0], ids=["one-frame-launches", "automatic"])
@pytest.mark.parametrize("which", ["whole", "pieces", "ring"])
def test_snake(snake, snake_wants, which, mf):
    x, _ = snake
    box, label, want = snake_wants[which]
    frames = 6
    with _device(np.repeat(x[None], frames, axis=0), label, 1, None, mf) as c:
        got = c.components(1.0, box)
    _same(got, _repeat(want, frames), which)
    for a in _tables(got):
        assert (a == a[0]).all()


# ---- one crowded cell

def test_crowded_cell():
    rng = np.random.default_rng(3)
    d = 0.5

    def ball(n, radius, centre):
        v = rng.normal(size=(n, 3))
        return centre + v / np.linalg.norm(v, axis=1)[:, None] * radius * rng.uniform(size=(n, 1)) ** (1 / 3)

    lone = np.array([7.0, 7.0, 7.0]) + 5 * d * np.arange(20)[:, None] * np.array([1.0, 0.0, 0.0]) + rng.uniform(0, 0.1 * d, size=(20, 3))
    x = np.concatenate([ball(700, 0.3 * d, np.array([1.0, 1.0, 1.0])), ball(50, 0.3 * d, np.array([1.0, 1.0 + 3 * d, 1.0])), lone])
    x = x[rng.permutation(len(x))].astype(np.float32)
    want = cr.components(x, d, n_size_bins=64)
    assert want[1][0].tolist() == [770, 22, 700, 700 ** 2 + 50 ** 2 + 20]
    assert want[2][0, 0] == 20 and want[2][0, 49] == 1 and want[2][0, 63] == 1 and want[2][0].sum() == 22
    for box in (None, (40.0, 40.0, 80.0)):
        with _device(x[None]) as c:
            _same(c.components(d, box), want if box is None else cr.components(x, d, box, n_size_bins=64), box)


# ---- near percolation, periodic

PERC_N, PERC_BOX = 20000, (10.0, 10.0, 10.0)


@pytest.fixture(scope="module")
def percolation():
    rng = np.random.default_rng(20220101)
    x = rng.uniform(0, 10, size=(PERC_N, 3)).astype(np.float32)
    roots = {}
    for d in (0.30, 0.318, 0.34):
        sel, i, j = cr.edges(x, d, PERC_BOX, candidates=cr.kdtree_candidates(d, PERC_BOX))
        roots[d] = (cr.roots_union_find(PERC_N, sel, i, j), cr.roots_scipy(PERC_N, sel, i, j), len(i))
    return x, roots


def test_near_percolation(percolation):
    x, roots = percolation
    a, b, n_edges = roots[0.318]
    summary, _ = cr.tables(a, 64)
    sizes = np.bincount(a)
    print("d = 0.318:", n_edges, "edges,", int(summary[1]), "clusters, largest", int(summary[2]), ",", len(np.unique(sizes[sizes > 0])), "distinct sizes;",
          "d = 0.34: largest", int(cr.tables(roots[0.34][0], 1)[0][2]))
    assert 0.05 * PERC_N <= summary[2] <= 0.5 * PERC_N and len(np.unique(sizes[sizes > 0])) >= 50      # neither a gas nor one gel
    with _device(x[None]) as c:
        for d, bins in ((0.30, (64,)), (0.318, (1, 64, 4096)), (0.34, (64,))):
            for nb in bins:
                got = c.components(d, PERC_BOX, size_bins=nb)
                for route in roots[d][:2]:
                    s, h = cr.tables(route, nb)
                    _same(got, (route[None], s[None], h[None]), (d, nb))


# ---- a small periodic box: one axis with fewer than three cells

@pytest.mark.parametrize("thin", [False, True], ids=["all-beads", "one-in-seven"])
def test_small_periodic_box(thin):
    rng = np.random.default_rng(5)
    d, N = 0.4, 3000
    box = (2.5 * d, 7 * d, 40 * d)
    x = (rng.uniform(-1, 2, size=(1, N, 3)) * np.array(box)).astype(np.float32)      # also outside the box
    label = np.where(rng.uniform(size=N) < 0.85, -1, 0) if thin else None      # thinned to the threshold, where the clusters are many
    want = cr.components(x, d, box, label, 1, n_size_bins=32)
    if thin:
        assert want[1][0, 1] > 20 and want[1][0, 2] > 5
    with _device(x, label, 1) as c:
        _same(c.components(d, box, size_bins=32), want)
    with _device(x.astype(np.float64), label, 1) as c:
        _same(c.components(d, box, size_bins=32), want)


# ---- labels and masks

LABEL_N, LABEL_K, LABEL_BOX, LABEL_D = 6000, 3, (6.0, 6.0, 6.0), 0.3
MASKS = {"all": "all", "same": "same", "0-2": [(0, 2)]}


@pytest.fixture(scope="module")
def labelled():
    """9 frames of 6 000 beads, three labels, a tenth of the beads taking no part; the restatement of frame 0 under every mask and of
    all frames under "same".  The tests read them and change nothing."""
    rng = np.random.default_rng(6)
    x = rng.uniform(0, 6, size=(9, LABEL_N, 3)).astype(np.float32)
    label = np.where(rng.uniform(size=LABEL_N) < 0.1, -1, rng.integers(0, LABEL_K, size=LABEL_N))
    cand = cr.kdtree_candidates(LABEL_D, LABEL_BOX)
    first = {name: cr.components(x[:1], LABEL_D, LABEL_BOX, label, LABEL_K, links, 64, candidates=cand) for name, links in MASKS.items()}
    every = cr.components(x, LABEL_D, LABEL_BOX, label, LABEL_K, "all", 64, candidates=cand)
    return x, label, first, every


@pytest.mark.parametrize("mask", list(MASKS))
def test_labels_and_masks(labelled, mask):
    x, label, first, _ = labelled
    assert first["same"][1][0, 1] >= first["all"][1][0, 1] and first["0-2"][1][0, 1] > first["all"][1][0, 1]
    assert first["all"][1][0, 2] > 10
    with _device(x[:1], label, LABEL_K, MASKS[mask]) as c:
        _same(c.components(LABEL_D, LABEL_BOX), first[mask], mask)
        _same(c.components(LABEL_D, LABEL_BOX), cr.components_scipy(x[:1], LABEL_D, LABEL_BOX, label, LABEL_K, MASKS[mask], 64,
                                                                    candidates=cr.kdtree_candidates(LABEL_D, LABEL_BOX)), mask)


# ---- invariance

def test_invariance(labelled):
    x, label, _, every = labelled
    rows = lambda want, idx: tuple(w[idx] for w in want)      # noqa: E731
    full = None
    for mf in (1, 2, 0):
        with _device(x, label, LABEL_K, None, mf) as c:
            a = c.components(LABEL_D, LABEL_BOX)
            b = c.components(LABEL_D, LABEL_BOX)
            assert _bytes(a) == _bytes(b), mf      # from run to run
            full = full or _bytes(a)
            assert _bytes(a) == full, mf           # for every max_frames_per_launch
            _same(a, every, mf)
            _same(c.components(LABEL_D, LABEL_BOX, first_frame=2, n_frames=5), rows(every, slice(2, 7)), (mf, "2:5"))
            _same(c.components(LABEL_D, LABEL_BOX, first_frame=1, frame_stride=2), rows(every, slice(1, 9, 2)), (mf, "stride 2"))
            _same(c.components(LABEL_D, LABEL_BOX, first_frame=0, n_frames=3, frame_stride=4), rows(every, slice(0, 9, 4)), (mf, "stride 4"))
            bare = c.components(LABEL_D, LABEL_BOX, roots=False)
            assert bare.root is None and _bytes(bare)[1:] == full[1:]
    assert len({every[0][f].tobytes() for f in range(9)}) == 9      # the frames differ


# ---- the live feed

def test_live_feed_equals_the_host_feed(hip):
    s = g.System(hip, 300, 2)
    s.set_positions(np.random.default_rng(11).normal(size=(2, 300, 3)))
    with s, live.History(s, frames_per_block=4) as hist, live.History(s, replicas=[0]) as empty, cluster.Clusters(0) as fed, cluster.Clusters(0) as dev:
        _refused("GD_ESTATE", dev.set_history_from, empty, 0)      # no frame yet
        for k in range(6):
            s.run(5, 1e-4, 1.0, seed=30 + k, noise=g.NOISE_PHILOX)
            hist.record(quantize=True)
        frames = hist.fetch(1)
        assert frames.shape == (6, 300, 3)
        fed.set_history(frames)
        dev.set_history_from(hist, 1)
        assert dev.shape == fed.shape == (6, 300)
        label = np.arange(300) % 3 - 1
        for c in (fed, dev):
            c.set_labels(label, 2)
            c.set_links("same")
        a, b = dev.components(0.5, size_bins=16), fed.components(0.5, size_bins=16)
        assert _bytes(a) == _bytes(b) and (a.clusters > 1).all() and (a.largest > 1).all()
        _same(a, cr.components(frames, 0.5, None, label, 2, "same", 16))
        _refused("GD_EINVAL", dev.set_history_from, empty, 1)      # a replica that is not recorded
        assert _bytes(dev.components(0.5, size_bins=16)) == _bytes(a)      # a refused call leaves the handle as it was


# ---- the program gd_clusters end to end (HDF5 in, HDF5 out)

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5DUMP = "/opt/conda/bin/h5dump"
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


@pytest.fixture(scope="module")
def progs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_clusters"])
    return {k: os.path.join(HOST, k) for k in ("gd_h5tool", "gd_clusters")}


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


@needs_h5
def test_program_end_to_end(progs, tmp_path):
    import json
    rng = np.random.default_rng(17)
    F, N = 23, 40
    walk = np.cumsum(rng.normal(scale=0.2, size=(F, N, 3)), axis=0) + np.cumsum(rng.normal(scale=0.5, size=(1, N, 3)), axis=1)
    hist = (np.round(walk * 65536) / 65536).astype(np.float32)      # what a trajectory file stores
    a = _traj(progs, tmp_path / "traj_a.h5", hist)
    b = _traj(progs, tmp_path / "traj_b.h5", hist[::-1])
    out = tmp_path / "clusters.h5"

    def same_as_class(root, c, frames, want, roots):
        at = f"/clusters/interphase/{root}"
        assert _dataset(progs, tmp_path, out, f"{at}/frames").tolist() == frames
        summary = np.stack([want.selected, want.clusters, want.largest, want.sum_s2], axis=1)
        for name, w in (("summary", summary), ("histogram", want.histogram)) + ((("root", want.root),) if roots else ()):
            got = _dataset(progs, tmp_path, out, f"{at}/{name}")
            assert got.shape == w.shape and np.array_equal(got, w.astype(np.float64)), name
        assert (want.clusters > 1).any() and (want.largest > 1).any()

    # no metadata: one label of all beads; two samples in one run
    subprocess.run([progs["gd_clusters"], "--distance", "1.25", "--roots", str(out), str(a), str(b)], check=True, capture_output=True)
    for sample, frames in (("traj_a", hist), ("traj_b", hist[::-1])):
        with cluster.Clusters(0) as c:
            c.set_history(np.ascontiguousarray(frames))
            same_as_class(sample, c, list(range(F)), c.components(1.25), True)
    hdr = subprocess.check_output([H5DUMP, "-H", "-g", "/clusters/interphase/traj_a", str(out)], text=True)
    for name in ("distance", "links", "link_mask", "frame_stride", "size_bins"):
        assert f'ATTRIBUTE "{name}"' in hdr, name
    assert 'ATTRIBUTE "box"' not in hdr and "H5T_STD_U64LE" in hdr and "H5T_STD_I32LE" in hdr
    # with metadata: labels by particle type, a window of frames, a periodic box, a link list
    meta = tmp_path / "meta"
    meta.mkdir()
    types = (np.arange(N) % 3).astype("i1")
    (meta / "config.json").write_text(json.dumps({"made": "for this test"}))
    np.zeros((N, 2), "<f4").tofile(meta / "ab.f32")
    types.tofile(meta / "types.i8")
    np.zeros((0, 2), "<i4").tofile(meta / "nucleolus_bonds.i32")
    (meta / "chromosomes.tsv").write_text("chrA 0 15 3 5\nchrB 15 36 20 22\n")
    (meta / "nucleoli.tsv").write_text("")
    c_path = tmp_path / "traj_c.h5"
    subprocess.check_call([progs["gd_h5tool"], "make-metadata", str(c_path), str(meta)])
    _traj(progs, c_path, hist)
    subprocess.run([progs["gd_clusters"], "--name", "interphase", "--groups", "types", "--links", "0-0,2-1", "--frames=3:6", "--frame-stride", "3",
                    "--box", "6,7,8", "--size-bins=4", "--distance=1.5", str(out), str(c_path)], check=True, capture_output=True)
    with cluster.Clusters(0) as c:
        c.set_history(hist)
        c.set_labels(types, 3)
        c.set_links([(0, 0), (1, 2)])
        same_as_class("traj_c", c, [3, 6, 9, 12, 15, 18], c.components(1.5, (6.0, 7.0, 8.0), size_bins=4, first_frame=3, n_frames=6, frame_stride=3), False)
    hdr = subprocess.check_output([H5DUMP, "-H", "-g", "/clusters/interphase/traj_c", str(out)], text=True)
    assert 'ATTRIBUTE "box"' in hdr and 'DATASET "root"' not in hdr
    assert _dataset(progs, tmp_path, out, "/clusters/interphase/traj_a/frames").tolist() == list(range(F))      # earlier samples stay
    r = subprocess.run([progs["gd_clusters"], "--distance", "1", "--links", "0-1", str(out), str(a)], capture_output=True, text=True)
    assert r.returncode == 1 and "gd_clusters: error:" in r.stderr and "the beads have 1 labels" in r.stderr
    r = subprocess.run([progs["gd_clusters"], "--distance", "1", "--frames", "20:4", str(out), str(a)], capture_output=True, text=True)
    assert r.returncode == 1 and "--frames 20:4" in r.stderr

"""The inputs of test_flow_edges_gpu.py, each from a fixed seed, with the branch of csrc/gdyn_flow.hip it is there for (a helper,
not collected).  test_flow_host.py asserts on the CPU, through flow_restatement.cell_grid, that every input reaches its branch;
the GPU tests assert the same before they call the device."""
import numpy as np

import flow_restatement as fr

# ---- launch shape: the caps of stream_blocks and the rule of frames_per_launch (csrc/gdyn_flow.hip)
STREAM_BLOCK, STREAM_MAX_BLOCKS = 256, 256 * 64
BIG_F, BIG_N, BIG_W, BIG_DELAY, BIG_R = 23, 62178, 5, 3, 0.6
BIG_FRAMES = (0, 16, 17, 22)


def auto_batch(N, F, lanes_per_frame):
    """frames_per_launch with max_frames_per_launch = 0."""
    return min((1 << 20) // max(lanes_per_frame, 1) + 1, max(1, (1 << 30) // N), F)


def big_history():
    """A random walk of BIG_N beads inside a sphere of radius 8 (the 62 178-bead model's density), BIG_F frames, float32 on a
    2^-16 lattice."""
    rng = np.random.default_rng(23)
    u = rng.normal(size=(BIG_N, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x = u * 8.0 * rng.uniform(size=(BIG_N, 1)) ** (1 / 3)
    out = np.empty((BIG_F, BIG_N, 3))
    for f in range(BIG_F):
        x = x + rng.normal(scale=0.05, size=x.shape)
        nr = np.linalg.norm(x, axis=1)
        x[nr > 8.0] *= (8.0 / nr[nr > 8.0])[:, None]
        out[f] = x
    return (np.round(out * 65536) / 65536).astype(np.float32)


# ---- windows
WINDOW_SHAPES = [(1, 130), (2, 130), (3, 130), (5, 130), (3, 1)]


def window_history(F, N, dtype):
    """Coordinates offset by +-1e3 with small displacements from frame to frame, so the velocity's mean subtraction matters."""
    rng = np.random.default_rng(1000 * F + N)
    x0 = rng.choice([-1e3, 1e3], size=(N, 3)) + rng.normal(scale=2.0, size=(N, 3))
    u = rng.normal(scale=0.05, size=(N, 3))
    x = np.stack([x0 + f * u + rng.normal(scale=0.02, size=(N, 3)) for f in range(F)])
    return x.astype(dtype)


def window_smoothings(F):
    return sorted({1, 2, F, 2 * F - 1, 2 * F, 3 * F + 1, 40})      # from 2 F on the reflection repeats (W // 2 > F - 1)


def window_delays(F):
    return sorted({0, 1, 2, F - 1, F, F + 3, 50})                  # F: clipped at either end; F + 3, 50: at both ends of one frame


# ---- grid kinds: a blob of 300 beads (normal, sigma 0.8), 4 frames, float64; the outliers stay in place (velocity 0)
KIND_R, KIND_F, KIND_DELAY = 0.35, 4, 2
KINDS = ["blob", "outlier_1e3", "fallback_1e8", "outlier_1e8", "coincident", "line", "plane", "uniform"]


def _moving(rng, x0, frames=KIND_F):
    u = rng.normal(scale=0.05, size=x0.shape)
    return np.stack([x0 + f * u + rng.normal(scale=0.01, size=x0.shape) for f in range(frames)])


def _blob(rng, n=300):
    return rng.normal(scale=0.8, size=(n, 3))


def kind_history(kind):
    """(history (4, N, 3) float64, r) of one grid kind."""
    rng = np.random.default_rng(KINDS.index(kind) + 77)
    r = KIND_R
    if kind == "blob":
        h = _moving(rng, _blob(rng))
    elif kind == "outlier_1e3":            # one far-away bead: the side grows past r
        h = _moving(rng, _blob(rng))
        h[:, 0] = [1e3, 0.0, 0.0]
    elif kind == "fallback_1e8":           # no side fits: the cbrt fallback, cells == cap
        h = _moving(rng, _blob(rng))
        h[:, 0] = [1e8, 1e8, 1e8]
        h[:, 1] = [-1e8, -1e8, -1e8]
    elif kind == "outlier_1e8":            # dozens of growths, a row of cells along x
        h = _moving(rng, _blob(rng))
        h[:, 0] = [1e8, 0.0, 0.0]
    elif kind == "coincident":             # every extent 0; frame 0 at the origin
        c = _moving(rng, np.zeros((1, 3)))
        c[0] = 0.0
        h = np.repeat(c, 50, axis=1)
    elif kind == "line":                   # y = z = 0: dims (n, 1, 1); the beads slide along the line
        x0 = np.zeros((200, 3))
        x0[:, 0] = rng.uniform(-3, 3, size=200)
        h = _moving(rng, x0)
        h[:, :, 1:] = 0.0
    elif kind == "plane":                  # z = 0: dims (n, m, 1)
        x0 = np.zeros((200, 3))
        x0[:, :2] = rng.uniform(-2, 2, size=(200, 2))
        h = _moving(rng, x0)
        h[:, :, 2] = 0.0
    elif kind == "uniform":                # the cap is 4 N and the side ends at 9 r
        r = 0.1
        h = _moving(rng, rng.uniform(-8, 8, size=(2000, 3)))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(h), r


def boundary_pair(x, a, r, sign):
    """The last point inside and the first outside the ball of bead x, going from x along axis a in direction sign: two
    neighbouring float64, found with fr.inside from fl(x_a + sign r)."""
    def at(c):
        q = np.array(x, np.float64)
        q[a] = c
        return q
    c = float(x[a]) + sign * r
    while not fr.inside(x, at(c), r):
        c = float(np.nextafter(c, x[a]))
    while fr.inside(x, at(np.nextafter(c, sign * np.inf)), r):
        c = float(np.nextafter(c, sign * np.inf))
    return at(c), at(np.nextafter(c, sign * np.inf))


def kind_points(kind, hist, r):
    """(points, outside, ties): a mesh over the blob, then
    outside: six points beyond the box of every frame by more than r, one per side of each axis, and one ten extents away;
    ties:    for frame 0's extreme beads along +x and -x, the last float64 inside and the first outside their ball along that
             axis; where a bead has a zero coordinate (the outliers, the origin, the line, the plane) also the points at
             exactly r and at the next float64 after r along that axis, for which dx = r holds without rounding.
    outside and ties are index arrays into points; ties is (T, 2): (inside, outside) pairs."""
    half = 8.0 if kind == "uniform" else 2.0
    step = 2.0 if kind == "uniform" else 0.5
    ax = np.arange(-half, half + step / 2, step)
    pts = [np.moveaxis(np.meshgrid(ax, ax, ax), 0, -1).reshape(-1, 3)]
    if kind == "uniform":      # (a mesh of 2.0 meets next to nothing at r = 0.1) points near beads of frame 1
        pts.append(hist[1, :150] + np.random.default_rng(5).uniform(-0.06, 0.06, size=(150, 3)))
    lo, hi = hist.min(axis=(0, 1)), hist.max(axis=(0, 1))
    mid = 0.5 * (lo + hi)
    out = []
    for a in range(3):
        for side in (lo[a] - 1.5 * r - 1e-3 * (hi[a] - lo[a]), hi[a] + 1.5 * r + 1e-3 * (hi[a] - lo[a])):
            q = mid.copy()
            q[a] = side
            out.append(q)
    out.append(mid + 10.0 * (hi - lo + 1.0))
    pairs = []
    f0 = hist[0]
    for sign, b in ((1.0, int(np.argmax(f0[:, 0]))), (-1.0, int(np.argmin(f0[:, 0])))):
        pairs.append(boundary_pair(f0[b], 0, r, sign))
    zero = [(b, a) for b in (0, 1, len(f0) - 1) for a in range(3) if f0[b, a] == 0.0]
    for b, a in zero[:6]:
        for sign in (1.0, -1.0):
            q_in, q_out = f0[b].copy(), f0[b].copy()
            q_in[a] = sign * r
            q_out[a] = sign * np.nextafter(r, np.inf)
            pairs.append((q_in, q_out))
    n0 = sum(len(p) for p in pts)
    outside = np.arange(n0, n0 + len(out))
    ties = n0 + len(out) + np.arange(2 * len(pairs)).reshape(-1, 2)
    pts += [np.array(out), np.array([q for pair in pairs for q in pair])]
    return np.concatenate(pts), outside, ties


def assert_kind_branch(kind, hist, r):
    """The branch of k_flow_bounds each kind is named after, for every frame of its history."""
    for frame in hist:
        g = fr.cell_grid(frame, r)
        if kind == "blob":
            assert g.fits and g.growths == 3 and g.side < r, g
        elif kind == "outlier_1e3":
            assert g.fits and g.growths == 12 and g.side > r and g.dims[0] > 300 and g.dims[1] > 1 and g.dims[2] > 1, g
        elif kind == "fallback_1e8":
            assert not g.fits and g.growths == 64 and g.dims == (16, 16, 16) and g.cells == g.cap == 4096, g
        elif kind == "outlier_1e8":
            assert g.fits and g.growths >= 50 and g.dims[0] > 2048 and g.dims[1:] == (1, 1), g
        elif kind == "coincident":
            assert g.fits and g.growths == 0 and g.dims == (1, 1, 1), g
        elif kind == "line":
            assert g.fits and g.dims[0] > 1 and g.dims[1:] == (1, 1), g
        elif kind == "plane":
            assert g.fits and g.dims[0] > 1 and g.dims[1] > 1 and g.dims[2] == 1, g
        elif kind == "uniform":
            assert g.fits and g.growths == 13 and g.cap == 8000 and 9.0 * r < g.side < 9.2 * r, g


def assert_points(hist, r, pts, outside, ties):
    """outside: beyond every frame's box by more than r on its axis; ties: inside / outside their bead in frame 0."""
    for f in range(len(hist)):
        lo, hi = hist[f].min(axis=0), hist[f].max(axis=0)
        for k, i in enumerate(outside[:6]):
            a = k // 2
            assert pts[i, a] < lo[a] - r if k % 2 == 0 else pts[i, a] > hi[a] + r, (f, k)
        assert not fr.inside(hist[f][:, None], pts[outside][None], r).any()
    cov0 = fr.inside(hist[0][:, None], pts[ties.ravel()][None], r).sum(axis=0).reshape(-1, 2)
    assert (cov0[:, 0] > cov0[:, 1]).all(), cov0      # the step across the boundary loses a bead
    return cov0


# ---- ties at density: 600 beads on the 1/8 lattice in [0, 4)^3, r = 5/8, cell side 5/16
LATTICE_R, LATTICE_N = 0.625, 600


def lattice_history():
    """(3, 600, 3): frame 1 is the lattice (distinct sites, the origin among them), frames 0 and 2 lie off it on either side."""
    rng = np.random.default_rng(8)
    sites = np.concatenate([[0], 1 + rng.choice(32 ** 3 - 1, size=LATTICE_N - 1, replace=False)])
    x = np.stack([sites // 1024, (sites // 32) % 32, sites % 32], axis=1) / 8.0
    u = rng.normal(scale=0.05, size=x.shape)
    return np.stack([x - u, x, x + u + rng.normal(scale=0.01, size=x.shape)])


def lattice_census(x, r):
    """(pairs at exactly r, pairs strictly inside) of one frame, i < j, in exact arithmetic (the lattice is dyadic)."""
    k = np.round(x * 8).astype(np.int64)
    assert np.array_equal(k / 8.0, x)
    d2 = ((k[:, None] - k[None]) ** 2).sum(axis=2)[np.triu_indices(len(k), 1)]
    r2 = int(round(r * 8)) ** 2
    return int((d2 == r2).sum()), int((d2 < r2).sum())


# ---- mixed batch: one history whose frames have different grids
MIXED_KINDS = ["blob", "outlier_1e3", "fallback_1e8", "coincident", "line", "blob"]


def mixed_history():
    """(6, 300, 3): the same 300 beads as a blob, with an outlier, with two at +-1e8, coincident, on a line, and a blob again."""
    rng = np.random.default_rng(61)
    h = np.stack([_blob(rng) for _ in MIXED_KINDS])
    h[1, 0] = [1e3, 0.0, 0.0]
    h[2, 0] = [1e8, 1e8, 1e8]
    h[2, 1] = [-1e8, -1e8, -1e8]
    h[3] = h[3, 0]
    h[4, :, 1:] = 0.0
    return h


def assert_mixed_branches(hist, r):
    for kind, frame in zip(MIXED_KINDS, hist):
        assert_kind_branch(kind, frame[None], r)
    grids = [fr.cell_grid(frame, r) for frame in hist]
    assert len({g.dims for g in grids}) >= 5 and len({g.cells for g in grids}) >= 5      # no two neighbouring frames share a grid

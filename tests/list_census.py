"""A census of the Verlet lists: what gd_context.list_entries / near_entries count and what gd_search_pairs serves from the
resident list, restated in plain numpy + scipy.spatial.cKDTree in fp64 from one replica's positions.  No GPU, no libgdyn.

The device forms r^2 in fp32, so a pair whose distance lies within a few ulps of a radius may fall either side of it;
clear_of_boundaries() moves such pairs out of the way, after which the counts of a correct build EQUAL the census."""
import numpy as np
from scipy.spatial import cKDTree

PUSH = 1e-3                                        # clear_of_boundaries: how far a bead is moved
PUSH_DIR = np.array([2.0, -3.0, 6.0]) / 7.0        # ... and along which (fixed, unit) direction


def f32(v):
    """`v` rounded to fp32, as a float."""
    return float(np.float32(v))


def near_radius(rv, cutoff, bead_scale, skin, near_fraction, single_class=False):
    """Near-class radius of a build with list radius `rv`, the rule of the host (fp32, csrc/gdyn_capi.hip, enqueue_build):
    cutb = rv - cutoff * skin, the (look-ahead) cutoff the list radius was derived from; rn = cutb + near_fraction * (rv - cutb);
    rn = rv for single-class lists and where cutb is not inside (0, rv).  `bead_scale` is the scale the radius was derived with
    (list radius = cutoff * (bead_scale + skin), gdyn.h: the largest of the handle's replicas): cutb has to equal cutoff *
    bead_scale to fp32 rounding, which is asserted -- a handle whose radius follows another scale fails here."""
    rv32, cut32 = np.float32(rv), np.float32(cutoff)
    cutb = rv32 - np.float32(float(cut32) * float(skin))           # (float cutoff x double skin, rounded to float)
    assert abs(float(cutb) - float(cut32) * bead_scale) <= 4 * float(np.spacing(rv32)), (float(cutb), float(cut32) * bead_scale)
    if single_class or not (0 < cutb < rv32):
        return float(rv32)
    return float(cutb + np.float32(near_fraction) * (rv32 - cutb))


def displacement(x, i, j, box):
    """x[i] - x[j] in fp64, its minimum image where `box` (three periods) is given."""
    d = x[i] - x[j]
    if box is not None:
        L = np.asarray(box, dtype=np.float64)
        d = d - L * np.rint(d / L)
    return d


def pairs_within(x, box, r):
    """(pairs i < j, distances) of all pairs with d <= r + a hair (the caller filters): cKDTree on the positions, wrapped into the
    box where one is given (the tree's periodic metric is the minimum image per axis), distances recomputed in fp64 from the
    unwrapped input."""
    x = np.asarray(x, dtype=np.float64)
    if box is None:
        tree = cKDTree(x)
    else:
        L = np.asarray(box, dtype=np.float64)
        xw = x - L * np.floor(x / L)
        xw[xw >= L] = 0.0                          # (x = -tiny wraps to L in floating point)
        tree = cKDTree(xw, boxsize=L)
    p = tree.query_pairs(r * (1 + 1e-9) + 1e-12, output_type="ndarray")
    p = np.sort(p.reshape(-1, 2), axis=1)
    d = np.linalg.norm(displacement(x, p[:, 0], p[:, 1], box), axis=1)
    return p, d


class Census:
    """Per-bead neighbour counts within rv (n_all) and rn (n_near), and what the handle's counters are defined as."""

    def __init__(self, x, box, rv, rn):
        self.n, self.rv, self.rn = len(x), float(rv), float(rn)
        p, d = pairs_within(x, box, rv)
        keep = d < rv
        self._p, self._d = p[keep], d[keep]
        self.n_all = np.bincount(self._p.ravel(), minlength=self.n)
        self.n_near = np.bincount(self._p[self._d < rn].ravel(), minlength=self.n)
        self.n_far = self.n_all - self.n_near
        # L: directed entries stored (gdyn.h, list_entries)
        self.list_entries = int(self.n_all.sum())
        # the near class, in the fours k_step walks it in (gdyn.h, near_entries); single-class lists: rn = rv, so all of them
        self.near_entries = int((4 * ((self.n_near + 3) // 4)).sum())

    def pairs(self, r):
        """The set of pairs i < j with d < r (r <= rv)."""
        assert r <= self.rv
        return {(int(i), int(j)) for i, j in self._p[self._d < r]}

    def pair_keys(self, r):
        """The same as sorted keys i * n + j (large sets compare faster as arrays; see pair_keys() below)."""
        assert r <= self.rv
        return pair_keys(self._p[self._d < r], self.n)

    def chunks(self, two_class=True):
        """Chunks of 8 entries per bead: each class padded to whole chunks (tiled lists), or the whole list (generic lists)."""
        if two_class:
            return (self.n_near + 7) // 8 + (self.n_far + 7) // 8
        return (self.n_all + 7) // 8


def census(x, box, rv, rn):
    return Census(np.asarray(x, dtype=np.float64), box, rv, rn)


def pair_keys(pairs, n):
    """(k, 2) pairs in any order and orientation as sorted keys min * n + max."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.sort(p.min(axis=1) * n + p.max(axis=1))


def boundary_window(x, box):
    """Half-width of the window around a radius inside which the device's fp32 r^2 may fall either side of it: 16 fp32 ulps of the
    largest coordinate magnitude of the input (open boxes), or of the box period (periodic boxes).  Derived, not measured.  Both
    sides see the same fp32 coordinates, so only the arithmetic on them differs.  Open boxes: a coordinate difference is rounded to
    at most half an ulp of its larger operand, three of them are squared and summed (relative 2^-23 each) and compared with a
    rounded rv^2 -- about two ulps of the largest coordinate in d.  Periodic boxes: a coordinate is wrapped into [0, L) by one fused
    multiply-add (half an ulp of L) with the fp32 period, which is off by up to half an ulp of L per period the bead lies outside
    the box -- up to 2 ulps of L per bead within 3 periods, 4 per difference, under 8 in d over three axes (the generic path's
    x_i - x_j - L rint(.) stays below that).  16 leaves a factor of two and more; it holds for beads within 4 periods of the box,
    which is asserted."""
    m = float(np.abs(x).max())
    if box is not None:
        assert np.all(np.abs(x).max(axis=0) <= 4.5 * np.asarray(box)), (np.abs(x).max(axis=0), box)
        m = float(np.max(box))
    return 16.0 * float(np.spacing(np.float32(m)))


def boundary_pairs(x, box, radii, w):
    """Pairs whose distance lies within w of one of the radii."""
    p, d = pairs_within(x, box, max(radii) + w)
    hit = np.zeros(len(d), dtype=bool)
    for r in radii:
        hit |= np.abs(d - r) < w
    return p[hit]


def clear_of_boundaries(x, box, radii, w=None, max_moved=0.01):
    """`x` (N, 3) with one bead of every pair that lies within `w` of a radius moved by PUSH along PUSH_DIR, repeated until no pair lies
    in a window; fp32-exact like the input the device keeps.  Deterministic.  Asserts that it converges within 20 passes and that it
    moved fewer than `max_moved` (1 %) of the beads: the input stays the state it was.  Returns (x, number of beads moved)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if w is None:
        w = boundary_window(x, box)
    moved = np.zeros(len(x), dtype=bool)
    for _ in range(20):
        p = boundary_pairs(x, box, radii, w)
        if len(p) == 0:
            break
        j = np.unique(p[:, 1])                     # the higher index of every pair, once
        x[j] += PUSH * PUSH_DIR
        x = x.astype(np.float32).astype(np.float64)
        moved[j] = True
    else:
        assert len(boundary_pairs(x, box, radii, w)) == 0, "clear_of_boundaries: no convergence within 20 passes"
    assert moved.sum() < max_moved * len(x), ("clear_of_boundaries moved too many beads", int(moved.sum()), len(x))
    return x, int(moved.sum())

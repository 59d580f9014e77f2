"""numpy restatement of include/gdyn_flow.h (a helper of test_flow_host.py and test_flow_edges_gpu.py; not collected), written
from the header, DESIGN.md 7a and the file header of csrc/gdyn_flow.hip; no device code.

    smooth, velocity      the time-axis filter and the windowed least-squares slope, accumulated in np.longdouble
    inside                the pair test, in float64 exactly as the device associates it: membership is bit-exact
    particle, grid        brute force over all beads of a frame, velocities summed in np.longdouble
    bound_*               what |device - restatement| may be, derived from the kernels' arithmetic in each docstring
    cell_grid             a mirror of k_flow_bounds' rule, used only to assert which branch an input reaches

EPS is the unit roundoff of fp64 (2^-53), EPSL that of np.longdouble (2^-64 where it is the x87 format).  The bounds are to
first order in EPS and carry EPSL beside EPS for the restatement's own rounding, so they also hold where np.longdouble is
float64."""
import collections

import numpy as np

EPS = 2.0 ** -53
EPSL = float(np.finfo(np.longdouble).eps) / 2
EPS32 = 2.0 ** -24
LD = np.longdouble


# ---- smoothing

def weights(W):
    """utils.gaussian_smooth's kernel: exp(-linspace(-3, 3, W)^2 / 2) normalised, float64.  The normalising sum is taken left
    to right (np.cumsum) as gd_flow_velocities takes it, so the two sums round alike wherever the two exp agree."""
    e = np.exp(-np.linspace(-3.0, 3.0, W) ** 2 / 2)
    return e / np.cumsum(e)[-1]


def smooth(x, W):
    """x (F, ...) float64 smoothed along axis 0 with window W (0: none): numpy's "reflect" padding (repeated when the window is
    longer than the history; a one-frame history pads with its frame) by lpad = W // 2, rpad = W - lpad - 1, then the "valid"
    convolution out[t] = sum_j padded[t + j] kernel[W - 1 - j], accumulated in np.longdouble; float64 out."""
    x = np.asarray(x, np.float64)
    if W == 0:
        return x.copy()
    F = x.shape[0]
    lpad = W // 2
    padded = np.pad(x, [(lpad, W - lpad - 1)] + [(0, 0)] * (x.ndim - 1), mode="reflect")
    w = weights(W).astype(LD)
    acc = np.zeros(x.shape, LD)
    for j in range(W):
        acc += w[W - 1 - j] * padded[j:j + F].astype(LD)
    return acc.astype(np.float64)


def bound_smooth(x, W):
    """|k_flow_smooth - smooth| per element, with X = max over the frames of |x| of that element (the reflection may reach any
    frame):  (W + 4) EPS X.

    The device computes acc = sum_k w'_k x_k left to right in fp64, with or without contraction.  Either way a term passes
    through at most W roundings (contracted: one per fma; not contracted: its product's and W - 1 additions'), so
    |acc - sum w'_k x_k| <= W EPS sum |w'_k x_k| <= W EPS X, as the weights are positive and sum to 1.  The host's weights
    w'_k = fl(e'_k / S') differ from numpy's w_k = fl(e_k / S) by the two roundings of the divisions (2 EPS X in the sum) and
    where the C library's exp is an ulp (2 EPS relative) off numpy's: e'_k = e_k (1 + a_k), |a_k| <= 2 EPS, S' = S (1 + abar)
    with abar the w-weighted mean of the a_k, so the sum changes by sum w_k (a_k - abar) x_k, at most X times the mean absolute
    deviation of a, which is at most 2 EPS.  W + 2 + 2.  Not counted: a differing exp also changes how the partial sums of S'
    round (at most (W - 1) EPS each way); with the sums in the same order that is the first term to add should the figure be
    exceeded.  The restatement's own rounding is (W + 1) EPSL X."""
    X = np.abs(np.asarray(x, np.float64)).max(axis=0, keepdims=True)
    if W == 0:
        return np.zeros_like(X)
    return ((W + 4) * EPS + (W + 1) * EPSL) * X


# ---- velocity

def window(t, F, delay):
    """estimate_velocity's window of frame t: (first frame, length)."""
    w = delay + 1
    back = w // 2
    forw = w - back
    if t - back < 0:
        back = t
    if t + forw > F:
        forw = F - t
    return t - back, back + forw


def velocity(p, delay):
    """The least-squares slope of every element of p (F, ...) over each frame's window, sum c_k (p_k - pbar) / sum c_k^2 with
    c_k = k - (w - 1) / 2, in np.longdouble; float64 out.  A one-frame window gives NaN (0 * (1 / 0) in the reference)."""
    p = np.asarray(p, np.float64)
    F = p.shape[0]
    out = np.full(p.shape, np.nan)
    for t in range(F):
        first, w = window(t, F, delay)
        if w < 2:
            continue
        c = (np.arange(w) - LD(w - 1) / 2).astype(LD)
        win = p[first:first + w].astype(LD)
        win = win - win.sum(axis=0) / w
        out[t] = (np.tensordot(c, win, axes=(0, 0)) / (c * c).sum()).astype(np.float64)
    return out


def bound_velocity(p, delay):
    """|k_flow_velocity - velocity| per element, with P = max |p| over the frame's window, w its length and c_k as above:

        (2 w + 6) EPS P sum |c_k| / sum c_k^2.

    On the device tmean = (w - 1) / 2, the c_k (half-integers) and ssq = sum c_k^2 are exact.  pmean' carries up to w EPS P of
    rounding, but d_k = p_k - pmean' enters as sum c_k d_k and sum c_k = 0 exactly, so an error of the mean drops out whole.
    What remains: the rounding of each d_k (EPS |d_k|, |d_k| <= 2 P): 2 EPS P sum |c_k|; the accumulation, in which a term
    passes through at most w roundings with or without contraction: 2 w EPS P sum |c_k|; 1 / ssq and the last product, two
    roundings of a value of at most 2 P sum |c_k| / ssq: 4.  The restatement's own rounding has the same form in EPSL.
    Where the window has one frame both are NaN and the bound is 0."""
    p = np.asarray(p, np.float64)
    F = p.shape[0]
    out = np.zeros(p.shape)
    for t in range(F):
        first, w = window(t, F, delay)
        if w < 2:
            continue
        c = np.arange(w) - (w - 1) / 2
        P = np.abs(p[first:first + w]).max(axis=0)
        out[t] = (2 * w + 6) * (EPS + EPSL) * P * np.abs(c).sum() / (c * c).sum()
    return out


# ---- flows

def inside(x, q, r):
    """Membership of beads x (..., 3) in the ball of radius r around q (..., 3), float64, every operation rounded on its own in
    the device's association (dx*dx + dy*dy) + dz*dz <= r*r.  numpy neither fuses nor reassociates these, so the result is the
    device's bit for bit and coverage is compared with ==."""
    x = np.asarray(x, np.float64)
    q = np.asarray(q, np.float64)
    dx = x[..., 0] - q[..., 0]
    dy = x[..., 1] - q[..., 1]
    dz = x[..., 2] - q[..., 2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    s = xx + yy
    s = s + zz
    return s <= np.float64(r) * np.float64(r)


Flows = collections.namedtuple("Flows", "flows coverage mean sabs")
Flows.__doc__ = """flows (F, Q, 3) float32 and coverage (F, Q) int32 as the device returns them; mean (F, Q, 3) np.longdouble, the
quotient before its rounding to float32; sabs (F, Q, 3) np.longdouble, the sum of |v| over the members (for bound_flow)."""


def _gather(pos, vel, r, queries, empty_ok):
    F = pos.shape[0]
    Q = queries.shape[1]
    mean = np.zeros((F, Q, 3), LD)
    sabs = np.zeros((F, Q, 3), LD)
    cov = np.zeros((F, Q), np.int32)
    for f in range(F):
        v = vel[f].astype(LD)
        for k in range(Q):
            m = inside(pos[f], queries[f, k], r)
            n = int(m.sum())
            cov[f, k] = n
            if n:
                mean[f, k] = v[m].sum(axis=0) / n
                sabs[f, k] = np.abs(v[m]).sum(axis=0)
            elif not empty_ok:
                raise AssertionError("a bead is within any r of itself")
    return Flows(mean.astype(np.float32), cov, mean, sabs)


def particle(pos, vel, r):
    """gd_flow_particle by brute force: for every bead of every frame, the mean velocity of the beads within r (itself and
    coincident beads included), summed in np.longdouble, divided by their number, rounded to float32."""
    pos = np.asarray(pos, np.float64)
    return _gather(pos, np.asarray(vel, np.float64), r, pos, False)


def grid(pos, vel, r, points):
    """gd_flow_grid by brute force: the same mean around each of points (G, 3), divided by max(n, 1), and n as coverage."""
    pos = np.asarray(pos, np.float64)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    return _gather(pos, np.asarray(vel, np.float64), r, np.broadcast_to(pts, (pos.shape[0],) + pts.shape), True)


def bound_flow(want):
    """|device float32 - want.mean| per element, n the number of members:

        2^-24 |mean| + n EPS (sum of |v| over the members) / n.

    The device sums the n velocities in fp64 in its sorted order: any order of n terms is within (n - 1) EPS sum |v| of the
    sum; the division adds EPS |mean| <= EPS sum |v| / n; the cast to float32 adds half a float32 ulp, 2^-24 |mean|.  The
    comparison is with the quotient before its own rounding to float32, not with want.flows: two values an fp64 rounding
    apart may round to neighbouring float32, a whole ulp (up to 2^-23 |mean|) from each other, which no bound of this form
    admits.  The restatement's own sum has the same form in EPSL.  Where the velocities are NaN so is the bound."""
    n = np.maximum(want.coverage, 1).astype(np.float64)[..., None]
    return (EPS32 * np.abs(want.mean) + n * (EPS + EPSL) * want.sabs / n).astype(np.float64)


# ---- the cell grid of a frame (branch assertions only, never expected results)

CellGrid = collections.namedtuple("CellGrid", "growths fits side dims cells cap")


def cell_grid(frame, r):
    """k_flow_bounds' rule for one frame (N, 3): cap = max(4 N, 4096); side r / 2 grown by 1.25 until the cell count
    prod(floor(extent / side) + 1) fits the cap, at most 64 sides tried; then floor(cbrt(cap)) - 1 cells along the longest
    extent.  growths: how often the side grew (64: none fitted)."""
    frame = np.asarray(frame, np.float64)
    cap = max(4 * len(frame), 4096)
    ext = [float(e) for e in frame.max(axis=0) - frame.min(axis=0)]
    h = 0.5 * float(r)
    fits, growths, inv_h = False, 0, 0.0
    for it in range(64):
        inv_h = 1.0 / h
        cells = 1.0
        for e in ext:
            cells *= np.floor(e * inv_h) + 1.0
        growths = it
        if cells <= cap:
            fits = True
            break
        h *= 1.25
    if not fits:
        growths = 64
        inv_h = float(np.floor(np.cbrt(float(cap))) - 1.0) / max(ext)
    dims = tuple(int(np.floor(e * inv_h) + 1.0) for e in ext)
    return CellGrid(growths, fits, 1.0 / inv_h, dims, dims[0] * dims[1] * dims[2], cap)


def reflect_index(i, F):
    """csrc/gdyn_flow.hip's reflect_index in Python (test_flow_host.py holds it to np.pad)."""
    if F == 1:
        return 0
    P = 2 * (F - 1)
    j = i % P
    return j if j < F else P - j

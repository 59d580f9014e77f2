"""numpy restatement of include/gdyn_sq.h (a helper of test_sq_host.py, test_sq_gpu.py and tools/bench_sq.py; not collected).

The phase of a bead and a vector is computed in float64 by the header's rounded operations,

    phi = ((qx * x) + (qy * y)) + qz * z          on the widened coordinates (numpy neither contracts nor reassociates these),

so it is the device's phi bit for bit and the argument carries no error of its own.  cos and sin of it are then taken in
np.longdouble and summed in np.longdouble: with 63 bits of mantissa or more that is the exact sum of the true cos and sin as far
as a float64 comparison can tell.  Where np.longdouble is no wider than float64 the fallback is math.fsum over math.cos / math.sin
(correctly summed, the terms within an ulp), and T grows by 1.

bound(n) is what the device may differ by for a label of n beads: every term has |.| <= 1, so an ulp is at most 2^-53; a term is
off by at most T of them, a chunk's serial sum of GD_SQ_CHUNK_BEADS terms adds at most GD_SQ_CHUNK_BEADS - 1 roundings of partial
sums no larger than n, the serial sum of the ceil(n / GD_SQ_CHUNK_BEADS) chunk partials as many again:

    bound(n) = n (T + GD_SQ_CHUNK_BEADS - 1 + ceil(n / GD_SQ_CHUNK_BEADS)) 2^-53.

T is the ulp bound of the device library's fp64 sin and cos.  The library's documentation is not part of the ROCm installation this
was written against (it ships ocml as bitcode only), so T = 4 here: the OpenCL bound for double-precision sin and cos, which the
library is written to.  The GPU tests print the largest observed error / bound.

collective() restates gd_sq_collective with the header's rounded float64 operations in a Python loop over the origins: fed the
device's amplitudes it must give the device's sums byte for byte."""
import math

import numpy as np

EPS = 2.0 ** -53
CHUNK = 256                 # GD_SQ_CHUNK_BEADS
LONG = np.finfo(np.longdouble).nmant >= 63
T_ULP = 4 if LONG else 5


def phase(q, x):
    """phi (..., n, Q) float64 of the coordinates x (..., n, 3) (widened) and the vectors q (Q, 3), by the header's operations."""
    q = np.asarray(q, dtype=np.float64)
    x = np.asarray(x).astype(np.float64)[..., None, :]
    return ((q[:, 0] * x[..., 0]) + (q[:, 1] * x[..., 1])) + q[:, 2] * x[..., 2]


def _sums(phi):
    """(sum of cos, sum of sin) over axis -2 of phi (..., n, Q), as float-like arrays (..., Q) that hold the sums to well below an ulp."""
    if LONG:
        wide = phi.astype(np.longdouble)
        return np.cos(wide).sum(axis=-2), np.sin(wide).sum(axis=-2)
    flat = np.moveaxis(phi, -2, -1).reshape(-1, phi.shape[-2])
    shape = phi.shape[:-2] + phi.shape[-1:]
    c = np.array([math.fsum(math.cos(v) for v in row) for row in flat]).reshape(shape)
    s = np.array([math.fsum(math.sin(v) for v in row) for row in flat]).reshape(shape)
    return c, s


def _members(labels, n_beads, n_labels):
    """the beads of every label, ascending; labels None: one label of all beads"""
    if labels is None:
        return [np.arange(n_beads)]
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == a) for a in range(n_labels)]


def amplitudes(x, q, labels=None, n_labels=1, first_frame=0, n_frames=None):
    """C, S (n_frames, K, Q) of gd_sq_amplitudes."""
    F, N, _ = x.shape
    n_frames = F - first_frame if n_frames is None else n_frames
    w = x[first_frame:first_frame + n_frames]
    members = _members(labels, N, n_labels)
    c, s = (np.zeros((n_frames, len(members), len(q)), np.longdouble if LONG else np.float64) for _ in range(2))
    for a, beads in enumerate(members):
        if len(beads):
            c[:, a], s[:, a] = _sums(phase(q, w[:, beads]))
    return c, s


def origins(n_frames, lag, stride):
    """the origins of a lag, relative to the first frame of the window"""
    return list(range(0, n_frames - lag, stride))


def self_part(x, q, lags, labels=None, n_labels=1, first_frame=0, n_frames=None, origin_stride=1):
    """cos_sum, sin_sum (L, K, Q) and count (L, K) of gd_sq_self."""
    F, N, _ = x.shape
    n_frames = F - first_frame if n_frames is None else n_frames
    w = x[first_frame:first_frame + n_frames].astype(np.float64)
    members = _members(labels, N, n_labels)
    c, s = (np.zeros((len(lags), len(members), len(q)), np.longdouble if LONG else np.float64) for _ in range(2))
    count = np.zeros((len(lags), len(members)), np.uint64)
    for k, lag in enumerate(lags):
        o = origins(n_frames, int(lag), origin_stride)
        d = w[[t + int(lag) for t in o]] - w[o]      # rounded once
        for a, beads in enumerate(members):
            count[k, a] = len(o) * len(beads)
            if len(beads):
                ca, sa = _sums(phase(q, d[:, beads]))
                c[k, a], s[k, a] = ca.sum(axis=0), sa.sum(axis=0)
    return c, s, count


def collective(cos_sum, sin_sum, lags, origin_stride=1):
    """sum_re, sum_im (L, K, K, Q) float64 and count (L,) of gd_sq_collective, from amplitudes (n_frames, K, Q) float64: the header's
    operations, each rounded on its own, the terms added serially over ascending origins from +0.0."""
    C, S = np.asarray(cos_sum, dtype=np.float64), np.asarray(sin_sum, dtype=np.float64)
    n_frames, K, Q = C.shape
    re, im = np.zeros((len(lags), K, K, Q)), np.zeros((len(lags), K, K, Q))
    count = np.zeros(len(lags), np.uint64)
    for k, lag in enumerate(lags):
        for t in origins(n_frames, int(lag), origin_stride):
            Ca, Sa, Cb, Sb = C[t + lag][:, None, :], S[t + lag][:, None, :], C[t][None, :, :], S[t][None, :, :]
            re[k] = re[k] + ((Ca * Cb) + (Sa * Sb))
            im[k] = im[k] + ((Ca * Sb) - (Sa * Cb))
            count[k] += 1
    return re, im, count


def bound(n):
    """What the device's C or S of a label of n beads (a number or an array of them) may differ by from amplitudes()."""
    n = np.asarray(n, dtype=np.float64)
    return n * (T_ULP + CHUNK - 1 + np.ceil(n / CHUNK)) * EPS

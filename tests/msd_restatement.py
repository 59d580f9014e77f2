"""numpy fp64 restatement of include/gdyn_msd.h (a helper of test_msd_host.py, test_msd_gpu.py and tools/bench_msd.py; not
collected).  The term of two items, every operation rounded on its own:

    d = double(b) - double(a) per axis;   t2 = (dx*dx + dy*dy) + dz*dz;   t4 = t2*t2

numpy neither contracts nor reassociates these; the sums over origins and beads are numpy's (pairwise), which the parity bound
(2 count + 8) 2^-53 covers as it covers any order of non-negative terms."""
import numpy as np

EPS = 2.0 ** -53


def terms(a, b):
    """t2 and t4 of items a, b (..., 3)."""
    d = b.astype(np.float64) - a.astype(np.float64)
    t2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return t2, t2 * t2


def per_bead(x, lag):
    """m2[:, lag], m4[:, lag] of a history x (F, N, 3): (N,) each."""
    F, N, _ = x.shape
    if lag >= F:
        return np.zeros(N), np.zeros(N)
    t2, t4 = terms(x[:F - lag], x[lag:])
    return t2.sum(axis=0), t4.sum(axis=0)


def time(x, lags, group=None, n_groups=1):
    """sum2, sum4 (G, L) float64 and count (G, L) uint64 of gd_msd_time."""
    F, N, _ = x.shape
    group = np.zeros(N, np.int64) if group is None else np.asarray(group)
    sum2 = np.zeros((n_groups, len(lags)))
    sum4 = np.zeros((n_groups, len(lags)))
    count = np.zeros((n_groups, len(lags)), np.uint64)
    for l, lag in enumerate(lags):
        m2, m4 = per_bead(x, int(lag))
        for g in range(n_groups):
            sel = group == g
            sum2[g, l] = m2[sel].sum()
            sum4[g, l] = m4[sel].sum()
            count[g, l] = int(sel.sum()) * max(0, F - int(lag))
    return sum2, sum4, count


def chain(x, ranges, seps, first_frame=0, n_frames=None):
    """sum2, sum4 (C, S) float64 and count (C, S) uint64 of gd_msd_chain."""
    F = x.shape[0]
    n_frames = F - first_frame if n_frames is None else n_frames
    w = x[first_frame:first_frame + n_frames]
    sum2 = np.zeros((len(ranges), len(seps)))
    sum4 = np.zeros((len(ranges), len(seps)))
    count = np.zeros((len(ranges), len(seps)), np.uint64)
    for c, (start, end) in enumerate(ranges):
        for k, s in enumerate(seps):
            s = int(s)
            if s >= end - start:
                continue
            t2, t4 = terms(w[:, start:end - s], w[:, start + s:end])
            sum2[c, k], sum4[c, k] = t2.sum(), t4.sum()
            count[c, k] = n_frames * (end - start - s)
    return sum2, sum4, count


def bound(count, value):
    """The parity bound of the header: |device - restatement| <= (2 count + 8) 2^-53 restatement."""
    return (2.0 * count.astype(np.float64) + 8.0) * EPS * np.abs(value)


def log_lags(k, longest):
    """The rule of gd_msd --log-lags K / --log-seps K: K values spaced geometrically over [1, longest], each rounded half up,
    duplicates dropped: floor(longest ** (i / (K - 1)) + 0.5) for i = 0 .. K-1 (K = 1: [1]); empty when longest < 1."""
    if longest < 1 or k < 1:
        return []
    out = []
    for i in range(k):
        v = 1 if k == 1 else int(np.floor(float(longest) ** (i / (k - 1)) + 0.5))
        v = min(max(v, 1), longest)
        if not out or v > out[-1]:
            out.append(v)
    return out

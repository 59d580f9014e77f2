"""numpy restatement of include/gdyn_gyr.h (a helper of test_gyr_host.py, test_gyr_gpu.py and tools/bench_gyr.py; not collected).

Every sum is restated in the header's order: the loops over beads, pieces, frames and frame ranges are serial and every operation is
one rounded fp64 operation, vectorised only across what the header leaves independent (frames, axes and segments for the tensors;
frames, window starts and axes for the profile).  So the results are the device's bit for bit."""
import numpy as np

PIECE_BEADS = 32          # GD_GYR_PIECE_BEADS
FRAME_RANGE = 64          # GD_GYR_FRAME_RANGE
MAX_WINDOWS = 8           # GD_GYR_MAX_WINDOWS
MAX_WINDOW = 2048         # GD_GYR_MAX_WINDOW
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx yy zz xy xz yz


def frames(F, first=0, stride=1, count=0):
    """The frames of a selection: first + k stride inside the history; count 0: all that fit."""
    assert stride >= 1
    fit = list(range(first, F, stride))
    if count:
        assert count <= len(fit)
        fit = fit[:count]
    assert fit, "no frame"
    return fit


def _pieces(values, start, end):
    """values (K, N, C): the sum over the beads [start, end) by pieces of PIECE_BEADS, (K, C)."""
    total = np.zeros((values.shape[0], values.shape[2]))
    for a in range(start, end, PIECE_BEADS):                # pieces ascending
        piece = np.zeros_like(total)
        for i in range(a, min(a + PIECE_BEADS, end)):       # beads ascending
            piece = piece + values[:, i]
        total = total + piece
    return total


def tensors(x, segments=None, first=0, stride=1, count=0):
    """(centre_sum (K, S, 3), centre (K, S, 3), moment (K, S, 6)) of gd_gyr_tensors for the history x (F, N, 3), float32 or float64."""
    F, N, _ = x.shape
    segments = [(0, N)] if segments is None else [(int(a), int(b)) for a, b in segments]
    X = x[frames(F, first, stride, count)].astype(np.float64)
    K = len(X)
    centre_sum, centre, moment = np.zeros((K, len(segments), 3)), np.zeros((K, len(segments), 3)), np.zeros((K, len(segments), 6))
    for s, (start, end) in enumerate(segments):
        own = X[:, start:end]                               # pieces are counted from the segment's start
        centre_sum[:, s] = _pieces(own, 0, end - start)
        centre[:, s] = centre_sum[:, s] / np.float64(end - start)
        d = own - centre[:, s][:, None, :]
        products = np.stack([d[..., a] * d[..., b] for a, b in PAIRS], axis=-1)      # each product rounded once
        moment[:, s] = _pieces(products, 0, end - start)
    return centre_sum, centre, moment


def valid(N, chains, w):
    """(N,) bool: the window [i, i + w) lies inside one chain."""
    ok = np.zeros(N, bool)
    for start, end in ([(0, N)] if chains is None else chains):
        if int(end) - int(start) >= w:
            ok[int(start):int(end) - w + 1] = True
    return ok


def profile_frames(x, w, chains=None, first=0, stride=1, count=0):
    """(K, N) float64: v(f_k, i, w) of gd_gyr_profile_frames, +0 where the window is not valid."""
    F, N, _ = x.shape
    X = x[frames(F, first, stride, count)].astype(np.float64)
    out = np.zeros((len(X), N))
    dw = np.float64(w)
    for start, end in ([(0, N)] if chains is None else chains):
        start, end = int(start), int(end)
        n = end - start - w + 1                              # valid window starts of the chain
        if n < 1:
            continue
        s = np.zeros((len(X), n, 3))
        for j in range(w):                                   # beads ascending
            s = s + X[:, start + j:start + j + n]
        c = s / dw
        m = np.zeros((len(X), n))
        for j in range(w):
            d = X[:, start + j:start + j + n] - c
            sq = d * d
            m = m + ((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        out[:, start:start + n] = m / dw
    return out


def add_ranges(v):
    """(K, ...) -> (...): the frames added in ranges of FRAME_RANGE, each serial from +0, the ranges serial from +0."""
    total = np.zeros(v.shape[1:])
    for k0 in range(0, len(v), FRAME_RANGE):
        part = np.zeros(v.shape[1:])
        for k in range(k0, min(k0 + FRAME_RANGE, len(v))):
            part = part + v[k]
        total = total + part
    return total


def profile(x, windows, chains=None, first=0, stride=1, count=0):
    """(sum (W, N), sum_sq (W, N), count (W, N) uint64) of gd_gyr_profile."""
    assert 1 <= len(windows) <= MAX_WINDOWS and all(2 <= w <= MAX_WINDOW for w in windows)
    F, N, _ = x.shape
    K = len(frames(F, first, stride, count))
    total, total_sq, cnt = np.zeros((len(windows), N)), np.zeros((len(windows), N)), np.zeros((len(windows), N), np.uint64)
    for m, w in enumerate(windows):
        v = profile_frames(x, int(w), chains, first, stride, count)
        total[m], total_sq[m] = add_ranges(v), add_ranges(v * v)
        cnt[m] = np.where(valid(N, chains, int(w)), np.uint64(K), np.uint64(0))
    return total, total_sq, cnt

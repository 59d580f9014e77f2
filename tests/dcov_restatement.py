"""numpy restatement of include/gdyn_dcov.h (a helper of test_dcov_host.py, test_dcov_gpu.py and tools/bench_dcov.py; not collected).

Stage 1, the row matrix A, is restated by the header's orders: the loops over frames (the mean), beads, pieces and bins are serial and
every operation is one rounded fp64 operation, vectorised across the columns only, so `rows` is the device's A bit for bit.  The
product is not restated in the device's order (the order inside the matrix instruction is not documented): `reference` is the sum of
products of given rows in np.longdouble and `bound` the header's any-order bound, widened by the reference's own error; `integer_map`
is the exact product of integer-valued rows."""
import numpy as np

PIECE_BEADS = 32          # GD_DCOV_PIECE_BEADS
COLUMN_RANGE = 768        # GD_DCOV_COLUMN_RANGE
U = 2.0 ** -53
LONGDOUBLE_64 = np.finfo(np.longdouble).nmant == 63      # an x87 extended: 64-bit significand.  Without it there is no reference


def origins(F, lag, first=0, stride=1, count=0):
    """The origin frames of gd_dcov_prepare: first + k stride with the frame `lag` later inside the history; count 0: all that fit."""
    fit = list(range(first, F - lag, stride))
    if count:
        assert count <= len(fit)
        fit = fit[:count]
    assert fit, "no origin"
    return fit


def padded(columns):
    return (columns + 3) // 4 * 4


def rows(x, bins=None, lag=1, first=0, stride=1, count=0, remove_drift=False):
    """A (B, 3 origins) float64 of gd_dcov_prepare for the history x (F, N, 3), float32 or float64."""
    F, N, _ = x.shape
    bins = [(i, i + 1) for i in range(N)] if bins is None else [(int(a), int(b)) for a, b in bins]
    frames = origins(F, lag, first, stride, count)
    if lag:
        d = x[[f + lag for f in frames]].astype(np.float64) - x[frames].astype(np.float64)      # (O, N, 3): one subtraction each
    else:
        mean = np.zeros((N, 3))
        for f in frames:                                    # serial over the frames, ascending
            mean = mean + x[f].astype(np.float64)
        mean = mean / np.float64(len(frames))
        d = x[frames].astype(np.float64) - mean[None]
    d = np.ascontiguousarray(d.transpose(1, 0, 2)).reshape(N, 3 * len(frames))      # D[i, 3 k + axis]
    raw = np.zeros((len(bins), d.shape[1]))
    for b, (start, end) in enumerate(bins):
        total = np.zeros(d.shape[1])
        for a in range(start, end, PIECE_BEADS):            # pieces ascending
            piece = np.zeros(d.shape[1])
            for i in range(a, min(a + PIECE_BEADS, end)):   # beads ascending
                piece = piece + d[i]
            total = total + piece
        raw[b] = total
    if not remove_drift:
        return raw
    m = np.zeros(d.shape[1])
    for b in range(len(bins)):                              # bins ascending
        m = m + raw[b]
    m = m / np.float64(sum(end - start for start, end in bins))
    out = np.empty_like(raw)
    for b, (start, end) in enumerate(bins):
        drift = np.float64(end - start) * m                 # rounded on its own
        out[b] = raw[b] - drift
    return out


def count(bins, n_origins):
    """count[I, J] = origins |I| |J| (uint64)."""
    size = np.array([int(b) - int(a) for a, b in bins], dtype=np.uint64)
    return np.uint64(n_origins) * np.outer(size, size)


def integer_map(a_rows, a_cols=None):
    """The exact product of integer-valued rows, by int64 matmul (float64)."""
    a_cols = a_rows if a_cols is None else a_cols
    ia, ib = a_rows.astype(np.int64), a_cols.astype(np.int64)
    assert np.array_equal(ia, a_rows) and np.array_equal(ib, a_cols), "rows are not integer-valued"
    s = ia @ ib.T
    assert np.abs(s).max() < 2 ** 53
    return s.astype(np.float64)


def reference(a_rows, a_cols=None):
    """(sum of products, sum of their absolute values) of the rows in np.longdouble."""
    assert LONGDOUBLE_64, "np.longdouble has no 64-bit significand here"
    a_cols = a_rows if a_cols is None else a_cols
    la, lb = a_rows.astype(np.longdouble), a_cols.astype(np.longdouble)
    return la @ lb.T, np.abs(la) @ np.abs(lb).T


def bound(abs_sum, columns):
    """Item 4 of the header for K = padded(columns): gamma sum|a||b| with gamma = (K + 1) u / (1 - (K + 1) u), widened by the
    reference's own (K + 1) 2^-64 sum|a||b| (its K products and additions are rounded to 64 bits)."""
    K = np.longdouble(padded(columns))
    gamma = (K + 1) * np.longdouble(U) / (1 - (K + 1) * np.longdouble(U))
    return (gamma + (K + 1) * np.longdouble(2.0) ** -64) * abs_sum

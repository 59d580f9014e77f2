"""numpy restatement of include/gdyn_dwell.h (a helper of test_dwell_host.py, test_dwell_gpu.py and tools/bench_dwell.py; not collected).

The pair term is fp64 on the widened coordinates, every operation one rounded numpy operation, vectorised over the pairs and the
frames; the state machine is one Python loop over the selected frames; the runs are found from the changes of the state.  Every output
is an integer, so the device's results are these, exactly."""
import numpy as np

MAX_BINS = 64             # GD_DWELL_MAX_BINS
MAX_LAGS = 64             # GD_DWELL_MAX_LAGS
MAX_SEPARATIONS = 32      # GD_DWELL_MAX_SEPARATIONS
KEYS = ("runs", "outside", "length_sum", "hits", "pairs")


def frames(F, first=0, stride=1, count=0):
    """The frames of a selection: first + k stride inside the history; count 0: all that fit."""
    assert stride >= 1
    fit = list(range(first, F, stride))
    if count:
        assert count <= len(fit)
        fit = fit[:count]
    assert fit, "no frame"
    return fit


def r2(x, pairs, box=None, first=0, stride=1, count=0):
    """(K, P) float64: the squared distance of every pair at every selected frame."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    X = x[frames(len(x), first, stride, count)].astype(np.float64)
    d = X[:, pairs[:, 0]] - X[:, pairs[:, 1]]
    if box is not None:
        b = np.broadcast_to(np.asarray(box, np.float64), (3,))
        d = d - b * np.rint(d / b)
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def states(x, pairs, r_on, r_off=None, box=None, first=0, stride=1, count=0):
    """(K, P) uint8: c_k of gd_dwell_states."""
    r_on = np.float64(r_on)
    r_off = r_on if r_off is None else np.float64(r_off)
    assert 0 < r_on <= r_off and np.isfinite(r_off)
    d2 = r2(x, pairs, box, first, stride, count)
    on, hold = d2 < r_on * r_on, d2 < r_off * r_off
    c = np.zeros(d2.shape, bool)
    c[0] = on[0]
    for k in range(1, len(c)):
        c[k] = np.where(c[k - 1], hold[k], on[k])
    return c.astype(np.uint8)


def chain_pairs(N, chains, s):
    """(n, 2) the pairs (i, i + s) with both beads inside one chain, ascending."""
    out = [np.stack([np.arange(a, b - s), np.arange(a + s, b)], axis=1) for a, b in ([(0, N)] if chains is None else chains) if int(b) - int(a) > s]
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def runs_of(c):
    """The runs of the states c (K, P): (pair, state, kind, length) arrays, one entry per run."""
    K, P = c.shape
    ct = np.ascontiguousarray(c.T).astype(bool)
    begins = np.ones((P, K), bool)
    begins[:, 1:] = ct[:, 1:] != ct[:, :-1]
    p, start = np.nonzero(begins)                            # by pair, then by frame
    end = np.append(start[1:], K)
    end[np.append(p[1:] != p[:-1], True)] = K                # the last run of a pair ends with the selection
    kind = (start == 0).astype(np.int64) + 2 * (end == K)
    return p, ct[p, start].astype(np.int64), kind, end - start


def accumulate(c, rows, R, edges, lags):
    """The outputs of the states c (K, P) of pairs of the rows `rows` (P,) of R: {runs, outside, length_sum, hits, pairs}, uint64."""
    K, P = c.shape
    rows, edges, lags = np.asarray(rows, np.int64), np.asarray(edges, np.int64), np.asarray(lags, np.int64)
    B = len(edges) - 1
    assert 1 <= B <= MAX_BINS and edges[0] >= 1 and (np.diff(edges) > 0).all() and len(lags) <= MAX_LAGS and (rows < R).all()
    out = {"runs": np.zeros((R, 2, 4, B), np.uint64), "outside": np.zeros((R, 2, 4), np.uint64), "length_sum": np.zeros((R, 2, 4), np.uint64),
           "hits": np.zeros((R, len(lags)), np.uint64), "pairs": np.bincount(rows, minlength=R).astype(np.uint64)}
    if P:
        p, state, kind, length = runs_of(c)
        b = np.searchsorted(edges, length, side="right") - 1      # e_b <= length < e_{b+1}
        inside = (b >= 0) & (b < B)
        np.add.at(out["runs"], (rows[p][inside], state[inside], kind[inside], b[inside]), np.uint64(1))
        np.add.at(out["outside"], (rows[p][~inside], state[~inside], kind[~inside]), np.uint64(1))
        np.add.at(out["length_sum"], (rows[p], state, kind), length.astype(np.uint64))
        wide = c.astype(np.uint64)
        for l, lag in enumerate(lags):
            if lag < K:
                np.add.at(out["hits"][:, l], rows, (wide[:K - lag] * wide[lag:]).sum(axis=0, dtype=np.uint64))
    return out


def separations(x, seps, r_on, r_off=None, edges=(1, 2), lags=(), chains=None, box=None, first=0, stride=1, count=0):
    """gd_dwell_separations: one row per separation."""
    assert 1 <= len(seps) <= MAX_SEPARATIONS and all(s >= 1 for s in seps)
    N = x.shape[1]
    pairs = [chain_pairs(N, chains, int(s)) for s in seps]
    rows = np.concatenate([np.full(len(p), m, np.int64) for m, p in enumerate(pairs)])
    pairs = np.concatenate(pairs)
    K = len(frames(len(x), first, stride, count))
    c = states(x, pairs, r_on, r_off, box, first, stride, count) if len(pairs) else np.zeros((K, 0), np.uint8)
    return accumulate(c, rows, len(seps), edges, lags)


def pairs(x, pairs, r_on, r_off=None, rows=None, n_rows=None, edges=(1, 2), lags=(), box=None, first=0, stride=1, count=0):
    """gd_dwell_pairs: rows None makes every pair its own row."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert len(pairs) and (pairs[:, 0] != pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < x.shape[1]
    R = len(pairs) if rows is None else int(np.max(rows)) + 1 if n_rows is None else int(n_rows)
    rows = np.arange(len(pairs)) if rows is None else np.asarray(rows, np.int64)
    return accumulate(states(x, pairs, r_on, r_off, box, first, stride, count), rows, R, edges, lags)

"""Numpy restatement of include/gdyn_vanhove.h by brute force: the displacement of every selected bead per (origin, lag) for the self
part, all ordered pairs per (origin, lag) with the minimum image for the distinct part, O(n^2).  Squared distances are binned by
np.searchsorted on the squared edges; no square root is taken.  Shares no code with the module under test."""
import numpy as np


def origins(F, first=0, stride=1, count=0):
    """The origin frames first + k stride: k < count, or with count 0 all below F."""
    return [first + k * stride for k in range(count)] if count else list(range(first, F, stride))


def _labels(N, label, K):
    if label is None:
        return np.zeros(N, np.int64), 1
    return np.asarray(label, np.int64), int(K)


def _cells(r2, e2):
    """0: below e_0^2; 1 + b: bin b; B + 1: at or above e_B^2."""
    return np.searchsorted(e2, r2, side="right")


def self_part(x, lags, edges, label=None, K=1, axes="xyz", first=0, stride=1, count=0):
    """counts (L, K, B), below, above (L, K), per_origin (L, O, K, B), origins (L,), all uint64."""
    x = np.asarray(x)
    F, N, _ = x.shape
    lab, K = _labels(N, label, K)
    e = np.asarray(edges, np.float64)
    e2, B = e * e, len(e) - 1
    og = origins(F, first, stride, count)
    L, O = len(lags), len(og)
    out = {"counts": np.zeros((L, K, B), np.uint64), "below": np.zeros((L, K), np.uint64), "above": np.zeros((L, K), np.uint64),
           "per_origin": np.zeros((L, O, K, B), np.uint64), "origins": np.zeros(L, np.uint64)}
    sel = np.flatnonzero(lab >= 0)
    for l, lag in enumerate(lags):
        for k, f in enumerate(og):
            if f + lag >= F:
                continue
            out["origins"][l] += 1
            d = x[f + lag, sel].astype(np.float64) - x[f, sel].astype(np.float64)
            t = [d[:, a] * d[:, a] if "xyz"[a] in axes else np.zeros(len(sel)) for a in range(3)]
            r2 = (t[0] + t[1]) + t[2]
            table = np.bincount(lab[sel] * (B + 2) + _cells(r2, e2), minlength=K * (B + 2)).reshape(K, B + 2).astype(np.uint64)
            out["per_origin"][l, k] = table[:, 1:B + 1]
            out["counts"][l] += table[:, 1:B + 1]
            out["below"][l] += table[:, 0]
            out["above"][l] += table[:, B + 1]
    return out


def pair_r2(a, b, box=None):
    """(n, m) squared distances from every a[i] to every b[j], d = b - a, reduced to the minimum image in a periodic box."""
    d = np.asarray(b, np.float64)[None, :, :] - np.asarray(a, np.float64)[:, None, :]
    if box is not None:
        bx = np.broadcast_to(np.asarray(box, np.float64), (3,))
        d = d - bx * np.rint(d / bx)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def distinct(x, lags, edges, label=None, K=1, box=None, first=0, stride=1, count=0):
    """counts (L, K, K, B) [lag, label of i at the origin, label of j a lag later, bin] over ordered pairs i != j, and origins (L,)."""
    x = np.asarray(x)
    F, N, _ = x.shape
    lab, K = _labels(N, label, K)
    e = np.asarray(edges, np.float64)
    e2, B = e * e, len(e) - 1
    og = origins(F, first, stride, count)
    out = {"counts": np.zeros((len(lags), K, K, B), np.uint64), "origins": np.zeros(len(lags), np.uint64)}
    sel = np.flatnonzero(lab >= 0)
    cls = (lab[sel][:, None] * K + lab[sel][None, :])
    off = ~np.eye(len(sel), dtype=bool)
    for l, lag in enumerate(lags):
        for f in og:
            if f + lag >= F:
                continue
            out["origins"][l] += 1
            cell = _cells(pair_r2(x[f, sel], x[f + lag, sel], box), e2)
            keep = off & (cell >= 1) & (cell <= B)
            out["counts"][l] += np.bincount(cls[keep] * B + cell[keep] - 1, minlength=K * K * B).reshape(K, K, B).astype(np.uint64)
    return out

"""An independent restatement of the contact-map accumulations for the tests: plain loops over the rows (the rules as the
issue states them, one row at a time) and np.add.at / np.bincount forms of the same sums for the scale cases.  Nothing here
imports the package under test."""
import numpy as np


# ---- one row at a time

def region_loop(rows, beg, end):
    m = np.zeros((end - beg, end - beg), np.int64)
    for i, j, v in np.asarray(rows).tolist():
        if beg <= i < end and beg <= j < end:
            m[i - beg, j - beg] += v
    return m


def finish(m):
    s = m + m.T
    if s.size:
        top = s.max()
        for k in range(len(s)):
            s[k, k] = top
    return s


def binned_loop(rows, rebin, n_bins):
    m = np.zeros((n_bins, n_bins), np.int64)
    n = len(rebin)
    for i, j, v in np.asarray(rows).tolist():
        if i >= n or j >= n:
            continue
        m[rebin[i], rebin[j]] += v
        m[rebin[j], rebin[i]] += v
    return m


def nucleolus_loop(rows, beg, end, is_nucleolus):
    p = np.zeros(end - beg, np.int64)
    n = len(is_nucleolus)
    for i, j, v in np.asarray(rows).tolist():
        if beg <= i < end and j < n and is_nucleolus[j]:
            p[i - beg] += v
        if beg <= j < end and i < n and is_nucleolus[i]:
            p[j - beg] += v
    return p


def separation_loop(rows, chain_id, size):
    p = np.zeros(size, np.int64)
    n = len(chain_id)
    for i, j, v in np.asarray(rows).tolist():
        if i < n and j < n and chain_id[i] == chain_id[j] and chain_id[i] != -1:
            p[abs(i - j)] += v
    return p


# ---- the same sums for millions of rows

def _ijv(rows):
    r = np.asarray(rows).astype(np.int64)
    return r[:, 0], r[:, 1], r[:, 2]


def region(rows, beg, end):
    i, j, v = _ijv(rows)
    size = end - beg
    s = (i >= beg) & (i < end) & (j >= beg) & (j < end)
    return np.bincount((i[s] - beg) * size + (j[s] - beg), weights=None if not s.any() else v[s], minlength=size * size).astype(np.int64).reshape(size, size)


def binned(rows, rebin, n_bins):
    i, j, v = _ijv(rows)
    rebin = np.asarray(rebin).astype(np.int64)
    s = (i < len(rebin)) & (j < len(rebin))
    bi, bj, v = rebin[i[s]], rebin[j[s]], v[s]
    m = np.zeros(n_bins * n_bins, np.int64)
    np.add.at(m, bi * n_bins + bj, v)
    np.add.at(m, bj * n_bins + bi, v)
    return m.reshape(n_bins, n_bins)


def nucleolus(rows, beg, end, is_nucleolus):
    i, j, v = _ijv(rows)
    nuc = np.concatenate([np.asarray(is_nucleolus).astype(bool), np.zeros(int(max(i.max(initial=0), j.max(initial=0))) + 1, bool)])
    p = np.zeros(end - beg, np.int64)
    s = (i >= beg) & (i < end) & nuc[j]
    np.add.at(p, i[s] - beg, v[s])
    s = (j >= beg) & (j < end) & nuc[i]
    np.add.at(p, j[s] - beg, v[s])
    return p


def separation(rows, chain_id, size):
    i, j, v = _ijv(rows)
    chain = np.concatenate([np.asarray(chain_id), np.full(int(max(i.max(initial=0), j.max(initial=0))) + 1, -1, np.int64)])
    s = (chain[i] == chain[j]) & (chain[i] != -1)
    p = np.zeros(size, np.int64)
    np.add.at(p, np.abs(i[s] - j[s]), v[s])
    return p


# ---- what the programs do around the sums

def select_steps(steps, before=None, after=None):
    """contact_map.py:52-55: by step value."""
    return [s for s in steps if (before is None or s < before) and (after is None or s >= after)]


def fit(x, y):
    """The weighted least-squares slope of log y on log x, weights 1 / x, from the normal equations."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    keep = (x > 0) & (y > 0)
    X, Y, w = np.log(x[keep]), np.log(y[keep]), 1 / x[keep]
    A = np.array([[np.sum(w), np.sum(w * X)], [np.sum(w * X), np.sum(w * X * X)]])
    b = np.array([np.sum(w * Y), np.sum(w * X * Y)])
    return float(np.linalg.solve(A, b)[1])

"""An independent brute-force restatement of the spatial correlation of bead displacements (include/gdyn_dcorr.h) for the tests
of csrc/gdyn_dcorr.hip, dcorr.py and gd_dcorr.  numpy, O(N^2) in chunks, fp64 in exactly the header's operation order (numpy
rounds every elementwise operation on its own), np.rint fixed point; it shares no code with the package.  The pair rules are
those of tests/rdf_restatement.py (minimum image, strict cutoff, size_t(sqrt(r2) * (1 / bin_width)), each unordered pair once)."""
import math
from fractions import Fraction

import numpy as np

MAX_SCALE_BITS = 40
LIMIT = 1 << 62


def n_bins(bin_width, max_distance):
    return int(math.ceil(max_distance / bin_width))


def n_classes(K, chains=False):
    return K * (K + 1) // 2 * (2 if chains else 1)


def class_index(a, b, K, different_chain=None):
    """The class of an unordered pair with labels a and b (arrays or scalars): p = lo K - lo (lo - 1) / 2 + (hi - lo) with
    lo <= hi, and 2 p + (chain_i != chain_j) when chains are set (different_chain not None)."""
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    p = lo * K - lo * (lo - 1) // 2 + (hi - lo)
    return p if different_chain is None else 2 * p + np.asarray(different_chain, np.int64)


def legal(n, M, S):
    """The guard: max(n (n - 1) / 2, 1) (M 2^S + 1) < 2^62, in exact rational arithmetic (M is a double)."""
    M = float(M)
    if not (M >= 0.0) or math.isinf(M):
        return False
    return max(n * (n - 1) // 2, 1) * (Fraction(M) * Fraction(2) ** S + 1) < LIMIT


def auto_scale(n, M):
    """The largest legal S in [0, 40], or None."""
    for S in range(MAX_SCALE_BITS, -1, -1):
        if legal(n, M, S):
            return S
    return None


def origins(F, lag, first=0, count=0, stride=1):
    if count:
        return [first + k * stride for k in range(count)]
    return list(range(first, F - lag, stride)) if first + lag < F else []


def displacements(x, lag, f):
    """D (N, 3) and t2 (N) of origin f, fp64 on the widened coordinates."""
    d = x[f + lag].astype(np.float64) - x[f].astype(np.float64)
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _selection(N, label, K):
    if label is None:
        return np.arange(N), np.zeros(N, np.int64), 1
    label = np.asarray(label, np.int64)
    return np.flatnonzero(label >= 0), label, K


def largest_t2(x, lag, label=None, first=0, count=0, stride=1):
    """M of the guard: the largest t2 over the selected beads (label >= 0; None: all) and the origins."""
    x = np.asarray(x)
    sel = _selection(x.shape[1], label, 1)[0]
    m = 0.0
    for f in origins(len(x), lag, first, count, stride):
        t2 = displacements(x, lag, f)[1][sel]
        m = max(m, float(t2.max())) if len(t2) else m
    return m


def _pair_terms(p, d, lab, ch, K, i, j, box, bin_width, max_distance, S, out_count, out_sum):
    """Adds the candidate pairs (i, j) (index arrays into the selected beads, each unordered pair at most once) to the tables."""
    r = p[i] - p[j]
    if box is not None:
        b = np.asarray(box, np.float64)
        r = r - b * np.rint(r / b)
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    keep = r2 < max_distance * max_distance
    bins = np.zeros(len(r2), np.uint64)
    bins[keep] = (np.sqrt(r2[keep]) * (1 / bin_width)).astype(np.uint64)
    keep &= bins < n_bins(bin_width, max_distance)
    i, j, bins = i[keep], j[keep], bins[keep].astype(np.int64)
    dot = (d[i, 0] * d[j, 0] + d[i, 1] * d[j, 1]) + d[i, 2] * d[j, 2]
    q = np.rint(dot * 2.0 ** S).astype(np.int64)
    cls = class_index(lab[i], lab[j], K, None if ch is None else ch[i] != ch[j])
    np.add.at(out_count, (cls, bins), np.uint64(1))
    np.add.at(out_sum, (cls, bins), q)


def pairs(x, lag, bin_width, max_distance, box=None, label=None, K=1, chain=None, scale_bits=0, first=0, count=0, stride=1, candidates=None,
          chunk=256):
    """(count (O, P, n_bins) uint64, sum (O, P, n_bins) int64, self_count (O, K) uint64, self_sum (O, K) int64, S).
    scale_bits 0: automatic; otherwise S itself ("unit" for S = 0).  candidates: a function (positions of the selected beads)
    -> (i, j) candidate pairs that replaces the walk over all pairs."""
    x = np.asarray(x)
    M = largest_t2(x, lag, label, first, count, stride)
    sel, label, K = _selection(x.shape[1], label, K)
    og = origins(len(x), lag, first, count, stride)
    S = 0 if scale_bits == "unit" else scale_bits
    if scale_bits == 0:
        S = auto_scale(len(sel), M)
    P, nb = n_classes(K, chain is not None), n_bins(bin_width, max_distance)
    out_count, out_sum = np.zeros((len(og), P, nb), np.uint64), np.zeros((len(og), P, nb), np.int64)
    self_count, self_sum = np.zeros((len(og), K), np.uint64), np.zeros((len(og), K), np.int64)
    lab = label[sel]
    ch = None if chain is None else np.asarray(chain)[sel]
    for o, f in enumerate(og):
        d, t2 = displacements(x, lag, f)
        p, d, t2 = x[f].astype(np.float64)[sel], d[sel], t2[sel]
        np.add.at(self_count[o], lab, np.uint64(1))
        np.add.at(self_sum[o], lab, np.rint(t2 * 2.0 ** S).astype(np.int64))
        if candidates is not None:
            i, j = candidates(p)
            _pair_terms(p, d, lab, ch, K, np.asarray(i, np.int64), np.asarray(j, np.int64), box, bin_width, max_distance, S, out_count[o], out_sum[o])
            continue
        for i0 in range(0, len(p), chunk):
            i, j = np.meshgrid(np.arange(i0, min(i0 + chunk, len(p))), np.arange(len(p)), indexing="ij")
            first_of = i < j
            _pair_terms(p, d, lab, ch, K, i[first_of], j[first_of], box, bin_width, max_distance, S, out_count[o], out_sum[o])
    return out_count, out_sum, self_count, self_sum, S

"""The Hi-C signal analyses on the device: ctypes binding of ``include/gdyn_hic.h`` (exported by ``csrc/libgdyn.so``), one
pass over a cooler's pixel table for the reference's 2-signal/src/{compute_interactions, compute_local_alpha} and
5-sim-genome/scripts/hic_power_law.

    with HicSignals(chrom_code, device=0) as hs:
        b = hs.add_band(4)                                   # compute_interactions: band[i, d], d < 4
        a = hs.add_band(width + 1)                           # compute_local_alpha -w width
        p = hs.add_distance_profile(excluded, weights, size) # hic_power_law; weights=None is RAW
        for bin1, bin2, count in chunks:                     # int64, int64, int32 as stored
            hs.accumulate(bin1, bin2, count)                 # one pass over the pixels for every target
        D, I = hs.decay_insulation(b)                        # (n_bins, 3), (n_bins, 2)
        alpha = hs.local_alpha(a)
        total, n, mean = hs.fetch_profile(p)

The compartment analysis of hic_analysis/cool.py (dense cis matrices, observed / expected, leading principal components):

        d = hs.add_dense(weights)                            # before the pass: one float32 (n, n) matrix per chromosome
        contacts, counts, mean = hs.dense_profile(d, excluded)
        E = hs.fetch_dense(d, code, DENSE_ENRICHMENT)
        pcs, variances, axes, iterations = hs.dense_pca(d, code, mask=hs.dense_valid(d)[chrom_code == code], k=3)
        pcs, variances, axes, iterations = hs.pca_matrix(any_square_matrix, k=3)

``dense_matrices``, ``mean_contact_profile``, ``enrichment``, ``dense_valid`` and ``contact_pca`` are their numpy counterparts.
``band_matrix``, ``decay_insulation``, ``local_alpha``, ``distance_profile`` and ``downsample`` are the same rules in numpy for
users without a GPU; the device path never calls them.  ``chromosome_runs``, ``std_chrom_order``, ``excluded_bins`` and
``largest_chromosome`` are the bookkeeping of the three programs.  Band sums are int64; the signals are fp64.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, Handle, load_library

HIC_ABI_VERSION = 2      # GD_HIC_ABI_VERSION of the include/gdyn_hic.h this binding mirrors
HIC_SYMBOLS = ["gd_hic_abi_version", "gd_hic_create", "gd_hic_destroy", "gd_hic_add_band", "gd_hic_add_distance_profile",
               "gd_hic_accumulate", "gd_hic_decay_insulation", "gd_hic_local_alpha", "gd_hic_fetch_band", "gd_hic_fetch_profile",
               "gd_hic_fetch_profile_raw", "gd_hic_reset", "gd_hic_clear", "gd_hic_add_dense", "gd_hic_dense_profile", "gd_hic_fetch_dense",
               "gd_hic_dense_valid", "gd_hic_dense_pca", "gd_hic_pca_matrix"]
HIC_MAX_PCS = 8                              # GD_HIC_MAX_PCS
DENSE_CONTACT, DENSE_ENRICHMENT = 0, 1       # GD_HIC_DENSE_*
INTERACTIONS_BLACKLIST = ("MT",)             # compute_interactions.py: BLACKLISTED_CHROMS
PROFILE_BLACKLIST = ("X", "Y", "MT")         # hic_power_law: BLACKLISTED_CHROMS
NAMED_CHROM_RANK = {"X": 1, "Y": 2, "MT": 3, "M": 3}


class _HicDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_pixels_per_launch", C.c_uint32)]


def load_hic_library(path=None):
    """Loads libgdyn and checks the gd_hic_* symbols and their ABI version."""
    d = load_library("hic", HIC_SYMBOLS, HIC_ABI_VERSION, path)
    P32 = C.POINTER(C.c_int32)
    d.gd_hic_create.argtypes = [C.POINTER(_HicDesc), C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    d.gd_hic_destroy.argtypes = [C.c_void_p]
    d.gd_hic_add_band.argtypes = [C.c_void_p, C.c_uint32, P32]
    d.gd_hic_add_distance_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, P32]
    d.gd_hic_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    d.gd_hic_decay_insulation.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    d.gd_hic_local_alpha.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    d.gd_hic_fetch_band.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    d.gd_hic_fetch_profile.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    d.gd_hic_fetch_profile_raw.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    d.gd_hic_reset.argtypes = [C.c_void_p]
    d.gd_hic_clear.argtypes = [C.c_void_p]
    d.gd_hic_add_dense.argtypes = [C.c_void_p, C.c_void_p, P32]
    d.gd_hic_dense_profile.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    d.gd_hic_fetch_dense.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    d.gd_hic_dense_valid.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    d.gd_hic_dense_pca.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, P32]
    d.gd_hic_pca_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, P32]
    return d


# ---- bookkeeping of the programs

def chromosome_runs(chrom_code):
    """enumerate_runs (compute_local_alpha/command.py): the (start, end) of every run of equal codes."""
    c = np.asarray(chrom_code)
    if len(c) == 0:
        return []
    cuts = np.flatnonzero(c[1:] != c[:-1]) + 1
    return list(zip([0, *cuts.tolist()], [*cuts.tolist(), len(c)]))


def std_chrom_order(name):
    """by_std_chrom_order (compute_interactions.py): numbered chromosomes first, then X, Y, MT / M.  KeyError for other names."""
    if name.startswith("chr"):
        name = name[3:]
    try:
        return 0, int(name)
    except ValueError:
        return NAMED_CHROM_RANK[name], 0


def excluded_bins(chrom_code, names, blacklist=PROFILE_BLACKLIST):
    """uint8 mask of the bins of blacklisted chromosomes.  names: {name: code}; a name matches with or without a chr prefix and
    blacklisted names that the file does not have are skipped."""
    c = np.asarray(chrom_code)
    codes = [code for name, code in names.items() if (name[3:] if name.startswith("chr") else name) in blacklist]
    return np.isin(c, codes).astype(np.uint8)


def largest_chromosome(chrom_code):
    """The size of hic_power_law's profile: the largest number of bins of any chromosome code."""
    return int(np.unique(np.asarray(chrom_code), return_counts=True)[1].max())


# ---- numpy: the same rules on the host

def _pixels(bin1, bin2, count, n_bins):
    b1, b2, c = np.asarray(bin1).astype(np.int64), np.asarray(bin2).astype(np.int64), np.asarray(count).astype(np.int64)
    ok = (b1 >= 0) & (b1 < n_bins) & (b2 >= 0) & (b2 < n_bins)
    b1, b2, c = b1[ok], b2[ok], c[ok]
    return np.minimum(b1, b2), np.maximum(b1, b2), c


def band_matrix(bin1, bin2, count, chrom_code, W, out=None):
    """Rule 1: exact int64 sums band[i, d] += c over cis pixels with d < W; pixels with a bin id outside the table are ignored."""
    chrom = np.asarray(chrom_code)
    i, j, c = _pixels(bin1, bin2, count, len(chrom))
    band = np.zeros((len(chrom), W), np.int64) if out is None else out
    s = (chrom[i] == chrom[j]) & (j - i < W)
    np.add.at(band, (i[s], (j - i)[s]), c[s])
    return band


def _nanmean2(a, b):
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, (a + b) / 2))


def _symmetric_decay(band, chrom_code):
    """D(i, k) for k = 0 .. W-1 of every run of equal codes, fp64, NaN for zero cells."""
    band = np.asarray(band)
    n_bins, W = band.shape
    x = np.where(band == 0, np.nan, band.astype(np.float64))
    D = np.full((n_bins, W), np.nan)
    for beg, end in chromosome_runs(chrom_code):
        n = end - beg
        if n <= 1:
            continue
        r = x[beg:end]
        D[beg:end, 0] = 1.0
        for k in range(1, W):
            forw, back = np.full(n, np.nan), np.full(n, np.nan)
            if k < n:
                f = r[:n - k, k] / np.sqrt(r[:n - k, 0] * r[k:, 0])
                forw[:n - k] = f
                back[k:] = f
            D[beg:end, k] = _nanmean2(forw, back)
    return D


def decay_insulation(band, chrom_code):
    """Rule 2: (D1 .. D(W-1), I1 .. I(W-2)) of a band of W >= 2 columns."""
    with np.errstate(divide="ignore", invalid="ignore"):
        D = _symmetric_decay(band, chrom_code)
        return D[:, 1:].copy(), D[:, 1:-1] / D[:, 2:]


def local_alpha(band, chrom_code):
    """Rule 3: alpha of a band of width + 1 columns."""
    with np.errstate(divide="ignore", invalid="ignore"):
        D = _symmetric_decay(band, chrom_code)
        xs = np.log(np.arange(1, D.shape[1], dtype=np.float64))
        ys = np.log(D[:, 1:])
        finite = ~np.isnan(ys)
        count = finite.sum(axis=1)
        my = np.where(finite, ys, 0).sum(axis=1) / count
        mxy = np.where(finite, xs * ys, 0).sum(axis=1) / count
        mx, mxx = xs.mean(), (xs * xs).mean()
        return -((mxy - mx * my) / (mxx - mx * mx))


def distance_profile(bin1, bin2, count, chrom_code, excluded=None, weights=None, size=None):
    """Rule 4: (sum, n, mean) per distance.  Without weights sum is int64 and exact."""
    chrom = np.asarray(chrom_code)
    size = largest_chromosome(chrom) if size is None else size
    i, j, c = _pixels(bin1, bin2, count, len(chrom))
    s = chrom[i] == chrom[j]
    if excluded is not None:
        ex = np.asarray(excluded).astype(bool)
        s &= ~(ex[i] | ex[j])
    i, j, c = i[s], j[s], c[s]
    if len(i) and (j - i).max() >= size:
        raise ValueError(f"a distance of {(j - i).max()} bins in a profile of {size} bins")
    n = np.zeros(size, np.int64)
    if weights is None:
        total = np.zeros(size, np.int64)
        np.add.at(total, j - i, c)
        np.add.at(n, j - i, 1)
    else:
        w = np.asarray(weights, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = c / (w[i] * w[j])
        keep = ~np.isnan(v)
        total = np.bincount((j - i)[keep], weights=v[keep], minlength=size)
        n += np.bincount((j - i)[keep], minlength=size)
    with np.errstate(divide="ignore", invalid="ignore"):
        return total, n, total / n


def downsample(values, rate=2, window=None):
    """Rule 5 for one chromosome: values (n, columns) -> (ceil(n / rate), columns)."""
    v = np.asarray(values, np.float64)
    window = rate if window is None else window
    n = len(v)
    out = np.full(((n + rate - 1) // rate, v.shape[1]), np.nan)
    for m in range(len(out)):
        lo, hi = max(rate * (m + 1) - window + 1, 0), min(rate * (m + 1), n - 1)
        part = v[lo:hi + 1]
        finite = ~np.isnan(part)
        count = finite.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[m] = np.where(count > 0, np.where(finite, part, 0).sum(axis=0) / count, np.nan)
    return out


# ---- the compartment analysis (hic_analysis/cool.py) in numpy

def dense_matrices(bin1, bin2, count, chrom_code, weights=None):
    """load_contact_matrices: {code: float32 (n, n)} for every run of equal codes.  v = c / (w[i] w[j]) in fp64, rounded to
    float32 once and added at [li, lj] and [lj, li] (two adds: a diagonal pixel counts twice); a NaN or infinite v is stored."""
    chrom = np.asarray(chrom_code)
    i, j, c = _pixels(bin1, bin2, count, len(chrom))
    runs = chromosome_runs(chrom)
    beg = np.zeros(len(chrom), np.int64)
    for b, e in runs:
        beg[b:e] = b
    s = (chrom[i] == chrom[j]) & (beg[i] == beg[j])
    i, j, c = i[s], j[s], c[s]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (c.astype(np.float64) if weights is None else c / (np.asarray(weights, np.float64)[i] * np.asarray(weights, np.float64)[j])).astype(np.float32)
    out = {}
    for b, e in runs:
        m = np.zeros((e - b, e - b), np.float32)
        k = (i >= b) & (i < e)
        np.add.at(m, (i[k] - b, j[k] - b), v[k])
        np.add.at(m, (j[k] - b, i[k] - b), v[k])
        out[int(chrom[b])] = m
    return out


def mean_contact_profile(matrices, valid=None):
    """_compute_mean_contact_profile: (contacts, counts, mean) over the upper diagonals of the matrices with a key in `valid`
    (None: all); cells equal to 0 and NaN cells are skipped, the float32 cells are added in fp64."""
    size = max(m.shape[0] for m in matrices.values())
    contacts, counts = np.zeros(size), np.zeros(size, np.int64)
    for key, m in matrices.items():
        if valid is not None and key not in valid:
            continue
        n = m.shape[0]
        i, j = np.triu_indices(n)
        x = m[i, j]
        keep = (x != 0) & ~np.isnan(x)
        contacts[:n] += np.bincount((j - i)[keep], weights=x[keep].astype(np.float64), minlength=n)
        counts[:n] += np.bincount((j - i)[keep], minlength=n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return contacts, counts, contacts / counts


def enrichment(matrix, mean):
    """_compute_enrichment_matrices for one chromosome: (double)C[i, j] / mean[|i - j|]."""
    k = np.arange(matrix.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return matrix.astype(np.float64) / np.asarray(mean)[np.abs(k[:, None] - k[None, :])]


def dense_valid(matrix):
    """A bin is valid when its row has a finite non-zero cell and no non-finite cell."""
    finite = np.isfinite(matrix)
    return (finite & (matrix != 0)).any(axis=1) & finite.all(axis=1)


def contact_pca(matrix, mask=None, k=3):
    """compute_contact_pca for the leading k components with np.linalg.svd: (pcs (n, k), variances (k), axes (k, n)).  The
    element of an axis of largest magnitude (lowest index on a tie) is positive."""
    matrix = np.asarray(matrix, np.float64)
    n = matrix.shape[0]
    mask = np.any(matrix != 0, axis=1) if mask is None else np.asarray(mask).astype(bool)
    m = int(mask.sum())
    if m < 2 or not 1 <= k <= m:
        raise ValueError(f"{k} components of {m} valid bins")
    x = matrix[mask][:, mask]
    xc = x - np.mean(x, axis=0)[None, :]
    u, s, vh = np.linalg.svd(xc)
    pcs, axes = np.full((n, k), np.nan), np.full((k, n), np.nan)
    for j in range(k):
        sign = 1.0 if vh[j, np.argmax(np.abs(vh[j]))] >= 0 else -1.0
        axes[j, mask] = sign * vh[j]
        pcs[mask, j] = sign * u[:, j] * np.sqrt(m - 1)
    return pcs, s[:k] ** 2, axes


# ---- the device

class HicSignals(Handle):
    """One device-side handle for one bin table.  max_pixels_per_launch: 0 = automatic (no integer result depends on it)."""

    _destroy = "gd_hic_destroy"

    def __init__(self, chrom_code, device=0, max_pixels_per_launch=0, path=None):
        super().__init__(load_hic_library(path))
        self._targets = []
        chrom = np.ascontiguousarray(chrom_code, dtype=np.int32)
        if chrom.ndim != 1:
            raise ValueError(f"chrom_code must be one-dimensional, got {chrom.shape}")
        self.n_bins = len(chrom)
        self._chrom = chrom
        self._run_of = np.concatenate([[0], np.cumsum(chrom[1:] != chrom[:-1])]) if len(chrom) else np.zeros(0, np.int64)
        self._check(self.dll.gd_hic_create(C.byref(_HicDesc(device, max_pixels_per_launch)), chrom.ctypes.data, self.n_bins, C.byref(self._h)))

    def _added(self, rc, target, what):
        self._check(rc)
        assert target.value == len(self._targets)
        self._targets.append(what)
        return target.value

    def add_band(self, W):
        t = C.c_int32(-1)
        return self._added(self.dll.gd_hic_add_band(self._h, W, C.byref(t)), t, ("band", W))

    def add_distance_profile(self, excluded=None, weights=None, size=None):
        ex = None if excluded is None else np.ascontiguousarray(np.asarray(excluded).astype(bool), dtype=np.uint8)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        for name, arr in (("excluded", ex), ("weights", w)):
            if arr is not None and arr.shape != (self.n_bins,):
                raise ValueError(f"{name} must have one value per bin ({self.n_bins}), got {arr.shape}")
        if size is None:
            raise ValueError("size is required: the largest number of bins of any chromosome (largest_chromosome)")
        t = C.c_int32(-1)
        rc = self.dll.gd_hic_add_distance_profile(self._h, None if ex is None else ex.ctypes.data, None if w is None else w.ctypes.data, size, C.byref(t))
        return self._added(rc, t, ("profile", size))

    def add_dense(self, weights=None):
        """One float32 (n, n) matrix per chromosome; weights=None is RAW."""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != (self.n_bins,):
            raise ValueError(f"weights must have one value per bin ({self.n_bins}), got {w.shape}")
        t = C.c_int32(-1)
        return self._added(self.dll.gd_hic_add_dense(self._h, None if w is None else w.ctypes.data, C.byref(t)), t, ("dense", 0))

    def dense_profile(self, target, excluded=None):
        """(contacts, counts, mean) per distance over the chromosomes whose first bin is not excluded; the mean stays in the
        target for the enrichment."""
        ex = None if excluded is None else np.ascontiguousarray(np.asarray(excluded).astype(bool), dtype=np.uint8)
        if ex is not None and ex.shape != (self.n_bins,):
            raise ValueError(f"excluded must have one value per bin ({self.n_bins}), got {ex.shape}")
        size = int(np.bincount(self._run_of).max())
        contacts, counts, mean = np.empty(size), np.empty(size, np.int64), np.empty(size)
        self._check(self.dll.gd_hic_dense_profile(self._h, target, None if ex is None else ex.ctypes.data, contacts.ctypes.data, counts.ctypes.data, mean.ctypes.data))
        return contacts, counts, mean

    def _size_of(self, code):
        return int((self._chrom == code).sum())

    def fetch_dense(self, target, code, which=DENSE_CONTACT):
        """The float32 contact matrix or the fp64 enrichment matrix of the chromosome with this code."""
        n = self._size_of(code)
        out = np.empty((n, n), np.float64 if which == DENSE_ENRICHMENT else np.float32)
        self._check(self.dll.gd_hic_fetch_dense(self._h, target, code, which, out.ctypes.data))
        return out

    def dense_valid(self, target):
        out = np.empty(self.n_bins, np.uint8)
        self._check(self.dll.gd_hic_dense_valid(self._h, target, out.ctypes.data))
        return out.astype(bool)

    @staticmethod
    def _mask(mask, n):
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.shape != (n,):
            raise ValueError(f"the mask must have one value per bin of the matrix ({n}), got {m.shape}")
        return m

    def dense_pca(self, target, code, which=DENSE_ENRICHMENT, mask=None, k=3):
        """(pcs (n, k), variances (k), axes (k, n), iterations) of a chromosome's matrix; mask=None is the reference's default."""
        n = self._size_of(code)
        m = self._mask(mask, n)
        kk = min(max(k, 1), HIC_MAX_PCS)      # the library reports a k outside its range
        pcs, var, axes, it = np.empty((n, kk)), np.empty(kk), np.empty((kk, n)), C.c_int32(0)
        self._check(self.dll.gd_hic_dense_pca(self._h, target, code, which, None if m is None else m.ctypes.data, k, pcs.ctypes.data, var.ctypes.data,
                                              axes.ctypes.data, C.byref(it)))
        return pcs, var, axes, it.value

    def pca_matrix(self, matrix, mask=None, k=3):
        """The same for any square fp64 matrix of the host (it need not be symmetric)."""
        a = np.ascontiguousarray(matrix, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError(f"a square matrix is required, got {a.shape}")
        n = a.shape[0]
        m = self._mask(mask, n)
        kk = min(max(k, 1), HIC_MAX_PCS)
        pcs, var, axes, it = np.empty((n, kk)), np.empty(kk), np.empty((kk, n)), C.c_int32(0)
        self._check(self.dll.gd_hic_pca_matrix(self._h, a.ctypes.data, n, None if m is None else m.ctypes.data, k, pcs.ctypes.data, var.ctypes.data, axes.ctypes.data,
                                               C.byref(it)))
        return pcs, var, axes, it.value

    def accumulate(self, bin1, bin2, count):
        """The three pixel columns; every target of the handle is updated in one pass."""
        b1, b2 = np.ascontiguousarray(bin1, dtype=np.int64), np.ascontiguousarray(bin2, dtype=np.int64)
        c = np.ascontiguousarray(count, dtype=np.int32)
        if not (b1.ndim == 1 and b1.shape == b2.shape == c.shape):
            raise ValueError(f"the pixel columns must be one-dimensional and of one length, got {b1.shape}, {b2.shape}, {c.shape}")
        self._check(self.dll.gd_hic_accumulate(self._h, b1.ctypes.data, b2.ctypes.data, c.ctypes.data, len(c)))

    def _width(self, target, kind):
        if not 0 <= target < len(self._targets) or self._targets[target][0] != kind:
            return 1      # the library reports the error
        return self._targets[target][1]

    def fetch_band(self, target):
        out = np.empty((self.n_bins, self._width(target, "band")), np.int64)
        self._check(self.dll.gd_hic_fetch_band(self._h, target, out.ctypes.data))
        return out

    def decay_insulation(self, target):
        W = max(self._width(target, "band"), 2)
        D, I = np.empty((self.n_bins, W - 1)), np.empty((self.n_bins, W - 2))
        self._check(self.dll.gd_hic_decay_insulation(self._h, target, D.ctypes.data, I.ctypes.data))
        return D, I

    def local_alpha(self, target):
        out = np.empty(self.n_bins)
        self._check(self.dll.gd_hic_local_alpha(self._h, target, out.ctypes.data))
        return out

    def fetch_profile(self, target):
        """(sum, n, mean): fp64, int64, fp64."""
        size = self._width(target, "profile")
        total, n, mean = np.empty(size), np.empty(size, np.int64), np.empty(size)
        self._check(self.dll.gd_hic_fetch_profile(self._h, target, total.ctypes.data, n.ctypes.data, mean.ctypes.data))
        return total, n, mean

    def fetch_profile_raw(self, target):
        """The exact int64 sums of a profile without weights."""
        out = np.empty(self._width(target, "profile"), np.int64)
        self._check(self.dll.gd_hic_fetch_profile_raw(self._h, target, out.ctypes.data))
        return out

    def reset(self):
        """Zeroes every accumulator; the targets stay."""
        self._check(self.dll.gd_hic_reset(self._h))

    def clear(self):
        """Removes every target."""
        self._check(self.dll.gd_hic_clear(self._h))
        self._targets = []

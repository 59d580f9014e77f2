"""The contact-map analyses on the device: ctypes binding of ``include/gdyn_cmap.h`` (exported by ``csrc/libgdyn.so``), the
accumulations of the reference's 5-sim-genome/src/{contact_map, gw_contact_matrix, nad_profile, power_law} over stored
``(i, j, count)`` rows.

    with ContactMaps(device=0) as cm:
        r = cm.add_region(beg, end)                          # contact_map: dense (end - beg)^2
        b = cm.add_binned(rebin, n_bins)                     # gw_contact_matrix
        p = cm.add_nucleolus_profile(beg, end, is_nucleolus) # nad_profile
        s = cm.add_separation_profile(chain_id, size)        # power_law
        for rows in maps:                                    # uint32 (M, 3)
            cm.accumulate(rows)                              # one pass over the rows for every target
        cm.finish(r)                                         # M + M^T, diagonal = max
        matrix, profile = cm.fetch(r), cm.fetch(s)

``region_matrix``, ``finish_region``, ``binned_matrix``, ``nucleolus_profile`` and ``separation_profile`` are the same sums in
numpy for users without a GPU; the device path never calls them.  ``rebin_map`` is determine_rebin_map and ``fit_power_law``
the weighted fit of power_law.py in closed form.  Sums are int32; a cell above 2**31 - 1 is outside the contract.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, Handle, load_library

CMAP_ABI_VERSION = 1     # GD_CMAP_ABI_VERSION of the include/gdyn_cmap.h this binding mirrors
CMAP_SYMBOLS = ["gd_cmap_abi_version", "gd_cmap_create", "gd_cmap_destroy", "gd_cmap_add_region", "gd_cmap_add_binned",
                "gd_cmap_add_nucleolus_profile", "gd_cmap_add_separation_profile", "gd_cmap_accumulate", "gd_cmap_finish",
                "gd_cmap_target_size", "gd_cmap_fetch", "gd_cmap_reset", "gd_cmap_clear", "gd_cmap_counters"]
FIT_RANGES = ((3, 20), (20, 100), (100, 1500))      # power_law.py: NEAR_RANGE, LONG_RANGE, FAR_RANGE


class _CmapDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_rows_per_launch", C.c_uint32)]


def load_cmap_library(path=None):
    """Loads libgdyn and checks the gd_cmap_* symbols and their ABI version."""
    d = load_library("cmap", CMAP_SYMBOLS, CMAP_ABI_VERSION, path)
    P32 = C.POINTER(C.c_int32)
    d.gd_cmap_create.argtypes = [C.POINTER(_CmapDesc), C.POINTER(C.c_void_p)]
    d.gd_cmap_destroy.argtypes = [C.c_void_p]
    d.gd_cmap_add_region.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, P32]
    d.gd_cmap_add_binned.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P32]
    d.gd_cmap_add_nucleolus_profile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, P32]
    d.gd_cmap_add_separation_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P32]
    d.gd_cmap_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    d.gd_cmap_finish.argtypes = [C.c_void_p, C.c_int32]
    d.gd_cmap_target_size.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    d.gd_cmap_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    d.gd_cmap_reset.argtypes = [C.c_void_p]
    d.gd_cmap_clear.argtypes = [C.c_void_p]
    d.gd_cmap_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    return d


# ---- numpy: the same sums on the host

def _rows(rows):
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] != 3:
        raise ValueError(f"rows must be (M, 3), got {r.shape}")
    return r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), r[:, 2].astype(np.int64)


def region_matrix(rows, beg, end, out=None):
    """collect_contact_matrix's accumulation (contact_map.py:76-90): adds the rows inside [beg, end)^2 into an int32 matrix."""
    i, j, v = _rows(rows)
    size = end - beg
    m = np.zeros((size, size), np.int32) if out is None else out
    s = (i >= beg) & (i < end) & (j >= beg) & (j < end)
    np.add.at(m, (i[s] - beg, j[s] - beg), v[s].astype(np.int32))
    return m


def finish_region(m):
    """contact_map.py:92-93: M + M^T with the diagonal set to the maximum of that sum."""
    m = m + m.T
    if m.size:
        np.fill_diagonal(m, m.max())
    return m


def binned_matrix(rows, rebin, n_bins, out=None):
    """collect_contacts (gw_contact_matrix/command.py:87-100)."""
    i, j, v = _rows(rows)
    rebin = np.asarray(rebin)
    m = np.zeros((n_bins, n_bins), np.int32) if out is None else out
    s = (i < len(rebin)) & (j < len(rebin))
    bi, bj, v = rebin[i[s]], rebin[j[s]], v[s].astype(np.int32)
    np.add.at(m, (bi, bj), v)
    np.add.at(m, (bj, bi), v)
    return m


def nucleolus_profile(rows, beg, end, is_nucleolus, out=None):
    """The true sums of nad_profile.py:88-94 (np.add.at; the reference's fancy-index += keeps one row per repeated index)."""
    i, j, v = _rows(rows)
    nuc = np.asarray(is_nucleolus).astype(bool)
    p = np.zeros(end - beg, np.int32) if out is None else out
    i_nuc, j_nuc = np.zeros(len(i), bool), np.zeros(len(j), bool)
    i_nuc[i < len(nuc)] = nuc[i[i < len(nuc)]]
    j_nuc[j < len(nuc)] = nuc[j[j < len(nuc)]]
    s = (i >= beg) & (i < end) & j_nuc
    np.add.at(p, i[s] - beg, v[s].astype(np.int32))
    s = (j >= beg) & (j < end) & i_nuc
    np.add.at(p, j[s] - beg, v[s].astype(np.int32))
    return p


def separation_profile(rows, chain_id, size, out=None):
    """collect_contact_profile (power_law.py:61-82); chain_id is -1 outside every chain."""
    i, j, v = _rows(rows)
    chain = np.asarray(chain_id)
    p = np.zeros(size, np.int32) if out is None else out
    s = (i < len(chain)) & (j < len(chain))
    i, j, v = i[s], j[s], v[s]
    s = (chain[i] == chain[j]) & (chain[i] != -1)
    d = np.abs(i[s] - j[s])
    if len(d) and d.max() >= size:
        raise ValueError(f"a separation of {d.max()} beads in a profile of {size} bins")
    np.add.at(p, d, v[s].astype(np.int32))
    return p


def chain_ids(chromosome_ranges, n_particles):
    """power_law.py:41-47 with -1 for the reference's NaN; returns (chain_id int32, longest chain)."""
    ids = np.full(n_particles, -1, np.int32)
    longest = 0
    for k, (beg, end) in enumerate(np.asarray(chromosome_ranges)):
        ids[beg:end] = k
        longest = max(longest, int(end - beg))
    return ids, longest


def rebin_map(chromosome_ranges, rate):
    """determine_rebin_map (gw_contact_matrix/command.py:103-126): (rebin_map int32, binned_ranges (K, 2) int32).  Beads
    between ranges map to bin 0; the number of bins is binned_ranges.max()."""
    src = np.asarray(chromosome_ranges)
    out = np.zeros(int(src.max()), np.int32)
    binned = []
    chrom_start = 0
    for start, end in src:
        bins = np.arange(end - start) // rate
        out[start:end] = bins + chrom_start
        chrom_end = chrom_start + int(bins[-1]) + 1
        binned.append((chrom_start, chrom_end))
        chrom_start = chrom_end
    return out, np.array(binned, np.int32)


def fit_power_law(x, y):
    """fit_power_law (power_law.py:85-92) without sklearn: the weighted least-squares line of log y on log x with weights
    1 / x over x > 0 and y > 0, in closed form in float64.  Returns (slope, exp(intercept))."""
    x, y = np.asarray(x), np.asarray(y)
    mask = (x > 0) & (y > 0)
    if not mask.any():
        raise ValueError("no point with x > 0 and y > 0 to fit")
    X, Y = np.log(x[mask].astype(np.float64)), np.log(y[mask].astype(np.float64))
    w = 1 / x[mask].astype(np.float64)
    xm, ym = np.average(X, weights=w), np.average(Y, weights=w)
    dx = X - xm
    var = np.sum(w * dx * dx)
    slope = np.sum(w * dx * (Y - ym)) / var if var > 0 else 0.0
    return float(slope), float(np.exp(ym - slope * xm))


def power_law_exponents(profile):
    """run_once's three exponents of a separation profile."""
    profile = np.asarray(profile)
    x = np.arange(len(profile))
    return tuple(fit_power_law(x[a:b], profile[a:b])[0] for a, b in FIT_RANGES)


# ---- the device

class ContactMaps(Handle):
    """One device-side handle.  max_rows_per_launch: 0 = automatic (no result depends on it)."""

    _destroy = "gd_cmap_destroy"

    def __init__(self, device=0, max_rows_per_launch=0, path=None):
        super().__init__(load_cmap_library(path))
        self._shapes = []
        self._check(self.dll.gd_cmap_create(C.byref(_CmapDesc(device, max_rows_per_launch)), C.byref(self._h)))

    def _added(self, rc, target, shape):
        self._check(rc)
        assert target.value == len(self._shapes)
        self._shapes.append(shape)
        return target.value

    def add_region(self, beg, end):
        t = C.c_int32(-1)
        return self._added(self.dll.gd_cmap_add_region(self._h, beg, end, C.byref(t)), t, (end - beg, end - beg))

    def add_binned(self, rebin, n_bins):
        m = np.ascontiguousarray(rebin, dtype=np.int32)
        t = C.c_int32(-1)
        return self._added(self.dll.gd_cmap_add_binned(self._h, m.ctypes.data, len(m), n_bins, C.byref(t)), t, (n_bins, n_bins))

    def add_nucleolus_profile(self, beg, end, is_nucleolus):
        nuc = np.ascontiguousarray(np.asarray(is_nucleolus).astype(bool), dtype=np.uint8)
        t = C.c_int32(-1)
        return self._added(self.dll.gd_cmap_add_nucleolus_profile(self._h, beg, end, nuc.ctypes.data, len(nuc), C.byref(t)), t, (end - beg,))

    def add_separation_profile(self, chain_id, size):
        ids = np.ascontiguousarray(chain_id, dtype=np.int32)
        t = C.c_int32(-1)
        return self._added(self.dll.gd_cmap_add_separation_profile(self._h, ids.ctypes.data, len(ids), size, C.byref(t)), t, (size,))

    def accumulate(self, rows):
        """rows: (M, 3) uint32 (i, j, count); every target of the handle is updated in one pass."""
        r = np.asarray(rows)
        if r.ndim != 2 or r.shape[1] != 3:
            raise ValueError(f"rows must be (M, 3), got {r.shape}")
        r = np.ascontiguousarray(r, dtype=np.uint32)
        self._check(self.dll.gd_cmap_accumulate(self._h, r.ctypes.data, len(r)))

    def finish(self, target):
        self._check(self.dll.gd_cmap_finish(self._h, target))

    def fetch(self, target):
        n = C.c_uint64()
        self._check(self.dll.gd_cmap_target_size(self._h, target, C.byref(n)))
        out = np.empty(self._shapes[target], np.int32)
        assert out.size == n.value
        self._check(self.dll.gd_cmap_fetch(self._h, target, out.ctypes.data))
        return out

    def reset(self):
        """Zeroes every accumulator; the targets stay."""
        self._check(self.dll.gd_cmap_reset(self._h))

    def clear(self):
        """Removes every target."""
        self._check(self.dll.gd_cmap_clear(self._h))
        self._shapes = []

    def counters(self):
        """(updates of binned targets the rows asked for, global atomics issued for them after the wave-level combine)."""
        out = (C.c_uint64 * 2)()
        self._check(self.dll.gd_cmap_counters(self._h, out))
        return int(out[0]), int(out[1])

"""Spatial correlation of bead displacements on the device, C(r, tau): ctypes binding of ``include/gdyn_dcorr.h`` (exported by
``csrc/libgdyn.so``).  The mean of D_i(tau) . D_j(tau) over pairs of beads a distance r apart at the origin frame, by pair
class (bead labels, same or different chain).  The reference has no such analysis: this is a capability beyond it.  The header
states the definitions; the sums are fixed-point integers (quantum 2^-scale_bits), exact and bit-identical from run to run,
for every ``max_frames_per_launch`` and on every code path.

    d = Dcorr(device=0)
    d.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    d.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    d.set_labels(types, n_labels=4)             # label[i] in [-1, K), K <= 8; -1: takes no part; None: one label of all beads
    d.set_chains(chain_of_bead)                 # splits every class into same chain / different chain; None: no split
    r = d.pairs(5, bin_width=0.02, max_distance=1.0, box=None)      # .count .sum (O, P, n_bins), .self_count .self_sum (O, K), .scale_bits
    c = d.correlation(5, bin_width=0.02, max_distance=1.0)          # .r (n_bins), .dot .normalised (P, n_bins)

Nothing is subtracted from the displacements: a caller who wants drift or rotation removed subtracts it from a host-fed history.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._binding import GdynError, HistoryHandle, _u32, box3, load_history_library

DCORR_ABI_VERSION = 1      # GD_DCORR_ABI_VERSION of the include/gdyn_dcorr.h this binding mirrors
DCORR_SYMBOLS = ["gd_dcorr_abi_version", "gd_dcorr_create", "gd_dcorr_destroy", "gd_dcorr_set_history", "gd_dcorr_set_history_live",
                 "gd_dcorr_set_labels", "gd_dcorr_set_chains", "gd_dcorr_bins", "gd_dcorr_classes", "gd_dcorr_origins", "gd_dcorr_pairs"]
LDS_BINS = 8192            # GD_DCORR_LDS_BINS: above this many cells P * n_bins the device adds every pair with global atomics
MAX_LABELS = 8             # GD_DCORR_MAX_LABELS
MAX_SCALE_BITS = 40        # GD_DCORR_MAX_SCALE_BITS
SCALE_UNIT = -1            # GD_DCORR_SCALE_UNIT: asks for scale_bits 0 proper (quantum 1), 0 itself being "automatic"

Pairs = namedtuple("Pairs", "count sum self_count self_sum scale_bits")
Correlation = namedtuple("Correlation", "r dot normalised count")


class _DcorrDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_launch", C.c_uint32)]


def load_dcorr_library(path=None):
    """Loads libgdyn and checks the gd_dcorr_* symbols and their ABI version."""
    d = load_history_library("dcorr", DCORR_SYMBOLS, DCORR_ABI_VERSION, path)
    d.gd_dcorr_create.argtypes = [C.POINTER(_DcorrDesc), C.POINTER(C.c_void_p)]
    d.gd_dcorr_destroy.argtypes = [C.c_void_p]
    d.gd_dcorr_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_dcorr_set_chains.argtypes = [C.c_void_p, C.c_void_p]
    d.gd_dcorr_bins.argtypes = [C.c_double, C.c_double]
    d.gd_dcorr_bins.restype = C.c_uint32
    d.gd_dcorr_classes.argtypes = [C.c_void_p]
    d.gd_dcorr_classes.restype = C.c_uint32
    d.gd_dcorr_origins.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    d.gd_dcorr_origins.restype = C.c_uint32
    d.gd_dcorr_pairs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                 C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return d


# ---- pure Python: the definitions of the header that a caller needs without a device

def n_bins(bin_width, max_distance):
    """ceil(max_distance / bin_width)."""
    return int(math.ceil(max_distance / bin_width))


def n_classes(n_labels, chains=False):
    """P: the unordered label pairs, doubled when chains split them."""
    return n_labels * (n_labels + 1) // 2 * (2 if chains else 1)


def class_index(a, b, n_labels, different_chain=None):
    """The class of a pair with labels a and b: lo K - lo (lo - 1) / 2 + (hi - lo); with chains 2 p + different_chain."""
    lo, hi = min(int(a), int(b)), max(int(a), int(b))
    p = lo * n_labels - lo * (lo - 1) // 2 + (hi - lo)
    return p if different_chain is None else 2 * p + int(bool(different_chain))


def class_labels(n_labels, chains=False):
    """[(a, b, different_chain or None)] in class order."""
    out = []
    for a in range(n_labels):
        for b in range(a, n_labels):
            out += [(a, b, False), (a, b, True)] if chains else [(a, b, None)]
    return out


def scale_is_legal(n_selected, largest_t2, scale_bits):
    """The overflow guard: max(n (n - 1) / 2, 1) (M 2^S + 1) < 2^62, exactly."""
    from fractions import Fraction
    m = float(largest_t2)
    if not (m >= 0.0) or math.isinf(m):
        return False
    return max(n_selected * (n_selected - 1) // 2, 1) * (Fraction(m) * Fraction(2) ** int(scale_bits) + 1) < (1 << 62)


def automatic_scale(n_selected, largest_t2):
    """The largest legal scale_bits in [0, 40], or None when there is none."""
    for s in range(MAX_SCALE_BITS, -1, -1):
        if scale_is_legal(n_selected, largest_t2, s):
            return s
    return None


def bin_edges(bin_width, max_distance):
    """n_bins + 1 edges k * bin_width, the last clipped at max_distance."""
    nb = n_bins(bin_width, max_distance)
    return np.minimum(np.arange(nb + 1, dtype=np.float64) * float(bin_width), float(max_distance))


def _total(table):
    """The sum over origins (axis 0) in Python integers."""
    t = np.asarray(table)
    out = np.zeros(t.shape[1:], object)
    for row in t:
        out = out + row.astype(object)
    return out


def totals(pairs):
    """What gd_dcorr writes for one lag: (count (P, n_bins) uint64, sum (P, n_bins) float64, self_count (K) uint64, self_sum (K)
    float64) of a Pairs, the sums taken over origins in integers and then divided by 2^scale_bits."""
    unit = float(1 << pairs.scale_bits)
    as_f64 = lambda t: np.array([float(v) for v in _total(t).ravel()], np.float64).reshape(t.shape[1:]) / unit
    as_u64 = lambda t: np.array([int(v) for v in _total(t).ravel()], np.uint64).reshape(t.shape[1:])
    return as_u64(pairs.count), as_f64(pairs.sum), as_u64(pairs.self_count), as_f64(pairs.self_sum)


def curves(count, total, self_count, self_sum, scale_bits, n_labels, chains, bin_width, max_distance):
    """Correlation of per-origin tables: sums over origins in Python integers, <D_i . D_j>(r) = sum / 2^S / count per class and
    the same over sqrt(<|D|^2>_a <|D|^2>_b) of the labels involved; NaN where a count is zero."""
    n, s = _total(count), _total(total)
    sn, ss = _total(self_count), _total(self_sum)
    unit = 1 << scale_bits
    dot = np.full(n.shape, np.nan)
    for idx in np.ndindex(*n.shape):
        if n[idx]:
            dot[idx] = float(s[idx]) / unit / float(n[idx])      # the header's order: sum / 2^S, then / count
    msd = np.array([float(ss[l]) / unit / float(sn[l]) if sn[l] else np.nan for l in range(n_labels)])
    norm = np.array([math.sqrt(msd[a] * msd[b]) if msd[a] >= 0 and msd[b] >= 0 else np.nan for a, b, _ in class_labels(n_labels, chains)])
    with np.errstate(divide="ignore", invalid="ignore"):
        normalised = dot / norm[:, None]
    edges = bin_edges(bin_width, max_distance)
    return Correlation(0.5 * (edges[:-1] + edges[1:]), dot, normalised, np.array(n, dtype=np.uint64))


class Dcorr(HistoryHandle):
    """One device-side history with its bead labels and chains.  max_frames_per_launch: 0 = automatic (no result depends on it)."""

    _prefix = "dcorr"
    _destroy = "gd_dcorr_destroy"

    def __init__(self, device=0, max_frames_per_launch=0, path=None):
        super().__init__(load_dcorr_library(path))
        self._check(self.dll.gd_dcorr_create(C.byref(_DcorrDesc(device, max_frames_per_launch)), C.byref(self._h)))
        self.n_labels = 1
        self.chains = False

    def _beads_changed(self, n_beads):      # the library drops labels and chains of another N
        self.n_labels, self.chains = 1, False

    def set_labels(self, label, n_labels=None):
        """label: (N,) integers in [-1, n_labels), -1 for a bead that takes no part; None: one label of all beads.
        n_labels=None: the largest label + 1."""
        self.n_labels, _ = self._set_labels(label, n_labels)

    def set_chains(self, chain):
        """chain: (N,) non-negative integers below 2^32, the chain of every bead; None: classes are not split by chain."""
        if chain is None:
            self._check(self.dll.gd_dcorr_set_chains(self._h, None))
            self.chains = False
            return
        c = np.asarray(chain).reshape(-1)
        if self.shape is not None and len(c) != self.shape[1]:
            raise ValueError(f"chain must have one entry per bead ({self.shape[1]}), got {len(c)}")
        c = _u32(c, "chain ids")
        self._check(self.dll.gd_dcorr_set_chains(self._h, c.ctypes.data))
        self.chains = True

    @property
    def n_classes(self):
        return int(self.dll.gd_dcorr_classes(self._h))

    def pairs(self, lag, bin_width, max_distance, box=None, scale_bits=0, first_origin=0, n_origins=0, origin_stride=1):
        """The tables of one lag: Pairs(count (O, P, n_bins) uint64, sum (O, P, n_bins) int64, self_count (O, K) uint64,
        self_sum (O, K) int64, scale_bits).  box: a period or three, None: open.  scale_bits 0: automatic, SCALE_UNIT: quantum 1.
        Origins first_origin + k origin_stride; n_origins 0: all that fit."""
        box_at, _keep = box3(box)
        nb = int(self.dll.gd_dcorr_bins(float(bin_width), float(max_distance)))
        O = int(self.dll.gd_dcorr_origins(self._h, int(lag), int(first_origin), int(n_origins), int(origin_stride)))
        P, K = self.n_classes, self.n_labels
        count, total = np.zeros((O, P, max(nb, 1)), np.uint64), np.zeros((O, P, max(nb, 1)), np.int64)
        self_count, self_sum = np.zeros((O, K), np.uint64), np.zeros((O, K), np.int64)
        used = C.c_int32(0)
        self._check(self.dll.gd_dcorr_pairs(self._h, int(lag), int(first_origin), int(n_origins), int(origin_stride),
                                            box_at, float(bin_width), float(max_distance), int(scale_bits), C.byref(used),
                                            count.ctypes.data, total.ctypes.data, self_count.ctypes.data, self_sum.ctypes.data))
        return Pairs(count[:, :, :nb], total[:, :, :nb], self_count, self_sum, int(used.value))

    def correlation(self, lag, bin_width, max_distance, box=None, scale_bits=0, first_origin=0, n_origins=0, origin_stride=1):
        """Correlation(r (n_bins) bin centres, dot (P, n_bins) = <D_i . D_j>(r), normalised (P, n_bins) = dot over the geometric mean of
        <|D|^2> of the two labels, count (P, n_bins)), over all origins of the call; NaN where no pair was counted."""
        p = self.pairs(lag, bin_width, max_distance, box, scale_bits, first_origin, n_origins, origin_stride)
        return curves(p.count, p.sum, p.self_count, p.self_sum, p.scale_bits, self.n_labels, self.chains, bin_width, max_distance)

"""Displacement covariance maps of a trajectory history on the device: ctypes binding of ``include/gdyn_dcov.h`` (exported by
``csrc/libgdyn.so``).  For every pair of bins of beads, the sum behind the covariance of their displacements over a lag ("which loci
move together"), or with lag 0 of their positions about the time mean (the essential-dynamics matrix).  The reference has neither:
this is a capability beyond it.  The header states the definitions; the map is the fp64 product of the row matrix with its
transpose on the matrix cores, bit-identical from run to run, for every ``columns_per_stage``, for a cell whatever rectangle it is
asked in, and between ``M[I, J]`` and ``M[J, I]``.

    d = Dcov(device=0)
    d.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    d.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    d.set_bins(Dcov.bins_from_chains(chains, 10))      # (B, 2) bead ranges; none set: every bead is its own bin
    d.prepare(lag=5, remove_drift=True)         # the rows A (B, 3 origins); lag=0: positions about their time mean
    d.rows()                                    # (B, columns) float64: every bin's displacement series
    m = d.map()                                 # the whole map; rows=(first, count), cols=(first, count) for a rectangle
    m["sum"], m["count"], m["diag_rows"], m["diag_cols"]      # (R, C) float64, (R, C) uint64, (R,) and (C,) float64
    Dcov.mean(m), Dcov.correlation(m)           # sum / count; sum / sqrt(diag_rows x diag_cols), NaN where a diagonal is 0
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, HistoryHandle, _ratio, load_history_library
from .dmap import Dmap

DCOV_ABI_VERSION = 1      # GD_DCOV_ABI_VERSION of the include/gdyn_dcov.h this binding mirrors
DCOV_PIECE_BEADS = 32     # GD_DCOV_PIECE_BEADS
DCOV_COLUMN_RANGE = 768   # GD_DCOV_COLUMN_RANGE
DCOV_SYMBOLS = ["gd_dcov_abi_version", "gd_dcov_create", "gd_dcov_destroy", "gd_dcov_set_history", "gd_dcov_set_history_live",
                "gd_dcov_set_bins", "gd_dcov_prepare", "gd_dcov_columns", "gd_dcov_last_times", "gd_dcov_rows", "gd_dcov_map"]


class _DcovDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("columns_per_stage", C.c_uint32)]


def load_dcov_library(path=None):
    """Loads libgdyn and checks the gd_dcov_* symbols and their ABI version."""
    d = load_history_library("dcov", DCOV_SYMBOLS, DCOV_ABI_VERSION, path)
    d.gd_dcov_create.argtypes = [C.POINTER(_DcovDesc), C.POINTER(C.c_void_p)]
    d.gd_dcov_destroy.argtypes = [C.c_void_p]
    d.gd_dcov_set_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_dcov_prepare.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_int]
    d.gd_dcov_columns.argtypes = [C.c_void_p]
    d.gd_dcov_columns.restype = C.c_uint32
    d.gd_dcov_last_times.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    d.gd_dcov_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    d.gd_dcov_map.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 4
    return d


class Dcov(HistoryHandle):
    """One device-side history with its bins and the prepared rows.  columns_per_stage: 0 = automatic (no result depends on it)."""

    _prefix = "dcov"
    _destroy = "gd_dcov_destroy"
    bins_from_chains = staticmethod(Dmap.bins_from_chains)      # the same rule, the same code

    def __init__(self, device=0, columns_per_stage=0, path=None):
        super().__init__(load_dcov_library(path))
        self._check(self.dll.gd_dcov_create(C.byref(_DcovDesc(device, columns_per_stage)), C.byref(self._h)))
        self.n_bins = 0            # B: N without bins of the caller's

    def _beads_changed(self, n_beads):      # the library drops the bins of another N
        self.n_bins = n_beads

    @property
    def columns(self):
        """The columns of the preparation, 3 per origin; 0 without one."""
        return int(self.dll.gd_dcov_columns(self._h))

    def last_times(self):
        """Device milliseconds of the last prepare (stage 1) and of the product and the merge kernel of the last map."""
        return self._last_times("stage1_ms", "product_ms", "merge_ms")

    def set_bins(self, ranges):
        """ranges: (B, 2) [start, end) bead ranges, ascending, non-empty and not overlapping; None: every bead is its own bin.
        The preparation is dropped."""
        every_bead = range((self.shape or (0, 0))[1])
        self.n_bins = len(self._set_ranges(self.dll.gd_dcov_set_bins, ranges, "bin ranges", "no bins (None makes every bead its own bin)", every_bead))

    def prepare(self, lag, first=0, stride=1, count=0, remove_drift=False):
        """Builds the rows on the device.  lag >= 1: the displacements over ``lag`` frames from the origins first + k stride, k < count
        (0: all that fit); lag == 0: the positions of those frames about their mean.  Returns the number of columns, 3 per origin."""
        if min(int(lag), int(first), int(stride), int(count)) < 0:
            raise ValueError("negative lag, frame, stride or count")
        self._check(self.dll.gd_dcov_prepare(self._h, int(lag), int(first), int(stride), int(count), int(bool(remove_drift))))
        return self.columns

    def rows(self, first_bin=0, n_bins=None):
        """The rows [first_bin, first_bin + n_bins) of the prepared matrix (None: up to the last bin): (n_bins, columns) float64."""
        n = max(self.n_bins - int(first_bin), 0) if n_bins is None else int(n_bins)
        if min(int(first_bin), n) < 0:
            raise ValueError("negative bin range")
        out = np.zeros((n, self.columns), np.float64)
        self._check(self.dll.gd_dcov_rows(self._h, int(first_bin), n, out.ctypes.data))
        return out

    def map(self, rows=None, cols=None):
        """The cells rows x cols of the map, each (first bin, number of bins) or None for all bins.  A dict: ``sum`` (R, C) float64,
        ``count`` (R, C) uint64, ``diag_rows`` (R,) and ``diag_cols`` (C,) float64: the cells (I, I) of the rows' and the columns' bins."""
        r0, nr = (0, self.n_bins) if rows is None else (int(rows[0]), int(rows[1]))
        c0, nc = (0, self.n_bins) if cols is None else (int(cols[0]), int(cols[1]))
        if min(r0, nr, c0, nc) < 0:
            raise ValueError("negative bin range")
        total, count = np.zeros((nr, nc), np.float64), np.zeros((nr, nc), np.uint64)
        diag_rows, diag_cols = np.zeros(nr, np.float64), np.zeros(nc, np.float64)
        self._check(self.dll.gd_dcov_map(self._h, r0, nr, c0, nc, total.ctypes.data, count.ctypes.data, diag_rows.ctypes.data, diag_cols.ctypes.data))
        return {"sum": total, "count": count, "diag_rows": diag_rows, "diag_cols": diag_cols}

    @staticmethod
    def mean(m):
        """Mean covariance sum / count, NaN where count is 0."""
        return _ratio(m["sum"], m["count"])

    @staticmethod
    def correlation(m):
        """sum / sqrt(diag_rows x diag_cols): the normalised correlation of the rectangle, NaN where a diagonal is 0."""
        norm = np.sqrt(np.outer(m["diag_rows"], m["diag_cols"]))
        out = np.full(m["sum"].shape, np.nan)
        np.divide(m["sum"], norm, out=out, where=norm > 0)
        return out

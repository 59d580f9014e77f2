"""Distance and contact-frequency maps of a trajectory history on the device: ctypes binding of ``include/gdyn_dmap.h`` (exported
by ``csrc/libgdyn.so``).  For every pair of bins of beads, the sums behind the mean spatial distance (what chromatin tracing and
FISH report), the rms distance and the contact frequency at thresholds chosen after the run.  The reference has neither: this is
a capability beyond it.  The header states the definitions; the sums are fp64, bit-identical from run to run, for every
``max_frames_per_stage``, for a cell whatever rectangle it is asked in, and between ``M[I, J]`` and ``M[J, I]``.

    d = Dmap(device=0)
    d.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    d.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    d.set_bins(Dmap.bins_from_chains(chains, 10))      # (B, 2) bead ranges; none set: every bead is its own bin
    m = d.map(thresholds=(1.5, 2.5))            # the whole map; rows=(first, count), cols=(first, count) for a rectangle
    m["sum1"], m["sum2"], m["hits"], m["count"] # (R, C) float64, (R, C) float64, (T, R, C) uint64, (R, C) uint64
    Dmap.mean(m), Dmap.rms(m), Dmap.frequency(m)       # sum1 / count, sqrt(sum2 / count), hits / count; NaN where count is 0
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, HistoryHandle, _ratio, load_history_library

DMAP_ABI_VERSION = 1      # GD_DMAP_ABI_VERSION of the include/gdyn_dmap.h this binding mirrors
DMAP_MAX_THRESHOLDS = 4   # GD_DMAP_MAX_THRESHOLDS
DMAP_FRAME_RANGE = 64     # GD_DMAP_FRAME_RANGE
DMAP_PIECE_BEADS = 32     # GD_DMAP_PIECE_BEADS
DMAP_SYMBOLS = ["gd_dmap_abi_version", "gd_dmap_create", "gd_dmap_destroy", "gd_dmap_set_history", "gd_dmap_set_history_live",
                "gd_dmap_set_bins", "gd_dmap_map"]


class _DmapDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_stage", C.c_uint32)]


def load_dmap_library(path=None):
    """Loads libgdyn and checks the gd_dmap_* symbols and their ABI version."""
    d = load_history_library("dmap", DMAP_SYMBOLS, DMAP_ABI_VERSION, path)
    d.gd_dmap_create.argtypes = [C.POINTER(_DmapDesc), C.POINTER(C.c_void_p)]
    d.gd_dmap_destroy.argtypes = [C.c_void_p]
    d.gd_dmap_set_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_dmap_map.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    return d


class Dmap(HistoryHandle):
    """One device-side history with its bins.  max_frames_per_stage: 0 = automatic (no result depends on it)."""

    _prefix = "dmap"
    _destroy = "gd_dmap_destroy"

    def __init__(self, device=0, max_frames_per_stage=0, path=None):
        super().__init__(load_dmap_library(path))
        self._check(self.dll.gd_dmap_create(C.byref(_DmapDesc(device, max_frames_per_stage)), C.byref(self._h)))
        self.n_bins = 0            # B: N without bins of the caller's

    def _beads_changed(self, n_beads):      # the library drops the bins of another N
        self.n_bins = n_beads

    def set_bins(self, ranges):
        """ranges: (B, 2) [start, end) bead ranges, ascending, non-empty and not overlapping; None: every bead is its own bin."""
        every_bead = range((self.shape or (0, 0))[1])
        self.n_bins = len(self._set_ranges(self.dll.gd_dmap_set_bins, ranges, "bin ranges", "no bins (None makes every bead its own bin)", every_bead))

    @staticmethod
    def bins_from_chains(chain_ranges, rate):
        """``rate`` consecutive beads per bin within each chain [start, end): the last bin of a chain is shorter, no bin spans two
        chains, an empty chain has no bin.  (B, 2) uint32."""
        rate = int(rate)
        if rate < 1:
            raise ValueError("rate must be at least 1")
        out = [(a, min(a + rate, int(end))) for start, end in np.asarray(chain_ranges).reshape(-1, 2) for a in range(int(start), int(end), rate)]
        return np.array(out, dtype=np.uint32).reshape(-1, 2)

    def map(self, rows=None, cols=None, first_frame=0, n_frames=None, box=None, thresholds=(), want_sum1=True, want_sum2=True):
        """The cells rows x cols of the map, each (first bin, number of bins) or None for all bins, over the frames
        [first_frame, first_frame + n_frames) (None: up to the last).  A dict: ``sum1`` and ``sum2`` (R, C) float64 (None when not
        wanted), ``hits`` (T, R, C) uint64, ``count`` (R, C) uint64, ``thresholds`` (T,) float64."""
        r0, nr = (0, self.n_bins) if rows is None else (int(rows[0]), int(rows[1]))
        c0, nc = (0, self.n_bins) if cols is None else (int(cols[0]), int(cols[1]))
        if n_frames is None:
            n_frames = max((self.shape or (0, 0))[0] - int(first_frame), 0)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        b = None if box is None else np.ascontiguousarray(box, dtype=np.float64).reshape(3)
        if min(r0, nr, c0, nc, int(first_frame), int(n_frames)) < 0:
            raise ValueError("negative bin or frame range")
        shape = (max(nr, 0), max(nc, 0))
        sum1 = np.zeros(shape, np.float64) if want_sum1 else None
        sum2 = np.zeros(shape, np.float64) if want_sum2 else None
        hits = np.zeros((len(thr),) + shape, np.uint64)
        count = np.zeros(shape, np.uint64)
        self._check(self.dll.gd_dmap_map(self._h, r0, nr, c0, nc, int(first_frame), int(n_frames), None if b is None else b.ctypes.data,
                                         thr.ctypes.data if len(thr) else None, len(thr), None if sum1 is None else sum1.ctypes.data,
                                         None if sum2 is None else sum2.ctypes.data, hits.ctypes.data if len(thr) else None, count.ctypes.data))
        return {"sum1": sum1, "sum2": sum2, "hits": hits, "count": count, "thresholds": thr}

    @staticmethod
    def mean(m):
        """Mean distance sum1 / count, NaN where count is 0."""
        return _ratio(m["sum1"], m["count"])

    @staticmethod
    def rms(m):
        """Root mean squared distance sqrt(sum2 / count), NaN where count is 0."""
        return np.sqrt(_ratio(m["sum2"], m["count"]))

    @staticmethod
    def frequency(m):
        """Contact frequency hits / count per threshold (T, R, C), NaN where count is 0."""
        return _ratio(m["hits"].astype(np.float64), m["count"][None])

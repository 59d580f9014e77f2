"""Lag statistics of a trajectory history on the device: ctypes binding of ``include/gdyn_msd.h`` (exported by
``csrc/libgdyn.so``).  The time-averaged mean squared displacement of beads against lag time, MSD(tau), by bead group, and the
mean squared spatial distance of beads against their separation along a chain, R2(s), by chain.  The reference has neither:
this is a capability beyond it.  The header states the definitions; the sums are fp64, bit-identical from run to run, for
every ``max_items_per_tile`` and for a lag whatever else the call lists.

    m = Msd(device=0)
    m.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    m.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    m.set_groups(types, n_groups=4)             # group[i] in [-1, G); None: one group of all beads
    sum2, count = m.time([1, 2, 5, 10])         # (G, L) float64 and uint64
    msd = m.msd([1, 2, 5, 10])                  # sum2 / count, NaN where count is 0
    m2 = m.time_per_bead(5)                     # (N,) the mobility profile along the genome
    m.set_chains([[0, 300], [300, 700]])
    sum2, count = m.chain([1, 2, 4, 8], first_frame=0, n_frames=None)      # (C, S)
    r2 = m.r2([1, 2, 4, 8])
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, HistoryHandle, _ratio, _u32, load_history_library

MSD_ABI_VERSION = 1       # GD_MSD_ABI_VERSION of the include/gdyn_msd.h this binding mirrors
MSD_SYMBOLS = ["gd_msd_abi_version", "gd_msd_create", "gd_msd_destroy", "gd_msd_set_history", "gd_msd_set_history_live",
               "gd_msd_set_groups", "gd_msd_set_chains", "gd_msd_time", "gd_msd_time_per_bead", "gd_msd_chain"]


class _MsdDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_items_per_tile", C.c_uint32)]


def load_msd_library(path=None):
    """Loads libgdyn and checks the gd_msd_* symbols and their ABI version."""
    d = load_history_library("msd", MSD_SYMBOLS, MSD_ABI_VERSION, path)
    d.gd_msd_create.argtypes = [C.POINTER(_MsdDesc), C.POINTER(C.c_void_p)]
    d.gd_msd_destroy.argtypes = [C.c_void_p]
    d.gd_msd_set_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_msd_set_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_msd_time.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    d.gd_msd_time_per_bead.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    d.gd_msd_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return d


class Msd(HistoryHandle):
    """One device-side history with its bead groups and chains.  max_items_per_tile: 0 = automatic (no result depends on it)."""

    _prefix = "msd"
    _destroy = "gd_msd_destroy"

    def __init__(self, device=0, max_items_per_tile=0, path=None):
        super().__init__(load_msd_library(path))
        self._check(self.dll.gd_msd_create(C.byref(_MsdDesc(device, max_items_per_tile)), C.byref(self._h)))
        self.n_groups = 1
        self.n_chains = 0

    def _beads_changed(self, n_beads):      # the library drops groups and chains of another N
        self.n_groups, self.n_chains = 1, 0

    def set_groups(self, group, n_groups=None):
        """group: (N,) integers in [-1, n_groups), -1 for a bead in no group; None: one group of all beads.
        n_groups=None: the largest id + 1."""
        if group is None:
            self._check(self.dll.gd_msd_set_groups(self._h, None, 1))
            self.n_groups = 1
            return
        g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if self.shape is not None and len(g) != self.shape[1]:
            raise ValueError(f"group must have one entry per bead ({self.shape[1]}), got {len(g)}")
        G = int(n_groups) if n_groups is not None else max(int(g.max()) + 1, 1) if len(g) else 1
        self._check(self.dll.gd_msd_set_groups(self._h, g.ctypes.data, G))
        self.n_groups = G

    def set_chains(self, ranges):
        """ranges: (C, 2) [start, end) bead ranges, ascending and not overlapping."""
        r = _u32(ranges, "chain ranges").reshape(-1, 2)
        self._check(self.dll.gd_msd_set_chains(self._h, r.ctypes.data if len(r) else None, len(r)))
        self.n_chains = len(r)

    def _sums(self, call, rows, lags, want_sum4, *window):
        l = _u32(lags, "lags").reshape(-1)
        sum2 = np.zeros((rows, len(l)), np.float64)
        sum4 = np.zeros((rows, len(l)), np.float64) if want_sum4 else None
        count = np.zeros((rows, len(l)), np.uint64)
        self._check(call(self._h, l.ctypes.data, len(l), *window, sum2.ctypes.data, None if sum4 is None else sum4.ctypes.data,
                         count.ctypes.data))
        return (sum2, sum4, count) if want_sum4 else (sum2, count)

    def time(self, lags, want_sum4=False):
        """(sum2, [sum4,] count), each (G, len(lags)): the sums of t2 (and of t2^2) over the origins and the beads of each group."""
        return self._sums(self.dll.gd_msd_time, self.n_groups, lags, want_sum4)

    def time_per_bead(self, lag, want_m4=False):
        """m2[:, lag] as (N,) float64 (and m4 with want_m4)."""
        N = (self.shape or (0, 0))[1]
        m2 = np.zeros(N, np.float64)
        m4 = np.zeros(N, np.float64) if want_m4 else None
        self._check(self.dll.gd_msd_time_per_bead(self._h, int(lag), m2.ctypes.data, None if m4 is None else m4.ctypes.data))
        return (m2, m4) if want_m4 else m2

    def chain(self, seps, first_frame=0, n_frames=None, want_sum4=False):
        """(sum2, [sum4,] count), each (C, len(seps)), over the frames [first_frame, first_frame + n_frames); None: up to the last."""
        if n_frames is None:
            n_frames = max((self.shape or (0, 0))[0] - int(first_frame), 0)
        return self._sums(self.dll.gd_msd_chain, self.n_chains, seps, want_sum4, int(first_frame), int(n_frames))

    def msd(self, lags):
        """sum2 / count of time(lags): (G, len(lags)), NaN where count is 0."""
        sum2, count = self.time(lags)
        return _ratio(sum2, count)

    def r2(self, seps, first_frame=0, n_frames=None):
        """sum2 / count of chain(seps, ...): (C, len(seps)), NaN where count is 0."""
        sum2, count = self.chain(seps, first_frame, n_frames)
        return _ratio(sum2, count)

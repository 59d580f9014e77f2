"""Gyration tensors and compaction profiles of a trajectory history on the device: ctypes binding of ``include/gdyn_gyr.h`` (exported by
``csrc/libgdyn.so``).  Per frame, the centre and the six centred second-moment sums of every segment of beads (a chromosome territory:
its radius, semi-axes, asphericity and orientation), and Rg^2 of a sliding window of ``w`` beads along the chains (the compaction
profile that chromatin tracing reports).  The reference has neither: this is a capability beyond it.  The header states the
definitions and the order of every sum; the results are bit-identical from run to run, for every ``beads_per_tile`` and
``frames_per_launch``, and equal ``tests/gyr_restatement.py`` byte for byte.

    g = Gyration(device=0)
    g.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    g.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    g.set_segments(Gyration.segments_from_chains(chains, 10))      # (S, 2) bead ranges; none set: one segment of all beads
    g.set_chains(chains)                        # (C, 2) bead ranges a window must lie in; none set: one chain of all beads
    t = g.tensors(first=0, stride=1, count=0)   # centre_sum, centre (K, S, 3), moment (K, S, 6: xx yy zz xy xz yz), n (S,)
    d = Gyration.descriptors(t)                 # rg2, eigenvalues, axes, asphericity, acylindricity, anisotropy (host, numpy.linalg.eigh)
    p = g.profile([10, 100, 1000])              # windows (W,), sum, sum_sq (W, N) float64, count (W, N) uint64, by first bead
    Gyration.mean(p), Gyration.fluctuation(p), Gyration.centred(p)
    Gyration.scaling(p, labels)                 # mean Rg^2(w) by bead class
    g.profile_frames(100)                       # (K, N) float64: Rg^2 of the window at every selected frame, the kymograph
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, HistoryHandle, _ratio, _u32, load_history_library
from .dmap import Dmap

GYR_ABI_VERSION = 1       # GD_GYR_ABI_VERSION of the include/gdyn_gyr.h this binding mirrors
GYR_PIECE_BEADS = 32      # GD_GYR_PIECE_BEADS
GYR_FRAME_RANGE = 64      # GD_GYR_FRAME_RANGE
GYR_MAX_WINDOWS = 8       # GD_GYR_MAX_WINDOWS
GYR_MAX_WINDOW = 2048     # GD_GYR_MAX_WINDOW
GYR_SYMBOLS = ["gd_gyr_abi_version", "gd_gyr_create", "gd_gyr_destroy", "gd_gyr_set_history", "gd_gyr_set_history_live", "gd_gyr_set_segments",
               "gd_gyr_set_chains", "gd_gyr_tensors", "gd_gyr_profile", "gd_gyr_profile_frames", "gd_gyr_last_times"]


class _GyrDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("beads_per_tile", C.c_uint32), ("frames_per_launch", C.c_uint32)]


def load_gyr_library(path=None):
    """Loads libgdyn and checks the gd_gyr_* symbols and their ABI version."""
    d = load_history_library("gyr", GYR_SYMBOLS, GYR_ABI_VERSION, path)
    d.gd_gyr_create.argtypes = [C.POINTER(_GyrDesc), C.POINTER(C.c_void_p)]
    d.gd_gyr_destroy.argtypes = [C.c_void_p]
    d.gd_gyr_set_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_gyr_set_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_gyr_tensors.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] * 3
    d.gd_gyr_profile.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 3
    d.gd_gyr_profile_frames.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p]
    d.gd_gyr_last_times.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    return d


def _selection(first, stride, count):
    if min(int(first), int(stride), int(count)) < 0:
        raise ValueError("negative frame, stride or count")
    return int(first), int(stride), int(count)


class Gyration(HistoryHandle):
    """One device-side history with its segments and chains.  beads_per_tile, frames_per_launch: 0 = automatic (no result depends on them)."""

    _prefix = "gyr"
    _destroy = "gd_gyr_destroy"
    segments_from_chains = staticmethod(Dmap.bins_from_chains)      # the same rule, the same code

    def __init__(self, device=0, beads_per_tile=0, frames_per_launch=0, path=None):
        super().__init__(load_gyr_library(path))
        self._check(self.dll.gd_gyr_create(C.byref(_GyrDesc(device, beads_per_tile, frames_per_launch)), C.byref(self._h)))
        self.segments = None       # (S, 2) uint32; None before a history
        self.chains = None         # (C, 2) uint32

    def _beads_changed(self, n_beads):      # the library drops the ranges of another N
        self.segments = np.array([[0, n_beads]], np.uint32)
        self.chains = np.array([[0, n_beads]], np.uint32)

    def last_times(self):
        """Device milliseconds of the last tensors call, and of the window kernel and the merge kernel of the last profile call."""
        return self._last_times("tensors_ms", "windows_ms", "merge_ms")

    def _bead_ranges(self, call, ranges, what):
        whole = np.array([[0, (self.shape or (0, 0))[1]]], np.uint32)
        return self._set_ranges(call, ranges, what, f"no {what} (None makes one range of all beads)", whole).copy()

    def set_segments(self, ranges):
        """ranges: (S, 2) [start, end) bead ranges, ascending, non-empty and not overlapping; None: one segment of all beads."""
        self.segments = self._bead_ranges(self.dll.gd_gyr_set_segments, ranges, "segment ranges")

    def set_chains(self, ranges):
        """ranges: (C, 2) [start, end) bead ranges, ascending and not overlapping, empty ones allowed; None: one chain of all beads."""
        self.chains = self._bead_ranges(self.dll.gd_gyr_set_chains, ranges, "chain ranges")

    def selected(self, first=0, stride=1, count=0):
        """The frames a call with this selection takes (count 0: all from ``first`` on, ``stride`` apart)."""
        frames = range(int(first), (self.shape or (0, 0))[0], max(int(stride), 1))
        return np.array(frames[:int(count)] if count else frames, dtype=np.int64)

    def tensors(self, first=0, stride=1, count=0):
        """Per selected frame and segment: ``centre_sum`` and ``centre`` (K, S, 3), ``moment`` (K, S, 6), the centred second-moment
        sums xx yy zz xy xz yz, and ``n`` (S,), the beads of the segments.  Sums: the gyration tensor is moment / n (descriptors)."""
        first, stride, count = _selection(first, stride, count)
        K, S = count or len(self.selected(first, stride)), 0 if self.segments is None else len(self.segments)
        out = {"centre_sum": np.zeros((K, S, 3)), "centre": np.zeros((K, S, 3)), "moment": np.zeros((K, S, 6))}
        self._check(self.dll.gd_gyr_tensors(self._h, first, stride, count, *[out[k].ctypes.data for k in ("centre_sum", "centre", "moment")]))
        out["n"] = (self.segments[:, 1] - self.segments[:, 0]).astype(np.int64)
        return out

    def profile(self, windows, first=0, stride=1, count=0):
        """Rg^2 of the windows [i, i + w) summed over the selected frames, for up to 8 window sizes w: ``sum`` and ``sum_sq`` (W, N)
        float64, ``count`` (W, N) uint64 (the frames where the window lies inside one chain, else 0), ``windows`` (W,), indexed by the
        window's first bead."""
        first, stride, count = _selection(first, stride, count)
        w = _u32(windows, "window sizes").reshape(-1)
        N = (self.shape or (0, 0))[1]
        out = {"windows": w.copy(), "sum": np.zeros((len(w), N)), "sum_sq": np.zeros((len(w), N)), "count": np.zeros((len(w), N), np.uint64)}
        self._check(self.dll.gd_gyr_profile(self._h, w.ctypes.data, len(w), first, stride, count, out["sum"].ctypes.data, out["sum_sq"].ctypes.data,
                                            out["count"].ctypes.data))
        return out

    def profile_frames(self, window, first=0, stride=1, count=0):
        """(K, N) float64: Rg^2 of the window [i, i + window) at every selected frame, 0 where it does not lie inside one chain."""
        first, stride, count = _selection(first, stride, count)
        if int(window) < 0:
            raise ValueError("negative window")
        K, N = count or len(self.selected(first, stride)), (self.shape or (0, 0))[1]
        out = np.zeros((K, N))
        self._check(self.dll.gd_gyr_profile_frames(self._h, int(window), first, stride, count, out.ctypes.data))
        return out

    # ---- on the host

    @staticmethod
    def descriptors(t):
        """Shape descriptors of ``tensors``' result per (frame, segment): ``tensor`` (K, S, 3, 3) = moment / n, ``rg2`` its trace,
        ``eigenvalues`` (K, S, 3) with l1 >= l2 >= l3 and ``axes`` (K, S, 3, 3), axes[..., :, j] the unit principal axis of
        eigenvalue j (numpy.linalg.eigh), ``asphericity`` l1 - (l2 + l3) / 2, ``acylindricity`` l2 - l3 and ``anisotropy``
        1 - 3 (l1 l2 + l2 l3 + l3 l1) / (l1 + l2 + l3)^2, NaN where Rg^2 is 0."""
        m = np.asarray(t["moment"], np.float64) / np.asarray(t["n"], np.float64)[:, None]
        G = np.empty(m.shape[:-1] + (3, 3))
        for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            G[..., a, b] = G[..., b, a] = m[..., c]
        lam, vec = np.linalg.eigh(G)
        lam, vec = lam[..., ::-1], vec[..., ::-1]      # descending
        l1, l2, l3 = lam[..., 0], lam[..., 1], lam[..., 2]
        trace = l1 + l2 + l3
        return {"tensor": G, "rg2": (m[..., 0] + m[..., 1]) + m[..., 2], "eigenvalues": lam, "axes": vec, "asphericity": l1 - (l2 + l3) / 2,
                "acylindricity": l2 - l3, "anisotropy": 1 - 3 * _ratio(l1 * l2 + l2 * l3 + l3 * l1, trace * trace)}

    @staticmethod
    def mean(p):
        """Time-mean Rg^2 of every window, sum / count, NaN where the window is not valid."""
        return _ratio(p["sum"], p["count"])

    @staticmethod
    def fluctuation(p):
        """The variance over the frames of every window's Rg^2, sum_sq / count - mean^2 (not below 0), NaN where not valid."""
        mean = _ratio(p["sum"], p["count"])
        return np.maximum(_ratio(p["sum_sq"], p["count"]) - mean * mean, 0.0)

    @staticmethod
    def centred(p, values=None):
        """``values`` (default: mean(p)) moved from the window's first bead to its centre bead i + w // 2; NaN where no window is centred."""
        v = Gyration.mean(p) if values is None else np.asarray(values, np.float64)
        out = np.full(v.shape, np.nan)
        for m, w in enumerate(p["windows"]):
            h = int(w) // 2
            out[m, h:] = v[m, :v.shape[1] - h]
        return out

    @staticmethod
    def scaling(p, labels):
        """Mean Rg^2(w) by bead class: ``labels`` (N,) integers, the class of a window being that of its centre bead i + w // 2;
        negative labels take no part.  {"classes": (L,), "rg2": (L, W) float64, "count": (L, W) uint64}: sum over the class's valid
        windows of sum, divided by the sum of count."""
        labels = np.asarray(labels)
        if labels.shape != (p["sum"].shape[1],) or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError("labels must be one integer per bead")
        classes = np.unique(labels[labels >= 0])
        total, count = np.zeros((len(classes), len(p["windows"]))), np.zeros((len(classes), len(p["windows"])), np.uint64)
        for m, w in enumerate(p["windows"]):
            N = len(labels)
            mid = np.minimum(np.arange(N) + int(w) // 2, N - 1)
            for k, c in enumerate(classes):
                pick = (labels[mid] == c) & (p["count"][m] > 0)
                total[k, m] = p["sum"][m][pick].sum()
                count[k, m] = p["count"][m][pick].sum()
        return {"classes": classes, "rg2": _ratio(total, count), "count": count}

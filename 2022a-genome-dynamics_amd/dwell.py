"""Contact dwell times and the contact autocorrelation of pairs of beads of a trajectory history on the device: ctypes binding of
``include/gdyn_dwell.h`` (exported by ``csrc/libgdyn.so``).  For how long a contact lasts, how long two beads wait until they first
meet, and how a contact is correlated with itself in time: the runs of the contact state of every pair (two radii, with hysteresis) by
state, kind (complete, left-, right-censored, both) and length bin, the sums of their lengths, and the products c_k c_{k+lag}.  The
reference has none of it: this is a capability beyond it.  The header states the definitions; every output is an integer, equal to
``tests/dwell_restatement.py`` exactly and bit-identical from run to run, for every ``pairs_per_launch``.

    d = Dwell(device=0)
    d.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    d.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    d.set_chains(chains)                        # (C, 2) bead ranges a pair (i, i + s) must lie in; none set: one chain of all beads
    r = d.separations([1, 10, 100], 1.0, 1.3, edges=Dwell.log_edges(700, 2), lags=[0, 1, 2, 4, 8])
    r = d.pairs(pairs, 1.0, 1.3, rows=rows, n_rows=3, edges=..., lags=...)
    # r: runs (R, 2, 4, B), outside, length_sum (R, 2, 4), hits (R, L), pairs (R,) uint64; edges, lags, frames (K)
    Dwell.mean_dwell(r), Dwell.transitions(r), Dwell.first_passage(r), Dwell.correlation(r), Dwell.survival(r)
    d.states(pairs, 1.0, 1.3)                   # (K, P) uint8: the contact kymograph
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import HistoryHandle, _ratio, _u32, box3, load_history_library

DWELL_ABI_VERSION = 1            # GD_DWELL_ABI_VERSION of the include/gdyn_dwell.h this binding mirrors
DWELL_MAX_BINS = 64              # GD_DWELL_MAX_BINS
DWELL_MAX_LAGS = 64              # GD_DWELL_MAX_LAGS
DWELL_MAX_SEPARATIONS = 32       # GD_DWELL_MAX_SEPARATIONS
DWELL_PLANE_BYTES = 1 << 28      # GD_DWELL_PLANE_BYTES
DWELL_SYMBOLS = ["gd_dwell_abi_version", "gd_dwell_create", "gd_dwell_destroy", "gd_dwell_set_history", "gd_dwell_set_history_live", "gd_dwell_set_chains",
                 "gd_dwell_separations", "gd_dwell_pairs", "gd_dwell_states", "gd_dwell_last_times"]
COMPLETE, LEFT, RIGHT, BOTH = 0, 1, 2, 3      # the kinds of a run


class _DwellDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("pairs_per_launch", C.c_uint32)]


class _DwellRule(C.Structure):
    _fields_ = [("r_on", C.c_double), ("r_off", C.c_double), ("box", C.c_void_p), ("first", C.c_uint32), ("stride", C.c_uint32), ("count", C.c_uint32)]


class _DwellSpec(C.Structure):
    _fields_ = [("edges", C.c_void_p), ("n_bins", C.c_uint32), ("lags", C.c_void_p), ("n_lags", C.c_uint32)]


class _DwellOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("runs", "outside", "length_sum", "hits", "pairs")]


def load_dwell_library(path=None):
    """Loads libgdyn and checks the gd_dwell_* symbols and their ABI version."""
    d = load_history_library("dwell", DWELL_SYMBOLS, DWELL_ABI_VERSION, path)
    d.gd_dwell_create.argtypes = [C.POINTER(_DwellDesc), C.POINTER(C.c_void_p)]
    d.gd_dwell_destroy.argtypes = [C.c_void_p]
    d.gd_dwell_set_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_dwell_separations.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_DwellRule), C.POINTER(_DwellSpec), C.POINTER(_DwellOut)]
    d.gd_dwell_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(_DwellRule), C.POINTER(_DwellSpec), C.POINTER(_DwellOut)]
    d.gd_dwell_states.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_DwellRule), C.c_void_p]
    d.gd_dwell_last_times.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    return d


def _run_counts(r):
    """(R, 2, 4): the runs of a result by row, state and kind, whatever their length."""
    return r["runs"].sum(axis=-1) + r["outside"]


class Dwell(HistoryHandle):
    """One device-side history with its chains.  pairs_per_launch: 0 = automatic (no result depends on it)."""

    _prefix = "dwell"
    _destroy = "gd_dwell_destroy"

    def __init__(self, device=0, pairs_per_launch=0, path=None):
        super().__init__(load_dwell_library(path))
        self._check(self.dll.gd_dwell_create(C.byref(_DwellDesc(device, pairs_per_launch)), C.byref(self._h)))
        self.chains = None         # (C, 2) uint32; None before a history

    def _beads_changed(self, n_beads):      # the library drops the chains of another N
        self.chains = np.array([[0, n_beads]], np.uint32)

    def last_times(self):
        """Device milliseconds of the three kernels of the last separations or pairs call."""
        return self._last_times("states_ms", "runs_ms", "corr_ms")

    def set_chains(self, ranges):
        """ranges: (C, 2) [start, end) bead ranges, ascending and not overlapping, empty ones allowed; None: one chain of all beads."""
        whole = np.array([[0, (self.shape or (0, 0))[1]]], np.uint32)
        self.chains = self._set_ranges(self.dll.gd_dwell_set_chains, ranges, "chain ranges", "no chain ranges (None makes one range of all beads)", whole).copy()

    def selected(self, first=0, stride=1, count=0):
        """The frames a call with this selection takes (count 0: all from ``first`` on, ``stride`` apart)."""
        frames = range(int(first), (self.shape or (0, 0))[0], max(int(stride), 1))
        return np.array(frames[:int(count)] if count else frames, dtype=np.int64)

    def _rule(self, r_on, r_off, box, first, stride, count):
        if min(int(first), int(stride), int(count)) < 0:
            raise ValueError("negative frame, stride or count")
        address, keep = box3(box)
        return _DwellRule(float(r_on), float(r_on if r_off is None else r_off), address, int(first), int(stride), int(count)), keep

    def _accumulate(self, call, head, R, r_on, r_off, edges, lags, box, first, stride, count):
        rule, keep = self._rule(r_on, r_off, box, first, stride, count)
        frames = self.selected(first, stride, count)
        e = _u32(Dwell.log_edges(max(len(frames), 1), 2) if edges is None else edges, "edges").reshape(-1)
        l = _u32(lags, "lags").reshape(-1)
        if len(e) < 2:
            raise ValueError("at least two edges make a bin")
        B = len(e) - 1
        out = {"edges": e.copy(), "lags": l.copy(), "frames": frames, "runs": np.zeros((R, 2, 4, B), np.uint64), "outside": np.zeros((R, 2, 4), np.uint64),
               "length_sum": np.zeros((R, 2, 4), np.uint64), "hits": np.zeros((R, len(l)), np.uint64), "pairs": np.zeros(R, np.uint64)}
        spec = _DwellSpec(e.ctypes.data, B, l.ctypes.data if len(l) else None, len(l))
        to = _DwellOut(*[out[k].ctypes.data if out[k].size else None for k in ("runs", "outside", "length_sum", "hits", "pairs")])
        self._check(call(self._h, *head, C.byref(rule), C.byref(spec), C.byref(to)))
        del keep
        return out

    def separations(self, seps, r_on, r_off=None, edges=None, lags=(), box=None, first=0, stride=1, count=0):
        """The runs and the correlation of all pairs (i, i + s) inside one chain, one row per separation s of ``seps`` (up to 32).
        r_off None: r_on (a plain threshold).  edges None: log_edges(K, 2).  Returns ``runs`` (R, 2, 4, B), ``outside`` and
        ``length_sum`` (R, 2, 4), ``hits`` (R, L) and ``pairs`` (R,), all uint64, with ``separations``, ``edges``, ``lags`` and
        ``frames``, the selected frames."""
        s = _u32(seps, "separations").reshape(-1)
        out = self._accumulate(self.dll.gd_dwell_separations, (s.ctypes.data, len(s)), len(s), r_on, r_off, edges, lags, box, first, stride, count)
        out["separations"] = s.copy()
        return out

    def pairs(self, pairs, r_on, r_off=None, rows=None, n_rows=None, edges=None, lags=(), box=None, first=0, stride=1, count=0):
        """The same of the given (P, 2) bead pairs.  rows (P,) in [0, n_rows) names the row of every pair (n_rows None: the largest
        row + 1); rows None: every pair is its own row."""
        p = _u32(pairs, "pairs").reshape(-1, 2)
        if rows is None:
            head, R = (p.ctypes.data, len(p), None, 0), len(p)
        else:
            w = _u32(rows, "rows").reshape(-1)
            if len(w) != len(p):
                raise ValueError(f"rows must have one entry per pair ({len(p)}), got {len(w)}")
            R = int(n_rows) if n_rows is not None else (int(w.max()) + 1 if len(w) else 0)
            head = (p.ctypes.data, len(p), w.ctypes.data, R)
        return self._accumulate(self.dll.gd_dwell_pairs, head, R, r_on, r_off, edges, lags, box, first, stride, count)

    def states(self, pairs, r_on, r_off=None, box=None, first=0, stride=1, count=0):
        """(K, P) uint8: the contact state of every given pair at every selected frame, the contact kymograph."""
        p = _u32(pairs, "pairs").reshape(-1, 2)
        rule, keep = self._rule(r_on, r_off, box, first, stride, count)
        out = np.zeros((count or len(self.selected(first, stride)), len(p)), np.uint8)
        self._check(self.dll.gd_dwell_states(self._h, p.ctypes.data, len(p), C.byref(rule), out.ctypes.data))
        del keep
        return out

    # ---- on the host

    @staticmethod
    def log_edges(max_length, per_octave=1):
        """Ascending edges from 1 that grow by 2^(1 / per_octave), floored and made distinct, up to the first one beyond max_length:
        every length of 1 to max_length falls in a bin."""
        if int(max_length) < 1 or int(per_octave) < 1:
            raise ValueError("max_length and per_octave are at least 1")
        out, k = [], 0
        while not out or out[-1] <= int(max_length):
            e = int(np.floor(2.0 ** (k / int(per_octave)) + 1e-9))
            if not out or e > out[-1]:
                out.append(e)
            k += 1
        if len(out) > DWELL_MAX_BINS + 1:
            raise ValueError(f"{len(out) - 1} bins exceed {DWELL_MAX_BINS}")
        return np.array(out, np.uint32)

    @staticmethod
    def transitions(r):
        """How often a contact formed and broke within the selection, per row: ``formed`` the contact runs that begin after the first
        frame (kinds complete and right-censored), ``broken`` the runs apart that do."""
        n = _run_counts(r)
        return {"formed": n[:, 1, COMPLETE] + n[:, 1, RIGHT], "broken": n[:, 0, COMPLETE] + n[:, 0, RIGHT]}

    @staticmethod
    def mean_dwell(r, state=1, kinds=(COMPLETE, LEFT, RIGHT, BOTH)):
        """(R,) the mean length in selected frames of the runs of ``state`` of the given kinds, length_sum / runs; NaN without a run."""
        kinds = list(kinds)
        return _ratio(r["length_sum"][:, state, kinds].sum(axis=-1).astype(np.float64), _run_counts(r)[:, state, kinds].sum(axis=-1))

    @staticmethod
    def first_passage(r):
        """The waiting time until the two beads of a pair first meet: ``met`` (R, B) the pairs by the length of their left-censored
        run apart, ``met_outside`` (R,) those in no bin, ``mean`` (R,) the mean of those lengths, ``never`` (R,) the pairs apart in every
        frame, ``in_contact`` (R,) the pairs that begin in contact."""
        n = _run_counts(r)
        return {"met": r["runs"][:, 0, LEFT].copy(), "met_outside": r["outside"][:, 0, LEFT].copy(),
                "mean": _ratio(r["length_sum"][:, 0, LEFT].astype(np.float64), n[:, 0, LEFT]), "never": n[:, 0, BOTH], "in_contact": n[:, 1, LEFT] + n[:, 1, BOTH]}

    @staticmethod
    def correlation(r):
        """(R, L) the contact autocorrelation <c_k c_{k+lag}> = hits / (pairs (K - lag)); NaN where no term exists."""
        K = len(r["frames"])
        terms = r["pairs"].astype(np.float64)[:, None] * np.maximum(K - r["lags"].astype(np.int64), 0)[None, :]
        return _ratio(r["hits"].astype(np.float64), terms)

    @staticmethod
    def survival(r, state=1):
        """(R, B) the Kaplan-Meier estimate S(t), t = 1 .. B, that a run of ``state`` lasts longer than t frames, from the complete
        runs (ended at t) and the right-censored ones (still going at t); left-censored runs take no part.  The bins must be unit-wide
        from 1 and hold every such run (ValueError)."""
        B = r["runs"].shape[-1]
        if r["edges"].tolist() != list(range(1, B + 2)):
            raise ValueError("survival needs unit-wide bins from 1: edges 1, 2, ..., B + 1")
        if r["outside"][:, state, [COMPLETE, RIGHT]].any():
            raise ValueError("survival needs every complete and right-censored run inside the bins")
        ended = r["runs"][:, state, COMPLETE].astype(np.float64)
        going = r["runs"][:, state, RIGHT].astype(np.float64)
        at_risk = np.cumsum((ended + going)[:, ::-1], axis=1)[:, ::-1]
        return np.cumprod(1.0 - np.divide(ended, at_risk, out=np.zeros_like(ended), where=at_risk > 0), axis=1)

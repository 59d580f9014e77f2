"""Van Hove functions of a trajectory history on the device: ctypes binding of ``include/gdyn_vanhove.h`` (exported by
``csrc/libgdyn.so``).  The self part G_s(r, tau) is the distribution of the displacements of single beads over a lag, per label and
with an axis mask (``xy`` is what a microscope sees); the distinct part G_d(r, tau) is the density of the OTHER beads at distance r
from where a bead was tau ago, per ordered label pair.  The reference has neither: this is a capability beyond it.  The header states
the definitions; every output is an integer count, equal to ``tests/vanhove_restatement.py`` exactly and bit-identical from run to run.

    v = VanHove(device=0)
    v.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    v.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    v.set_labels(label, n_labels)               # (N,) in [-1, K); -1 takes no part
    s = v.self_part([1, 4, 16], linear_edges(0.05, 3.0), axes="xy", per_origin=True)
    # s: counts (L, K, B), below, above (L, K), per_origin (L, O, K, B), origins (L,) uint64; lags, edges
    d = v.distinct([0, 16], linear_edges(0.05, 2.0), box=(L, L, L))
    # d: counts (L, K, K, B), origins (L,) uint64; lags, edges
    density(s["counts"], s["edges"], 2, s["below"], s["above"]); q = overlap(s["per_origin"], s["edges"], 0.3); chi4(q, members)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._binding import HistoryHandle, _u32, box3, load_history_library

VANHOVE_ABI_VERSION = 1          # GD_VANHOVE_ABI_VERSION of the include/gdyn_vanhove.h this binding mirrors
VANHOVE_MAX_LAGS = 32            # GD_VANHOVE_MAX_LAGS
VANHOVE_MAX_BINS = 256           # GD_VANHOVE_MAX_BINS
VANHOVE_MAX_LABELS = 8           # GD_VANHOVE_MAX_LABELS
VANHOVE_LDS_CELLS = 6144         # GD_VANHOVE_LDS_CELLS
VANHOVE_SYMBOLS = ["gd_vanhove_abi_version", "gd_vanhove_create", "gd_vanhove_destroy", "gd_vanhove_set_history", "gd_vanhove_set_history_live",
                   "gd_vanhove_set_labels", "gd_vanhove_origins", "gd_vanhove_self", "gd_vanhove_distinct", "gd_vanhove_last_times"]
AXES = {"x": 1, "y": 2, "z": 4}


class _VanHoveDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_tile", C.c_uint32), ("max_frames_per_launch", C.c_uint32)]


class _VanHoveSpec(C.Structure):
    _fields_ = [("lags", C.c_void_p), ("n_lags", C.c_uint32), ("edges", C.c_void_p), ("n_bins", C.c_uint32), ("first", C.c_uint32), ("stride", C.c_uint32),
                ("count", C.c_uint32)]


class _VanHoveSelfOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("counts", "below", "above", "per_origin", "origins")]


def load_vanhove_library(path=None):
    """Loads libgdyn and checks the gd_vanhove_* symbols and their ABI version."""
    d = load_history_library("vanhove", VANHOVE_SYMBOLS, VANHOVE_ABI_VERSION, path)
    d.gd_vanhove_create.argtypes = [C.POINTER(_VanHoveDesc), C.POINTER(C.c_void_p)]
    d.gd_vanhove_destroy.argtypes = [C.c_void_p]
    d.gd_vanhove_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_vanhove_origins.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    d.gd_vanhove_origins.restype = C.c_uint32
    d.gd_vanhove_self.argtypes = [C.c_void_p, C.POINTER(_VanHoveSpec), C.c_uint32, C.POINTER(_VanHoveSelfOut)]
    d.gd_vanhove_distinct.argtypes = [C.c_void_p, C.POINTER(_VanHoveSpec), C.c_void_p, C.c_void_p, C.c_void_p]
    d.gd_vanhove_last_times.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    return d


def axes_mask(axes):
    """"xyz", "xy", "z", ... as the mask of gd_vanhove_self (x = 1, y = 2, z = 4); an integer is passed on."""
    if isinstance(axes, str):
        if not axes or any(a not in AXES for a in axes) or len(set(axes)) != len(axes):
            raise ValueError(f"axes must name each of x, y, z at most once, got {axes!r}")
        return sum(AXES[a] for a in axes)
    return int(axes)


class VanHove(HistoryHandle):
    """One device-side history with its labels.  max_frames_per_tile (self part) and max_frames_per_launch (distinct part): 0 =
    automatic; no result depends on either."""

    _prefix = "vanhove"
    _destroy = "gd_vanhove_destroy"

    def __init__(self, device=0, max_frames_per_tile=0, max_frames_per_launch=0, path=None):
        super().__init__(load_vanhove_library(path))
        self._check(self.dll.gd_vanhove_create(C.byref(_VanHoveDesc(device, max_frames_per_tile, max_frames_per_launch)), C.byref(self._h)))
        self.K = 1
        self.label = None

    def _beads_changed(self, n_beads):      # the library drops the labels of another N
        self.K, self.label = 1, None

    def set_labels(self, label, n_labels=None):
        """label (N,) integers in [-1, n_labels), -1 for a bead that takes no part; None: one label of all beads."""
        self.K, self.label = self._set_labels(label, n_labels)

    def members(self):
        """(K,) the beads of every label."""
        if self.label is None:
            return np.array([(self.shape or (0, 0))[1]], np.uint64)
        return np.bincount(self.label[self.label >= 0], minlength=self.K).astype(np.uint64)

    def last_times(self):
        """Device milliseconds of the last self_part or distinct call: the counting kernel, the cell index, the clearing."""
        return self._last_times("count_ms", "index_ms", "other_ms")

    def _spec(self, lags, edges, first, stride, count):
        if min(int(first), int(stride), int(count)) < 0:
            raise ValueError("negative origin, stride or count")
        l = _u32(lags, "lags").reshape(-1)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if len(e) < 2:
            raise ValueError("at least two edges make a bin")
        spec = _VanHoveSpec(l.ctypes.data if len(l) else None, len(l), e.ctypes.data, len(e) - 1, int(first), int(stride), int(count))
        O = int(self.dll.gd_vanhove_origins(self._h, int(first), int(stride), int(count)))
        return spec, l, e, O

    def self_part(self, lags, edges, axes="xyz", first=0, stride=1, count=0, per_origin=False):
        """The displacement histograms of the lags (frames of the history, >= 1, up to 32) over the origins first + k stride, k < count
        (0: all).  Returns ``counts`` (L, K, B), ``below`` and ``above`` (L, K), ``origins`` (L,), with per_origin ``per_origin``
        (L, O, K, B), all uint64, and ``lags``, ``edges``."""
        spec, l, e, O = self._spec(lags, edges, first, stride, count)
        L, K, B = len(l), self.K, len(e) - 1
        out = {"lags": l.copy(), "edges": e.copy(), "counts": np.zeros((L, K, B), np.uint64), "below": np.zeros((L, K), np.uint64),
               "above": np.zeros((L, K), np.uint64), "origins": np.zeros(L, np.uint64)}
        if per_origin:
            out["per_origin"] = np.zeros((L, O, K, B), np.uint64)
        to = _VanHoveSelfOut(*[out[k].ctypes.data if k in out and out[k].size else None for k in ("counts", "below", "above", "per_origin", "origins")])
        self._check(self.dll.gd_vanhove_self(self._h, C.byref(spec), axes_mask(axes), C.byref(to)))
        return out

    def distinct(self, lags, edges, box=None, first=0, stride=1, count=0):
        """The histograms of the distances from a bead at an origin to every OTHER bead a lag later (lags >= 0), per ordered label pair
        (label at the origin, label of the other).  box: a period or three, None: open.  Returns ``counts`` (L, K, K, B) and
        ``origins`` (L,), uint64, and ``lags``, ``edges``."""
        spec, l, e, _ = self._spec(lags, edges, first, stride, count)
        L, K, B = len(l), self.K, len(e) - 1
        out = {"lags": l.copy(), "edges": e.copy(), "counts": np.zeros((L, K, K, B), np.uint64), "origins": np.zeros(L, np.uint64)}
        address, keep = box3(box)
        self._check(self.dll.gd_vanhove_distinct(self._h, C.byref(spec), address, out["counts"].ctypes.data, out["origins"].ctypes.data if L else None))
        del keep
        return out


# ---- on the host


def linear_edges(width, max_distance):
    """Edges 0, width, 2 width, ... up to the first at or beyond max_distance."""
    if not (width > 0 and max_distance > 0 and math.isfinite(width) and math.isfinite(max_distance)):
        raise ValueError("width and max_distance must be positive and finite")
    n = int(math.ceil(max_distance / width))
    if n > VANHOVE_MAX_BINS:
        raise ValueError(f"{n} bins exceed {VANHOVE_MAX_BINS}")
    return np.arange(n + 1, dtype=np.float64) * float(width)


def log_edges(first, last, per_decade):
    """Edges first * 10^(k / per_decade), k = 0, 1, ..., up to the first at or beyond last."""
    if not (0 < first < last and math.isfinite(last)) or int(per_decade) < 1:
        raise ValueError("0 < first < last, finite, and per_decade at least 1")
    n = int(math.ceil(math.log10(last / first) * int(per_decade) - 1e-9))
    if n > VANHOVE_MAX_BINS:
        raise ValueError(f"{n} bins exceed {VANHOVE_MAX_BINS}")
    return float(first) * 10.0 ** (np.arange(n + 1, dtype=np.float64) / int(per_decade))


def shell_volumes(edges, dim):
    """The volumes of the shells between the edges in 1, 2 or 3 dimensions (1: both sides, 2 dr; 2: annuli; 3: spherical shells)."""
    e = np.asarray(edges, np.float64)
    if dim == 1:
        return 2.0 * np.diff(e)
    if dim == 2:
        return math.pi * np.diff(e ** 2)
    if dim == 3:
        return 4.0 / 3.0 * math.pi * np.diff(e ** 3)
    raise ValueError("dim is 1, 2 or 3")


def density(counts, edges, dim, below=None, above=None):
    """counts (..., B) as the probability per unit volume of the shell: counts / (total * shell volume), the total including
    ``below`` and ``above`` (...,) where given; NaN where the total is 0.  Its integral over the shells is the fraction inside them."""
    c = np.asarray(counts, np.float64)
    total = c.sum(axis=-1)
    for extra in (below, above):
        if extra is not None:
            total = total + np.asarray(extra, np.float64)
    out = np.full(c.shape, np.nan)
    np.divide(c, total[..., None] * shell_volumes(edges, dim), out=out, where=(total > 0)[..., None])
    return out


def gaussian(edges, msd, dim):
    """The probability of every bin for a displacement whose ``dim`` components are independent Gaussians of the total second moment
    ``msd`` (variance msd / dim each): the Gaussian of the same MSD integrated over the same bins, to lay beside density * volume."""
    e = np.asarray(edges, np.float64)
    var = float(msd) / dim
    if not var > 0:
        raise ValueError("msd must be positive")
    u = e / math.sqrt(2.0 * var)
    erf = np.array([math.erf(v) for v in u])
    if dim == 1:
        cdf = erf
    elif dim == 2:
        cdf = 1.0 - np.exp(-u * u)
    elif dim == 3:
        cdf = erf - 2.0 / math.sqrt(math.pi) * u * np.exp(-u * u)
    else:
        raise ValueError("dim is 1, 2 or 3")
    return np.diff(cdf)


def overlap(per_origin, edges, a):
    """Q per lag, origin and label: the number of beads that moved less than ``a``, the cumulative sum of per_origin (L, O, K, B) up
    to the edge a (which must be one of the edges: ValueError).  With e_0 > 0 the caller adds what lies below e_0 itself."""
    e = np.asarray(edges, np.float64)
    at = np.nonzero(e == float(a))[0]
    if not len(at):
        raise ValueError(f"a = {a} is not one of the edges")
    return np.asarray(per_origin)[..., :int(at[0])].sum(axis=-1)


def chi4(q, members):
    """chi_4 per lag and label from q (L, O, K) of overlap(): N (<(Q/N)^2> - <Q/N>^2) over the origins, with N = members (K,).  Rows of
    origins that take no part in a lag must be cut by the caller (origins[l] says how many do)."""
    n = np.asarray(members, np.float64)
    x = np.asarray(q, np.float64) / n
    return n * (np.mean(x * x, axis=-2) - np.mean(x, axis=-2) ** 2)


def distinct_density(counts, edges, members, volume, origins=None):
    """G_d / rho: counts (L, K, K, B) of distinct() over what an ideal gas of the partners' density gives, members[a] * origins *
    (members[b] - (a == b)) / volume * shell volume.  Tends to 1 in a homogeneous box.  origins (L,) None: 1."""
    c = np.asarray(counts, np.float64)
    m = np.asarray(members, np.float64)
    o = np.ones(c.shape[0]) if origins is None else np.asarray(origins, np.float64)
    partners = m[None, :] - np.eye(len(m))
    ideal = o[:, None, None, None] * (m[:, None] * partners)[None, :, :, None] / float(volume) * shell_volumes(edges, 3)
    out = np.full(c.shape, np.nan)
    np.divide(c, ideal, out=out, where=ideal > 0)
    return out

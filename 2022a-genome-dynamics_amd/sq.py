"""Structure factors and scattering functions of a trajectory history on the device: ctypes binding of ``include/gdyn_sq.h``
(exported by ``csrc/libgdyn.so``).  The Fourier amplitudes rho_a(q, f) = sum over the beads of label a of exp(-i q . x) = C - i S
at chosen wave vectors, frame by frame, and from them the partial structure factors S_ab(q), the collective intermediate
scattering function F_ab(q, tau) and its self part F_s(q, tau).  The reference has none of it: this is a capability beyond it.
The header states the definitions; the sums are fp64 direct sums, bit-identical from run to run, for every
``max_frames_per_pass``, whatever other vectors or frames a call lists, and between a host-fed and a live-fed history.

    s = Sq(device=0)
    s.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    s.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    s.set_labels(types, n_labels=2)             # label[i] in [-1, K), K <= 8; -1: takes no part; None: one label of all beads
    n, q = Sq.lattice_vectors(box, 8)           # the wave vectors of a periodic box; Sq.sphere_vectors(...) for an open nucleus
    s.set_vectors(q)                            # (Q, 3) float64; they survive a new history
    a = s.amplitudes()                          # "cos_sum", "sin_sum" (F, K, Q)
    c = s.collective([0, 1, 10])                # "sum_re", "sum_im" (L, K, K, Q), "count" (L,), "lags"
    f = s.self_part([1, 10], origin_stride=5)   # "cos_sum", "sin_sum" (L, K, Q), "count" (L, K), "lags"
    S_ab = Sq.partial(c, s.label_sizes.sum())[0]            # lag 0: the static partial structure factors
    S_of_q = Sq.shells(q, S_ab, edges)                      # the mean over the vectors of each shell of |q|
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, HistoryHandle, _u32, load_history_library

SQ_ABI_VERSION = 1         # GD_SQ_ABI_VERSION of the include/gdyn_sq.h this binding mirrors
SQ_MAX_LABELS = 8          # GD_SQ_MAX_LABELS
SQ_MAX_VECTORS = 1 << 20   # GD_SQ_MAX_VECTORS
SQ_CHUNK_BEADS = 256       # GD_SQ_CHUNK_BEADS
SQ_SYMBOLS = ["gd_sq_abi_version", "gd_sq_create", "gd_sq_destroy", "gd_sq_set_history", "gd_sq_set_history_live", "gd_sq_set_labels",
              "gd_sq_set_vectors", "gd_sq_amplitudes", "gd_sq_collective", "gd_sq_self"]
TWO_PI = 6.283185307179586
GOLDEN_ANGLE = 2.399963229728653      # pi (3 - sqrt 5)


class _SqDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_pass", C.c_uint32)]


def load_sq_library(path=None):
    """Loads libgdyn and checks the gd_sq_* symbols and their ABI version."""
    d = load_history_library("sq", SQ_SYMBOLS, SQ_ABI_VERSION, path)
    d.gd_sq_create.argtypes = [C.POINTER(_SqDesc), C.POINTER(C.c_void_p)]
    d.gd_sq_destroy.argtypes = [C.c_void_p]
    d.gd_sq_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_sq_set_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_sq_amplitudes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    for f in (d.gd_sq_collective, d.gd_sq_self):
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return d


class Sq(HistoryHandle):
    """One device-side history with its bead labels and wave vectors.  max_frames_per_pass: 0 = automatic (no result depends on it)."""

    _prefix = "sq"
    _destroy = "gd_sq_destroy"

    def __init__(self, device=0, max_frames_per_pass=0, path=None):
        super().__init__(load_sq_library(path))
        self._check(self.dll.gd_sq_create(C.byref(_SqDesc(device, max_frames_per_pass)), C.byref(self._h)))
        self.n_labels = 1
        self.label_sizes = np.zeros(1, np.uint64)      # n_a
        self.n_vectors = 0

    def _beads_changed(self, n_beads):      # the library drops the labels of another N
        self.n_labels, self.label_sizes = 1, np.array([n_beads], np.uint64)

    def set_labels(self, label, n_labels=None):
        """label: (N,) integers in [-1, n_labels), -1 for a bead that takes no part; None: one label of all beads.
        n_labels=None: the largest label + 1."""
        K, l = self._set_labels(label, n_labels)
        if l is None:
            self._beads_changed(self.shape[1])
        else:
            self.n_labels, self.label_sizes = K, np.bincount(l[l >= 0], minlength=K).astype(np.uint64)

    def set_vectors(self, q):
        """q: (Q, 3) finite wave vectors, the zero vector allowed."""
        v = np.ascontiguousarray(q, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"vectors must be (Q, 3), got {v.shape}")
        self._check(self.dll.gd_sq_set_vectors(self._h, v.ctypes.data, len(v)))
        self.n_vectors = len(v)

    def _window(self, frames):
        """(first frame, number of frames) of ``frames``: the same pair, or None for the whole history."""
        if frames is None:
            return 0, (self.shape or (0, 0))[0]
        first, count = int(frames[0]), int(frames[1])
        if first < 0 or count < 0:
            raise ValueError("negative frame range")
        return first, count

    def amplitudes(self, frames=None):
        """C and S of every frame of the window ``frames`` = (first, count): ``cos_sum``, ``sin_sum`` (n_frames, K, Q) float64."""
        first, n = self._window(frames)
        c, s = (np.zeros((n, self.n_labels, self.n_vectors), np.float64) for _ in range(2))
        self._check(self.dll.gd_sq_amplitudes(self._h, first, n, c.ctypes.data, s.ctypes.data))
        return {"cos_sum": c, "sin_sum": s}

    def _lagged(self, call, lags, frames, origin_stride, cells, count_shape):
        first, n = self._window(frames)
        l = _u32(np.atleast_1d(lags), "lags").reshape(-1)
        a, b = (np.zeros((len(l),) + cells, np.float64) for _ in range(2))
        count = np.zeros((len(l),) + count_shape, np.uint64)
        if int(origin_stride) < 0:
            raise ValueError("negative origin stride")
        self._check(call(self._h, first, n, l.ctypes.data, len(l), int(origin_stride), a.ctypes.data, b.ctypes.data, count.ctypes.data))
        return a, b, count, l

    def collective(self, lags, frames=None, origin_stride=1):
        """rho_a(t + tau) conj rho_b(t) summed over the origins t = first + k origin_stride of the window: ``sum_re``, ``sum_im``
        (L, K, K, Q) float64, ``count`` (L,) uint64 origins, ``lags`` (L,) uint32.  Lag 0: the static partial structure factors."""
        K = self.n_labels
        re, im, count, l = self._lagged(self.dll.gd_sq_collective, lags, frames, origin_stride, (K, K, self.n_vectors), ())
        return {"sum_re": re, "sum_im": im, "count": count, "lags": l}

    def self_part(self, lags, frames=None, origin_stride=1):
        """The amplitudes of the displacements X[t + tau] - X[t] summed over the origins: ``cos_sum``, ``sin_sum`` (L, K, Q) float64,
        ``count`` (L, K) uint64 = origins n_a, ``lags`` (L,) uint32.  F_s = cos_sum / count."""
        c, s, count, l = self._lagged(self.dll.gd_sq_self, lags, frames, origin_stride, (self.n_labels, self.n_vectors), (self.n_labels,))
        return {"cos_sum": c, "sin_sum": s, "count": count, "lags": l}

    # ---- pure numpy: wave vectors and what a caller makes of the sums

    @staticmethod
    def lattice_vectors(box, n_max):
        """The wave vectors of a periodic box (Lx, Ly, Lz): (n, q) with n (M, 3) int64 the integer triples with 0 < max |n_k| <= n_max
        in the half space where the first non-zero component is positive, in lexicographic order, M = ((2 n_max + 1)^3 - 1) / 2,
        and q (M, 3) float64, q_k = (TWO_PI * n_k) / L_k, each operation rounded once."""
        n_max = int(n_max)
        L = np.asarray(box, dtype=np.float64).reshape(3)
        if n_max < 1 or not (np.isfinite(L).all() and (L > 0).all()):
            raise ValueError("n_max must be at least 1 and the box positive and finite")
        r = np.arange(-n_max, n_max + 1)
        n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)      # lexicographic
        first = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
        n = n[first > 0].astype(np.int64)
        return n, (TWO_PI * n.astype(np.float64)) / L

    @staticmethod
    def sphere_vectors(magnitudes, n_directions):
        """Fibonacci-sphere directions times each magnitude, for an open nucleus: (len(magnitudes) * n_directions, 3) float64,
        magnitude by magnitude.  Direction i of D: z = 1 - (2 i + 1) / D, azimuth i times the golden angle, normalised."""
        m = np.asarray(magnitudes, dtype=np.float64).reshape(-1)
        D = int(n_directions)
        if D < 1 or not len(m) or not (np.isfinite(m).all() and (m >= 0).all()):
            raise ValueError("n_directions must be at least 1 and the magnitudes non-negative and finite")
        i = np.arange(D, dtype=np.float64)
        z = 1.0 - (2.0 * i + 1.0) / D
        r = np.sqrt(1.0 - z * z)
        u = np.stack([r * np.cos(GOLDEN_ANGLE * i), r * np.sin(GOLDEN_ANGLE * i), z], axis=1)
        u = u / np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])[:, None]
        return (m[:, None, None] * u[None]).reshape(-1, 3)

    @staticmethod
    def partial(result, n_labelled):
        """sum_re / (count * n_labelled) of a ``collective`` result, (L, K, K, Q): S_ab(q) at lag 0, F_ab(q, tau) beyond."""
        return result["sum_re"] / (result["count"].astype(np.float64) * float(n_labelled))[:, None, None, None]

    @staticmethod
    def shells(q, values, edges):
        """The mean of ``values`` (..., Q) over the vectors with |q| in [edges[k], edges[k + 1]), (..., len(edges) - 1); NaN for an
        empty shell."""
        q, values, edges = np.asarray(q, dtype=np.float64), np.asarray(values, dtype=np.float64), np.asarray(edges, dtype=np.float64)
        norm = np.sqrt((q * q).sum(axis=1))
        shell = np.searchsorted(edges, norm, side="right") - 1
        out = np.full(values.shape[:-1] + (len(edges) - 1,), np.nan)
        for k in range(len(edges) - 1):
            if (shell == k).any():
                out[..., k] = values[..., shell == k].mean(axis=-1)
        return out

"""What the ctypes bindings of the device analyses (flow, rdf, lamina, cmap, hic, msd, dcorr, dmap, sq, cluster, dcov, gyr, dwell, vanhove) share: loading libgdyn with a check of
one module's symbols and ABI version, the life cycle of a ``gd_<x>`` handle, the normalisation of frames, and the trajectory history
that the msd, dcorr, dmap, sq, cluster, dcov, gyr, dwell and vanhove handles hold, with the bodies of their label, range and timing methods."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import LIBGDYN_PATH, GdynError      # GdynError: the binding modules pass it on under their own names


def load_library(prefix, symbols, abi_version, path=None):
    """Loads libgdyn and checks the gd_<prefix>_* symbols and their ABI version; the caller sets the argtypes."""
    path = path or LIBGDYN_PATH
    d = C.CDLL(path)
    for name in symbols + ["gd_last_error"]:
        if not hasattr(d, name):
            raise OSError(f"{path}: missing symbol {name}")
    version = getattr(d, f"gd_{prefix}_abi_version")
    version.restype = C.c_int
    if version() != abi_version:
        raise OSError(f"{path}: {prefix} ABI version {version()}, this binding mirrors {abi_version}")
    d.gd_last_error.restype = C.c_char_p
    return d


def load_history_library(prefix, symbols, abi_version, path=None):
    """load_library for a module whose handle holds a trajectory history (HistoryHandle); sets the argtypes of its two history calls."""
    d = load_library(prefix, symbols, abi_version, path)
    getattr(d, f"gd_{prefix}_set_history").argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    getattr(d, f"gd_{prefix}_set_history_live").argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return d


class Handle:
    """A ``gd_<x>`` handle of the library ``dll``; a subclass names its destroy symbol and creates ``_h``."""

    _destroy = None

    def __init__(self, dll):
        self.dll = dll
        self._h = C.c_void_p()

    def _check(self, rc):
        if rc != 0:
            raise GdynError(rc, self.dll.gd_last_error().decode())

    def close(self):
        if self._h:
            getattr(self.dll, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HistoryHandle(Handle):
    """A ``gd_<prefix>`` handle that holds one trajectory history on the device (msd, dcorr, dmap, sq, cluster, dcov, gyr).  ``shape`` is (F, N) of the
    history, None before the first.  A subclass names its ``_prefix``, loads ``dll`` with load_history_library and overrides
    ``_beads_changed``."""

    _prefix = None

    def __init__(self, dll):
        super().__init__(dll)
        self.shape = None

    def _beads_changed(self, n_beads):
        """The history has another N than the last: the library has dropped what the handle kept per bead."""

    def _new_shape(self, shape):
        if self.shape is None or self.shape[1] != shape[1]:
            self._beads_changed(shape[1])
        self.shape = shape

    def set_history(self, frames):
        """frames (F, N, 3), float32 or float64 (anything else becomes float32)."""
        h = np.asarray(frames)
        if h.ndim != 3 or h.shape[2] != 3:
            raise ValueError(f"history must be (F, N, 3), got {h.shape}")
        h, is64 = as_frames(h)
        F, N, _ = h.shape
        self._check(getattr(self.dll, f"gd_{self._prefix}_set_history")(self._h, h.ctypes.data, F, N, int(is64)))
        self._new_shape((F, N))

    def set_history_from(self, history, replica):
        """The history becomes the frames that ``history`` (a live.History) recorded of ``replica``, float32 as recorded, going from
        the recorder to this handle on the device."""
        self._check(getattr(self.dll, f"gd_{self._prefix}_set_history_live")(self._h, history._h, int(replica)))
        self._new_shape((history.frames, history.N))

    # ---- what the history modules' setters and getters share; a subclass keeps its public method and its own attributes

    def _set_labels(self, label, n_labels):
        """The body of set_labels: label (N,) integers in [-1, n_labels) or None, n_labels None: the largest label + 1.  Returns
        (K, the labels as int32 or None)."""
        call = getattr(self.dll, f"gd_{self._prefix}_set_labels")
        if label is None:
            self._check(call(self._h, None, 1))
            return 1, None
        l = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
        if self.shape is not None and len(l) != self.shape[1]:
            raise ValueError(f"label must have one entry per bead ({self.shape[1]}), got {len(l)}")
        K = int(n_labels) if n_labels is not None else max(int(l.max()) + 1, 1) if len(l) else 1
        self._check(call(self._h, l.ctypes.data, K))
        return K, l

    def _set_ranges(self, call, ranges, what, empty, default):
        """The body of a setter of (R, 2) [start, end) bead ranges (``what``: "bin ranges"; ``empty``: the refusal of an empty list).
        Returns them as uint32, or ``default`` for ``ranges`` None, which makes the library's own default."""
        if ranges is None:
            self._check(call(self._h, None, 0))
            return default
        r = _u32(ranges, what).reshape(-1, 2)
        if not len(r):
            raise ValueError(empty)
        self._check(call(self._h, r.ctypes.data, len(r)))
        return r

    def _last_times(self, *names):
        """The three device times of gd_<prefix>_last_times under ``names``."""
        t = [C.c_double() for _ in range(3)]
        self._check(getattr(self.dll, f"gd_{self._prefix}_last_times")(self._h, *[C.byref(v) for v in t]))
        return {name: v.value for name, v in zip(names, t)}


def box3(box):
    """A period or three as the three doubles of a ``const double *box`` argument: (their address or None, the array to keep alive)."""
    if box is None:
        return None, None
    b = (C.c_double * 3)(*np.broadcast_to(np.asarray(box, dtype=np.float64), (3,)))
    return C.addressof(b), b


def _u32(values, what):
    """``values`` as a contiguous uint32 array; ``what`` names them in the refusal of anything but integers in [0, 2^32)."""
    v = np.asarray(values)
    if v.size and (not np.issubdtype(v.dtype, np.integer) or v.min() < 0 or v.max() > 0xFFFFFFFF):
        raise ValueError(f"{what} must be integers in [0, 2^32)")
    return np.ascontiguousarray(v, dtype=np.uint32)


def _ratio(total, count):
    """total / count with ``count`` broadcast to ``total``, NaN where count is 0."""
    count = np.broadcast_to(count, total.shape)
    out = np.full(total.shape, np.nan)
    np.divide(total, count, out=out, where=count > 0)
    return out


def as_frames(x):
    """(F, N, 3) frames, or one (N, 3) frame, as a contiguous float32 or float64 (F, N, 3) array: (array, is_f64)."""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"frames must be (F, N, 3), got {x.shape}")
    is64 = x.dtype == np.float64
    return np.ascontiguousarray(x, dtype=np.float64 if is64 else np.float32), is64

"""What the ctypes bindings of the device analyses (flow, rdf, lamina, cmap, hic, msd, dcorr, dmap) share: loading libgdyn with a check of
one module's symbols and ABI version, the life cycle of a ``gd_<x>`` handle, and the normalisation of frames."""
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


def as_frames(x):
    """(F, N, 3) frames, or one (N, 3) frame, as a contiguous float32 or float64 (F, N, 3) array: (array, is_f64)."""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"frames must be (F, N, 3), got {x.shape}")
    is64 = x.dtype == np.float64
    return np.ascontiguousarray(x, dtype=np.float64 if is64 else np.float32), is64

"""The lamina analysis on the device: ctypes binding of ``include/gdyn_lamina.h`` (exported by ``csrc/libgdyn.so``), the
wall distances and lamina contacts of the reference's 5-sim-genome/src/analyze_lamina (geometry.py, command.py).

    lam = Lamina(device=0)
    d = lam.distances(frames, semiaxes)             # (F, N) float64; dtype=np.float32 for what the programs store
    c = lam.contacts(d.astype(np.float32), 0.3)     # (F, N) bool, added into the handle's sum
    avg = lam.average()                             # float32 sum / number of contacts() calls since reset()

``distance_from_surface`` is the same arithmetic in numpy for users without a GPU; the device path never calls it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import GdynError, Handle, as_frames, load_library

LAMINA_ABI_VERSION = 1     # GD_LAMINA_ABI_VERSION of the include/gdyn_lamina.h this binding mirrors
LAMINA_SYMBOLS = ["gd_lamina_abi_version", "gd_lamina_create", "gd_lamina_destroy", "gd_lamina_distances", "gd_lamina_contacts",
                  "gd_lamina_average", "gd_lamina_reset"]
EPSILON = 1e-6             # geometry.py:4


class _LaminaDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_launch", C.c_uint32)]


def load_lamina_library(path=None):
    """Loads libgdyn and checks the gd_lamina_* symbols and their ABI version."""
    d = load_library("lamina", LAMINA_SYMBOLS, LAMINA_ABI_VERSION, path)
    d.gd_lamina_create.argtypes = [C.POINTER(_LaminaDesc), C.POINTER(C.c_void_p)]
    d.gd_lamina_destroy.argtypes = [C.c_void_p]
    d.gd_lamina_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    d.gd_lamina_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p]
    d.gd_lamina_average.argtypes = [C.c_void_p, C.c_void_p]
    d.gd_lamina_reset.argtypes = [C.c_void_p]
    return d


def distance_from_surface(points, semiaxes):
    """geometry.py:13-28 for (N, 3) points and one set of semiaxes, in float64: |u v| with u the smaller root of the
    second-order expansion (EPSILON in its denominator) and v = |semiaxes**-2 * x|.  NaN where b*b - a*c < 0."""
    x = np.asarray(points)
    if x.dtype != np.float64:
        x = x.astype(np.float32).astype(np.float64)
    inv = np.asarray(semiaxes, dtype=np.float64) ** -2
    s1 = inv[None, :] * x
    s2 = inv[None, :] * s1
    s3 = inv[None, :] * s2

    def dot(p, q):
        t = p * q
        return (t[:, 0] + t[:, 1]) + t[:, 2]

    a, b, c = dot(s3, x), dot(s2, x), dot(s1, x) - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (b - np.sqrt(b * b - a * c)) / (a + EPSILON)
        v = np.sqrt(dot(s1, s1))
        return np.abs(u * v)


class Lamina(Handle):
    """One device-side handle.  max_frames_per_launch: 0 = automatic (no result depends on it)."""

    _destroy = "gd_lamina_destroy"

    def __init__(self, device=0, max_frames_per_launch=0, path=None):
        super().__init__(load_lamina_library(path))
        self._shape = None
        self._check(self.dll.gd_lamina_create(C.byref(_LaminaDesc(device, max_frames_per_launch)), C.byref(self._h)))

    def distances(self, frames, semiaxes, dtype=np.float64):
        """frames (F, N, 3) float32 or float64 (or one (N, 3) frame); semiaxes: three values for every frame or (F, 3).
        Returns (F, N) float64, or its float32 rounding for dtype=np.float32."""
        x, is64 = as_frames(frames)
        F, N, _ = x.shape
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(semiaxes, dtype=np.float64), (F, 3)))
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"dtype must be float32 or float64, got {dtype}")
        out = np.empty((F, N), dtype)
        self._check(self.dll.gd_lamina_distances(self._h, x.ctypes.data, int(is64), F, N, s.ctypes.data, out.ctypes.data,
                                                 int(dtype == np.float64)))
        return out

    def contacts(self, distances, contact_distance):
        """distances (F, N) float32; returns distances < contact_distance as (F, N) bool and adds it to the handle's sum."""
        d = np.ascontiguousarray(distances, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError(f"distances must be (F, N), got {d.shape}")
        out = np.empty(d.shape, np.uint8)
        self._check(self.dll.gd_lamina_contacts(self._h, d.ctypes.data, d.shape[0], d.shape[1], float(contact_distance), out.ctypes.data))
        self._note_shape(d.shape)
        return out.view(np.bool_)

    def _note_shape(self, shape):
        """The (F, N) of the handle's sum, which average() returns: set by every call that adds contacts (live.lamina_contacts too)."""
        self._shape = tuple(shape)

    def average(self):
        """float32 (F, N): the sum of the contacts since reset() over the number of contacts() calls."""
        out = np.empty(self._shape if self._shape is not None else (0, 0), np.float32)
        self._check(self.dll.gd_lamina_average(self._h, out.ctypes.data))
        return out

    def reset(self):
        self._check(self.dll.gd_lamina_reset(self._h))
        self._shape = None

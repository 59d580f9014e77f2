"""Radial distribution functions on the device: ctypes binding of ``include/gdyn_rdf.h`` (exported by ``csrc/libgdyn.so``)
and the normalisation of the reference's 4-sim-ab/box/src/rdf_analysis and rdf_analysis_hetero (distance_histogram.cc).

    r = Rdf(device=0)
    counts = r.counts(frames, box, 0.1, 1.0, centers)            # self mode: unordered pairs, (F, n_bins) uint64
    counts = r.counts(frames, box, 0.1, 1.0, centers, targets)   # cross mode: (centre, target) pairs
    g = posterior(counts, 0.1, 1.0, box_size, len(centers))      # rdf_analysis's values; n_target=len(targets) for hetero
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._binding import GdynError, Handle, as_frames, load_library

RDF_ABI_VERSION = 1        # GD_RDF_ABI_VERSION of the include/gdyn_rdf.h this binding mirrors
RDF_SYMBOLS = ["gd_rdf_abi_version", "gd_rdf_create", "gd_rdf_destroy", "gd_rdf_set_selection", "gd_rdf_bins", "gd_rdf_counts"]
LDS_BINS = 8192            # GD_RDF_LDS_BINS: above this many bins the device counts with global atomics
PI = 3.1416                # distance_histogram.cc:12


class _RdfDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_launch", C.c_uint32)]


def load_rdf_library(path=None):
    """Loads libgdyn and checks the gd_rdf_* symbols and their ABI version."""
    d = load_library("rdf", RDF_SYMBOLS, RDF_ABI_VERSION, path)
    d.gd_rdf_create.argtypes = [C.POINTER(_RdfDesc), C.POINTER(C.c_void_p)]
    d.gd_rdf_destroy.argtypes = [C.c_void_p]
    d.gd_rdf_set_selection.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    d.gd_rdf_bins.argtypes = [C.c_double, C.c_double]
    d.gd_rdf_bins.restype = C.c_uint32
    d.gd_rdf_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_double * 3), C.c_double, C.c_double, C.c_void_p]
    return d


def n_bins(bin_width, max_distance):
    """distance_histogram.cc:25: ceil(max_distance / bin_width)."""
    return int(math.ceil(max_distance / bin_width))


def bin_volumes(bin_width, max_distance):
    """distance_histogram.cc:27-36: 4 PI / 3 (r_max^3 - r_min^3) with r_max clipped at max_distance, PI = 3.1416."""
    out = []
    for i in range(n_bins(bin_width, max_distance)):
        r_min = bin_width * float(i)
        r_max = bin_width * float(i + 1)
        if r_max > max_distance:
            r_max = max_distance
        out.append(4 * PI / 3 * (r_max * r_max * r_max - r_min * r_min * r_min))
    return np.array(out, np.float64)


def posterior(counts, bin_width, max_distance, box_size, n_center, n_target=None):
    """The printed values: count * unit_weight / bin_volume / expected_density per frame and bin (float64).
    Self mode (n_target None, rdf_analysis): unit_weight 2 / n_center, expected density n_center / box^3.
    Cross mode (rdf_analysis_hetero): unit_weight 1 / n_center, expected density n_target / box^3."""
    c = np.asarray(counts, dtype=np.uint64)
    volume = box_size * box_size * box_size
    with np.errstate(divide="ignore", invalid="ignore"):
        if n_target is None:
            weight, expected = np.float64(2) / np.float64(n_center), np.float64(n_center) / np.float64(volume)
        else:
            weight, expected = np.float64(1) / np.float64(n_center), np.float64(n_target) / np.float64(volume)
        return c.astype(np.float64) * weight / bin_volumes(bin_width, max_distance) / expected


class Rdf(Handle):
    """One device-side selection; counts() uploads frames and returns their pair counts per bin.
    max_frames_per_launch: 0 = automatic (the counts do not depend on it)."""

    _destroy = "gd_rdf_destroy"

    def __init__(self, device=0, max_frames_per_launch=0, path=None):
        super().__init__(load_rdf_library(path))
        self._check(self.dll.gd_rdf_create(C.byref(_RdfDesc(device, max_frames_per_launch)), C.byref(self._h)))

    def set_selection(self, n_points, centers, targets=None):
        """The selection of the counts to come: centres alone (self mode) or centres against targets, as indices into
        n_points beads.  counts() sets it itself; live.rdf_counts uses the one in force."""
        c = np.ascontiguousarray(centers, dtype=np.uint32).ravel()
        t = None if targets is None else np.ascontiguousarray(targets, dtype=np.uint32).ravel()
        self._check(self.dll.gd_rdf_set_selection(self._h, n_points, c.ctypes.data, len(c), None if t is None else t.ctypes.data,
                                                  0 if t is None else len(t)))

    def counts(self, frames, box, bin_width, max_distance, centers, targets=None):
        """frames (F, N, 3) float32 or float64 (or one (N, 3) frame); box: a period or three; centers / targets: bead indices.
        Returns uint64 (F, n_bins)."""
        x, is64 = as_frames(frames)
        F, N, _ = x.shape
        self.set_selection(N, centers, targets)
        b = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
        nb = self.dll.gd_rdf_bins(float(bin_width), float(max_distance))
        out = np.zeros((F, max(nb, 1)), np.uint64)
        self._check(self.dll.gd_rdf_counts(self._h, x.ctypes.data, int(is64), F, C.byref((C.c_double * 3)(*b)), float(bin_width),
                                           float(max_distance), out.ctypes.data))
        return out[:, :nb]

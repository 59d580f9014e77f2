"""The device analyses fed from a running stepper: ctypes binding of ``include/gdyn_live.h`` (exported by
``csrc/libgdyn.so``).  Each function equals, byte for byte, the host-fed sequence it replaces, without the positions or the
contact rows leaving the device:

    sys.run(...); sys.contacts_update(0.12)
    live.contacts(sys, cm)                          # for r: cm.accumulate(sys.contacts(r))
    d = live.lamina_distances(sys, lam)             # lam.distances(sys.positions_f32(), semiaxes of every replica, float32)
    c = live.lamina_contacts(sys, lam, 0.3)         # lam.contacts(d, 0.3); want_contacts=False: only the handle's sum
    n = live.rdf_counts(sys, rdf, 0.05, 1.0)        # rdf's selection over sys.positions_f32() in the system's box

The flow analyses need a history of frames, which ``History`` records on the device:

    with live.History(sys, replicas=[0, 2]) as hist:
        for _ in range(frames):
            sys.run(...); hist.record()             # what sys.positions_f32(quantize=True) gives, kept on the device
        pos, vel = fl.velocities_from(hist, 2)      # fl.velocities(np.stack(those frames of replica 2)); fl: a flow.Flow

The frames of the lamina and rdf calls are the R replicas at the present step.  The system and the analysis handle must live
on one device and in one loaded library (the product library, as ``load()`` gives it).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import ALL_REPLICAS, GdynError
from ._binding import Handle, load_library

LIVE_ABI_VERSION = 2       # GD_LIVE_ABI_VERSION of the include/gdyn_live.h this binding mirrors
LIVE_SYMBOLS = ["gd_live_abi_version", "gd_live_contacts", "gd_live_lamina_distances", "gd_live_lamina_contacts", "gd_live_rdf_counts",
                "gd_live_history_create", "gd_live_history_destroy", "gd_live_history_record", "gd_live_history_frames",
                "gd_live_history_fetch", "gd_live_history_clear", "gd_live_flow_set_history"]

_dll = None


def load_live_library(path=None):
    """Loads libgdyn and checks the gd_live_* symbols and their ABI version."""
    d = load_library("live", LIVE_SYMBOLS, LIVE_ABI_VERSION, path)
    d.gd_live_contacts.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    d.gd_live_lamina_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    d.gd_live_lamina_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    d.gd_live_rdf_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
    d.gd_live_history_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    d.gd_live_history_destroy.argtypes = [C.c_void_p]
    d.gd_live_history_record.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    d.gd_live_history_frames.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    d.gd_live_history_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    d.gd_live_history_clear.argtypes = [C.c_void_p]
    d.gd_live_flow_set_history.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return d


def _call(fn, *args):
    global _dll
    if _dll is None:
        _dll = load_live_library()
    rc = getattr(_dll, fn)(*args)
    if rc != 0:
        raise GdynError(rc, _dll.gd_last_error().decode(errors="replace"))


def contacts(system, contact_maps, replica=ALL_REPLICAS):
    """Streams the contact table of one replica, or of all, through every target of ``contact_maps`` (a ContactMaps)."""
    _call("gd_live_contacts", system._h, int(replica), contact_maps._h)


def lamina_distances(system, lamina, quantize=False, dtype=np.float32):
    """(R, N) distances of every replica's beads from its current wall, float32 or float64."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"dtype must be float32 or float64, got {dtype}")
    out = np.empty((system.R, system.N), dtype)
    _call("gd_live_lamina_distances", system._h, lamina._h, int(quantize), out.ctypes.data, int(dtype == np.float64))
    return out


def lamina_contacts(system, lamina, contact_distance, quantize=False, want_contacts=True):
    """Adds float32 distance < contact_distance of every (replica, bead) into ``lamina``'s sum, as Lamina.contacts does;
    returns the (R, N) bool contacts, or None for want_contacts=False (nothing is copied back: the mode of a long run)."""
    out = np.empty((system.R, system.N), np.uint8) if want_contacts else None
    _call("gd_live_lamina_contacts", system._h, lamina._h, int(quantize), float(contact_distance), None if out is None else out.ctypes.data)
    lamina._note_shape((system.R, system.N))
    return None if out is None else out.view(np.bool_)


def rdf_counts(system, rdf, bin_width, max_distance, quantize=False):
    """uint64 (R, n_bins) pair counts of ``rdf``'s current selection (gd_rdf_set_selection) in every replica."""
    nb = rdf.dll.gd_rdf_bins(float(bin_width), float(max_distance))
    out = np.zeros((system.R, max(nb, 1)), np.uint64)
    _call("gd_live_rdf_counts", system._h, rdf._h, int(quantize), float(bin_width), float(max_distance), out.ctypes.data)
    return out[:, :nb]


class History(Handle):
    """A device-resident recorder of ``system``'s frames: float32 (F, N, 3) per recorded replica, in blocks of ``frames_per_block``
    frames (0: about 256 MiB) that are allocated as needed and never moved.  replicas: the ids to record, None for all."""

    _destroy = "gd_live_history_destroy"

    def __init__(self, system, replicas=None, frames_per_block=0, path=None):
        super().__init__(load_live_library(path))
        ids = np.ascontiguousarray([] if replicas is None else replicas, dtype=np.uint32)
        self.replicas = list(range(system.R)) if replicas is None else [int(r) for r in ids]
        self.N = system.N
        self._system = system
        self._check(self.dll.gd_live_history_create(system._h, ids.ctypes.data if len(ids) else None, len(ids), int(frames_per_block),
                                                    C.byref(self._h)))

    def record(self, quantize=True, system=None):
        """Appends the present frame of every recorded replica: positions_f32(quantize)[r] of the system the recorder was made
        for (or of another one of its shape and device), without leaving the device."""
        self._check(self.dll.gd_live_history_record(self._h, (system or self._system)._h, int(quantize)))

    @property
    def frames(self):
        n = C.c_uint32()
        self._check(self.dll.gd_live_history_frames(self._h, C.byref(n)))
        return n.value

    def fetch(self, replica, first=0, count=None):
        """Frames [first, first + count) of one recorded replica, float32 (count, N, 3); count=None: up to the last one."""
        if count is None:
            count = max(self.frames - int(first), 0)
        out = np.empty((int(count), self.N, 3), np.float32)
        self._check(self.dll.gd_live_history_fetch(self._h, int(replica), int(first), int(count), out.ctypes.data))
        return out

    def set_history(self, flow, replica):
        """flow's history becomes the recorded frames of ``replica`` (a flow.Flow; Flow.velocities_from calls this)."""
        self._check(self.dll.gd_live_flow_set_history(self._h, int(replica), flow._h))

    def clear(self):
        """Forgets the frames and keeps the blocks."""
        self._check(self.dll.gd_live_history_clear(self._h))

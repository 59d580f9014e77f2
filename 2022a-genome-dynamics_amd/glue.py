"""Glue kinetics on the device: ctypes binding of ``include/gdyn_glue.h`` (exported by ``csrc/libgdyn.so``).  The stochastic binding
and unbinding of bead pairs of every replica of a handle in one call, from the positions and the pair search the device holds; the
bound pairs act through a per-replica slot of ``replica.py``:

    replica.define(sys, 1, glue_bond)                               # the pairs' potential
    glue.define(sys, 1, max_glues, reach, binding_rate, unbinding_rate)
    for epoch in range(n):
        sys.run(...)
        glue.update(sys, dt, epoch, seeds)                          # all replicas; the new sets are installed in the slot
    glue.counts(sys); glue.fetch(sys, r)                            # (n, 2) sorted, i < j

The rule is stated in the header and in DESIGN.md section 7k; ``tests/glue_restatement.py`` restates it in numpy.  The draws are
counter-based (Philox of pair, epoch and the replica's seed): the same state, epoch and seeds give the same sets.  The system must
come from the product library (``load()``): the oracle has no device glue kinetics.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import GdynError
from ._binding import load_library

GLUE_ABI_VERSION = 1    # GD_GLUE_ABI_VERSION of the include/gdyn_glue.h this binding mirrors
GLUE_SYMBOLS = ["gd_glue_abi_version", "gd_glue_define", "gd_glue_update", "gd_glue_set", "gd_glue_fetch", "gd_glue_counts"]


class GlueParams(C.Structure):
    _fields_ = [("max_glues", C.c_uint32), ("reach", C.c_double), ("binding_rate", C.c_double), ("unbinding_rate", C.c_double)]


_dll = None


def load_glue_library(path=None):
    """Loads libgdyn and checks the gd_glue_* symbols and their ABI version."""
    d = load_library("glue", GLUE_SYMBOLS, GLUE_ABI_VERSION, path)
    d.gd_glue_define.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(GlueParams)]
    d.gd_glue_update.argtypes = [C.c_void_p, C.c_double, C.c_uint64, C.c_void_p]
    d.gd_glue_set.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    d.gd_glue_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    d.gd_glue_counts.argtypes = [C.c_void_p, C.c_void_p]
    return d


def _call(fn, *args):
    global _dll
    if _dll is None:
        _dll = load_glue_library()
    rc = getattr(_dll, fn)(*args)
    if rc != 0:
        raise GdynError(rc, _dll.gd_last_error().decode(errors="replace"))


def define(system, slot, max_glues, reach, binding_rate, unbinding_rate):
    """Manages per-replica slot ``slot`` (declared with replica.define); again: new parameters, the sets are kept."""
    p = GlueParams(int(max_glues), float(reach), float(binding_rate), float(unbinding_rate))
    _call("gd_glue_define", system._h, int(slot), C.byref(p))


def update(system, dt, epoch, seeds):
    """One update of every replica over the time ``dt``; ``seeds``: one unsigned 64-bit seed per replica."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    if seeds.shape != (system.R,):
        raise ValueError(f"seeds must hold one seed per replica ({system.R}), got shape {seeds.shape}")
    _call("gd_glue_update", system._h, float(dt), int(epoch), seeds.ctypes.data)


def set_pairs(system, replica, pairs):
    """Replaces one replica's set: (n, 2) bead ids in any order and orientation; empty: no pairs."""
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    _call("gd_glue_set", system._h, int(replica), pairs.ctypes.data if len(pairs) else None, len(pairs))


def fetch(system, replica):
    """The set of one replica: (n, 2) uint32, i < j, ascending."""
    n = C.c_uint32()
    _call("gd_glue_fetch", system._h, int(replica), None, 0, C.byref(n))
    out = np.zeros((n.value, 2), dtype=np.uint32)
    if n.value:
        _call("gd_glue_fetch", system._h, int(replica), out.ctypes.data, n.value, C.byref(n))
    return out


def counts(system):
    """The sizes of all replicas' sets."""
    out = np.zeros(system.R, dtype=np.uint32)
    _call("gd_glue_counts", system._h, out.ctypes.data)
    return out

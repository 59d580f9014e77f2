"""Per-replica A/B tables of a stepper: ctypes binding of ``include/gdyn_ensemble.h`` (exported by ``csrc/libgdyn.so``).
Where ``System.set_bead_params(a=, b=)`` gives every replica of a handle the same (a, b) factors, each replica gets its own here --
a genome model and its randomised controls, the same beads and bonds under other annotations, batched in one handle:

    for r, (a, b) in enumerate(tables):
        ensemble.set_ab(sys, r, a, b)               # either column may be left out: that column of the replica is kept
    sys.run(...)                                    # the mixed pair, wall and bond terms of replica r read table r
    ensemble.get_ab(sys, r)                         # what the next evaluation uses (the shared table if never set)
    ensemble.classes(sys)                           # (class of every replica, number of classes): equal tables share a class

A handle whose replicas all hold one table -- never set, or set to equal tables -- runs exactly as before.  The system must come
from the product library (``load()``): the oracle has one table per handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import GdynError
from ._binding import load_library

ENSEMBLE_ABI_VERSION = 1    # GD_ENSEMBLE_ABI_VERSION of the include/gdyn_ensemble.h this binding mirrors
ENSEMBLE_SYMBOLS = ["gd_ensemble_abi_version", "gd_ensemble_set_ab", "gd_ensemble_get_ab", "gd_ensemble_classes"]

_dll = None


def load_ensemble_library(path=None):
    """Loads libgdyn and checks the gd_ensemble_* symbols and their ABI version."""
    d = load_library("ensemble", ENSEMBLE_SYMBOLS, ENSEMBLE_ABI_VERSION, path)
    d.gd_ensemble_set_ab.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    d.gd_ensemble_get_ab.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    d.gd_ensemble_classes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    return d


def _call(fn, *args):
    global _dll
    if _dll is None:
        _dll = load_ensemble_library()
    rc = getattr(_dll, fn)(*args)
    if rc != 0:
        raise GdynError(rc, _dll.gd_last_error().decode(errors="replace"))


def _column(system, v, name):
    if v is None:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.shape != (system.N,):
        raise ValueError(f"{name} must hold one value per bead ({system.N}), got shape {v.shape}")
    return v


def set_ab(system, replica, a=None, b=None):
    """Replaces the table of one replica; a column left None is kept."""
    a, b = _column(system, a, "a"), _column(system, b, "b")
    _call("gd_ensemble_set_ab", system._h, int(replica), None if a is None else a.ctypes.data, None if b is None else b.ctypes.data)


def get_ab(system, replica):
    """(a, b) of one replica as the next evaluation uses them."""
    a, b = np.empty(system.N), np.empty(system.N)
    _call("gd_ensemble_get_ab", system._h, int(replica), a.ctypes.data, b.ctypes.data)
    return a, b


def classes(system):
    """(class_of, n_classes): replicas with identical tables share a class, classes numbered by first appearance."""
    class_of = np.empty(system.R, dtype=np.uint32)
    n = C.c_uint32()
    _call("gd_ensemble_classes", system._h, class_of.ctypes.data, C.byref(n))
    return class_of, n.value

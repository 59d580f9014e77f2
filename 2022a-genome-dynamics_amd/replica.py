"""Per-replica dynamic pair lists of a stepper: ctypes binding of ``include/gdyn_replica.h`` (exported by ``csrc/libgdyn.so``).
Where ``System.set_dynamic_pairs`` gives every replica of a handle the same list, each replica gets its own here -- the loops and
glues of one trajectory of an ensemble:

    replica.define(sys, 0, loop_params)             # slot 0 .. 3, separate from the shared slots; lists start empty
    for r in range(sys.R):
        replica.set_pairs(sys, 0, r, loops[r])      # stored on the host; no topology work, the resident neighbour list stays
    sys.run(...)                                    # one upload for all the sets since the last evaluation
    replica.count(sys, 0, r)

The pairs contribute to TERM_DYNAMIC in ``run``, ``forces`` and ``energy``.  The system must come from the product library
(``load()``): the oracle has no per-replica lists.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import BondParams, GdynError
from ._binding import load_library

REPLICA_ABI_VERSION = 1    # GD_REPLICA_ABI_VERSION of the include/gdyn_replica.h this binding mirrors
REPLICA_SYMBOLS = ["gd_replica_abi_version", "gd_replica_pairs_define", "gd_replica_pairs_set", "gd_replica_pairs_count"]

_dll = None


def load_replica_library(path=None):
    """Loads libgdyn and checks the gd_replica_* symbols and their ABI version."""
    d = load_library("replica", REPLICA_SYMBOLS, REPLICA_ABI_VERSION, path)
    d.gd_replica_pairs_define.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(BondParams)]
    d.gd_replica_pairs_set.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    d.gd_replica_pairs_count.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return d


def _call(fn, *args):
    global _dll
    if _dll is None:
        _dll = load_replica_library()
    rc = getattr(_dll, fn)(*args)
    if rc != 0:
        raise GdynError(rc, _dll.gd_last_error().decode(errors="replace"))


def define(system, slot, params):
    """Declares per-replica slot ``slot`` with ``params`` (System.bond_params); again: new parameters, the lists are kept."""
    _call("gd_replica_pairs_define", system._h, int(slot), C.byref(params))


def set_pairs(system, slot, replica, pairs):
    """Replaces the list of one replica of a defined slot: (n, 2) bead ids, i != j; empty: no pairs."""
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    _call("gd_replica_pairs_set", system._h, int(slot), int(replica), pairs.ctypes.data if len(pairs) else None, len(pairs))


def count(system, slot, replica):
    """Pairs currently set: what the next evaluation uses."""
    n = C.c_uint32()
    _call("gd_replica_pairs_count", system._h, int(slot), int(replica), C.byref(n))
    return n.value

"""Flow fields of a trajectory history on the device: ctypes binding of ``include/gdyn_flow.h`` (exported by
``csrc/libgdyn.so``) and the host-side helpers of the reference's analyses (5-sim-genome/src/analyze_particle_flow,
analyze_grid_flow): the grid mesh, the stored config JSON and its hashed name.

    fl = Flow(device=0)
    pos, vel = fl.velocities(history, smoothing=0, delay=1)   # history: (F, N, 3) float32 or float64
    flows = fl.particle(0.6)                                  # (F, N, 3) float32
    flows, coverage = fl.grid(0.6, points)                    # (F, G, 3) float32, (F, G) int32
    pos, vel = fl.velocities_from(recorder, replica)          # the same from frames a live.History recorded on the device
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json

import numpy as np

from ._binding import GdynError, Handle, as_frames, load_library

FLOW_ABI_VERSION = 1       # GD_FLOW_ABI_VERSION of the include/gdyn_flow.h this binding mirrors
FLOW_SYMBOLS = ["gd_flow_abi_version", "gd_flow_create", "gd_flow_destroy", "gd_flow_set_history", "gd_flow_velocities",
                "gd_flow_particle", "gd_flow_grid"]
HASHNAME_LENGTH = 7


class _FlowDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_launch", C.c_uint32)]


def load_flow_library(path=None):
    """Loads libgdyn and checks the gd_flow_* symbols and their ABI version."""
    d = load_library("flow", FLOW_SYMBOLS, FLOW_ABI_VERSION, path)
    d.gd_flow_create.argtypes = [C.POINTER(_FlowDesc), C.POINTER(C.c_void_p)]
    d.gd_flow_destroy.argtypes = [C.c_void_p]
    d.gd_flow_set_history.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    d.gd_flow_velocities.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    d.gd_flow_particle.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    d.gd_flow_grid.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return d


class Flow(Handle):
    """One device-side history.  velocities() uploads it and computes the (smoothed) positions and velocities; particle()
    and grid() then reduce them around beads or points.  max_frames_per_launch: 0 = automatic (results do not depend on it)."""

    _destroy = "gd_flow_destroy"

    def __init__(self, device=0, max_frames_per_launch=0, path=None):
        super().__init__(load_flow_library(path))
        self._check(self.dll.gd_flow_create(C.byref(_FlowDesc(device, max_frames_per_launch)), C.byref(self._h)))
        self.shape = None

    def velocities(self, history, smoothing=0, delay=1):
        """history (F, N, 3): returns the (smoothed, float64) positions and the float64 velocities, both (F, N, 3)."""
        h = np.asarray(history)      # a single (N, 3) frame, which as_frames would take, is no history
        if h.ndim != 3 or h.shape[2] != 3:
            raise ValueError(f"history must be (F, N, 3), got {h.shape}")
        h, is64 = as_frames(h)
        F, N, _ = h.shape
        self._check(self.dll.gd_flow_set_history(self._h, h.ctypes.data, F, N, int(is64)))
        pos = np.empty((F, N, 3), np.float64)
        vel = np.empty((F, N, 3), np.float64)
        self._check(self.dll.gd_flow_velocities(self._h, int(smoothing or 0), int(delay), pos.ctypes.data, vel.ctypes.data))
        self.shape = (F, N)
        return pos, vel

    def velocities_from(self, history, replica, smoothing=0, delay=1):
        """velocities(the stacked frames that ``history`` (a live.History) recorded of ``replica``, smoothing, delay), with the
        frames going from the recorder to this handle on the device."""
        history.set_history(self, replica)
        F, N = history.frames, history.N
        pos = np.empty((F, N, 3), np.float64)
        vel = np.empty((F, N, 3), np.float64)
        self._check(self.dll.gd_flow_velocities(self._h, int(smoothing or 0), int(delay), pos.ctypes.data, vel.ctypes.data))
        self.shape = (F, N)
        return pos, vel

    def particle(self, radius):
        F, N = self.shape or (0, 0)
        out = np.empty((F, N, 3), np.float32)
        self._check(self.dll.gd_flow_particle(self._h, float(radius), out.ctypes.data))
        return out

    def grid(self, radius, points):
        F = (self.shape or (0, 0))[0]
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        G = len(p)
        flows = np.empty((F, G, 3), np.float32)
        cov = np.empty((F, G), np.int32)
        self._check(self.dll.gd_flow_grid(self._h, float(radius), p.ctypes.data, G, flows.ctypes.data, cov.ctypes.data))
        return flows, cov


def make_grid(x_range, y_range, z_range, interval):
    """analyze_grid_flow's mesh: inclusive aranges, points in np.meshgrid(x, y, z) ('xy') order.
    Returns (points (G,3) float64, indices (G,3) int64, shape [len(x), len(y), len(z)])."""
    eps = interval * 0.1
    axes = [np.arange(a, b + eps, interval) for a, b in (x_range, y_range, z_range)]
    points = np.moveaxis(np.meshgrid(*axes), 0, -1).reshape(-1, 3)
    indices = np.moveaxis(np.meshgrid(*[np.arange(len(a)) for a in axes]), 0, -1).reshape(-1, 3).astype(np.int64)
    return points, indices, [len(a) for a in axes]


def config_json(smoothing, velocity_delay, scan_radius, grid_interval=None, x_range=None, y_range=None, z_range=None):
    """The .config string the analyses store (grid mode when grid_interval is given)."""
    c = {"smoothing": smoothing, "velocity_delay": velocity_delay, "scan_radius": scan_radius}
    if grid_interval is not None:
        c.update(grid_interval=grid_interval, x_range=list(x_range), y_range=list(y_range), z_range=list(z_range))
    return json.dumps(c)


def config_name(config):
    """The analysis name when --name is absent: the first 7 hex digits of the config's SHA-256."""
    return hashlib.sha256(config.encode("utf-8")).hexdigest()[:HASHNAME_LENGTH]

#!/usr/bin/env python3
"""Generates tests/golden/flow_fixtures.npz (+ .json) by IMPORTING the reference's own analysis modules
(5-sim-genome/src/analyze_particle_flow/analysis.py, analyze_grid_flow/analysis.py and their utils.py) and recording their
outputs for small fixed inputs.  numba and h5py are not installed here: both are stubbed in sys.modules (numba.njit = the
identity; no h5py function is called).  Only inputs and outputs are stored; run where the reference tree exists:
    python tests/golden/make_flow_fixtures.py"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.modules.setdefault("numba", types.SimpleNamespace(njit=lambda f: f))
sys.modules.setdefault("h5py", types.ModuleType("h5py"))
sys.path.insert(0, "/root/reference/5-sim-genome/src")
from analyze_grid_flow import analysis as grid_ref  # noqa: E402
from analyze_particle_flow import analysis as particle_ref  # noqa: E402
from analyze_particle_flow.utils import gaussian_smooth  # noqa: E402

F, N = 9, 240
SMOOTHINGS = [1, 2, 4, 7, 12]          # 12 > F: numpy's repeated reflection
DELAYS = [0, 1, 2, 3, 6]
RADII = [0.35, 0.6]
GRID = dict(x_range=(-1.5, 1.55), y_range=(-1.2, 1.4), z_range=(-1.0, 1.0), interval=0.3)     # lengths not multiples of 0.3
TIE_GRID = dict(x_range=(-1.5, 1.5), y_range=(-1.5, 1.5), z_range=(-1.5, 1.5), interval=0.5)


def quantize(x):
    return np.round(np.asarray(x, np.float64) * 65536.0) / 65536.0


def history():
    rng = np.random.default_rng(2022)
    x = rng.uniform(-1.5, 1.5, size=(N, 3)) + np.cumsum(rng.normal(scale=0.05, size=(F, N, 3)), axis=0)
    x[:, 1] = x[:, 0]                         # a coincident pair in every frame
    x[:, 2] = x[:, 0] + [0.5, 0.0, 0.0]       # an exact dyadic tie at r = 0.5 (after quantisation)
    x[:, 3] = [0.5, 0.0, 0.0]                 # at 0.5 from the tie grid's points (0,0,0), (1,0,0), (0.5,+-0.5,0) ...
    x[:, 4] = [-1.0, -1.0, -1.0]              # on a tie-grid point
    return quantize(x).astype(np.float32)


def grid_of(g):
    eps = g["interval"] * 0.1
    axes = [np.arange(a, b + eps, g["interval"]) for a, b in (g["x_range"], g["y_range"], g["z_range"])]
    pts, idx = grid_ref.make_grid(*axes)
    return pts, idx, np.array([len(a) for a in axes])


def particle_flows(pos, vel, r):
    return np.array([particle_ref.compute_flow(pos[f], vel[f], r) for f in range(len(pos))], dtype=np.float32)


def grid_flows(points, pos, vel, r):
    import scipy.spatial
    tree = scipy.spatial.cKDTree(points)
    res = [grid_ref.compute_flow(tree, pos[f], vel[f], r) for f in range(len(pos))]
    return np.array([a for a, _ in res], np.float32), np.array([b for _, b in res], np.int32)


def main():
    hist = history()
    out = {"history": hist}
    cases = {"particle": [], "grid": []}
    for w in SMOOTHINGS:
        # float32 input: scipy's FFT of the padded history runs in single precision (rounding ~1e-7 of max|x|);
        # the float64 copy pins the filter itself
        out[f"smooth_w{w}"] = gaussian_smooth(hist, w)
        out[f"smooth64_w{w}"] = gaussian_smooth(hist.astype(np.float64), w)
    sources = {"raw": hist, "s4": out["smooth_w4"]}
    for sname, pos in sources.items():
        for d in DELAYS:
            out[f"vel_{sname}_d{d}"] = particle_ref.compute_velocities(pos, d)
    for sname, d in [("raw", 1), ("s4", 2)]:
        pos, vel = sources[sname], out[f"vel_{sname}_d{d}"]
        for r in RADII:
            key = f"pflow_{sname}_d{d}_r{r}"
            out[key] = particle_flows(pos, vel, r)
            cases["particle"].append({"key": key, "source": sname, "delay": d, "radius": r})
    # exact ties and coincident beads: raw history, delay 2 (no NaN frame)
    out["pflow_tie"] = particle_flows(hist, out["vel_raw_d2"], 0.5)
    cases["particle"].append({"key": "pflow_tie", "source": "raw", "delay": 2, "radius": 0.5})

    for gname, g in [("grid", GRID), ("tiegrid", TIE_GRID)]:
        pts, idx, shape = grid_of(g)
        out[f"{gname}_points"], out[f"{gname}_indices"], out[f"{gname}_shape"] = pts, idx, shape
    for sname, d, r, gname in [("raw", 1, 0.6, "grid"), ("s4", 2, 0.35, "grid"), ("raw", 2, 0.5, "tiegrid")]:
        key = f"gflow_{sname}_d{d}_r{r}_{gname}"
        fl, cov = grid_flows(out[f"{gname}_points"], sources[sname], out[f"vel_{sname}_d{d}"], r)
        out[key], out[key.replace("gflow", "gcov")] = fl, cov
        factor = grid_ref.estimate_scaleoffset_factor(fl, q=1)
        cases["grid"].append({"key": key, "source": sname, "delay": d, "radius": r, "grid": gname, "scaleoffset": factor})
    np.savez_compressed(os.path.join(HERE, "flow_fixtures.npz"), **out)
    meta = {"frames": F, "beads": N, "smoothings": SMOOTHINGS, "delays": DELAYS, "grids": {"grid": GRID, "tiegrid": TIE_GRID},
            "cases": cases}
    with open(os.path.join(HERE, "flow_fixtures.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print("ok", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Flow analyses at the 62 178-bead scale: one history of 701 frames (a seeded random walk in a sphere of radius 8, the
model's density), scan radius 0.6, a +-8.5 grid at 0.3.  Prints one JSON line (and writes it to --out):
  device     host-clock seconds of Flow.velocities / particle / grid (each ends in a device synchronise), per frame;
  programs   gd_particle_flow / gd_grid_flow on one file of the same history: wall time and their read / compute / write split;
  kdtree     the cKDTree restatement (query_pairs + accumulation) in seconds per frame on this host's CPU.
Kernel times come from a separate run under rocprofv3 (--device-only skips the programs and the CPU restatement):
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_flow.py --device-only"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flow = importlib.import_module("2022a-genome-dynamics_amd.flow")
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
N, R, GRID = 62178, 0.6, ((-8.5, 8.5), (-8.5, 8.5), (-8.5, 8.5), 0.3)


def walk(n, frames, radius, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x = u * radius * rng.uniform(size=(n, 1)) ** (1 / 3)
    out = np.empty((frames, n, 3), np.float32)
    for f in range(frames):
        x = x + rng.normal(scale=0.05, size=x.shape)
        nr = np.linalg.norm(x, axis=1)
        x[nr > radius] *= (radius / nr[nr > radius])[:, None]
        out[f] = np.round(x * 65536) / 65536
    return out


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=701)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hist = walk(N, a.frames, 8.0, 11)
    points = flow.make_grid(*GRID)[0]
    res = {"beads": N, "frames": a.frames, "grid_points": len(points), "radius": R}
    with flow.Flow(0) as f:
        f.velocities(hist[:4], 0, 1)       # warm-up: code objects, rocPRIM's algorithm choice
        f.particle(R)
        f.grid(R, points)
        (_, vel), t_v = timed(lambda: f.velocities(hist, 0, 1))
        _, t_p = timed(lambda: f.particle(R))
        (_, cov), t_g = timed(lambda: f.grid(R, points))
    res["device_s_per_frame"] = {"velocities": t_v / a.frames, "particle": t_p / a.frames, "grid": t_g / a.frames}
    res["mean_grid_coverage"] = float(cov[1:].mean())
    if not a.device_only:
        import scipy.spatial
        ts = []
        for fr in (1, a.frames // 2, a.frames - 1):
            x, v = hist[fr].astype(np.float64), np.nan_to_num(vel[fr])
            t = time.perf_counter()
            p = scipy.spatial.cKDTree(x).query_pairs(R, output_type="ndarray")
            s = v.copy()
            np.add.at(s, p[:, 0], v[p[:, 1]])
            np.add.at(s, p[:, 1], v[p[:, 0]])
            ts.append(time.perf_counter() - t)
        res["kdtree_s_per_frame"] = float(np.median(ts))
        res["mean_neighbours"] = 2 * len(p) / N
        with tempfile.TemporaryDirectory() as tmp:
            traj = os.path.join(tmp, "traj.h5")
            raw = os.path.join(tmp, "x.f64")
            for fr in range(a.frames):
                hist[fr].astype("<f8").tofile(raw)
                subprocess.check_call([os.path.join(HOST, "gd_h5tool"), "put-positions", traj, "interphase", str(100 * fr), raw])
            progs = {"particle": ["gd_particle_flow", "--scan-radius", str(R)],
                     "grid": ["gd_grid_flow", "--scan-radius", str(R), "--grid-interval", "0.3", "--x-range=-8.5,8.5",
                              "--y-range=-8.5,8.5", "--z-range=-8.5,8.5"]}
            res["programs"] = {}
            for key, cmd in progs.items():
                t = time.perf_counter()
                r = subprocess.run([os.path.join(HOST, cmd[0]), *cmd[1:], os.path.join(tmp, f"{key}.h5"), traj],
                                   capture_output=True, text=True, check=True)
                wall = time.perf_counter() - t
                m = re.search(r"read ([\d.]+) s, compute ([\d.]+) s, write ([\d.]+) s", r.stderr)
                res["programs"][key] = {"wall_s": wall, "read_s": float(m[1]), "compute_s": float(m[2]), "write_s": float(m[3])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

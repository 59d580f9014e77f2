#!/usr/bin/env python3
"""The displacement correlation (include/gdyn_dcorr.h, dcorr.py) at the size a user runs it, host clock around the synchronous
calls, median (min - max) of five each, one JSON line:

  genome shape: 62 178 beads float32 at ~120 beads per unit volume (a ball of radius 5: ~500 partners within 1.0), four bead
  classes in blocks along the genome, 46 chromosome-like chains, open box, max_distance 1.0, bin width 0.02 (50 bins, 20 classes);
  --frames frames (default 65: 64 origins at lag 1, 484 over 8 lags), so that the whole run takes seconds
    set_history          from host memory
    pairs, one lag       lag 1, all origins; the pair rate = counted pairs per second
    pairs, 8 lags        lags 1 .. 8, one call each
    Rdf.counts           yardstick (a): the same origin frames through rdf.py in a box wide enough to act as open -- the same pair
                         walk with a lighter body; the ratio is what the displacement payload and the 64-bit sums cost
    numpy + cKDTree      yardstick (b): tests/dcorr_restatement.py with cKDTree candidates on the same host, one frame pair, scaled
                         to the origins of the one-lag call: the only baseline there is.  Its tables must equal the device's.

--scale shrinks the bead count at the same density (a rehearsal, not a measurement).  --only pairs1 runs the one-lag case alone:
for a run under `rocprofv3 --kernel-trace --stats`, whose per-kernel means then belong to that case."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import scipy.spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dcorr_restatement as dr      # noqa: E402

dcorr = importlib.import_module("2022a-genome-dynamics_amd.dcorr")
rdf = importlib.import_module("2022a-genome-dynamics_amd.rdf")

REPEATS = 5
MD, BW = 1.0, 0.02


def timed(fn, *args, **kw):
    fn(*args, **kw)      # warm-up: code objects, buffers
    v = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        out = fn(*args, **kw)
        v.append(time.perf_counter() - t)
    return {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}, out


def ball_walk(frames, beads, radius, seed):
    """beads uniform in a ball, then independent steps plus a swirl common to neighbours"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((beads, 3))
    x0 = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(size=(beads, 1)) ** (1 / 3)
    steps = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.03) + (0.03 * np.sin(x0[:, ::-1])).astype(np.float32)
    steps[0] = 0
    return (x0.astype(np.float32) + np.cumsum(steps, axis=0, dtype=np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--only", choices=["pairs1"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, F = max(int(62178 * a.scale), 200), max(a.frames, 9)
    radius = (N / 119.4 / (4 / 3 * np.pi)) ** (1 / 3)
    x = ball_walk(F, N, radius, 1)
    label = (np.arange(N) // 50) % 4
    chain = np.searchsorted(np.round(np.cumsum(np.linspace(5.0, 1.0, 46)) / 138.0 * N), np.arange(N), side="right")
    res = {"beads": N, "frames": F, "radius": radius, "max_distance": MD, "bin_width": BW, "classes": 20, "repeats": REPEATS}
    with dcorr.Dcorr(0) as d:
        res["set_history"], _ = timed(d.set_history, x)
        d.set_labels(label, 4)
        d.set_chains(chain)
        res["pairs_1_lag"], one = timed(d.pairs, 1, BW, MD)
        res["origins_1_lag"], res["pairs_counted_1_lag"] = int(one.count.shape[0]), int(one.count.sum())
        res["scale_bits"] = one.scale_bits
        res["partners_per_bead"] = 2 * res["pairs_counted_1_lag"] / res["origins_1_lag"] / N
        res["pairs_per_s"] = res["pairs_counted_1_lag"] / res["pairs_1_lag"]["median_s"]
        if a.only:
            print(json.dumps(res))
            return
        lags = list(range(1, 9))
        res["pairs_8_lags"], many = timed(lambda: [d.pairs(lag, BW, MD) for lag in lags])
        res["origins_8_lags"] = int(sum(p.count.shape[0] for p in many))
        assert many[0].count.tobytes() == one.count.tobytes() and many[0].sum.tobytes() == one.sum.tobytes()
    # (a) the same pair walk with a lighter body
    shift = x[:F - 1] + np.float32(radius + 2.0)
    with rdf.Rdf(0) as r:
        res["rdf_counts_same_frames"], counts = timed(r.counts, shift, 2 * radius + 4.0, BW, MD, np.arange(N))
    res["rdf_pairs_counted"] = int(counts.sum())
    res["dcorr_over_rdf"] = res["pairs_1_lag"]["median_s"] / res["rdf_counts_same_frames"]["median_s"]
    # (b) numpy with cKDTree candidates, one frame pair
    if not a.skip_numpy:
        candidates = lambda p: scipy.spatial.cKDTree(p).query_pairs(MD + 1e-6, output_type="ndarray").T
        t = time.perf_counter()
        want = dr.pairs(x[:2], 1, BW, MD, None, label, 4, chain, one.scale_bits, candidates=candidates)
        res["numpy_one_frame_pair_s"] = time.perf_counter() - t
        assert np.array_equal(want[0][0], one.count[0]) and np.array_equal(want[1][0], one.sum[0]) and np.array_equal(want[3][0], one.self_sum[0])
        res["numpy_equals_device"] = True
        res["numpy_over_device"] = res["numpy_one_frame_pair_s"] * res["origins_1_lag"] / res["pairs_1_lag"]["median_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

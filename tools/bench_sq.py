#!/usr/bin/env python3
"""The structure factors and scattering functions (include/gdyn_sq.h, sq.py) at the sizes a user runs them, host clock around the
synchronous calls, median (min - max) of five each, one JSON line.  An evaluation is one (bead, vector, frame) pair of sin and cos.

  (a) amplitudes_lattice   the genome shape (701, 62 178) float32 against the lattice vectors n_max = 8 of a box: 2 456 vectors
  (b) amplitudes_64        the same history against 64 vectors: one tile of vectors, the grid filled by chunks and frames alone
  (c) self_part            8 log-spaced lags, every tenth origin, the lattice vectors
  (d) collective           the lags of (c), every origin: amplitudes of all frames plus the products
  numpy                    tests/sq_restatement.py on this host on 1/100 of (a), 7 of the 701 frames, extrapolated; and the device's
                           amplitudes of those frames checked against it within bound(n)
Beside the times: evaluations per second and the fp64 vector-unit issue slots that one evaluation takes, out of 256 CUs x 64 lanes x
2.4 GHz (a lane-instruction per slot).  These are reference points, not pass marks.  --scale shrinks every shape (a rehearsal, not
a measurement).  --only CASE runs one case alone.  --out FILE is rewritten after every case, so that a run that is cut short
leaves what it measured."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sq_restatement as sr      # noqa: E402

sq = importlib.import_module("2022a-genome-dynamics_amd.sq")

FP64_LANE_SLOTS_PER_S = 256 * 64 * 2.4e9      # CUs x lanes x clock: one fp64 vector instruction of one lane per slot


def timed(repeats, fn, *args, **kw):
    fn(*args, **kw)      # warm-up: code objects, buffers
    v = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn(*args, **kw)
        v.append(time.perf_counter() - t)
    return {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}, out


def walk(frames, beads, seed):
    """Beads spread over a box of 10 that drift a little from frame to frame."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.05)
    x[0] += rng.uniform(0, 10, size=(beads, 3)).astype(np.float32)
    return np.cumsum(x, axis=0, dtype=np.float32)


def log_lags(k, longest):
    """--log-lags of the programs (tests/msd_restatement.py)"""
    out = []
    for i in range(k):
        u = int(min(max(np.floor(float(longest) ** (i / (k - 1)) + 0.5), 1), longest))
        if not out or u > out[-1]:
            out.append(u)
    return out


def rate(t, evaluations):
    per_s = evaluations / t["median_s"]
    return dict(t, evaluations=int(evaluations), evaluations_per_s=per_s, fp64_lane_slots_per_evaluation=FP64_LANE_SLOTS_PER_S / per_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["amplitudes_lattice", "amplitudes_64", "self_part", "collective", "numpy"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(701 * a.scale), 9), max(int(62178 * a.scale), 700)
    n_max = 8 if a.scale == 1.0 else 3
    _, q = sq.Sq.lattice_vectors((10.0, 10.0, 10.0), n_max)
    Q = len(q)
    lags = log_lags(8, F - 1)
    res = {"frames": F, "beads": N, "vectors": Q, "lags": lags, "repeats": a.repeats}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    x = walk(F, N, 1)
    want = lambda name: a.only in (None, name)      # noqa: E731
    with sq.Sq(0) as s:
        res["set_history"], _ = timed(a.repeats, s.set_history, x)
        s.set_vectors(q)
        if want("amplitudes_lattice"):
            t, amp = timed(a.repeats, s.amplitudes)
            res["amplitudes_lattice"] = rate(t, F * N * Q)
            assert amp["cos_sum"].shape == (F, 1, Q)
            save()
        if want("self_part"):
            t, f = timed(a.repeats, s.self_part, lags, None, 10)
            res["self_part"] = rate(t, int(f["count"].sum()) * Q)
            res["self_part"]["origins"] = [int(c) // N for c in f["count"][:, 0]]
            save()
        if want("collective"):
            t, c = timed(a.repeats, s.collective, [0] + lags)
            res["collective"] = rate(t, F * N * Q)
            save()
        if want("amplitudes_64"):
            s.set_vectors(q[:64])
            t, _ = timed(a.repeats, s.amplitudes)
            res["amplitudes_64"] = rate(t, F * N * 64)
            save()
        if want("numpy"):
            # the restatement on this host on 1/100 of (a), a frame and 256 vectors at a time, and the device against it
            n = max(F // 100, 1)
            s.set_vectors(q)
            dev = s.amplitudes((0, n))
            t = time.perf_counter()
            worst = 0.0
            for f in range(n):
                for k in range(0, Q, 256):
                    c, sn = sr.amplitudes(x[f:f + 1], q[k:k + 256])
                    for got, ref in ((dev["cos_sum"][f, 0, k:k + 256], c[0, 0]), (dev["sin_sum"][f, 0, k:k + 256], sn[0, 0])):
                        worst = max(worst, float(np.abs(got.astype(np.longdouble) - ref).max()))
            res["numpy_slice_s"] = time.perf_counter() - t
            res["numpy_slice_frames"] = n
            res["numpy_evaluations_per_s"] = n * N * Q / res["numpy_slice_s"]
            res["numpy_extrapolated_s"] = res["numpy_slice_s"] * F / n
            res["largest_error_over_bound"] = worst / float(sr.bound(N))
            assert res["largest_error_over_bound"] <= 1.0, res["largest_error_over_bound"]
            if "amplitudes_lattice" in res:
                res["device_over_numpy"] = res["amplitudes_lattice"]["evaluations_per_s"] / res["numpy_evaluations_per_s"]
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

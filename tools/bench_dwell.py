#!/usr/bin/env python3
"""The contact dwell times (include/gdyn_dwell.h, dwell.py) at the size a user runs them, one JSON line.  Device times are the
library's own, between HIP events on the handle's stream (gd_dwell_last_times): the states kernel, the runs kernel and the correlation
kernel of a call; the host clock around the synchronous call stands beside them (it adds the copy of the results to the host).  Every
figure is the median (min - max) of --repeats calls after a warm-up call.

  genome        701 frames x 62 178 beads, float32, 46 chains with lengths proportional to hg19 (workloads.chain_lengths), contact radii
                1.0 and 1.3 of a coil with steps of 0.6 and a jitter of 0.15 per frame
    separations     8 separations 1 .. 128, 16 lags 0 .. 256, edges log_edges(701, 2)
    pairs           the pairs of the first separation given as a list, every pair its own row (straight global atomics)
  numpy         tests/dwell_restatement.py on the first --cpu-frames frames; the device's results on those frames are compared with it
                exactly.  One thread.

The design minimum of the traffic of a separations call is the history read once per separation (the second bead of a pair is the
first one's stream shifted by s), and the planes of states written once and read once by each of the two consumers; its ratio to the
time is set against the 6.3 TB/s that the memory-bound kernels of this device reach.  These are observations, not pass marks.  --scale
shrinks the shape (a rehearsal, not a measurement).  --out FILE is rewritten after every case."""
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
import dwell_restatement as dr      # noqa: E402

dwell = importlib.import_module("2022a-genome-dynamics_amd.dwell")
wl = importlib.import_module("2022a-genome-dynamics_amd.workloads")
SEPS = [1, 2, 4, 8, 16, 32, 64, 128]
LAGS = [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256]
RULE = (1.0, 1.3)
CEILING = 6.3e12      # bytes per second


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def coil(frames, beads, seed):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((1, beads, 3), dtype=np.float32) * np.float32(0.6), axis=1, dtype=np.float32)
    x = x + np.cumsum(rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.02), axis=0, dtype=np.float32)
    return x + rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.15)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def case(call, d, repeats):
    times, host, r = {"states_ms": [], "runs_ms": [], "corr_ms": []}, [], None
    for _ in range(repeats + 1):
        r, ms = timed(call)
        host.append(ms)
        for k, v in d.last_times().items():
            times[k].append(v)
    out = {k: spread(v[1:]) for k, v in times.items()}
    out["call_host_ms"] = spread(host[1:])
    return r, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(700 * a.scale), 4) + 1, max(int(62178 * a.scale), 2400)
    res = {"repeats": a.repeats, "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    x = coil(F, N, 1)
    ends = np.cumsum(wl.chain_lengths(N))
    chains = np.stack([ends - wl.chain_lengths(N), ends], axis=1)
    edges = dwell.Dwell.log_edges(F, 2)
    W = (F + 63) // 64
    with dwell.Dwell(0) as d:
        d.set_history(x)
        d.set_chains(chains)
        r, t = case(lambda: d.separations(SEPS, *RULE, edges=edges, lags=LAGS), d, a.repeats)
        pairs = int(r["pairs"].sum())
        history, planes = len(SEPS) * F * N * 3 * x.itemsize, 3 * len(SEPS) * W * N * 8
        total = sum(t[k]["median"] for k in ("states_ms", "runs_ms", "corr_ms")) * 1e-3
        t.update({"frames": F, "beads": N, "separations": SEPS, "lags": LAGS, "bins": len(edges) - 1, "pairs": pairs, "pair_frames_per_s": pairs * F / total,
                  "design_min_bytes": history + planes, "design_min_bytes_history": history, "design_min_bytes_planes": planes,
                  "design_min_ms_at_6.3_TB_per_s": (history + planes) / CEILING * 1e3, "fraction_of_6.3_TB_per_s": (history + planes) / total / CEILING,
                  "states_fraction_of_6.3_TB_per_s": (history + planes / 3) / (t["states_ms"]["median"] * 1e-3) / CEILING,
                  "contact_fraction": float(r["length_sum"][:, 1].sum() / (r["pairs"].sum() * F)), "mean_dwell_frames": dwell.Dwell.mean_dwell(r).tolist()})
        if a.cpu_frames:
            want, ms = timed(lambda: dr.separations(x, SEPS, *RULE, edges, LAGS, chains, None, 0, 1, a.cpu_frames))
            got = d.separations(SEPS, *RULE, edges=edges, lags=LAGS, count=a.cpu_frames)
            assert all(got[k].tobytes() == want[k].tobytes() for k in dr.KEYS)
            t.update({"numpy_frames": a.cpu_frames, "numpy_ms_on_those_frames": ms, "numpy_ms_extrapolated": ms * F / a.cpu_frames,
                      "numpy_is_extrapolated_by": f"frames / {a.cpu_frames}", "equal_to_numpy_exactly": True})
            t["device_over_numpy"] = t["numpy_ms_extrapolated"] / (total * 1e3)
        res["separations"] = t
        save()
        listed = dr.chain_pairs(N, chains, SEPS[0])
        r1, t = case(lambda: d.pairs(listed, *RULE, edges=edges, lags=LAGS), d, a.repeats)
        assert int(r1["pairs"].sum()) == len(listed) and all(r1[k].sum(axis=0).tobytes() == r[k][0].tobytes() for k in dr.KEYS[:4])
        t.update({"frames": F, "pairs": len(listed), "rows": len(listed), "sums_equal_the_separation_row": True})
        res["pairs"] = t
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

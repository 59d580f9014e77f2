#!/usr/bin/env python3
"""The gyration tensors and compaction profiles (include/gdyn_gyr.h, gyr.py) at the sizes a user runs them, one JSON line.  Device
times are the library's own, between HIP events on the handle's stream (gd_gyr_last_times): all kernels of a tensors call, the window
kernels and the merge kernel of a profile call; the host clock around the synchronous call stands beside them (it adds the copy of
the results to the host).  Every figure is the median (min - max) of --repeats calls after a warm-up call; the device calls and the
numpy calls of a case alternate.

  genome            701 frames x 62 178 beads, float32, 46 chains with lengths proportional to hg19 (workloads.chain_lengths)
    tensors_by_chain     46 segments
    tensors_domains_10   domains of 10 beads within the chains
    profile_3            windows 10, 100, 1 000
    profile_8            windows 2, 8, 32, 128, 512, 1 024, 1 536, 2 048
  single_chain      100 frames x 250 000 beads, one chain: tensors of one segment, profile of windows 10, 100, 1 000
  numpy             tests/gyr_restatement.py, the same sums in the same order, on --cpu-frames frames of the same history (at most 1 for the
                    profiles), extrapolated to the case's frames by the ratio of the frame counts and said so.  Its loops are numpy
                    element-wise operations, which use one thread whatever OMP_NUM_THREADS says.  profile_8 has no numpy figure.
                    The device's results on those frames are compared with numpy's byte for byte.

A window-bead is one bead of one window of one frame: the unit of the profile's work, walked twice.  These are observations, not pass
marks.  --scale shrinks every shape (a rehearsal, not a measurement).  --only CASE runs one case alone.  --out FILE is rewritten after
every case."""
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
import gyr_restatement as gr      # noqa: E402

gyr = importlib.import_module("2022a-genome-dynamics_amd.gyr")
wl = importlib.import_module("2022a-genome-dynamics_amd.workloads")
CASES = ["tensors_by_chain", "tensors_domains_10", "profile_3", "profile_8", "single_chain"]


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def coil(frames, beads, seed):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((1, beads, 3), dtype=np.float32) * np.float32(0.6), axis=1, dtype=np.float32)
    return x + np.cumsum(rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.02), axis=0, dtype=np.float32)


def window_beads(d, windows, frames):
    return float(sum(int(w) * sum(max(int(b) - int(a) - int(w) + 1, 0) for a, b in d.chains) for w in windows) * frames)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def tensors_case(res, name, d, x, repeats, cpu_frames):
    dev, host, cpu = [], [], []
    for r in range(repeats + 1):
        t, ms = timed(d.tensors)
        host.append(ms)
        dev.append(d.last_times()["tensors_ms"])
        if cpu_frames and r:
            want, ms = timed(lambda: gr.tensors(x, d.segments, 0, 1, cpu_frames))
            cpu.append(ms)
            assert [t[k][:cpu_frames].tobytes() for k in ("centre_sum", "centre", "moment")] == [w.tobytes() for w in want], name
    F, N = d.shape
    res[name] = {"frames": F, "beads": N, "segments": len(d.segments), "tensors_ms": spread(dev[1:]), "call_host_ms": spread(host[1:]),
                 "history_gb_read": 2 * F * N * 3 * x.itemsize / 1e9, "gb_per_s": 2 * F * N * 3 * x.itemsize / 1e9 / (np.median(dev[1:]) * 1e-3)}
    if cpu:
        res[name].update({"numpy_frames": cpu_frames, "numpy_ms_on_those_frames": spread(cpu), "numpy_ms_extrapolated": float(np.median(cpu)) * F / cpu_frames,
                          "numpy_is_extrapolated_by": f"frames / {cpu_frames}", "equal_to_numpy_byte_for_byte": True})
        res[name]["device_over_numpy"] = res[name]["numpy_ms_extrapolated"] / res[name]["tensors_ms"]["median"]


def profile_case(res, name, d, x, windows, repeats, cpu_frames):
    walk, merge, host, cpu = [], [], [], []
    for r in range(repeats + 1):
        p, ms = timed(lambda: d.profile(windows))
        host.append(ms)
        lt = d.last_times()
        walk.append(lt["windows_ms"])
        merge.append(lt["merge_ms"])
        if cpu_frames and r:
            want, ms = timed(lambda: gr.profile(x, windows, d.chains, 0, 1, cpu_frames))
            cpu.append(ms)
            if r == 1:
                part = d.profile(windows, 0, 1, cpu_frames)
                assert [part[k].tobytes() for k in ("sum", "sum_sq", "count")] == [w.tobytes() for w in want], name
    F, N = d.shape
    wb = window_beads(d, windows, F)
    res[name] = {"frames": F, "beads": N, "windows": [int(w) for w in windows], "windows_ms": spread(walk[1:]), "merge_ms": spread(merge[1:]),
                 "call_host_ms": spread(host[1:]), "window_beads": wb, "window_beads_per_s": wb / (np.median(walk[1:]) * 1e-3),
                 "lds_bytes_per_s": wb * 2 * 24 / (np.median(walk[1:]) * 1e-3), "fp64_operations_per_s": wb * 12 / (np.median(walk[1:]) * 1e-3)}
    if cpu:
        res[name].update({"numpy_frames": cpu_frames, "numpy_ms_on_those_frames": spread(cpu), "numpy_ms_extrapolated": float(np.median(cpu)) * F / cpu_frames,
                          "numpy_is_extrapolated_by": f"frames / {cpu_frames}", "equal_to_numpy_byte_for_byte": True})
        res[name]["device_over_numpy"] = res[name]["numpy_ms_extrapolated"] / res[name]["windows_ms"]["median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=4)
    ap.add_argument("--only", choices=CASES, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(700 * a.scale), 4) + 1, max(int(62178 * a.scale), 2400)
    F1, N1 = max(int(100 * a.scale), 4), max(int(250000 * a.scale), 2400)
    res = {"repeats": a.repeats, "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    want = lambda name: a.only in (None, name)      # noqa: E731
    if any(want(c) for c in CASES[:4]):
        x = coil(F, N, 1)
        ends = np.cumsum(wl.chain_lengths(N))
        chains = np.stack([ends - wl.chain_lengths(N), ends], axis=1)
        with gyr.Gyration(0) as d:
            d.set_history(x)
            d.set_chains(chains)
            if want("tensors_by_chain"):
                d.set_segments(chains)
                tensors_case(res, "tensors_by_chain", d, x, a.repeats, a.cpu_frames)
                save()
            if want("tensors_domains_10"):
                d.set_segments(gyr.Gyration.segments_from_chains(chains, 10))
                tensors_case(res, "tensors_domains_10", d, x, a.repeats, a.cpu_frames)
                save()
            if want("profile_3"):
                profile_case(res, "profile_3", d, x, [10, 100, 1000], a.repeats, min(a.cpu_frames, 1))
                save()
            if want("profile_8"):
                profile_case(res, "profile_8", d, x, [2, 8, 32, 128, 512, 1024, 1536, 2048], a.repeats, 0)
                save()
        del x
    if want("single_chain"):
        x = coil(F1, N1, 2)
        with gyr.Gyration(0) as d:
            d.set_history(x)
            tensors_case(res, "single_chain_tensors", d, x, a.repeats, a.cpu_frames)
            profile_case(res, "single_chain_profile", d, x, [10, 100, 1000], a.repeats, min(a.cpu_frames, 1))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

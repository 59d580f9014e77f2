#!/usr/bin/env python3
"""The van Hove functions (include/gdyn_vanhove.h, vanhove.py) at the size a user runs them, one JSON line.  Device times are the
library's own, between HIP events on the handle's stream (gd_vanhove_last_times); the host clock around the synchronous call stands
beside them (it adds the copy of the results to the host).  Every figure is the median (min - max) of --repeats calls after a warm-up
call.

  self part     701 frames x 62 178 beads, float32, four bead classes in blocks along the genome as labels (tools/bench_dcorr.py's),
                16 logarithmic lags, 64 logarithmic bins: a walk whose steps differ from bead to bead by a factor of 30
    self            counts, below, above
    self_per_origin the same with the per-origin table
    frozen          every frame the first one: every displacement in one cell of the histogram, the worst case of the LDS atomics
    msd             Msd.time on the same history and lags (host clock: it has no device timer), which makes the same reads
    two_bins        the same walk with two bins split near the median displacement: a bisection of two steps, not seven
    copy            a device-to-device hipMemcpyAsync of a buffer of the history's size, between events: it reads and writes that
                    many bytes, so the history read once at its bandwidth takes half its time
  distinct part 24 frames x 62 178 beads in a ball at ~120 beads per unit volume, open box, cutoff 1.0, bin width 0.02
                (tools/bench_dcorr.py's shape), 8 origins, lags 0 and 16
    distinct        both lags in one call
    dcorr           Dcorr.pairs of lag 16 on the same 8 origins with the same cutoff and bins: the same cell walk over unordered pairs

These are observations, not pass marks.  --scale shrinks the shape (a rehearsal, not a measurement).  --lib PATH loads another build of
the library (the wave-count variant of the LDS histogram, -DGD_VANHOVE_WAVE_COUNT).  --out FILE is rewritten after every case."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

vh = importlib.import_module("2022a-genome-dynamics_amd.vanhove")
msd = importlib.import_module("2022a-genome-dynamics_amd.msd")
dcorr = importlib.import_module("2022a-genome-dynamics_amd.dcorr")
MD, BW = 1.0, 0.02      # tools/bench_dcorr.py's


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def case(call, handle, repeats):
    """The result of the last call, the device times and the host clock of `repeats` calls after one warm-up."""
    times, host, r = {}, [], None
    for _ in range(repeats + 1):
        t = time.perf_counter()
        r = call()
        host.append((time.perf_counter() - t) * 1e3)
        if handle is not None:
            for k, v in handle.last_times().items():
                times.setdefault(k, []).append(v)
    out = {k: spread(v[1:]) for k, v in times.items()}
    out["call_host_ms"] = spread(host[1:])
    return r, out


def ball_walk(frames, beads, radius, seed):
    """tools/bench_dcorr.py's: beads uniform in a ball, then independent steps plus a swirl common to neighbours"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((beads, 3))
    x0 = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(size=(beads, 1)) ** (1 / 3)
    steps = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.03) + (0.03 * np.sin(x0[:, ::-1])).astype(np.float32)
    steps[0] = 0
    return (x0.astype(np.float32) + np.cumsum(steps, axis=0, dtype=np.float32)).astype(np.float32)


def log_lags(k, longest):
    return sorted({int(min(max(np.floor(longest ** (i / (k - 1)) + 0.5), 1), longest)) for i in range(k)})


def copy_ms(n_bytes, repeats):
    """A device-to-device hipMemcpyAsync of n_bytes between events on the null stream, through the HIP runtime the library runs on."""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipSetDevice(0))
    ok(hip.hipMalloc(C.byref(a), n_bytes))
    ok(hip.hipMalloc(C.byref(b), n_bytes))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    ok(hip.hipMemsetAsync(a, 1, n_bytes, None))
    out = []
    for _ in range(repeats + 1):
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(b, a, n_bytes, 3, None))      # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        out.append(ms.value)
    for e in (e0, e1):
        ok(hip.hipEventDestroy(e))
    for p in (a, b):
        ok(hip.hipFree(p))
    return spread(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--skip-distinct", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(700 * a.scale), 20) + 1, max(int(62178 * a.scale), 2400)
    res = {"repeats": a.repeats, "library": a.lib or "default"}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    rng = np.random.default_rng(1)
    steps = rng.standard_normal((F, N, 3), dtype=np.float32) * (np.float32(0.01) * np.float32(30.0) ** rng.uniform(size=(1, N, 1)).astype(np.float32))
    x = np.cumsum(steps, axis=0, dtype=np.float32)
    del steps
    label = (np.arange(N) // 50) % 4
    lags = log_lags(16, F - 1)
    edges = vh.log_edges(0.005, 50.0, 16)      # 64 bins
    history = x.nbytes
    res["self_shape"] = {"frames": F, "beads": N, "labels": 4, "lags": lags, "bins": len(edges) - 1, "history_bytes": history,
                         "cells": len(lags) * 4 * (len(edges) + 1), "lds_cells": vh.VANHOVE_LDS_CELLS}
    with vh.VanHove(0, path=a.lib) as v:
        v.set_history(x)
        v.set_labels(label, 4)
        r, res["self"] = case(lambda: v.self_part(lags, edges), v, a.repeats)
        total = r["counts"].sum(axis=-1) + r["below"] + r["above"]
        assert total.tolist() == (r["origins"][:, None] * v.members()[None, :]).tolist()
        res["self"]["displacements"] = int(total.sum())
        res["self"]["inside_the_bins"] = float(r["counts"].sum() / total.sum())
        res["self"]["fullest_cell_share"] = float(r["counts"].max(axis=-1).sum() / total.sum())
        save()
        split = float(edges[np.searchsorted(np.cumsum(r["counts"].sum(axis=(0, 1))), total.sum() / 2) + 1])      # the edge past the median
        r2, res["two_bins"] = case(lambda: v.self_part(lags, [0.0, split, 1e30]), v, a.repeats)
        res["two_bins"]["first_bin_share"] = float(r2["counts"][:, :, 0].sum() / total.sum())
        rp, res["self_per_origin"] = case(lambda: v.self_part(lags, edges, per_origin=True), v, a.repeats)
        assert rp["per_origin"].sum(axis=1).tobytes() == r["counts"].tobytes()
        res["self_per_origin"]["table_bytes"] = int(rp["per_origin"].nbytes)
        del rp
        save()
        with msd.Msd(0) as m:
            m.set_history(x)
            m.set_groups(label, 4)
            _, res["msd"] = case(lambda: m.time(lags, want_sum4=True), None, a.repeats)
        save()
        v.set_history(np.ascontiguousarray(np.broadcast_to(x[:1], x.shape)))
        v.set_labels(label, 4)
        rf, res["frozen"] = case(lambda: v.self_part(lags, edges), v, a.repeats)
        assert not rf["counts"].any() and rf["below"].sum() == total.sum()      # r2 = 0 is below e_0 > 0: one cell per lag and label
        rf, res["frozen_in_a_bin"] = case(lambda: v.self_part(lags, np.concatenate([[0.0], edges[1:]])), v, a.repeats)
        assert rf["counts"][:, :, 0].sum() == total.sum()
        save()
    res["copy"] = copy_ms(history, a.repeats)
    res["copy"]["bytes_per_s"] = 2 * history / (res["copy"]["median"] * 1e-3)
    read_once = res["copy"]["median"] / 2
    res["history_read_once_ms_at_copy_bandwidth"] = read_once
    res["ratios"] = {"self_device_over_read_once": res["self"]["count_ms"]["median"] / read_once,
                     "self_host_over_msd_host": res["self"]["call_host_ms"]["median"] / res["msd"]["call_host_ms"]["median"],
                     "self_device_over_msd_host": res["self"]["count_ms"]["median"] / res["msd"]["call_host_ms"]["median"],
                     "per_origin_over_self": res["self_per_origin"]["count_ms"]["median"] / res["self"]["count_ms"]["median"],
                     "frozen_over_self": res["frozen"]["count_ms"]["median"] / res["self"]["count_ms"]["median"],
                     "two_bins_over_self": res["two_bins"]["count_ms"]["median"] / res["self"]["count_ms"]["median"]}
    save()
    if not a.skip_distinct:
        del x
        Fd = 24
        radius = (N / 119.4 / (4 / 3 * np.pi)) ** (1 / 3)
        xd = ball_walk(Fd, N, radius, 1)
        d_edges = vh.linear_edges(BW, MD)
        with vh.VanHove(0, path=a.lib) as v:
            v.set_history(xd)
            v.set_labels(label, 4)
            r, res["distinct"] = case(lambda: v.distinct([0, 16], d_edges, count=8), v, a.repeats)
            assert r["origins"].tolist() == [8, 8]
            res["distinct"].update({"frames": Fd, "beads": N, "bins": len(d_edges) - 1, "classes": 16, "origins": 8, "lags": [0, 16],
                                    "ordered_pairs_counted": int(r["counts"].sum())})
        with dcorr.Dcorr(0) as d:
            d.set_history(xd)
            d.set_labels(label, 4)
            p, res["dcorr"] = case(lambda: d.pairs(16, BW, MD, n_origins=8), None, a.repeats)
            res["dcorr"]["unordered_pairs_counted"] = int(p.count.sum())
        device = res["distinct"]["count_ms"]["median"] + res["distinct"]["index_ms"]["median"]
        res["ratios"]["distinct_host_over_dcorr_host"] = res["distinct"]["call_host_ms"]["median"] / res["dcorr"]["call_host_ms"]["median"]
        res["ratios"]["distinct_device_over_dcorr_host"] = device / res["dcorr"]["call_host_ms"]["median"]
        res["ratios"]["distinct_ordered_pairs_over_dcorr_unordered"] = res["distinct"]["ordered_pairs_counted"] / max(res["dcorr"]["unordered_pairs_counted"], 1)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

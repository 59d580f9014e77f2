#!/usr/bin/env python3
"""The Hi-C signal analyses at the size of a 100 kb human cooler: 30 895 bins in 25 chromosomes (hg38 lengths; X, Y and MT
among them) and one pixel table of about 20 M unique pixels in cooler order, contacts falling as a power of the distance, a
third of the pixels trans.  The handle holds what the three programs would ask for at once: the band of compute_interactions
(W = 4), the bands of compute_local_alpha at widths 10 and 50, and the RAW and the weighted distance profile.
Prints one JSON line (and writes it to --out):
  device     host-clock seconds of HicSignals.accumulate over the whole table (upload, kernel, synchronise), the median of
             three runs, as pixels and bytes (20 B per pixel) per second; the post-passes with their downloads;
  numpy      hic.py's numpy functions for the same targets on this host's CPU;
  programs   the four programs on a file of the same pixels written by gd_h5tool put-cool: wall time and read / compute / write;
  kernels    with --kernel-stats <csv>: the kernels' times from a separate run under rocprofv3, k_hic_accumulate as pixels and
             bytes per second beside the 6.3 TB/s a copy achieves on this device.
The run the kernel statistics come from (--device-only skips the programs and the CPU comparison):
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_hic.py --device-only"""
import argparse
import csv
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
hic = importlib.import_module("2022a-genome-dynamics_amd.hic")
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
BINSIZE = 100_000
# hg38 chromosome lengths in 100 kb bins, 1 .. 22, X, Y, MT
SIZES = [2490, 2422, 1983, 1903, 1816, 1709, 1594, 1452, 1384, 1338, 1351, 1333, 1144, 1071, 1020, 904, 833, 804, 587, 645, 468, 509, 1561, 573, 1]
NAMES = [str(k) for k in range(1, 23)] + ["X", "Y", "MT"]
COPY_RATE = 6.3e12          # bytes per second of a float4 copy on the MI355X
RUNS = 3
WIDTHS = (10, 50)


def cooler(scale=1.0):
    rng = np.random.default_rng(30895)
    sizes = np.array(SIZES)
    chrom = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    n = len(chrom)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    last = (first + sizes)[chrom]
    mappable = rng.random(n) > 0.04
    bins = np.arange(n)
    ii, jj = [], []
    for d in range(int(2400 * scale)):                       # every separation, thinning with the distance
        keep = (bins + d < last) & (rng.random(n) < min(1.0, 60.0 / (d + 1) ** 0.75))
        ii.append(bins[keep])
        jj.append(bins[keep] + d)
    t = int(7_000_000 * scale)
    ti, tj = rng.integers(0, n, size=t), rng.integers(0, n, size=t)
    i, j = np.concatenate(ii + [np.minimum(ti, tj)]), np.concatenate(jj + [np.maximum(ti, tj)])
    ok = mappable[i] & mappable[j]
    key = np.unique(i[ok] * n + j[ok])
    i, j = key // n, key % n
    count = (1 + rng.poisson(np.where(chrom[i] == chrom[j], 2000.0 / (j - i + 1.0), 0.3))).astype(np.int32)
    weights = rng.uniform(0.4, 1.6, n)
    weights[~mappable] = np.nan
    within = bins - first[chrom]
    return chrom, within * BINSIZE, (within + 1) * BINSIZE, i.astype(np.int64), j.astype(np.int64), count, weights


def timed(fn, repeats=RUNS):
    ts, r = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return r, float(np.median(ts)), ts


def kernel_rates(path, n_pixels):
    out = {}
    for row in csv.DictReader(open(path)):
        for key in ("k_hic_accumulate", "k_hic_decay", "k_hic_insulation", "k_hic_alpha"):
            if key in row["Name"]:
                e = out.setdefault(key, {"calls": 0, "total_ns": 0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += int(row["TotalDurationNs"])
    e = out.get("k_hic_accumulate")
    if e:       # the automatic launch size is 2^22 pixels: a pass over the table is ceil(n / 2^22) launches
        launches = -(-n_pixels // (1 << 22))
        e["passes"] = e["calls"] / launches
        e["s_per_pass"] = e["total_ns"] * 1e-9 / e["passes"]
        e["pixels_per_s"] = n_pixels / e["s_per_pass"]
        e["bytes_per_s"] = 20 * e["pixels_per_s"]
        e["share_of_copy_rate"] = e["bytes_per_s"] / COPY_RATE
    return out


def run_programs(chrom, start, end, b1, b2, count, weights):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from hic_restatement import put_cool
        path = os.path.join(tmp, "bench.mcool")
        r = put_cool(os.path.join(HOST, "gd_h5tool"), tmp, path, BINSIZE, NAMES, chrom, start, end, b1, b2, count, weights)
        assert r.returncode == 0, r.stderr
        res["mcool_bytes"] = os.path.getsize(path)
        table = os.path.join(tmp, "signals.tsv")
        commands = {"gd_compute_interactions": ["-b", str(BINSIZE), "-o", table, path], "gd_compute_local_alpha_w10": ["-w", "10", "-b", str(BINSIZE), path],
                    "gd_compute_local_alpha_w50": ["-w", "50", "-b", str(BINSIZE), path], "gd_hic_power_law_RAW": ["--binsize", str(BINSIZE), path],
                    "gd_hic_power_law_weight": ["--binsize", str(BINSIZE), "--normalize", "weight", path], "gd_downsample": ["--rate", "5", table]}
        for key, args in commands.items():
            prog = re.sub(r"_(w\d+|RAW|weight)$", "", key)
            t = time.perf_counter()
            r = subprocess.run([os.path.join(HOST, prog), *args], capture_output=True, text=True, check=True)
            res[key] = {"wall_s": time.perf_counter() - t, "stdout_bytes": len(r.stdout)}
            m = re.search(r"read ([\d.]+) s, compute ([\d.]+) s, write ([\d.]+) s", r.stderr)
            up = re.search(r"device start-up ([\d.]+) s", r.stderr)
            if m:
                res[key].update({"read_s": float(m[1]), "compute_s": float(m[2]), "write_s": float(m[3]), "device_startup_s": float(up[1])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the pixel table to generate")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --device-only run under rocprofv3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    chrom, start, end, b1, b2, count, weights = cooler(a.scale)
    size = hic.largest_chromosome(chrom)
    excluded = hic.excluded_bins(chrom, {n: k for k, n in enumerate(NAMES)})
    nbytes = b1.nbytes + b2.nbytes + count.nbytes
    res = {"bins": int(len(chrom)), "pixels": int(len(count)), "trans_pixels": int((chrom[b1] != chrom[b2]).sum()), "pixel_bytes": int(nbytes), "profile_size": size}
    with hic.HicSignals(chrom) as hs:
        band4 = hs.add_band(4)
        alpha_bands = {w: hs.add_band(w + 1) for w in WIDTHS}
        raw, weighted = hs.add_distance_profile(excluded, None, size), hs.add_distance_profile(excluded, weights, size)
        hs.accumulate(b1, b2, count)                          # warm-up: code objects, the staging buffer
        ts = []
        for _ in range(RUNS):                                 # reset() ends in a synchronise and is not timed
            hs.reset()
            clock = time.perf_counter()
            hs.accumulate(b1, b2, count)
            ts.append(time.perf_counter() - clock)
        t_acc = float(np.median(ts))
        (D, I), t_di, _ = timed(lambda: hs.decay_insulation(band4))
        alphas, t_alpha = {}, {}
        for w, t in alpha_bands.items():
            alphas[w], t_alpha[w], _ = timed(lambda: hs.local_alpha(t))
        device = {"band4": hs.fetch_band(band4), "raw": hs.fetch_profile_raw(raw), "raw_n": hs.fetch_profile(raw)[1], "weighted": hs.fetch_profile(weighted)}
        device.update({f"band{w + 1}": hs.fetch_band(t) for w, t in alpha_bands.items()})
    res["device"] = {"accumulate_s": t_acc, "accumulate_s_runs": ts, "pixels_per_s": len(count) / t_acc, "bytes_per_s": nbytes / t_acc,
                     "decay_insulation_s": t_di, "local_alpha_s": {str(w): t for w, t in t_alpha.items()}}
    if a.kernel_stats:
        res["kernels"] = kernel_rates(a.kernel_stats, len(count))
    if not a.device_only:
        clock = time.perf_counter()
        want = {"band4": hic.band_matrix(b1, b2, count, chrom, 4)}
        want.update({f"band{w + 1}": hic.band_matrix(b1, b2, count, chrom, w + 1) for w in WIDTHS})
        want_raw = hic.distance_profile(b1, b2, count, chrom, excluded, None, size)
        want_weighted = hic.distance_profile(b1, b2, count, chrom, excluded, weights, size)
        t_sums = time.perf_counter() - clock
        want_D, want_I = hic.decay_insulation(want["band4"], chrom)
        want_alpha = {w: hic.local_alpha(want[f"band{w + 1}"], chrom) for w in WIDTHS}
        res["numpy_s"] = {"sums": t_sums, "signals": time.perf_counter() - clock - t_sums}
        res["speedup_vs_numpy_sums"] = t_sums / t_acc
        assert all(np.array_equal(device[k], v) for k, v in want.items())                       # the same integers
        assert np.array_equal(device["raw"], want_raw[0]) and np.array_equal(device["raw_n"], want_raw[1])
        assert np.array_equal(device["weighted"][1], want_weighted[1])
        np.testing.assert_allclose(device["weighted"][0], want_weighted[0], rtol=int(want_weighted[1].max()) * 2.0 ** -52)
        np.testing.assert_allclose(D, want_D, rtol=1e-15, equal_nan=True)
        np.testing.assert_allclose(I, want_I, rtol=1e-15, equal_nan=True)
        for w in WIDTHS:
            np.testing.assert_allclose(alphas[w], want_alpha[w], rtol=1e-8, equal_nan=True)
        res["programs"] = run_programs(chrom, start, end, b1, b2, count, weights)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

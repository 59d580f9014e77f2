#!/usr/bin/env python3
"""The compartment analysis at the size of a 100 kb human cooler: the pixel table of tools/bench_hic.py
(30 895 bins in 25 chromosomes, about 20 M unique pixels, the largest chromosome 2 490 bins) and one synthetic chromosome of
10 000 bins handed to pca_matrix.  Prints one JSON line (and writes it to --out):
  pass       host-clock seconds of HicSignals.accumulate over the whole table with the targets of bench_hic.py, without and with
             a dense target beside them (median of three runs);
  profile    dense_profile over the 22 autosomes, with its download;
  pca        per case (the enrichment of the largest chromosome with the mask of dense_valid, k = 3; the 10 000-bin matrix,
             k = 3): m, iterations to the residual, seconds of the whole call (median of three), and, without --device-only,
             np.linalg.svd of the same centred matrix on this host (the 10 000-bin one only with --svd-large);
  kernels    with --kernel-stats <csv>: the kernels' times from a separate run under rocprofv3; k_pca_xq and k_pca_xty as
             bytes of the matrix (m x ld x 8) over the mean time of a call, beside the 6.3 TB/s a copy achieves on this device.
             The csv mixes the calls of both cases, so --case picks the one a profiled run executes.
The run the kernel statistics come from:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_compartments.py --device-only --case large"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_hic as B      # noqa: E402

hic = B.hic
COPY_RATE = B.COPY_RATE
RUNS = 3
KERNELS = ("k_hic_accumulate", "k_dense_profile_sum", "k_dense_profile", "k_dense_f64", "k_row_flags", "k_pca_compact", "k_pca_center", "k_pca_xq", "k_pca_xty",
           "k_sum_parts", "k_pca_gram", "k_pca_rotate", "k_pca_mul", "k_pca_start")


def planted(n, period=137, seed=1):
    """A symmetric n x n matrix like an enrichment map: a checkerboard of compartments, a decay and noise."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    state = np.where((k // period) % 2 == 0, 1.0, -1.0) * (1 + 0.3 * np.sin(k / 211.0))
    m = 1 + 0.4 * state[:, None] * state[None, :] + 0.5 / (1 + np.abs(k[:, None] - k[None, :])) ** 0.5
    noise = 0.2 * rng.standard_normal((n, n))
    m += (noise + noise.T) / 2
    dead = rng.random(n) < 0.03
    m[dead, :] = 0
    m[:, dead] = 0
    return m


def kernel_table(path, m):
    out = {}
    for row in csv.DictReader(open(path)):
        for key in KERNELS:
            if key in row["Name"]:
                e = out.setdefault(key, {"calls": 0, "total_ns": 0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += int(row["TotalDurationNs"])
                break
    ld = (m + 1) // 2 * 2
    for key in ("k_pca_xq", "k_pca_xty"):
        e = out.get(key)
        if e and m:
            e["mean_s"] = e["total_ns"] * 1e-9 / e["calls"]
            e["matrix_bytes"] = m * ld * 8
            e["bytes_per_s"] = e["matrix_bytes"] / e["mean_s"]
            e["flop_per_s"] = 2.0 * m * m * 16 / e["mean_s"]
            e["share_of_copy_rate"] = e["bytes_per_s"] / COPY_RATE
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--case", choices=["both", "genome", "large", "none"], default="both", help="none: only read --kernel-stats")
    ap.add_argument("--large", type=int, default=10000, help="bins of the synthetic chromosome")
    ap.add_argument("--svd-large", action="store_true", help="also run np.linalg.svd on the synthetic chromosome (minutes)")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the pixel table to generate")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-m", type=int, default=0, help="valid bins of the case the profiled run executed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"pca": {}}
    if a.case in ("both", "genome"):
        chrom, start, end, b1, b2, count, weights = B.cooler(a.scale)
        size = hic.largest_chromosome(chrom)
        excluded = hic.excluded_bins(chrom, {n: k for k, n in enumerate(B.NAMES)})
        res.update({"bins": int(len(chrom)), "pixels": int(len(count)), "dense_cells": int((np.bincount(chrom).astype(np.int64) ** 2).sum())})
        times = {}
        for with_dense in (False, True):
            with hic.HicSignals(chrom) as hs:
                hs.add_band(4)
                for w in B.WIDTHS:
                    hs.add_band(w + 1)
                hs.add_distance_profile(excluded, None, size)
                hs.add_distance_profile(excluded, weights, size)
                dense = hs.add_dense() if with_dense else None
                hs.accumulate(b1, b2, count)                  # warm-up
                ts = []
                for _ in range(RUNS):
                    hs.reset()
                    clock = time.perf_counter()
                    hs.accumulate(b1, b2, count)
                    ts.append(time.perf_counter() - clock)
                times["with_dense" if with_dense else "without_dense"] = {"accumulate_s": float(np.median(ts)), "runs": ts}
                if with_dense:
                    (contacts, counts, mean), t_profile, _ = B.timed(lambda: hs.dense_profile(dense, excluded))
                    valid = hs.dense_valid(dense)[chrom == 0]
                    res["profile"] = {"s": t_profile, "size": size, "nan_distances": int(np.isnan(mean).sum())}
                    # the far corner of the largest chromosome may hold NaN (no pixel that far apart): the bins such a distance
                    # reaches are left out, as the explicit mask of the test fixture does
                    reach = int(np.flatnonzero(~np.isnan(mean)).max()) + 1
                    k = np.arange(size)
                    valid &= (k < reach) & (k >= size - reach)
                    got, t_pca, runs = B.timed(lambda: hs.dense_pca(dense, 0, hic.DENSE_ENRICHMENT, valid, 3))
                    entry = {"n": size, "m": int(valid.sum()), "k": 3, "iterations": got[3], "call_s": t_pca, "runs": runs, "variances": got[1].tolist()}
                    if not a.device_only:
                        E = hs.fetch_dense(dense, 0, hic.DENSE_ENRICHMENT)
                        clock = time.perf_counter()
                        want = hic.contact_pca(E, valid, 3)
                        entry["numpy_svd_s"] = time.perf_counter() - clock
                        entry["max_axis_difference"] = float(np.nanmax(np.abs(got[2] - want[2])))
                        entry["max_variance_rel"] = float(np.max(np.abs(got[1] - want[1]) / want[1]))
                    res["pca"]["largest_chromosome"] = entry
        res["pass"] = times
    if a.case in ("both", "large"):
        matrix = planted(a.large)
        with hic.HicSignals(np.zeros(2, np.int32)) as hs:
            hs.pca_matrix(matrix[:512, :512], None, 3)      # warm-up: code objects
            got, t_pca, runs = B.timed(lambda: hs.pca_matrix(matrix, None, 3))
        m = int(np.any(matrix != 0, axis=1).sum())
        entry = {"n": a.large, "m": m, "k": 3, "iterations": got[3], "call_s": t_pca, "runs": runs, "upload_bytes": int(matrix.nbytes), "variances": got[1].tolist()}
        if a.svd_large and not a.device_only:
            clock = time.perf_counter()
            want = hic.contact_pca(matrix, None, 3)
            entry["numpy_svd_s"] = time.perf_counter() - clock
            entry["max_axis_difference"] = float(np.nanmax(np.abs(got[2] - want[2])))
        res["pca"]["synthetic"] = entry
    if a.kernel_stats:
        res["kernels"] = kernel_table(a.kernel_stats, a.kernel_stats_m)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

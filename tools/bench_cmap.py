#!/usr/bin/env python3
"""The contact-map analyses at the paper's size: 62 178 chromatin beads in 46 chains plus 400 nucleolar beads and one stored
map of more than 3 M unique rows (ordered by i, then j; three quarters of them within 40 beads of the diagonal).  The handle
holds what the four programs would ask for at once: the regions and nucleolus profiles of the two largest chains, the
separation profile, a genome-wide nucleolus profile (beyond the LDS budget) and the genome-wide matrix at rebin rate 10.
Prints one JSON line (and writes it to --out):
  device     host-clock seconds of ContactMaps.accumulate over the whole map (upload, kernel, synchronise), the median of
             three runs, as rows and bytes (12 B per row) per second; fetch of the binned matrix (A + A^T, 155 MB);
  combine    updates of the binned target the rows ask for and the global atomics issued after the wave-level combine;
  numpy      cmap.py's numpy functions for the same targets on this host's CPU;
  programs   the four programs on two files of two frames each made of the same rows: wall time and read / compute / write;
  kernels    with --kernel-stats <csv>: k_cmap_accumulate's time from a separate run under rocprofv3, as rows and bytes per
             second beside the 6.3 TB/s a copy achieves on this device.
The run the kernel statistics come from (--device-only skips the programs and the CPU comparison):
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_cmap.py --device-only"""
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
cmap = importlib.import_module("2022a-genome-dynamics_amd.cmap")
wl = importlib.import_module("2022a-genome-dynamics_amd.workloads")
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
N, NUC, ROWS, RATE = 62178, 400, 3_300_000, 10
COPY_RATE = 6.3e12          # bytes per second of a float4 copy on the MI355X
RUNS = 3


def genome():
    lens = np.asarray(wl.chain_lengths(N))
    ends = np.cumsum(lens)
    ranges = np.stack([ends - lens, ends], axis=1).astype(np.int32)
    total = N + NUC
    rng = np.random.default_rng(62178)
    m = ROWS + ROWS // 4
    i = rng.integers(0, total, size=m)
    kind = rng.random(m)
    near = np.clip(i + rng.integers(-40, 41, size=m), 0, total - 1)
    j = np.where(kind < 0.75, near, np.where(kind < 0.93, rng.integers(0, total, size=m), rng.integers(N, total, size=m)))
    keys = np.unique(i * total + j)
    rows = np.stack([keys // total, keys % total, rng.integers(1, 5, size=len(keys))], axis=1).astype(np.uint32)
    nuc = np.zeros(total, bool)
    nuc[N:] = True
    largest = [int(c) for c in np.argsort(lens, kind="stable")[-2:]]
    return rows, ranges, nuc, largest, total


def add_targets(cm, ranges, nuc, largest, total):
    ids, longest = cmap.chain_ids(ranges, total)
    rebin, binned = cmap.rebin_map(ranges, RATE)
    t = {}
    for k, c in enumerate(largest):
        beg, end = map(int, ranges[c])
        t[f"region{k}"] = cm.add_region(beg, end)
        t[f"nad{k}"] = cm.add_nucleolus_profile(beg, end, nuc)
    t["separation"] = cm.add_separation_profile(ids, longest)
    t["genome_nad"] = cm.add_nucleolus_profile(0, N, nuc)
    t["binned"] = cm.add_binned(rebin, int(binned.max()))
    return t


def median_time(fn, repeats=RUNS):
    ts, r = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return r, float(np.median(ts))


def kernel_rates(path, n_rows):
    out = {}
    for row in csv.DictReader(open(path)):
        for key in ("k_cmap_accumulate", "k_cmap_symmetric_rows", "k_cmap_symmetrize", "k_cmap_max", "k_cmap_diagonal"):
            if key in row["Name"]:
                e = out.setdefault(key, {"calls": 0, "total_ns": 0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += int(row["TotalDurationNs"])
    e = out.get("k_cmap_accumulate")
    if e:       # every launch of the profiled run is one pass over the map (automatic batches hold it whole)
        e["rows"] = n_rows * e["calls"]
        e["rows_per_s"] = e["rows"] / (e["total_ns"] * 1e-9)
        e["bytes_per_s"] = 12 * e["rows_per_s"]
        e["share_of_copy_rate"] = e["bytes_per_s"] / COPY_RATE
    return out


def run_programs(rows, ranges, largest, total):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        meta = os.path.join(tmp, "meta")
        os.mkdir(meta)
        open(os.path.join(meta, "config.json"), "w").write("{}")
        np.tile(np.array([1, 0], "<f4"), (total, 1)).tofile(os.path.join(meta, "ab.f32"))
        types = np.ones(total, "i1")
        types[N:] = 7
        types.tofile(os.path.join(meta, "types.i8"))
        open(os.path.join(meta, "chromosomes.tsv"), "w").write("".join(f"chr{k + 1} {b} {e} {(b + e) // 2} {(b + e) // 2 + 1}\n" for k, (b, e) in enumerate(ranges)))
        open(os.path.join(meta, "nucleoli.tsv"), "w").write(f"nucleolus {N} {total}\n")
        open(os.path.join(meta, "nucleolus_bonds.i32"), "w").write("")
        tool, raw = os.path.join(HOST, "gd_h5tool"), os.path.join(tmp, "rows.u32")
        job = os.path.join(tmp, "job")
        os.mkdir(job)
        files = [os.path.join(job, f"output-{k}.h5") for k in range(2)]
        parts = np.array_split(rows, 4)
        for k, path in enumerate(files):
            subprocess.check_call([tool, "make-metadata", path, meta])
            for fr in range(2):
                parts[2 * k + fr].astype("<u4").tofile(raw)
                subprocess.check_call([tool, "put-contacts", path, "interphase", str(1000 * (fr + 1)), raw])
        res["trajectory_bytes"] = sum(os.path.getsize(p) for p in files)
        chroms = ",".join(f"chr{c + 1}" for c in largest)
        out = os.path.join(tmp, "gw.h5")
        commands = {"gd_contact_map": ["--chroms", chroms, job], "gd_nad_profile": ["--chroms", chroms, job],
                    "gd_gw_contact_matrix": ["--rebin-rate", str(RATE), "-o", out, *files], "gd_power_law": files}
        for prog, args in commands.items():
            t = time.perf_counter()
            r = subprocess.run([os.path.join(HOST, prog), *args], capture_output=True, text=True, check=True)
            wall = time.perf_counter() - t
            m = re.search(r"read ([\d.]+) s, compute ([\d.]+) s, write ([\d.]+) s", r.stderr)
            up = re.search(r"device start-up ([\d.]+) s", r.stderr)
            res[prog] = {"wall_s": wall, "read_s": float(m[1]), "compute_s": float(m[2]), "write_s": float(m[3]), "device_startup_s": float(up[1]),
                         "stdout_bytes": len(r.stdout)}
        res["gw_output_bytes"] = os.path.getsize(out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --device-only run under rocprofv3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, ranges, nuc, largest, total = genome()
    res = {"beads": N, "nucleolar": NUC, "rows": int(len(rows)), "rebin_rate": RATE, "row_bytes": int(rows.nbytes)}
    with cmap.ContactMaps(0) as cm:
        t = add_targets(cm, ranges, nuc, largest, total)
        cm.accumulate(rows)                                   # warm-up: code objects, the staging buffer
        cm.reset()

        ts = []
        for _ in range(RUNS):                                 # reset() ends in a synchronise and is not timed
            cm.reset()
            clock = time.perf_counter()
            cm.accumulate(rows)
            ts.append(time.perf_counter() - clock)
        t_acc = float(np.median(ts))
        requested, issued = cm.counters()
        binned, t_fetch = median_time(lambda: cm.fetch(t["binned"]), 1)
        device = {k: cm.fetch(v) for k, v in t.items() if k != "binned"}
    res["device"] = {"accumulate_s": t_acc, "accumulate_s_runs": ts, "rows_per_s": len(rows) / t_acc, "bytes_per_s": rows.nbytes / t_acc, "fetch_binned_s": t_fetch,
                     "binned_bytes": int(binned.nbytes)}
    res["combine"] = {"updates": requested, "atomics": issued, "ratio": issued / requested}
    if a.kernel_stats:
        res["kernels"] = kernel_rates(a.kernel_stats, len(rows))
    if not a.device_only:
        ids, longest = cmap.chain_ids(ranges, total)
        rebin, binned_ranges = cmap.rebin_map(ranges, RATE)
        clock = time.perf_counter()
        want = {}
        for k, c in enumerate(largest):
            beg, end = map(int, ranges[c])
            want[f"region{k}"] = cmap.region_matrix(rows, beg, end)
            want[f"nad{k}"] = cmap.nucleolus_profile(rows, beg, end, nuc)
        want["separation"] = cmap.separation_profile(rows, ids, longest)
        want["genome_nad"] = cmap.nucleolus_profile(rows, 0, N, nuc)
        want_binned = cmap.binned_matrix(rows, rebin, int(binned_ranges.max()))
        res["numpy_s"] = time.perf_counter() - clock
        res["speedup_vs_numpy"] = res["numpy_s"] / t_acc
        assert all(np.array_equal(device[k], v) for k, v in want.items()) and np.array_equal(binned, want_binned)      # same values
        res["programs"] = run_programs(rows, ranges, largest, total)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The distance and contact-frequency maps (include/gdyn_dmap.h, dmap.py) at the sizes a user runs them, host clock around the
synchronous calls, median (min - max) of five each, one JSON line.  A pair is one (bead, bead, frame) distance evaluation that the
map holds, both orders counted: count.sum(); the device evaluates each unordered pair once and mirrors it.

  (a) chromosome   one chromosome at bead resolution: 2 253 beads x 701 frames, two thresholds
  (b) genome       the genome shape (701, 62 178) float32 at 10 beads per bin within 46 chromosome-like chains, two thresholds
  (c) by_chain     the same history with every chain one bin: a 46 x 46 table
  numpy            tests/dmap_restatement.py on this host on a cut of (b) (64 frames of 600 beads): its pairs per second, and the
                   device's sums on the same cut checked against it (hits equal, sums within the header's bound)
  Rdf.counts       the frames of (a), and 16 frames of (b), through rdf.py with max_distance = the larger threshold in a box wide
                   enough to act as open: what a cell walk pays for the pairs inside one cutoff only
These are reference points, not pass marks.  --scale shrinks every shape (a rehearsal, not a measurement).  --only CASE runs one
case alone: for a run under `rocprofv3 --kernel-trace --stats`, whose per-kernel means then belong to that case.  --out FILE is
rewritten after every case, so that a run that is cut short leaves what it measured."""
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
import dmap_restatement as dm      # noqa: E402

dmap = importlib.import_module("2022a-genome-dynamics_amd.dmap")
rdf = importlib.import_module("2022a-genome-dynamics_amd.rdf")

THRESHOLDS = (0.5, 1.0)


def timed(repeats, fn, *args, **kw):
    fn(*args, **kw)      # warm-up: code objects, buffers
    v = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn(*args, **kw)
        v.append(time.perf_counter() - t)
    return {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}, out


def walk(frames, beads, seed):
    """Beads spread over a ball of radius about 5 that drift a little from frame to frame."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.05)
    x[0] += rng.standard_normal((beads, 3), dtype=np.float32) * np.float32(3.0)
    return np.cumsum(x, axis=0, dtype=np.float32)


def chromosomes(beads, n):
    w = np.linspace(1.0, 5.0, n)[::-1]
    ends = np.round(np.cumsum(w) / w.sum() * beads).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    return np.stack([starts, ends], axis=1)


def case(res, name, repeats, d, **kw):
    t, m = timed(repeats, d.map, thresholds=THRESHOLDS, **kw)
    pairs = int(m["count"].sum())
    res[name] = dict(t, bins=int(m["count"].shape[0]), pairs=pairs, pairs_per_s=pairs / t["median_s"],
                     contact_frequency=[float(h.sum()) / pairs for h in m["hits"]])
    assert m["sum1"].tobytes() == m["sum1"].T.tobytes()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["chromosome", "genome", "by_chain"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N, N1 = max(int(701 * a.scale), 9), max(int(62178 * a.scale), 700), max(int(2253 * a.scale), 100)
    res = {"frames": F, "beads": N, "chromosome_beads": N1, "thresholds": list(THRESHOLDS), "repeats": a.repeats}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    x = walk(F, N, 1)
    chains = chromosomes(N, 46)
    want = lambda name: a.only in (None, name)      # noqa: E731
    if want("chromosome"):
        with dmap.Dmap(0) as d:
            res["set_history_chromosome"], _ = timed(a.repeats, d.set_history, x[:, :N1])
            case(res, "chromosome", a.repeats, d)
        save()
    with dmap.Dmap(0) as d:
        if want("genome") or want("by_chain"):
            res["set_history_genome"], _ = timed(a.repeats, d.set_history, x)
        if want("genome"):
            d.set_bins(dmap.Dmap.bins_from_chains(chains, 10))
            case(res, "genome_rate_10", a.repeats, d)
            save()
        if want("by_chain"):
            d.set_bins(chains)
            case(res, "by_chain", a.repeats, d)
            save()
    if a.only is None:
        # the restatement on this host, and the device against it
        cut = np.ascontiguousarray(x[:64, :600])
        bins = dmap.Dmap.bins_from_chains([(0, 600)], 10)
        t = time.perf_counter()
        sum1, sum2, hits, count = dm.dmap(cut, bins, thresholds=THRESHOLDS)
        res["numpy_cut_s"] = time.perf_counter() - t
        res["numpy_pairs_per_s"] = int(count.sum()) / res["numpy_cut_s"]
        with dmap.Dmap(0) as d:
            d.set_history(cut)
            d.set_bins(bins)
            m = d.map(thresholds=THRESHOLDS)
        assert np.array_equal(m["hits"], hits) and np.array_equal(m["count"], count)
        err = max(float((np.abs(m[k] - w) / dm.bound(count, w)).max()) for k, w in (("sum1", sum1), ("sum2", sum2)))
        assert err <= 1.0, err
        res["largest_error_over_bound"] = err
        if "genome_rate_10" in res:
            res["device_over_numpy_pairs_per_s"] = res["genome_rate_10"]["pairs_per_s"] / res["numpy_pairs_per_s"]
        save()
        # the pairs inside one cutoff through the cell walk of rdf.py
        lo, hi = float(x.min()), float(x.max())
        with rdf.Rdf(0) as r:
            for name, frames in (("rdf_counts_chromosome", x[:, :N1]), ("rdf_counts_genome_16_frames", x[:16])):
                shifted = np.ascontiguousarray(frames - np.float32(lo - 1.0))
                res[name], counts = timed(a.repeats, r.counts, shifted, hi - lo + 4.0, THRESHOLDS[1] / 50, THRESHOLDS[1], np.arange(shifted.shape[1]))
                res[name]["frames"] = int(shifted.shape[0])
                res[name]["pairs_counted"] = int(counts.sum())
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

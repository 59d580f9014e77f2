#!/usr/bin/env python3
"""The displacement covariance maps (include/gdyn_dcov.h, dcov.py) at the sizes a user runs them, one JSON line.  Device times are
the library's own, between HIP events on the handle's stream (gd_dcov_last_times): stage 1 per prepare, the product kernel and the
merge kernel per map; the host clock around the synchronous map call stands beside them (it adds the copy of the map to the host).
Every figure is the median (min - max) of --repeats calls after a warm-up call.

  (a) bins_3000        3 000 bins x 1 000 origins (30 000 beads at 10 per bin, 1 001 frames, lag 1), the whole map
  (b) bins_12000       12 000 bins x 1 000 origins (the same history at bead resolution, the first 12 000 beads as one chain)
  (c) rectangle_4096   a rectangle of 4 096 x 4 096 cells at bead resolution of the 30 000-bead history, off the diagonal
  numpy                the same product, `A @ A.T` in fp64 by numpy on this host's threads, fed the device's rows of (a) (the whole
                       map) and the first --numpy-rows rows of (b), extrapolated to (b) by the square of the row ratio and said so

A flop is one multiply or one add of the cells the call returns: 2 * cells * K with K the padded column count; the device computes
the canonical half and mirrors it, so its product kernel does about half of that arithmetic for a whole map.  product_tflops is
(cells computed by the kernel: 64 x 64 per canonical tile) * 2 K / product time.  These are observations, not pass marks.  --scale
shrinks every shape (a rehearsal, not a measurement).  --only CASE runs one case alone.  --out FILE is rewritten after every case."""
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
import dcov_restatement as dc      # noqa: E402

dcov = importlib.import_module("2022a-genome-dynamics_amd.dcov")
TILE = 64


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def walk(frames, beads, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.05)
    x[0] += rng.standard_normal((beads, 3), dtype=np.float32) * np.float32(3.0)
    return np.cumsum(x, axis=0, dtype=np.float32)


def canonical_tiles(rows, cols):
    keys = {(min(i, j), max(i, j)) for i in range(rows[0] // TILE, (rows[0] + rows[1] - 1) // TILE + 1)
            for j in range(cols[0] // TILE, (cols[0] + cols[1] - 1) // TILE + 1)}
    keys |= {(t, t) for r in (rows, cols) for t in range(r[0] // TILE, (r[0] + r[1] - 1) // TILE + 1)}      # diag_rows, diag_cols
    return len(keys)


def case(res, name, repeats, d, lag, rows=None, cols=None):
    stage1 = []
    for _ in range(repeats + 1):
        columns = d.prepare(lag)
        stage1.append(d.last_times()["stage1_ms"])
    rows = rows or (0, d.n_bins)
    cols = cols or (0, d.n_bins)
    host, product, merge, m = [], [], [], None
    for _ in range(repeats + 1):
        t = time.perf_counter()
        m = d.map(rows=rows, cols=cols)
        host.append((time.perf_counter() - t) * 1e3)
        lt = d.last_times()
        product.append(lt["product_ms"])
        merge.append(lt["merge_ms"])
    K = dc.padded(columns)
    kernel_flop = canonical_tiles(rows, cols) * TILE * TILE * 2.0 * K
    res[name] = {"bins": d.n_bins, "rows": rows[1], "cols": cols[1], "columns": columns, "stage1_ms": spread(stage1[1:]), "product_ms": spread(product[1:]),
                 "merge_ms": spread(merge[1:]), "map_call_host_ms": spread(host[1:]), "kernel_flop": kernel_flop,
                 "product_tflops": kernel_flop / (np.median(product[1:]) * 1e-3) / 1e12,
                 "returned_cells_tflops": 2.0 * rows[1] * cols[1] * K / (np.median(product[1:]) * 1e-3) / 1e12}
    if rows == cols:
        assert m["sum"].tobytes() == np.ascontiguousarray(m["sum"].T).tobytes()
    return m


def numpy_product(a, repeats):
    v = []
    out = None
    for _ in range(repeats + 1):
        t = time.perf_counter()
        out = a @ a.T
        v.append((time.perf_counter() - t) * 1e3)
    return spread(v[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=3000)
    ap.add_argument("--only", choices=["bins_3000", "bins_12000", "rectangle_4096"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(1000 * a.scale), 8) + 1, max(int(30000 * a.scale), 400)
    N2, R = min(max(int(12000 * a.scale), 300), N), min(max(int(4096 * a.scale), 100), N // 2)
    res = {"frames": F, "beads": N, "lag": 1, "repeats": a.repeats, "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    x = walk(F, N, 1)
    want = lambda name: a.only in (None, name)      # noqa: E731
    with dcov.Dcov(0) as d:
        d.set_history(x)
        if want("bins_3000"):
            d.set_bins(dcov.Dcov.bins_from_chains([(0, N)], 10))
            m = case(res, "bins_3000", a.repeats, d, 1)
            if a.only is None:
                rows = d.rows()
                res["numpy_bins_3000_ms"], ref = numpy_product(rows, a.repeats)
                if dc.LONGDOUBLE_64:      # a corner of the map against the long-double product of the device's rows
                    exact, mag = dc.reference(rows[:96])
                    res["largest_error_over_bound"] = float(np.max(np.abs(m["sum"][:96, :96].astype(np.longdouble) - exact) / dc.bound(mag, d.columns)))
                    assert res["largest_error_over_bound"] <= 1.0
                res["numpy_max_relative_difference"] = float(np.max(np.abs(ref - m["sum"])) / np.max(np.abs(ref)))
                res["device_product_over_numpy_bins_3000"] = res["numpy_bins_3000_ms"]["median"] / res["bins_3000"]["product_ms"]["median"]
            save()
        if want("bins_12000"):
            d.set_bins([(i, i + 1) for i in range(N2)])
            case(res, "bins_12000", a.repeats, d, 1)
            if a.only is None:
                n = min(a.numpy_rows, N2)
                res["numpy_rows_of_bins_12000"] = n
                res["numpy_part_of_bins_12000_ms"], _ = numpy_product(d.rows(0, n), a.repeats)
                res["numpy_bins_12000_ms_extrapolated"] = res["numpy_part_of_bins_12000_ms"]["median"] * (N2 / n) ** 2
                res["numpy_bins_12000_is_extrapolated_by"] = f"(bins / {n})^2 from a product of {n} rows"
                res["device_product_over_numpy_bins_12000"] = res["numpy_bins_12000_ms_extrapolated"] / res["bins_12000"]["product_ms"]["median"]
            save()
        if want("rectangle_4096"):
            d.set_bins(None)
            case(res, "rectangle_4096", a.repeats, d, 1, rows=(TILE, R), cols=(N - R - 7, R))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

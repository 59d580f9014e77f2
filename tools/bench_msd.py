#!/usr/bin/env python3
"""The lag statistics (include/gdyn_msd.h, msd.py) at the sizes a user runs them, host clock around the synchronous calls, median
(min - max) of five each, one JSON line:

  genome shape, (701, 62 178) float32, groups = four bead classes in blocks along the genome, 46 chromosome-like chains
    set_history          from host memory, and from a live.History that recorded a free-bead system of that size
    time()               8 log-spaced lags and all 700, and their ratio
    chain()              40 log-spaced separations and all of them (up to the longest chain), all frames
    numpy                tests/msd_restatement.py on the same host for the 8-lag case: the only baseline there is, and the device
                         sums are checked against it within the header's bound (2 count + 8) 2^-53
  1 kb shape, (50, 250 000) float32, one chain: chain() with 40 log-spaced separations up to 100 000 (the windowed path)

--scale shrinks every shape (a rehearsal, not a measurement).  --only CASE runs one case of the genome shape alone (time8, timeall,
chain40, chainall): for a run under `rocprofv3 --kernel-trace --stats`, whose per-kernel means then belong to that case."""
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
import msd_restatement as mr      # noqa: E402

g = importlib.import_module("2022a-genome-dynamics_amd")
msd = importlib.import_module("2022a-genome-dynamics_amd.msd")
live = importlib.import_module("2022a-genome-dynamics_amd.live")

REPEATS = 5


def timed(fn, *args, **kw):
    fn(*args, **kw)      # warm-up: code objects, buffers
    v = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        out = fn(*args, **kw)
        v.append(time.perf_counter() - t)
    return {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)}, out


def walk(frames, beads, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.05)
    x[0] += rng.standard_normal((beads, 3), dtype=np.float32) * np.float32(5.0)
    return np.cumsum(x, axis=0, dtype=np.float32)


def coil(frames, beads, seed):
    """A walk along the chain in every frame."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((frames, beads, 3), dtype=np.float32) * np.float32(0.05), axis=1, dtype=np.float32)


def chromosomes(beads, n):
    w = np.linspace(1.0, 5.0, n)[::-1]
    ends = np.round(np.cumsum(w) / w.sum() * beads).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    return np.stack([starts, ends], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--only", choices=["time8", "timeall", "chain40", "chainall"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, N = max(int(701 * a.scale), 9), max(int(62178 * a.scale), 100)
    res = {"genome": {"frames": F, "beads": N, "history_bytes": F * N * 12}}
    gen = res["genome"]
    x = walk(F, N, 1)
    group = (np.arange(N) // 50) % 4
    chains = chromosomes(N, 46)
    longest = int((chains[:, 1] - chains[:, 0]).max())
    with msd.Msd(0) as m:
        gen["set_history_host"], _ = timed(m.set_history, x)
        m.set_groups(group, 4)
        m.set_chains(chains)
        lags8, lags_all = mr.log_lags(8, F - 1), list(range(1, F))
        if a.only:
            call, arg = {"time8": (m.time, lags8), "timeall": (m.time, lags_all), "chain40": (m.chain, mr.log_lags(40, longest - 1)),
                         "chainall": (m.chain, list(range(1, longest)))}[a.only]
            gen[a.only], _ = timed(call, arg)
            print(json.dumps(res))
            return
        gen["time_8_lags"], (sum2, count) = timed(m.time, lags8)
        gen["time_all_lags"], (all2, alln) = timed(m.time, lags_all)
        gen["lags_all"] = len(lags_all)
        gen["terms_8_lags"] = int(count.sum())
        gen["terms_all_lags"] = int(alln.sum())
        gen["all_over_8"] = gen["time_all_lags"]["median_s"] / gen["time_8_lags"]["median_s"]
        assert all2[:, [l - 1 for l in lags8]].tobytes() == sum2.tobytes()
        seps40, seps_all = mr.log_lags(40, longest - 1), list(range(1, longest))
        gen["chain_40_seps"], (c2, cn) = timed(m.chain, seps40)
        gen["chain_all_seps"], (call2, calln) = timed(m.chain, seps_all)
        gen["seps_all"] = len(seps_all)
        gen["terms_40_seps"] = int(cn.sum())
        gen["terms_all_seps"] = int(calln.sum())
        assert call2[:, [s - 1 for s in seps40]].tobytes() == c2.tobytes()
        if not a.skip_numpy:
            t = time.perf_counter()
            want2, _, wantn = mr.time(x, lags8, group, 4)
            gen["numpy_8_lags_s"] = time.perf_counter() - t
            assert np.array_equal(count, wantn)
            err, tol = np.abs(sum2 - want2), mr.bound(count, want2)
            assert (err <= tol).all(), (err / tol).max()
            gen["numpy_over_device_8_lags"] = gen["numpy_8_lags_s"] / gen["time_8_lags"]["median_s"]
            gen["largest_error_over_bound"] = float((err / tol).max())
        # the same history from a recorder on the device
        s = g.System(g.load(), N, 1)
        s.set_positions(x[0].astype(np.float64))
        with s, live.History(s) as hist:
            for k in range(F):
                s.run(1, 1e-4, 1.0, seed=3, noise=g.NOISE_PHILOX)
                hist.record(quantize=True)
            gen["set_history_live"], _ = timed(m.set_history_from, hist, 0)
            assert m.shape == (F, N)
    del x
    F1, N1 = max(int(50 * a.scale), 3), max(int(250000 * a.scale), 1000)
    x = coil(F1, N1, 2)
    seps = mr.log_lags(40, max(int(100000 * a.scale), 10))
    with msd.Msd(0) as m:
        m.set_history(x)
        m.set_chains([(0, N1)])
        kb = {"frames": F1, "beads": N1, "seps": len(seps), "largest_sep": seps[-1]}
        kb["chain_40_seps"], (c2, cn) = timed(m.chain, seps)
        kb["terms"] = int(cn.sum())
        if not a.skip_numpy:
            want2, _, wantn = mr.chain(x, [(0, N1)], seps[::8])
            assert np.array_equal(cn[:, ::8], wantn) and (np.abs(c2[:, ::8] - want2) <= mr.bound(wantn, want2)).all()
        res["one_kb"] = kb
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

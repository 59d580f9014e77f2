#!/usr/bin/env python3
"""What per-replica A/B tables (include/gdyn_ensemble.h) cost in the steady state: two handles of --replicas x --beads beads of
workloads.genome_interphase in one process, brought to the headline's relaxed state the same way (bench.py: --equil steps with static
scales and wall from the random-walk start, then the timed regime's flags),

homogeneous    every replica under the workload's shared table: bond records mixed per bond on the host;
heterogeneous  replica r under the shared table with its runs of equal type permuted under seed r (the composition is kept): one
               table per replica on the device, bond records mixed in the kernels from the two beads' factors.

--steps steps, --repeats alternating repetitions: milliseconds per step as median, minimum and maximum, the list entries per bead,
the rebuild interval and the list path of both.  One JSON line; --output writes it to a file as well."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
g = importlib.import_module("2022a-genome-dynamics_amd")
wl = importlib.import_module("2022a-genome-dynamics_amd.workloads")
ensemble = importlib.import_module("2022a-genome-dynamics_amd.ensemble")


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def permuted_runs(a, b, seed):
    """(a, b) with the maximal runs of equal (a, b) in another order"""
    cut = np.flatnonzero((np.diff(a) != 0) | (np.diff(b) != 0)) + 1
    order = np.random.default_rng(seed).permutation(len(cut) + 1)
    pa, pb = np.split(a, cut), np.split(b, cut)
    return np.concatenate([pa[k] for k in order]), np.concatenate([pb[k] for k in order])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--beads", type=int, default=30000)
    ap.add_argument("--replicas", type=int, default=128)
    ap.add_argument("--equil", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--output", default="")
    a = ap.parse_args()
    hip = g.load()
    flags = g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
    handles = {}
    for name in ("homogeneous", "heterogeneous"):
        s, info = wl.genome_interphase(hip, n_beads=a.beads, n_replicas=a.replicas)
        if name == "heterogeneous":
            a0, b0 = wl.ab_types(a.beads, np.random.default_rng(wl.MASTER_SEED))      # the workload's shared table
            assert np.array_equal(ensemble.get_ab(s, 0)[0], a0)
            for r in range(a.replicas):
                ensemble.set_ab(s, r, *permuted_runs(a0, b0, r))
        dt, kT = info["timestep"], info["temperature"]
        s.begin_phase()
        s.run(a.equil, dt, kT, seed=wl.MASTER_SEED + 17, flags=0)
        s.begin_phase()
        s.run(2 * a.steps, dt, kT, seed=wl.MASTER_SEED, flags=flags)      # (the interval adapts on complete intervals of the timed regime)
        handles[name] = s
        print(f"{name}: relaxed", file=sys.stderr, flush=True)
    per_step = {k: [] for k in handles}
    for rep in range(a.repeats):
        for name in (("homogeneous", "heterogeneous") if rep % 2 else ("heterogeneous", "homogeneous")):
            t = time.perf_counter()
            handles[name].run(a.steps, dt, kT, seed=wl.MASTER_SEED + 100 + rep, flags=flags)      # synchronous
            per_step[name].append((time.perf_counter() - t) * 1e3 / a.steps)
    res = {"beads": a.beads, "replicas": a.replicas, "equil_steps": a.equil, "steps": a.steps, "repeats": a.repeats}
    for name, s in handles.items():
        c = s.context(0)
        res[name] = {"ms_per_step": stats(per_step[name]), "classes": int(ensemble.classes(s)[1]),
                     "entries_per_bead": float(np.mean([s.context(r).list_entries for r in range(a.replicas)])) / a.beads,
                     "rebuild_interval": int(c.rebuild_interval), "list_path": int(c.list_path), "rollbacks": int(c.rollbacks)}
    res["heterogeneous_over_homogeneous"] = res["heterogeneous"]["ms_per_step"]["median"] / res["homogeneous"]["ms_per_step"]["median"]
    line = json.dumps(res)
    print(line)
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

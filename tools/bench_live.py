#!/usr/bin/env python3
"""The live bridge (include/gdyn_live.h) against the host-fed sequences it replaces, in one process on states the stepper
produces.  Per case the two paths alternate five times; the JSON line holds the median, minimum and maximum of the host-clock
seconds of each (every call ends in a device synchronise) and their ratio, and the results of the two paths are checked equal.
  genome models (workloads.genome_interphase) of 128 x 30 000 and 8 x 62 178 beads after --steps steps with a contact update
  every 100:
    contacts         live.contacts into one binned target at rebin rate 10
                     against System.contacts(r) + ContactMaps.accumulate for every replica; both timed calls start with
                     ContactMaps.reset and end with the fetch of the target, so the same fixed cost sits in both
    lamina_contacts  live.lamina_contacts (with the contacts copied back, and with want_contacts=False)
                     against System.positions_f32 + the contexts' semiaxes + Lamina.distances (float32) + Lamina.contacts
  the S-AB-box model (workloads.ab_box, 2 000 beads) with 16 replicas:
    rdf_counts       live.rdf_counts of all A beads, bin width 0.1, max distance 1
                     against System.positions_f32 + Rdf.counts
Kernel times: run it under `rocprofv3 --kernel-trace --stats` as a run of its own (--cases picks the cases)."""
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
cmap = importlib.import_module("2022a-genome-dynamics_amd.cmap")
lamina = importlib.import_module("2022a-genome-dynamics_amd.lamina")
rdf = importlib.import_module("2022a-genome-dynamics_amd.rdf")
live = importlib.import_module("2022a-genome-dynamics_amd.live")

REPEATS = 5


def alternate(paths):
    """paths: {name: callable}; runs them in turn REPEATS times; {name: {median_s, min_s, max_s}} and the last results."""
    ts, last = {k: [] for k in paths}, {}
    for _ in range(REPEATS):
        for name, fn in paths.items():
            t = time.perf_counter()
            last[name] = fn()
            ts[name].append(time.perf_counter() - t)
    return {k: {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v)} for k, v in ts.items()}, last


def with_ratio(times, base="host_fed"):
    for k, v in times.items():
        if k != base:
            v["host_fed_over_this"] = times[base]["median_s"] / v["median_s"]
    return times


def genome_case(hip, n_beads, replicas, steps):
    s, info = wl.genome_interphase(hip, n_beads=n_beads, n_replicas=replicas)
    res = {"beads": n_beads, "replicas": replicas, "steps": steps}
    with s, cmap.ContactMaps(0) as cm, lamina.Lamina(0) as host_lam, lamina.Lamina(0) as live_lam, lamina.Lamina(0) as quiet_lam:
        s.begin_phase()
        for k in range(steps // 100):
            s.run(100, info["timestep"], 1.0, seed=1 + k, flags=g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS)
            s.contacts_update(0.4)
        rebin, binned = cmap.rebin_map(np.array(info["ranges"]), 10)
        t = cm.add_binned(rebin, int(binned.max()))
        res["rows"] = int(sum(len(s.contacts(r)) for r in range(replicas)))

        def host_contacts():
            cm.reset()
            for r in range(replicas):
                cm.accumulate(s.contacts(r))
            return cm.fetch(t)

        def live_contacts():
            cm.reset()
            live.contacts(s, cm)
            return cm.fetch(t)

        host_contacts(), live_contacts()                         # warm-up: code objects, buffers
        times, last = alternate({"host_fed": host_contacts, "live": live_contacts})
        assert np.array_equal(last["host_fed"], last["live"]) and last["live"].any()
        res["contacts"] = with_ratio(times)

        def host_lamina():
            x = s.positions_f32()
            semi = np.array([list(s.context(r).semiaxes) for r in range(replicas)])
            return host_lam.contacts(host_lam.distances(x, semi, dtype=np.float32), 0.3)

        host_lamina(), live.lamina_contacts(s, live_lam, 0.3), live.lamina_contacts(s, quiet_lam, 0.3, want_contacts=False)
        times, last = alternate({"host_fed": host_lamina, "live": lambda: live.lamina_contacts(s, live_lam, 0.3),
                                 "live_sum_only": lambda: live.lamina_contacts(s, quiet_lam, 0.3, want_contacts=False)})
        assert np.array_equal(last["host_fed"], last["live"]) and np.array_equal(host_lam.average(), quiet_lam.average())
        res["lamina_contacts"] = with_ratio(times)
        res["contact_fraction"] = float(last["live"].mean())
    return res


def box_case(hip, replicas, steps):
    s, info = wl.ab_box(hip, n_replicas=replicas)
    n = info["n_beads"]
    centers = np.array([i for i in range(n) if (i // 20) % 2 == 0], np.uint32)
    res = {"beads": n, "replicas": replicas, "steps": steps, "box": info["box"]}
    with s, rdf.Rdf(0) as host_rdf, rdf.Rdf(0) as live_rdf:
        s.run(steps, info["timestep"], 1.0, seed=1)
        live_rdf.set_selection(n, centers)
        host = lambda: host_rdf.counts(s.positions_f32(), info["box"], 0.1, 1.0, centers)      # noqa: E731
        host(), live.rdf_counts(s, live_rdf, 0.1, 1.0)
        times, last = alternate({"host_fed": host, "live": lambda: live.rdf_counts(s, live_rdf, 0.1, 1.0)})
        assert np.array_equal(last["host_fed"], last["live"]) and last["live"].any()
        res["rdf_counts"] = with_ratio(times)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--cases", default="128x30000,8x62178,box", help="comma-separated: RxN genome models, box")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = g.load()
    res = {}
    for case in a.cases.split(","):
        if case == "box":
            res["S-AB-box x16"] = box_case(hip, 16, a.steps)
        else:
            r, n = (int(v) for v in case.split("x"))
            res[f"S-genome {r}x{n}"] = genome_case(hip, n, r, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""The threshold table of the prepared contexts: one handle per shape, two replica groups (mode 2), the
developer library's GDYN_CTX_PREP 0 (never) and 2 (every grouped span) alternating over four repetitions of 2 000 steps; wall time and
span time (gd_timing.step_kernel_ms) per step, median.  Needs csrc/libgdyn_dev.so (make -C csrc dev).
usage: ctx_prep_threshold.py [out.json]"""
import importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
g = importlib.import_module("2022a-genome-dynamics_amd")
wl = importlib.import_module("2022a-genome-dynamics_amd.workloads")
SHAPES = [(30000, 64), (30000, 32), (30000, 16), (15000, 16)]
STEPS, REPS, EQUIL, WARM = 2000, 4, 6000, 600
dev = g.load("libgdyn_dev.so")
flags = g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
rows = []
for n, r in SHAPES:
    s, info = wl.genome_interphase(dev, n_beads=n, n_replicas=r)
    dt, kT = info["timestep"], info["temperature"]
    s.begin_phase()
    s.run(EQUIL, dt, kT, seed=17, flags=0)
    s.begin_phase()
    s.set_step_groups(2)
    s.run(WARM, dt, kT, seed=3, flags=flags)
    wall, span, launches = {0: [], 2: []}, {0: [], 2: []}, {}
    for rep in range(REPS):
        for mode in (0, 2):
            os.environ["GDYN_CTX_PREP"] = str(mode)
            t0 = time.perf_counter()
            t = s.run(STEPS, dt, kT, seed=3, flags=flags)
            wall[mode].append((time.perf_counter() - t0) * 1e3 / STEPS)
            span[mode].append(t.step_kernel_ms / STEPS)
            launches[mode] = s.ctx_prepared()
            assert s.step_groups()[1] == 2
    c = s.context()
    row = {"n_beads": n, "replicas": r, "blocks_of_the_smaller_group": (r // 2) * -(-n // 512), "rebuild_interval": c.rebuild_interval, "rollbacks": c.rollbacks,
           "prep_launches": launches}
    for mode, name in ((0, "in_kernel"), (2, "prepared")):
        row[name] = {"wall_ms_per_step": statistics.median(wall[mode]), "span_ms_per_step": statistics.median(span[mode]),
                     "wall_all": wall[mode], "span_all": span[mode]}
    row["prepared_over_in_kernel_wall"] = row["prepared"]["wall_ms_per_step"] / row["in_kernel"]["wall_ms_per_step"]
    row["prepared_over_in_kernel_span"] = row["prepared"]["span_ms_per_step"] / row["in_kernel"]["span_ms_per_step"]
    rows.append(row)
    print(json.dumps({k: v for k, v in row.items() if k not in ("in_kernel", "prepared")}), row["in_kernel"]["wall_ms_per_step"], row["prepared"]["wall_ms_per_step"], flush=True)
    s.close()
os.environ.pop("GDYN_CTX_PREP", None)
if len(sys.argv) > 1:
    json.dump({"_comment": __doc__, "steps": STEPS, "repetitions": REPS, "rows": rows}, open(sys.argv[1], "w"), indent=1)

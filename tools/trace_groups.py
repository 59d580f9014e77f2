"""Step launches of a rocprofv3 --kernel-trace csv of a grouped run: k_step per launch, k_ctx_prep per launch, the gap a preparation
launch leaves on its queue (end of the step before it -> start of the step behind it, less the preparation kernel itself), the time
the step kernels cover and the share of it in which two of them run at once (profiles/*_trace_summary.json).
usage: trace_groups.py <dir> [skip_launches]"""
import csv, glob, json, statistics, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
iv = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
steps = [r for r in rows if r["Kernel_Name"].startswith(("void k_step<0", "k_step<0"))][skip:]
preps = [r for r in rows if "k_ctx_prep" in r["Kernel_Name"]]
t0 = int(steps[0]["Start_Timestamp"])
preps = [r for r in preps if int(r["Start_Timestamp"]) >= t0]
out = {"step_launches": len(steps), "queues": len({r["Queue_Id"] for r in steps}), "kernel": steps[-1]["Kernel_Name"].split("(")[0],
       "mean_step_launch_us": statistics.mean(e - s for s, e in map(iv, steps)) / 1e3,
       "median_step_launch_us": statistics.median(e - s for s, e in map(iv, steps)) / 1e3}
if preps:
    out["prep_launches"] = len(preps)
    out["mean_prep_us"] = statistics.mean(e - s for s, e in map(iv, preps)) / 1e3
# per queue: the idle time between two consecutive step kernels (whatever runs in it)
gaps = []
for q in {r["Queue_Id"] for r in steps}:
    qs = [iv(r) for r in steps if r["Queue_Id"] == q]
    gaps += [b[0] - a[1] for a, b in zip(qs, qs[1:]) if b[0] - a[1] < 50000]      # (a list build lies between two spans: not a gap of the span)
out["median_gap_between_steps_on_a_queue_us"] = statistics.median(gaps) / 1e3 if gaps else None
out["mean_gap_between_steps_on_a_queue_us"] = statistics.mean(gaps) / 1e3 if gaps else None
# covered time and the time two step kernels run at once: a sweep over the interval ends
ev = sorted([(s, 1) for s, _ in map(iv, steps)] + [(e, -1) for _, e in map(iv, steps)])
depth, last, covered, two = 0, ev[0][0], 0, 0
for t, d in ev:
    if depth >= 1: covered += t - last
    if depth >= 2: two += t - last
    depth += d; last = t
out.update(kernel_sum_ms=sum(e - s for s, e in map(iv, steps)) / 1e6, covered_ms=covered / 1e6, two_at_once_ms=two / 1e6, two_at_once_share=two / covered)
print(json.dumps(out, indent=1))

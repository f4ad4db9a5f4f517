"""The step pipeline's timeline from a rocprofv3 kernel trace (csv) of bench.py: the last dat_closed_loop call of
the run (from its unfiltered k_bucket on), per step the main drain (the k_cadmm after k_bucket or
k_bucket_adv<ADV_EARLY> in its queue), the rest drain (after k_bucket_adv<ADV_REST>) and the passes around them.
Prints median (min - max) in microseconds over the call's steps.

    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python bench.py --steps 10 --warmup 2
    python tools/pipeline_trace.py DIR/.../run_kernel_trace.csv
"""
import csv
import sys

import numpy as np

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"]))
rows.sort()


def kind(name):
    for key, tag in (("k_bucket_adv<1>", "sort_main"), ("k_bucket_adv<2>", "sort_rest"),
                     ("k_bucket_scatter<1>", "sort_main"), ("k_bucket_scatter<2>", "sort_rest"), ("k_bucket", "sort_all"),
                     ("k_cadmm_tail", "tail"), ("k_cadmm0_tail", "tail"), ("k_cadmm", "drain"),
                     ("k_rollout_agents<false, 1>", "roll_early"), ("k_rollout_agents<false, 2>", "roll_rest"),
                     ("k_env_class<1>", "env_early"), ("k_env_class<2>", "env_rest"),
                     ("k_desired<1>", "des_early"), ("k_desired<2>", "des_rest"),
                     ("k_advance<1>", "adv_early"), ("k_advance<2>", "adv_rest")):
        if key in name:
            return tag
    return None


ev = [(s, e, kind(nm), q) for s, e, nm, q in rows if kind(nm)]
first = max(i for i, v in enumerate(ev) if v[2] == "sort_all")
ev = ev[first:]


def drain_after(i):
    """the k_cadmm that follows sort ev[i] in its queue"""
    for v in ev[i + 1:]:
        if v[3] == ev[i][3] and v[2] == "drain":
            return v
    return None


mains = [(v, drain_after(i)) for i, v in enumerate(ev) if v[2] in ("sort_all", "sort_main")]
rests = [(v, drain_after(i)) for i, v in enumerate(ev) if v[2] == "sort_rest"]
mains = [(s, d) for s, d in mains if d]
rests = [(s, d) for s, d in rests if d]
of = lambda tag: [v for v in ev if v[2] == tag]  # noqa: E731


def line(label, vals):
    v = np.array(vals, dtype=float) / 1e3
    if len(v):
        print(f"| {label} | {np.median(v):.1f} | {v.min():.1f} | {v.max():.1f} | {len(v)} |")


print(f"main drains {len(mains)}, rest drains {len(rests)}")
print("| | median | min | max | count |\n|---|---|---|---|---|")
line("sort of a main drain (k_bucket, k_bucket_adv<EARLY>)", [s[1] - s[0] for s, _ in mains])
line("main drain k_cadmm", [d[1] - d[0] for _, d in mains])
line("main drain start -> next main drain start (the step)", [b[1][0] - a[1][0] for a, b in zip(mains, mains[1:])])
line("main drain starts before the previous main drain ends", [a[1][1] - b[1][0] for a, b in zip(mains, mains[1:])])
line("... both alive", [max(0, min(a[1][1], b[1][1]) - b[1][0]) for a, b in zip(mains, mains[1:])])
line("sort of a rest drain (k_bucket_adv<REST>)", [s[1] - s[0] for s, _ in rests])
line("rest drain k_cadmm", [d[1] - d[0] for _, d in rests])
# a rest drain belongs to the step of the main drain that started last before it
pairs = [(max((m for m in mains if m[1][0] <= d[0]), key=lambda m: m[1][0], default=None), d) for _, d in rests]
line("rest drain starts after its step's main drain starts", [d[0] - m[1][0] for m, d in pairs if m])
line("rest drain ends before (+) / after (-) its step's main drain ends", [m[1][1] - d[1] for m, d in pairs if m])
line("rest drain and its step's main drain both alive", [max(0, min(m[1][1], d[1]) - d[0]) for m, d in pairs if m])
for tag, label in (("roll_early", "early rollout"), ("env_early", "early env rows"), ("adv_early", "early k_advance"),
                   ("roll_rest", "rest rollout"), ("env_rest", "rest env rows"), ("adv_rest", "rest k_advance")):
    line(f"{label}: duration", [v[1] - v[0] for v in of(tag)])
    starts = [(max((m for m in mains if m[1][0] <= v[0]), key=lambda m: m[1][0], default=None), v) for v in of(tag)]
    line(f"{label}: starts after the latest main drain's start", [v[0] - m[1][0] for m, v in starts if m])
print(f"call span {(ev[-1][1] - ev[0][0]) / 1e3:.1f} us")

# The chain from one main drain's start to the next: what runs in the next main drain's queue in between (the early
# pass: the three kernels or k_advance, then the sort), link by link; the gaps are what the links leave of the period.
CHAIN = (("roll_early", "k_rollout_agents<ADV_EARLY>"), ("des_early", "k_desired<ADV_EARLY>"),
         ("env_early", "k_env_class<ADV_EARLY>"), ("adv_early", "k_advance<ADV_EARLY>"),
         ("sort_main", "k_bucket_adv<ADV_EARLY> / k_bucket_scatter<ADV_EARLY>"))
links = {tag: [] for tag, _ in CHAIN}
wait, gaps, period = [], [], []
for a, b in zip(mains, mains[1:]):
    t0, t1, q = a[1][0], b[1][0], b[1][3]
    mid = [v for v in ev if v[3] == q and t0 < v[0] < t1 and v[2] in links]
    if not mid:
        continue
    wait.append(mid[0][0] - t0)
    for v in mid:
        links[v[2]].append(v[1] - v[0])
    period.append(t1 - t0)
    gaps.append(t1 - t0 - (mid[0][0] - t0) - sum(v[1] - v[0] for v in mid))
print("\nthe chain, main drain's start -> next main drain's start\n| link | median | min | max | count |\n|---|---|---|---|---|")
line("main drain's start -> the early pass's first kernel starts", wait)
for tag, label in CHAIN:
    line(label, links[tag])
line("launch gaps (the rest of the period)", gaps)
line("period", period)

"""The active-set store's measurement table from its raw lines
(profiles/active_store_measure.jsonl: one JSON line per run; tag = library, setting = none | export |
min_steps | nonealt (the other layout, no store)). Means over the runs of a setting (the event-timed
us/step: the median, a run's first call can carry a millisecond of set-up); launch times
in microseconds from mpccbf_run::kernel_clock, it0 / it1 = per-step sum of iteration-0 / -1 solver
steps over the agents.

    python tools/store_measure_summary.py [profiles/active_store_measure.jsonl]
"""
import collections
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "active_store_measure.jsonl")
    runs = collections.defaultdict(list)
    for ln in open(path):
        r = json.loads(ln)
        runs[(r["per"], r["tag"], r["setting"])].append(r)
    for per in sorted({k[0] for k in runs}, reverse=True):
        print(f"{per} agents per launch")
        print(f"  {'library':7s} {'setting':8s} runs | driver window: us/step launch all / steps 10-19  it0max it0 it1 | "
              f"300 steps: us/step launch  it0max it1max it0 it1 | kernel")
        for (p, tag, s), rs in sorted(runs.items()):
            if p != per:
                continue
            d, st = [r["drv"] for r in rs], [r["steady"] for r in rs]
            lu = np.array([x["launch_us"] for x in d])
            print(f"  {tag:7s} {s:8s} {len(rs):4d} | {np.median([x['ms_per_step'] for x in d]) * 1e3:6.2f} {lu.mean():6.2f} / "
                  f"{lu[:, 10:].mean():6.2f}  {np.mean(d[0]['it0_max']):4.2f} {np.mean(d[0]['it0_sum']):4.0f} "
                  f"{np.mean(d[0]['it1_sum']):4.0f} | {np.median([x['ms_per_step'] for x in st]) * 1e3:6.2f} "
                  f"{np.mean([x['launch_us_mean'] for x in st]):6.2f}  {st[0]['it0_max_mean']:4.2f} "
                  f"{st[0]['it1_max_mean']:4.2f} {st[0]['it0_sum_mean']:4.0f} {st[0]['it1_sum_mean']:4.0f} | {d[0]['kernel']}")


if __name__ == "__main__":
    main()

"""Neighbour-cap audit of the benchmark's closed loop (DESIGN.md sections 2 and 5): the config-3
closed loop of bench.py's plain collision workload — the lattice swarm, K = 15, the 8 nearest within
6 m, the benchmark's state noise and seed — through Simulator(audit=True, record=False), every
step's solve audited against the all-others lists of the reference (mpccbf_cap_audit_run).
Writes one JSON file per lattice: the per-step audit summaries, the statuses' counts, the largest
scaled excess of each IMPC iteration, and the steps on which the cap was not exact.

    python tools/cap_audit.py [--agents 4096] [--steps 40] [--knn 8] [--out-dir profiles]
    python tools/cap_audit.py --time [--agents 4096] [--steps 8]     (a short audited loop to
        profile: rocprofv3 --kernel-trace --stats -- python tools/cap_audit.py --time ...)
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))


def nearest(p, chunk=512):
    """Distance of every point to its nearest other point (blockwise all-pairs)."""
    out = np.empty(len(p))
    for i in range(0, len(p), chunk):
        d2 = ((p[i:i + chunk, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(len(d2)), i + np.arange(len(d2))] = np.inf
        out[i:i + chunk] = np.sqrt(d2.min(axis=1))
    return out


def closed_loop(agents, steps, knn, crowded):
    import torch
    from mpccbf import swarm
    from mpccbf.sim import Simulator
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(agents, spacing_scale=0.6 if crowded else 1.0)
    sim = Simulator(cfg, states, targets, knn_k=knn, knn_radius=3.0 * cfg["d_min"], pos_std=0.001, vel_std=0.01,
                    noise_seed=20251015, record=False, audit=True)
    rows = []
    for s in range(steps):
        before = sim.states.cpu().numpy()
        status = sim.step()
        ex = sim.audit_excess.cpu().numpy()
        counts = sim.audit_counts.cpu().numpy()
        row = dict(step=s, **sim.audit_log[-1])
        row["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
        for it in range(2):
            e = ex[:, it]
            row[f"max_scaled_excess{it}"] = None if np.isnan(e).all() else float(np.nanmax(e))
        row["agents_violated0"] = int(np.count_nonzero(counts[:, 1] > 0))
        row["agents_violated1"] = int(np.count_nonzero(counts[:, 3] > 0))
        row["agents_live_dropped"] = int(np.count_nonzero((counts[:, 0] > 0) | (counts[:, 2] > 0)))
        row["agents_inside_d_min"] = int(np.count_nonzero(nearest(before[:, :2]) < cfg["d_min"]))
        rows.append(row)
    torch.cuda.synchronize()
    inexact = [r["step"] for r in rows if r["uncertified"] > 0]
    return dict(workload="collision closed loop" + (" crowded (0.6 x spacing)" if crowded else ""), agents=agents,
                k_hor=15, knn=knn, knn_radius=3.0 * cfg["d_min"], pos_std=0.001, vel_std=0.01, noise_seed=20251015,
                steps=steps, kernel=sim.ctx.kernel_name, steps_with_uncertified_agents=inexact,
                steps_with_violated_rows=[r["step"] for r in rows if r["violated0"] + r["violated1"] > 0],
                max_uncertified_agents=max(r["uncertified"] for r in rows),
                max_scaled_excess=max([r[f"max_scaled_excess{it}"] for r in rows for it in range(2)
                                       if r[f"max_scaled_excess{it}"] is not None], default=None),
                per_step=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--knn", type=int, default=8)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--time", action="store_true", help="a short audited loop only (no files), for a profiler")
    args = ap.parse_args()
    if args.time:
        r = closed_loop(args.agents, min(args.steps, 8), args.knn, False)
        print(json.dumps({k: v for k, v in r.items() if k != "per_step"}))
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for crowded, name in ((False, "cap_audit_config3.json"), (True, "cap_audit_crowded.json")):
        r = closed_loop(args.agents, args.steps, args.knn, crowded)
        with open(os.path.join(args.out_dir, name), "w") as f:
            json.dump(r, f, indent=1)
        print(json.dumps({k: v for k, v in r.items() if k != "per_step"}))


if __name__ == "__main__":
    main()

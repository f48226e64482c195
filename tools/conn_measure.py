"""What the connectivity rows cost (Context.set_connectivity): closed-loop runs of 4,096 agents as
256 teams of 16 and as 1,024 teams of 4 (square lattices of spacing 2.3 moving outwards at up to
0.5 m/s, d_max 4: the teams start well connected), with connectivity attached and, interleaved from the same
initial states, with nothing attached. Per run: the IMPC launch's device time from the launch clock
(kernel_clock: largest wave end minus smallest wave start), the step's device time from events
(step_ms) and the IMPC launch's from events (solve_ms); the spectrum launch is the attached runs'
(step_ms - solve_ms) minus the plain runs' — its kernel plus its dispatch gap. One JSON line per
(layout, mode) goes to profiles/connectivity_measure.jsonl. Needs a GPU (no fallback).

    python tools/conn_measure.py [--steps 300] [--rounds 3] [--out profiles/connectivity_measure.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))

def run(mpccbf, torch, cfg, states, targets, team_ptr, steps, attach, d_max):
    dev = torch.device("cuda", 0)
    ctx = mpccbf.Context(cfg)
    n = len(states)
    l2 = None
    if attach:
        l2 = torch.zeros((len(team_ptr) - 1,), dtype=torch.float64, device=dev)
        ctx.set_connectivity(team_ptr, d_max, lambda2=l2)
    a = torch.tensor(states, device=dev)
    b = torch.empty_like(a)
    tg = torch.tensor(targets, device=dev)
    out = ctx.alloc_outputs(n)
    W = ctx.launch_waves(n)
    clock = torch.zeros((steps, W, 2), dtype=torch.int64, device=dev)
    slog = torch.empty((steps, n, cfg["impc_iter"]), dtype=torch.int32, device=dev)
    kw = dict(targets=tg, knn_k=8, knn_radius=3.0 * cfg["d_min"], x=out["x"], status=out["status"], obj=out["obj"],
              iters=out["iters"])
    # warm-up on tables of its own (code objects, the context's buffers), then the timed run
    ctx.run_steps(a.clone(), b.clone(), 10, **kw)
    torch.cuda.synchronize()
    res = ctx.run_steps(a, b, steps, timing=True, kernel_clock=clock, status_log=slog, **kw)
    torch.cuda.synchronize()
    us = mpccbf._lib.kernel_clock_us(clock.cpu().numpy())
    st = slog.cpu().numpy()
    name = ctx.kernel_name
    return dict(kernel=name, clock_us=us, step_us=1e3 * res["step_ms"], solve_us=1e3 * res["solve_ms"],
                optimal=float(np.mean(st[:, :, 0] == 0)), infeasible=float(np.mean(st == 3)),
                error=float(np.mean(st == 4)), lambda2=None if l2 is None else l2.cpu().numpy(),
                final=res["final"].cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--shape", default="grid")
    ap.add_argument("--spacing", type=float, default=2.3)
    ap.add_argument("--d-max", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "connectivity_measure.jsonl"))
    args = ap.parse_args()
    import torch
    import mpccbf
    from mpccbf import swarm
    if not torch.cuda.is_available():
        sys.exit("conn_measure needs a GPU")
    cfg = swarm.config(15)
    lines = []
    for size in (16, 4):
        teams = args.agents // size
        states, targets, team_ptr = swarm.team_swarm([size] * teams, args.spacing, seed=7, shape=args.shape, speed=(0.0, 0.5),
                                                      target_scale=1.5, gap=12.0 + 2.0 * size)
        acc = {True: [], False: []}
        for _ in range(args.rounds):  # interleaved: attached, plain, attached, ...
            for attach in (True, False):
                acc[attach].append(run(mpccbf, torch, cfg, states, targets, team_ptr, args.steps, attach, args.d_max))
        gap = {}
        for attach in (True, False):
            rs = acc[attach]
            clock = np.concatenate([r["clock_us"] for r in rs])
            step = np.concatenate([r["step_us"] for r in rs])
            solve = np.concatenate([r["solve_us"] for r in rs])
            gap[attach] = float(np.median(step - solve))
            # (the same code on the same inputs: every round ends in the same table)
            same = all(np.array_equal(r["final"], rs[0]["final"]) for r in rs)
            line = dict(agents=args.agents, team_size=size, teams=teams, steps=args.steps, rounds=args.rounds,
                        shape=args.shape, spacing=args.spacing, d_max=args.d_max, attached=attach, kernel=rs[0]["kernel"],
                        impc_launch_clock_us=dict(median=float(np.nanmedian(clock)), p10=float(np.nanpercentile(clock, 10)),
                                                  p90=float(np.nanpercentile(clock, 90))),
                        impc_launch_event_us=float(np.median(solve)), step_event_us=float(np.median(step)),
                        round_medians_clock_us=[float(np.nanmedian(r["clock_us"])) for r in rs],
                        optimal_share_iter0=rs[0]["optimal"], infeasible_share=rs[0]["infeasible"],
                        error_share=rs[0]["error"], rounds_bit_identical=bool(same))
            if attach:
                l2 = rs[0]["lambda2"]
                line["lambda2_last_step"] = dict(min=float(np.nanmin(l2)), median=float(np.nanmedian(l2)),
                                                 max=float(np.nanmax(l2)))
            lines.append(line)
        lines[-2]["spectrum_launch_us"] = gap[True] - gap[False]  # (kernel + dispatch gap, from events)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()

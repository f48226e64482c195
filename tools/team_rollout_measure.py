"""What an MPC-CBF team rollout step costs on the device loop (mpccbf_team_rollout) and on the best
host loop the per-launch API allows: robots in turn-major order (robot i of every team contiguous),
all-others CSR lists, and per robot turn one impc_solve(agent_first = i * teams, num_agents = teams,
next_states = ...) over every team's robot i plus one copy of those rows into the table (the example's
Gauss-Seidel order from the host: per step of 8-robot teams 8 launches and 8 copies, whatever the
number of teams). The host loop is timed twice: with the next
states alone, and writing every turn's sub-step records as well (substeps=...: the samples the
device loop always forms, because its summary scores them).

Teams of 8 robots (the instance 8r/circle2 on the base config, the instance's noise 0.001 / 0.01) at
1, 64, 1,024 and 4,096 teams. First the two loops are compared with the noise off: their final
states must be equal value for value (the same agent body on the same tables). With the noise on
they cannot be: the host loop's draw is keyed by (one seed, step, row in the turn-major table), the
device loop's by (the team's seed, step, robot's index in its team); the timed runs use the noise as
each loop keys it. Both loops start every timed call from the same initial state; a call is `steps`
steps between two device events after one untimed call, `reps` calls each, alternating the two
loops; the figure is the median call's time over its steps. Then the time of one launch of the
default steps_per_launch at every batch size. The profiler is off. One JSON line per case goes to
profiles/team_rollout_measure.jsonl. Needs a GPU (no fallback).

    python tools/team_rollout_measure.py [--steps 16] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

INSTANCE = "8r/circle2"


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


class HostLoop:
    """The turn-major host loop over `teams` copies of one instance."""

    def __init__(self, torch, mpccbf, cfg, states, targets, teams, pos_std, vel_std, seed, substeps=False):
        dev = torch.device("cuda", 0)
        self.torch, self.teams, self.robots = torch, teams, len(states)
        n = teams * self.robots
        self.ctx = mpccbf.Context(cfg)
        tm = lambda a: np.repeat(np.asarray(a, dtype=np.float64), teams, axis=0)  # noqa: E731  (robot-major rows)
        self.st0 = torch.tensor(tm(states), device=dev)
        self.st = self.st0.clone()
        self.tg = torch.tensor(tm(targets), device=dev)
        row = np.arange(n)
        i, t = row // teams, row % teams
        col = np.concatenate([[j * teams + tt for j in range(self.robots) if j != ii] for ii, tt in zip(i, t)])
        self.rp = torch.tensor((np.arange(n + 1) * (self.robots - 1)).astype(np.int32), device=dev)
        self.col = torch.tensor(col.astype(np.int32), device=dev)
        self.out = self.ctx.alloc_outputs(n, device=dev)
        self.traj_t = torch.empty((n,), dtype=torch.float64, device=dev)
        self.nxt = torch.empty((teams, 6), dtype=torch.float64, device=dev)
        self.noise = dict(pos_std=pos_std, vel_std=vel_std, noise_seed=seed)
        nsub = int(cfg["h"] / cfg["Ts"])
        self.sub = torch.empty((teams, nsub, 6), dtype=torch.float64, device=dev) if substeps else None

    def run(self, steps):
        o, T = self.out, self.teams
        self.st.copy_(self.st0)
        o["x"].fill_(float("nan"))
        self.traj_t.fill_(-1.0)
        for s in range(steps):
            for i in range(self.robots):
                sl = slice(i * T, (i + 1) * T)
                self.ctx.impc_solve(self.st, nb_row_ptr=self.rp[i * T:(i + 1) * T + 1], nb_col=self.col,
                                    targets=self.tg[sl], agent_first=i * T, num_agents=T, x=o["x"][sl],
                                    status=o["status"][sl], obj=o["obj"][sl], iters=o["iters"][sl],
                                    next_states=self.nxt, traj_t=self.traj_t[sl], substeps=self.sub, step_index=s,
                                    **self.noise)
                self.st[sl].copy_(self.nxt)

    def team_major(self):
        """The table as the device loop orders it: team by team."""
        return self.st.cpu().numpy().reshape(self.robots, self.teams, 6).transpose(1, 0, 2).reshape(-1, 6)


def device_loop(torch, mpccbf, teams, noise, steps_per_launch=0):
    roll = mpccbf.TeamRollouts.from_instances([INSTANCE], range(1, teams + 1), record=False,
                                              steps_per_launch=steps_per_launch)
    if not noise:
        roll.pos_std = roll.vel_std = 0.0
    st0 = roll.states.clone()

    def run(steps):
        roll.states.copy_(st0)
        roll.x_keep.fill_(float("nan"))
        roll.traj_t.fill_(-1.0)
        roll.steps = 0
        roll.run(steps)

    return roll, run


def case(torch, mpccbf, teams, steps, reps):
    import parity_rule as PR
    from mpccbf import instances
    cfg, states, targets, shape, kind, noise = instances.instance(INSTANCE)
    out = dict(instance=INSTANCE, teams=teams, robots_per_team=len(states), steps_per_call=steps, reps=reps,
               steps_per_launch=mpccbf._lib.TEAM_STEPS_PER_LAUNCH)
    # the two loops agree (noise off: the draws are keyed differently)
    check_steps = min(steps, 6)
    roll, run = device_loop(torch, mpccbf, teams, noise=False)
    host = HostLoop(torch, mpccbf, cfg, states, targets, teams, 0.0, 0.0, 1)
    run(check_steps)
    host.run(check_steps)
    torch.cuda.synchronize()
    PR.same_values(roll.states.cpu().numpy(), host.team_major(), what=f"{teams} teams: device loop vs host loop")
    out["loops_agree_without_noise"] = dict(steps=check_steps, rule="same_values")
    out["host_loop_kernel"] = host.ctx.kernel_name
    # the timed runs, with the instance's noise
    roll, run = device_loop(torch, mpccbf, teams, noise=True)
    host = HostLoop(torch, mpccbf, cfg, states, targets, teams, noise["pos_std"], noise["vel_std"], 1)
    host_sub = HostLoop(torch, mpccbf, cfg, states, targets, teams, noise["pos_std"], noise["vel_std"], 1,
                        substeps=True)
    run(steps)
    host.run(steps)  # untimed: code objects, allocations
    host_sub.run(steps)
    torch.cuda.synchronize()
    dev_ms, host_ms, host_sub_ms = [], [], []
    for _ in range(reps):  # alternating: all see the same machine
        dev_ms.append(_timed(torch, lambda: run(steps)))
        host_ms.append(_timed(torch, lambda: host.run(steps)))
        host_sub_ms.append(_timed(torch, lambda: host_sub.run(steps)))
    out["device_loop_ms_per_step"] = float(np.median(dev_ms)) / steps
    out["device_loop_ms_per_step_all"] = [m / steps for m in dev_ms]
    out["host_loop_ms_per_step"] = float(np.median(host_ms)) / steps
    out["host_loop_ms_per_step_all"] = [m / steps for m in host_ms]
    out["host_over_device"] = out["host_loop_ms_per_step"] / out["device_loop_ms_per_step"]
    out["host_loop_substeps_ms_per_step"] = float(np.median(host_sub_ms)) / steps
    out["host_loop_substeps_ms_per_step_all"] = [m / steps for m in host_sub_ms]
    out["host_substeps_over_device"] = out["host_loop_substeps_ms_per_step"] / out["device_loop_ms_per_step"]
    # one launch of the default steps_per_launch
    per = mpccbf._lib.TEAM_STEPS_PER_LAUNCH
    one = [_timed(torch, lambda: run(per)) for _ in range(reps)]
    out["one_launch_ms"] = float(np.median(one))
    out["one_launch_ms_all"] = one
    # the whole call in one launch: what the split costs
    roll1, run1 = device_loop(torch, mpccbf, teams, noise=True, steps_per_launch=steps)
    run1(steps)
    torch.cuda.synchronize()
    whole = [_timed(torch, lambda: run1(steps)) for _ in range(reps)]
    out["single_launch_ms_per_step"] = float(np.median(whole)) / steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--teams", type=int, nargs="*", default=[1, 64, 1024, 4096])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "team_rollout_measure.jsonl"))
    args = ap.parse_args()
    import torch
    import mpccbf
    if not torch.cuda.is_available():
        sys.exit("team_rollout_measure needs a GPU")
    lines = []
    for teams in args.teams:
        lines.append(case(torch, mpccbf, teams, args.steps, args.reps))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

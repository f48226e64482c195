"""Batched formation-control rollouts on the device (mpccbf_formation_rollout in include/mpccbf.h):
the closed loop of the reference's CBFFormationControl_example.cpp for many independent teams in
one launch, robots in the example's order, with the example's record and a per-team safety summary
scored as mpccbf.metrics scores a trace.

FormationRollouts owns the device tensors; results_from_summary turns host copies of the summary
into the answers of metrics.instance_success (a pure function: no GPU, no library).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib, instances

TEAM_MAX = 16          # robots per team (CC_MAX, conn_spectrum.hpp)
SPRING_CONSTANT = 0.5  # CBFFormationControl_example.cpp:152
GOAL_RADIUS = 1.0      # collision_check.py's default


def results_from_summary(team_ptr, arrival_sample, first_collision, min_d2, fail_count, samples: int) -> list:
    """Per team: instance_success, makespan, first_collision, min_pair_distance_m, fail_count from
    host copies of the summary after `samples` samples (numbered from 0).

    The first three are the return values of metrics.instance_success on the same samples. The
    script walks the samples and stops at the first one before which every robot has reached its
    goal area: with R the last robot's arrival sample, a collision in a sample <= R fails the run
    ((False, inf, (sample, i, j))), a later one does not; a clean walk returns (True, R, None) when a
    sample follows R and (True, samples, None) otherwise (R is the last sample, or some robot never
    arrives)."""
    team_ptr = np.asarray(team_ptr, dtype=np.int64)
    arrival_sample = np.asarray(arrival_sample, dtype=np.int64)
    first_collision = np.asarray(first_collision, dtype=np.int64).reshape(-1, 3)
    out = []
    for t in range(len(team_ptr) - 1):
        ra = arrival_sample[team_ptr[t]:team_ptr[t + 1]]
        all_reached = bool(np.all(ra >= 0))
        last_arrival = int(ra.max()) if (all_reached and ra.size) else -1  # (no robots: reached before sample 0)
        first = tuple(int(v) for v in first_collision[t]) if first_collision[t, 0] >= 0 else None
        if first is not None and (not all_reached or first[0] <= last_arrival):
            ok, makespan, collision = False, float("inf"), first
        elif all_reached and last_arrival + 1 < samples:
            ok, makespan, collision = True, max(0, last_arrival), None
        else:
            ok, makespan, collision = True, samples, None
        out.append({"instance_success": ok, "makespan": makespan, "first_collision": collision,
                    "min_pair_distance_m": math.sqrt(float(min_d2[t])), "fail_count": int(fail_count[t])})
    return out


def control_cfg(cfg: dict, slack=None) -> dict:
    """The connectivity controller's keys of an instance config (instances.from_json; d_max from the
    instance JSON's cbf_params). slack: None keeps the instance's slack_mode, else overrides it."""
    c = {k: cfg[k] for k in ("d_min", "d_max", "v_min", "v_max", "slack_cost", "slack_decay_rate", "Ts")}
    c["control_slack_mode"] = int(cfg["slack_mode"] if slack is None else bool(slack))
    return c


def instance_groups(names, preprocess="base", slack=None) -> list:
    """The baseline instances `names` grouped by what one launch holds fixed — the controller's
    parameters (control_cfg), the noise and the collision box — in order of first appearance: dicts
    of cfg, names, teams = [(name, states, targets)], pos_std, vel_std, shape_half. No GPU."""
    fx = instances.load_fixture()
    base = preprocess in (True, "base")
    groups = {}
    for name in names:
        cfg, states, targets, shape, kind, noise = instances.instance(name, preprocess=preprocess)
        ins = fx["instances"][name]
        js = instances.overlay(fx["base_config"], ins) if base else instances.own_params(fx["base_config"], ins)
        if kind != "box":
            raise ValueError(f"{name}: the rollout scores the script's box test; the instance has no aligned_box")
        c = control_cfg(dict(cfg, d_max=float(js["cbf_params"]["d_max"])), slack)
        key = repr((sorted(c.items()), shape, sorted(noise.items())))
        g = groups.setdefault(key, dict(cfg=c, names=[], teams=[], pos_std=noise["pos_std"], vel_std=noise["vel_std"],
                                        shape_half=tuple(shape[:2])))
        g["names"].append(name)
        g["teams"].append((name, states, targets))
    return list(groups.values())


def _seed_bits(seeds) -> np.ndarray:
    """uint64 seeds as the int64 array that carries their bits to the device."""
    return np.array([int(s) & ((1 << 64) - 1) for s in np.asarray(seeds, dtype=object).reshape(-1)],
                    dtype=np.uint64).view(np.int64)


class FormationRollouts:
    """A batch of independent teams and the device tensors of their rollouts.

    cfg: d_min, d_max, v_min, v_max, control_slack_mode, slack_cost, slack_decay_rate (the keys of
    connectivity_control_solve) and Ts. team_ptr: teams + 1 offsets into the robot rows (teams of 1
    to 16 robots; checked here, on the host). states (robots x 6) / targets (robots x 3): host
    arrays. seeds: one integer per team, the noise key. record: keep the example's record (trace,
    desired_u, cbf_u, status, lambda2, iters) of every decision, one set of tensors per run(). The
    summary is always kept."""

    def __init__(self, cfg: dict, team_ptr, states, targets, seeds=None, pos_std: float = 0.0,
                 vel_std: float = 0.0, record: bool = True, shape_half=(0.2, 0.2), goal_radius: float = GOAL_RADIUS,
                 spring_constant: float = SPRING_CONSTANT, steps_per_launch: int = 0, device: int = 0):
        import torch
        team_ptr = np.ascontiguousarray(team_ptr, dtype=np.int32)
        states = np.ascontiguousarray(states, dtype=np.float64)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if team_ptr.ndim != 1 or len(team_ptr) < 1 or team_ptr[0] != 0:
            raise ValueError("team_ptr: offsets starting at 0")
        sizes = np.diff(team_ptr)
        if np.any(sizes < 1) or np.any(sizes > TEAM_MAX):
            bad = int(np.nonzero((sizes < 1) | (sizes > TEAM_MAX))[0][0])
            raise ValueError(f"team {bad} has {int(sizes[bad])} robots: teams of 1 .. {TEAM_MAX}")
        n = int(team_ptr[-1])
        if states.shape != (n, 6) or targets.shape != (n, 3):
            raise ValueError(f"states must be ({n}, 6) and targets ({n}, 3)")
        self.num_teams = len(team_ptr) - 1
        seeds = np.zeros(self.num_teams, dtype=np.int64) if seeds is None else _seed_bits(seeds)
        if len(seeds) != self.num_teams:
            raise ValueError("seeds: one per team")
        self.cfg = dict(cfg)
        self.Ts = float(cfg["Ts"])
        self.pos_std, self.vel_std = float(pos_std), float(vel_std)
        self.shape_half = (float(shape_half[0]), float(shape_half[1]))
        self.goal_radius = float(goal_radius)
        self.spring_constant = float(spring_constant)
        self.steps_per_launch = int(steps_per_launch)
        self.record = bool(record)
        self.device = int(device)
        self.team_ptr_host = team_ptr
        self.num_robots = n
        self.steps = 0  # steps run so far = samples scored
        dev = torch.device("cuda", self.device)
        self._dev = dev
        self.team_ptr = torch.tensor(team_ptr, device=dev)
        self.states = torch.tensor(states, device=dev)
        self.targets = torch.tensor(targets, device=dev)
        self.seeds = torch.tensor(seeds, device=dev)
        self.arrival_sample = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.first_collision = torch.full((self.num_teams, 3), -1, dtype=torch.int32, device=dev)
        self.min_d2 = torch.full((self.num_teams,), float("inf"), dtype=torch.float64, device=dev)
        self.fail_count = torch.zeros(self.num_teams, dtype=torch.int32, device=dev)
        self._rec = []  # per run(): dict of record tensors [steps][robots][.]

    def run(self, steps: int, stream=None):
        """Advance every team by `steps` steps (asynchronous: the launches are enqueued)."""
        import torch
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps < 0")
        rec = {}
        if self.record and steps > 0:
            n, dev = self.num_robots, self._dev
            rec = dict(trace=torch.empty((steps, n, 6), dtype=torch.float64, device=dev),
                       cbf_u=torch.empty((steps, n, 3), dtype=torch.float64, device=dev),
                       desired_u=torch.empty((steps, n, 3), dtype=torch.float64, device=dev),
                       status=torch.empty((steps, n), dtype=torch.int32, device=dev),
                       lambda2=torch.empty((steps, n), dtype=torch.float64, device=dev),
                       iters=torch.empty((steps, n), dtype=torch.int32, device=dev))
        _lib.formation_rollout(self.cfg, self.team_ptr, self.states, self.targets, self.seeds, steps, self.steps,
                               Ts=self.Ts, spring_constant=self.spring_constant, pos_std=self.pos_std,
                               vel_std=self.vel_std, shape_half=self.shape_half, goal_radius=self.goal_radius,
                               steps_per_launch=self.steps_per_launch, arrival_sample=self.arrival_sample,
                               first_collision=self.first_collision, min_d2=self.min_d2,
                               fail_count=self.fail_count, device=self.device, stream=stream, **rec)
        if rec:
            self._rec.append(rec)
        self.steps += steps
        return self

    def records(self) -> dict:
        """The record of every step run so far as host arrays [steps][robots][.] (record=True)."""
        if not self.record:
            raise _lib.MpccbfError("FormationRollouts(record=False) keeps no record")
        widths = dict(trace=(6,), cbf_u=(3,), desired_u=(3,), status=(), lambda2=(), iters=())
        out = {}
        for k, w in widths.items():
            parts = [r[k].cpu().numpy() for r in self._rec]
            dt = np.int32 if k in ("status", "iters") else np.float64
            out[k] = np.concatenate(parts) if parts else np.zeros((0, self.num_robots) + w, dtype=dt)
        return out

    def results(self) -> list:
        """Per team: instance_success, makespan, first_collision, min_pair_distance_m, fail_count
        (results_from_summary on the device summary)."""
        return results_from_summary(self.team_ptr_host, self.arrival_sample.cpu().numpy(),
                                    self.first_collision.cpu().numpy(), self.min_d2.cpu().numpy(),
                                    self.fail_count.cpu().numpy(), self.steps)

    def to_json(self, team: int, records=None) -> dict:
        """The example's states.json of one team (CBFFormationControl_example.cpp:117-121, 180-183):
        dt, Ts and per robot the states, desired_u and cbf_u of every step. records: a records()
        result to reuse."""
        rec = self.records() if records is None else records
        r0, r1 = int(self.team_ptr_host[team]), int(self.team_ptr_host[team + 1])
        robots = {}
        for i in range(r1 - r0):
            robots[str(i)] = {"states": rec["trace"][:, r0 + i].tolist(),
                              "desired_u": rec["desired_u"][:, r0 + i].tolist(),
                              "cbf_u": rec["cbf_u"][:, r0 + i].tolist()}
        return {"dt": self.Ts, "Ts": self.Ts, "robots": robots}

    @classmethod
    def from_instances(cls, names, seeds, preprocess="base", slack=None, **kw):
        """names x seeds batches of the baseline instances (mpccbf/data/reference_instances.json), one
        object per parameter set (instance_groups: one launch takes one parameter set), as a list
        of (object, [names of its group]) in order of first appearance; preprocess="base" (the
        reference's run semantics: every instance on the base config) is uniform and gives a list of
        one. In an object, team t = instance group_names[t // len(seeds)] with noise key
        seeds[t % len(seeds)], the group's pos_std / vel_std and collision box. slack: None = the
        configuration's slack_mode, else overrides it."""
        seeds = list(seeds)
        out = []
        for g in instance_groups(names, preprocess, slack):
            sizes = [len(st) for _, st, _ in g["teams"] for _ in seeds]
            team_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            obj = cls(g["cfg"], team_ptr, np.concatenate([st for _, st, _ in g["teams"] for _ in seeds]),
                      np.concatenate([tg for _, _, tg in g["teams"] for _ in seeds]), seeds=seeds * len(g["teams"]),
                      pos_std=g["pos_std"], vel_std=g["vel_std"], shape_half=g["shape_half"], **kw)
            out.append((obj, list(g["names"])))
        return out

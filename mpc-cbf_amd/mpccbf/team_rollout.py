"""Batched MPC-CBF team rollouts on the device (mpccbf_team_rollout in include/mpccbf.h): the closed
loop of the reference's MPCCBFFormationControl_example.cpp for many independent teams, robots in the
example's order (Gauss-Seidel), every other robot of the team a neighbour, with the example's record
and a per-team safety summary scored as mpccbf.metrics scores a trace.

A team run alone with seed s is, bit for bit, Simulator(order="gauss_seidel", neighbours="all",
noise_seed=s): TeamRollouts runs thousands of them in one launch sequence. TeamRollouts owns the
context and the device tensors.
"""
from __future__ import annotations

import numpy as np

from . import _lib, instances
from .formation import GOAL_RADIUS, _seed_bits, results_from_summary
from .sim import bezier_positions

TEAM_MAX = 16  # robots per team (TEAM_MAX, team_rollout.hpp)

_RECORDS = dict(status=("int32", "iter"), obj=("float64", "iter"), iters=("int32", "iter"), x=("float64", "n"),
                traj_t0=("float64", None), substeps=("float64", "sub"), trace=("float64", 6))


def check_config(cfg: dict):
    """What the rollout does not run, told on the host before a context exists."""
    if cfg.get("cbf_mode", 0) == 1:
        raise ValueError("TeamRollouts: the FoV controller (cbf_mode 1) is not supported")
    if cfg.get("slack_mode", 0):
        raise ValueError("TeamRollouts: slack mode is not supported")


class TeamRollouts:
    """A batch of independent teams and the device tensors of their MPC-CBF rollouts.

    cfg: a Context configuration (collision controller, no slack mode). team_ptr: teams + 1 offsets
    into the robot rows (teams of 1 to 16 robots; checked here, on the host). states (robots x 6) /
    targets (robots x 3): host arrays. seeds: one integer per team, the noise key. record: keep the
    record of every decision (status, obj, iters, x, traj_t0, substeps, trace), one set of tensors
    per run(); a tuple of those names keeps just those. The summary is always kept."""

    def __init__(self, cfg: dict, team_ptr, states, targets, seeds=None, pos_std: float = 0.0,
                 vel_std: float = 0.0, record=True, shape_half=(0.2, 0.2), goal_radius: float = GOAL_RADIUS,
                 steps_per_launch: int = 0, device: int = 0):
        check_config(cfg)
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
        if record is True:
            record = tuple(_RECORDS)
        elif not record:
            record = ()
        unknown = [k for k in record if k not in _RECORDS]
        if unknown:
            raise ValueError(f"record: unknown {unknown}; one of {list(_RECORDS)}")
        import torch
        self.cfg = dict(cfg)
        self.pos_std, self.vel_std = float(pos_std), float(vel_std)
        self.shape_half = (float(shape_half[0]), float(shape_half[1]))
        self.goal_radius = float(goal_radius)
        self.steps_per_launch = int(steps_per_launch)
        self.record = tuple(record)
        self.device = int(device)
        self.team_ptr_host = team_ptr
        self.states0 = states.copy()
        self.targets_host = targets
        self.num_robots = n
        self.nsub = int(cfg["h"] / cfg["Ts"])
        self.steps = 0  # steps run so far; samples scored = steps * nsub
        self.ctx = _lib.Context(cfg, device=device)
        dev = torch.device("cuda", self.device)
        self._dev = dev
        self.team_ptr = torch.tensor(team_ptr, device=dev)
        self.states = torch.tensor(states, device=dev)
        self.targets = torch.tensor(targets, device=dev)
        self.seeds = torch.tensor(seeds, device=dev)
        self.x_keep = torch.full((n, self.ctx.n), float("nan"), dtype=torch.float64, device=dev)
        self.traj_t = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        self.arrival_sample = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.first_collision = torch.full((self.num_teams, 3), -1, dtype=torch.int32, device=dev)
        self.min_d2 = torch.full((self.num_teams,), float("inf"), dtype=torch.float64, device=dev)
        self.fail_count = torch.zeros(self.num_teams, dtype=torch.int32, device=dev)
        self._rec = []  # per run(): dict of record tensors [steps][robots][.]

    def _record_shape(self, key, steps):
        dtype, w = _RECORDS[key]
        width = {"iter": (self.ctx.impc_iter,), "n": (self.ctx.n,), "sub": (self.nsub, 6), None: ()}.get(w, (w,))
        return dtype, (steps, self.num_robots) + width

    def run(self, steps: int, stream=None):
        """Advance every team by `steps` steps (asynchronous: the launches are enqueued)."""
        import torch
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps < 0")
        rec = {}
        if steps > 0:
            for k in self.record:
                dtype, shape = self._record_shape(k, steps)
                rec[k] = torch.empty(shape, dtype=getattr(torch, dtype), device=self._dev)
        _lib.team_rollout(self.ctx, self.team_ptr, self.states, self.targets, self.seeds, self.x_keep, self.traj_t,
                          steps, self.steps, pos_std=self.pos_std, vel_std=self.vel_std, shape_half=self.shape_half,
                          goal_radius=self.goal_radius, steps_per_launch=self.steps_per_launch,
                          arrival_sample=self.arrival_sample, first_collision=self.first_collision,
                          min_d2=self.min_d2, fail_count=self.fail_count, stream=stream, **rec)
        if rec:
            self._rec.append(rec)
        self.steps += steps
        return self

    def records(self) -> dict:
        """The kept records of every step run so far as host arrays [steps][robots][.]."""
        if not self.record:
            raise _lib.MpccbfError("TeamRollouts(record=False) keeps no record")
        out = {}
        for k in self.record:
            parts = [r[k].cpu().numpy() for r in self._rec]
            dtype, shape = self._record_shape(k, 0)
            out[k] = np.concatenate(parts) if parts else np.zeros(shape, dtype=dtype)
        return out

    def results(self) -> list:
        """Per team: instance_success, makespan, first_collision, min_pair_distance_m, fail_count
        (formation.results_from_summary on the device summary; the samples are the sub-steps)."""
        return results_from_summary(self.team_ptr_host, self.arrival_sample.cpu().numpy(),
                                    self.first_collision.cpu().numpy(), self.min_d2.cpu().numpy(),
                                    self.fail_count.cpu().numpy(), self.steps * self.nsub)

    def to_json(self, team: int, records=None) -> dict:
        """The example's states.json of one team (MPCCBFFormationControl_example.cpp:127-129, 166-205,
        229-231), built as Simulator._record builds it: per robot the predicted curve of every step
        (the kept curve from the time the decision left it at, or the position the step started from
        when there is none) and the state after every control sub-step. Needs the full record.
        records: a records() result to reuse."""
        rec = self.records() if records is None else records
        missing = [k for k in ("status", "x", "traj_t0", "substeps", "trace") if k not in rec]
        if missing:
            raise _lib.MpccbfError(f"to_json needs the records {missing}")
        cfg = self.cfg
        horizon = cfg["num_pieces"] * cfg["piece_max_parameter"]
        r0, r1 = int(self.team_ptr_host[team]), int(self.team_ptr_host[team + 1])
        robots = {}
        for i in range(r1 - r0):
            r = r0 + i
            pred, states = [], []
            for s in range(len(rec["trace"])):
                status, t_before = rec["status"][s, r], rec["traj_t0"][s, r]
                new = bool(np.any(status == 0))
                if new or t_before >= 0.0:
                    t0 = 0.0 if new else t_before
                    ts, t = [], 0.0
                    while t <= horizon:  # the example's accumulation (:172-181)
                        ts.append(min(t0 + t, horizon))
                        t += 0.05
                    pred.append([bezier_positions(cfg, rec["x"][s, r], ts).tolist()])
                else:
                    cur = self.states0[r] if s == 0 else rec["trace"][s - 1, r]
                    pred.append([[cur[:3].tolist()]])
                states.extend(rec["substeps"][s, r].tolist())
            robots[str(i)] = {"pred_curve": pred, "states": states}
        return {"dt": cfg["h"], "Ts": cfg["Ts"], "robots": robots}

    @classmethod
    def from_instances(cls, names, seeds, preprocess="base", **kw):
        """names x seeds teams of the baseline instances (mpccbf/data/reference_instances.json) in one
        object: team t = instance names[t // len(seeds)] with noise key seeds[t % len(seeds)], every
        other robot a neighbour, zero start velocity, the instances' noise and collision box.
        preprocess="base" (the reference's run semantics: every instance on the base config) gives
        one parameter set; instances that differ in their parameters, noise or box are refused (one
        context holds one parameter set)."""
        names, seeds = list(names), list(seeds)
        cfg0 = noise0 = shape0 = None
        teams = []
        for name in names:
            cfg, states, targets, shape, kind, noise = instances.instance(name, preprocess=preprocess)
            if kind != "box":
                raise ValueError(f"{name}: the rollout scores the script's box test; the instance has no aligned_box")
            if cfg0 is None:
                cfg0, noise0, shape0 = cfg, noise, shape
            elif (cfg, noise, shape) != (cfg0, noise0, shape0):
                raise ValueError(f"{name}: parameters differ from {names[0]}'s (one parameter set per object)")
            teams.append((states, targets))
        if cfg0 is None:
            raise ValueError("from_instances: no instance named")
        sizes = [len(st) for st, _ in teams for _ in seeds]
        team_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        obj = cls(cfg0, team_ptr, np.concatenate([st for st, _ in teams for _ in seeds]),
                  np.concatenate([tg for _, tg in teams for _ in seeds]), seeds=seeds * len(teams),
                  pos_std=noise0["pos_std"], vel_std=noise0["vel_std"], shape_half=tuple(shape0[:2]), **kw)
        obj.names = [name for name in names for _ in seeds]
        return obj

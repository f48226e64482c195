"""The closed loop of mpc_cbf/examples/fov/BezierIMPCCBFPFXYYaw_example.cpp:192-296 with the
estimator switched on: every robot tracks its neighbours with a particle filter (FovEstimator) and
plans with the FoV IMPC from its own estimates (Context.set_fov_estimator), where the example plans
from a fixed estimate and a covariance of 0.1 I (:198-203). Per control step, in order: the filter
step against the current states, the FoV IMPC on the estimates (slack mode, the example's setting,
by default), then the trajectory fallback and the int(h / Ts) integration sub-steps with state
noise that traj_t implements (:228-282). Jacobi order, as the example itself is (it plans every
robot from the states of the step's start, :285-293)."""
from __future__ import annotations

import json

import numpy as np

from . import _lib, swarm
from .estimator import FovEstimator
from .sim import bezier_positions

EXAMPLE_SLACK = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.9)  # (:138-142)


class FovImpcLoop:
    """states / targets: (n, 6) / (n, 3) host arrays. cfg: a FoV controller configuration
    (cbf_mode 1; swarm.fov_config) plus the optional pf_* keys of pf_params; unless it sets
    slack_mode itself the example's slack setting is switched on. neighbours: "visible" (the robots
    each robot observes at the start: inside its field of view and range, swarm.fov_csr), "all"
    (every other robot, the example's lists, for teams that start in view of each other) or
    (row_ptr, col); the lists are fixed over the run — each entry is one filter — and hold at most 8
    neighbours in slack mode, 16 without. seed: the filters'; pos_std / vel_std / noise_seed: the
    state noise of the sub-steps (math::addRandomNoise)."""

    def __init__(self, cfg: dict, states, targets, *, neighbours="visible", seed: int = 0, pos_std: float = 0.0,
                 vel_std: float = 0.0, noise_seed: int = 0, device: int = 0, record: bool = True):
        import torch
        self.cfg = dict(cfg)
        if self.cfg.get("cbf_mode", 0) != 1:
            raise _lib.MpccbfError("FovImpcLoop needs the FoV controller (cbf_mode 1)")
        if "slack_mode" not in cfg:
            self.cfg.update(EXAMPLE_SLACK)
        n = len(states)
        cap = 8 if self.cfg.get("slack_mode") else 16
        if isinstance(neighbours, str):
            if neighbours not in ("visible", "all"):
                raise ValueError("neighbours must be 'visible', 'all' or (row_ptr, col)")
            rp, col = (swarm.all_csr(n) if neighbours == "all" else
                       swarm.fov_csr(np.asarray(states, dtype=np.float64), cap, self.cfg["fov_Rs"], self.cfg["fov_beta"]))
        else:
            rp, col = (np.asarray(v, dtype=np.int32).reshape(-1) for v in neighbours)
        if len(rp) != n + 1 or np.any(np.diff(rp) > cap):
            raise _lib.MpccbfError(f"FovImpcLoop takes one list per robot of at most {cap} neighbours")
        self._init_record(n, rp, col, record)
        self.device = int(device)
        dev = torch.device("cuda", self.device)
        self.ctx = _lib.Context(self.cfg, device=device)
        self.states = torch.tensor(np.asarray(states, dtype=np.float64), device=dev)
        self.next = torch.empty_like(self.states)
        self.targets = torch.tensor(np.asarray(targets, dtype=np.float64), device=dev)
        self.traj_t = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        self.out = self.ctx.alloc_outputs(n, device=dev)
        self.out["x"].fill_(float("nan"))
        self.nsub = int(self.cfg["h"] / self.cfg["Ts"])
        self.substeps = torch.empty((n, self.nsub, 6), dtype=torch.float64, device=dev)
        self.estimator = FovEstimator(self.cfg, rp, col, n, device=device, seed=seed)
        self.estimator.init(self.states)
        self.ctx.set_fov_estimator(self.estimator)
        self.noise = dict(pos_std=float(pos_std), vel_std=float(vel_std), noise_seed=int(noise_seed))
        self.step_index = 0
        self.status_log = []

    def _init_record(self, n, rp, col, record=True):
        self.n, self.rp, self.col, self.record = int(n), np.asarray(rp), np.asarray(col), record
        self.log = {str(i): {"states": [], "pred_curve": [],
                             "estimates_mean": {str(j): [] for j in self.col[self.rp[i]:self.rp[i + 1]]},
                             "estimates_cov": {str(j): [] for j in self.col[self.rp[i]:self.rp[i + 1]]}}
                    for i in range(self.n)}

    def step(self):
        """One control step of every robot; returns its QP statuses (n x impc_iter)."""
        import torch
        o, est = self.out, self.estimator
        t_before = self.traj_t.cpu().numpy() if self.record else None
        est.step(self.states)
        self.ctx.impc_solve(self.states, nb_row_ptr=est.nb_row_ptr, nb_col=est.nb_col, targets=self.targets,
                            x=o["x"], status=o["status"], obj=o["obj"], iters=o["iters"], next_states=self.next,
                            traj_t=self.traj_t, substeps=self.substeps, step_index=self.step_index, **self.noise)
        torch.cuda.synchronize()
        status = o["status"].cpu().numpy()
        self.status_log.append(status.copy())
        if self.record:
            self._record(t_before, status, o["x"].cpu().numpy(), self.substeps.cpu().numpy(),
                         self.states.cpu().numpy(), est.est_xy.cpu().numpy(), est.est_cov.cpu().numpy())
        self.states, self.next = self.next, self.states
        self.step_index += 1
        return status

    def _record(self, t_before, status, x, sub, cur, est_xy, est_cov):
        """One step's entries of the example's record (:204-213, 246-258, 279-280), host arrays in."""
        cfg = self.cfg
        horizon = cfg["num_pieces"] * cfg["piece_max_parameter"]
        for i in range(self.n):
            r = self.log[str(i)]
            for e in range(self.rp[i], self.rp[i + 1]):
                j = str(self.col[e])
                cxx, cxy, cyy = (float(v) for v in est_cov[e])
                r["estimates_mean"][j].append([float(est_xy[e, 0]), float(est_xy[e, 1]), 0.0])
                r["estimates_cov"][j].append([cxx, cxy, 0.0, cxy, cyy, 0.0, 0.0, 0.0, 0.0])
            new = bool(np.any(status[i] == _lib.OPTIMAL))
            if new or t_before[i] >= 0.0:
                t0 = 0.0 if new else float(t_before[i])
                ts, t = [], 0.0
                while t <= horizon:  # the example's accumulation (:247-258)
                    ts.append(min(t0 + t, horizon))
                    t += 0.05
                r["pred_curve"].append([bezier_positions(cfg, x[i], ts).tolist()])
            else:  # (no curve yet: the example would dereference none; the held position)
                r["pred_curve"].append([[cur[i, :3].tolist()]])
            r["states"].extend(np.asarray(sub[i]).tolist())

    def run(self, steps: int):
        for _ in range(int(steps)):
            self.step()
        return self.states

    def to_json(self) -> dict:
        """The example's record (:101-104, 204-213, 255, 279): dt, Ts and per robot states,
        pred_curve, estimates_mean and estimates_cov keyed by the neighbour's id."""
        return {"dt": self.cfg["h"], "Ts": self.cfg["Ts"], "robots": self.log}

    def write_json(self, path: str):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=4)

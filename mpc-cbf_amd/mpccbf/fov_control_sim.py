"""The closed loop of cbf/examples/fov/CBFControl_example.cpp:171-279 with the estimator switched on:
every robot tracks every other robot with a particle filter (FovEstimator), steers at its target with
a critically damped spring and filters that input through the batched FovControl QP in slack mode.
Jacobi order, as the example itself is (it plans every robot from the states of the step's start)."""
from __future__ import annotations

import json
import math

import numpy as np

from . import _lib, swarm
from .estimator import FovEstimator


def closest_point_on_ellipse(robot_xy, mean, cov3):
    """math::closestPointOnEllipse (Geometry.cpp:7-57) for a finite covariance (cxx, cxy, cyy): the
    point of the 90 % ellipse (s = 4.605) on the ray from the estimate towards the robot. Host-side."""
    if math.isinf(cov3[0]):
        return 0.0, 0.0
    vals, vecs = np.linalg.eigh(np.array([[cov3[0], cov3[1]], [cov3[1], cov3[2]]]))  # ascending
    a, b = math.sqrt(4.605 * max(vals[1], 0.0)), math.sqrt(4.605 * max(vals[0], 0.0))
    theta = math.atan2(vecs[1, 1], vecs[0, 1])  # the major axis (its sign does not matter below)
    if theta < 0.0:
        theta += math.pi
    slope = math.atan2(robot_xy[1] - mean[1], robot_xy[0] - mean[0])
    c, s = math.cos(slope - theta), math.sin(slope - theta)
    return (mean[0] + a * c * math.cos(theta) - b * s * math.sin(theta),
            mean[1] + a * c * math.sin(theta) + b * s * math.cos(theta))


class FovControlLoop:
    """states / targets: (n, 6) / (n, 3) host arrays, n <= 17 (the slack-mode QP holds 16 observed
    neighbours). cfg: the FoV controller's keys (fov_beta, fov_Ds, fov_Rs, v_min / v_max, a_min /
    a_max, h = the step, as the example's Ts) plus the optional pf_* keys; slack mode is forced on
    with the example's slack_cost 1000 and slack_decay_rate 0.1 unless the cfg sets them under
    control_slack_mode. pos_std / vel_std: optional Gaussian state noise (math::addRandomNoise)."""

    def __init__(self, cfg: dict, states, targets, device: int = 0, seed: int = 0, pos_std: float = 0.0,
                 vel_std: float = 0.0, noise_seed: int = 0, record: bool = True):
        import torch
        n = len(states)
        if n < 2 or n > 17:
            raise _lib.MpccbfError("FovControlLoop takes 2 .. 17 robots")
        self.cfg = dict(cfg)
        if not self.cfg.get("control_slack_mode"):
            self.cfg.update(control_slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.1)
        self.n, self.Ts, self.device = n, float(cfg["h"]), int(device)
        dev = torch.device("cuda", self.device)
        st = np.array(states, dtype=np.float64)
        st[:, 2] = [self._yaw_in_range_host(y) for y in st[:, 2]]  # example :133
        self.states = torch.tensor(st, dtype=torch.float64, device=dev)
        self.targets = torch.tensor(np.asarray(targets, dtype=np.float64), device=dev)
        rp, col = swarm.all_csr(n)  # every other robot is a neighbour (:146-168)
        self.rp, self.col = rp, col
        self.estimator = FovEstimator(self.cfg, rp, col, n, device=device, seed=seed)
        self.estimator.init(self.states)
        self.u = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.desired_u = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.pos_std, self.vel_std = float(pos_std), float(vel_std)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(int(noise_seed))
        self.steps_done = 0
        self.record = record
        self.log = {str(i): {"states": [], "estimates_mean": {str(j): [] for j in col[rp[i]:rp[i + 1]]},
                             "estimates_cov": {str(j): [] for j in col[rp[i]:rp[i + 1]]},
                             "p_near_ellipse": {str(j): [] for j in col[rp[i]:rp[i + 1]]}} for i in range(n)}

    @staticmethod
    def _yaw_in_range_host(yaw):
        return yaw - 2 * math.pi if yaw > math.pi else (yaw + 2 * math.pi if yaw < -math.pi else yaw)

    def step(self):
        """One control step of every robot; returns the new states (device, n x 6)."""
        import torch
        s, Ts = self.states, self.Ts
        est_xy, est_cov = self.estimator.step(s)
        # convertToClosestYaw (Geometry.h:76-104): the goal yaw among g, g + 2 pi, g - 2 pi closest
        # to the current yaw (the first on ties)
        g, yaw = self.targets[:, 2], s[:, 2]
        pick, best = g.clone(), (g - yaw).abs()
        for cand in (g + 2 * math.pi, g - 2 * math.pi):
            d = (cand - yaw).abs()
            closer = d < best
            pick, best = torch.where(closer, cand, pick), torch.where(closer, d, best)
        goal = torch.cat([self.targets[:, :2], pick[:, None]], dim=1)
        # criticallyDampedSpringControl with constant 1 (Controls.h:18-27)
        self.desired_u = 1.0 * (goal - s[:, :3]) + (-s[:, 3:] * 2.0 * math.sqrt(1.0))
        _lib.fov_control_solve(self.cfg, s, self.desired_u, self.estimator.nb_row_ptr, est_xy, self.u,
                               status=self.status, device=self.device, nb_cov=est_cov)
        # zero control where the QP failed (:235-238)
        u = torch.where((self.status == _lib.OPTIMAL)[:, None], self.u, torch.zeros_like(self.u))
        # applyInput of the XYYaw double integrator (DoubleIntegratorXYYaw.cpp:14-20), convertYawInRange
        pos = s[:, :3] + Ts * s[:, 3:] + (0.5 * Ts * Ts) * u
        vel = s[:, 3:] + Ts * u
        y = pos[:, 2]
        y = torch.where(y > math.pi, y - 2 * math.pi, torch.where(y < -math.pi, y + 2 * math.pi, y))
        pos = torch.cat([pos[:, :2], y[:, None]], dim=1)
        if self.pos_std > 0.0:
            pos = pos + self.pos_std * torch.randn(pos.shape, dtype=pos.dtype, device=pos.device, generator=self._gen)
        if self.vel_std > 0.0:
            vel = vel + self.vel_std * torch.randn(vel.shape, dtype=vel.dtype, device=vel.device, generator=self._gen)
        new = torch.cat([pos, vel], dim=1).contiguous()
        if self.record:
            self._record(s.cpu().numpy(), est_xy.cpu().numpy(), est_cov.cpu().numpy(), new.cpu().numpy())
        # the update loop wraps the (possibly noisy) yaw once more (:270-277)
        y = new[:, 2]
        new[:, 2] = torch.where(y > math.pi, y - 2 * math.pi, torch.where(y < -math.pi, y + 2 * math.pi, y))
        self.applied_u = u
        self.states = new
        self.steps_done += 1
        return new

    def _record(self, s, xy, cov, new):
        for i in range(self.n):
            r = self.log[str(i)]
            for e in range(self.rp[i], self.rp[i + 1]):
                j = str(self.col[e])
                cxx, cxy, cyy = (float(v) for v in cov[e])
                r["estimates_mean"][j].append([float(xy[e, 0]), float(xy[e, 1]), 0.0])
                r["estimates_cov"][j].append([cxx, cxy, 0.0, cxy, cyy, 0.0, 0.0, 0.0, 0.0])
                r["p_near_ellipse"][j].append(list(closest_point_on_ellipse(s[i, :2], xy[e], cov[e])))
            r["states"].append([float(v) for v in new[i]])

    def run(self, steps: int):
        for _ in range(int(steps)):
            self.step()
        return self.states

    def to_json(self) -> dict:
        """The example's record (:103-105, 215-222, 258): dt, Ts and per robot states, estimates_mean,
        estimates_cov and p_near_ellipse keyed by the neighbour's id."""
        return {"dt": self.Ts, "Ts": self.Ts, "robots": self.log}

    def write_json(self, path: str):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=4)

"""Batched particle-filter estimates of the FoV controllers' neighbours (mpccbf_pf_init /
mpccbf_pf_step): one filter per (observer, neighbour) pair, as
cbf/examples/fov/CBFControl_example.cpp:145-168,192-194 keeps them."""
from __future__ import annotations

import numpy as np

from . import _lib


class FovEstimator:
    """The filters of a CSR list of (observer, neighbour) pairs on one device.

    nb_row_ptr / nb_col: integers (host arrays or device tensors): observer agent_first + i holds
    the pairs nb_row_ptr[i] .. nb_row_ptr[i+1]-1, pair e estimates row nb_col[e] of the state table
    (num_states x 6). cfg: fov_beta, fov_Rs and the optional pf_* keys of pf_params.

    The estimator owns the per-pair tensors: particles (pairs x 2 x P), weights (pairs x P), est_xy
    (pairs x 2), est_cov (pairs x 3), flags (pairs; bit 0 = measured this step, bit 1 = the weights
    were reset) and ancestors (pairs x P, the last step's resampling choices). est_xy / est_cov pass
    unchanged as nb_xy= / nb_cov= of fov_control_solve."""

    def __init__(self, cfg: dict, nb_row_ptr, nb_col, num_states: int, device: int = 0, seed: int = 0,
                 agent_first: int = 0):
        import torch
        self.params = _lib.pf_params(cfg, seed=seed)
        self.device = int(device)
        self.num_states = int(num_states)
        self.agent_first = int(agent_first)
        dev = torch.device("cuda", self.device)
        to_host = lambda v: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v))  # noqa: E731
        rp = to_host(nb_row_ptr).astype(np.int32).reshape(-1)
        col = to_host(nb_col).astype(np.int32).reshape(-1)
        if rp.size < 1 or np.any(np.diff(rp) < 0) or rp[0] < 0:
            raise _lib.MpccbfError("nb_row_ptr must hold non-decreasing offsets")
        if col.size < rp[-1]:
            raise _lib.MpccbfError("nb_col is shorter than nb_row_ptr[-1]")
        if col.size and (col[:rp[-1]].min() < 0 or col[:rp[-1]].max() >= self.num_states):
            raise _lib.MpccbfError("nb_col holds an index outside the state table")
        if self.agent_first < 0 or self.agent_first + rp.size - 1 > self.num_states:
            raise _lib.MpccbfError("the observers are not rows of the state table")
        self.num_agents = int(rp.size - 1)
        self.first_pair, self.num_pairs = int(rp[0]), int(rp[-1] - rp[0])
        self.rows = int(rp[-1])  # rows of the per-pair tensors
        P = self.num_particles = int(self.params.num_particles)
        alloc = max(self.rows, 1)  # (an empty tensor has no pointer to pass)
        self.nb_row_ptr = torch.tensor(rp, dtype=torch.int32, device=dev)
        self.nb_col = torch.tensor(col if col.size else np.zeros(1, np.int32), dtype=torch.int32, device=dev)
        self.particles = torch.zeros((alloc, 2, P), dtype=torch.float64, device=dev)
        self.weights = torch.zeros((alloc, P), dtype=torch.float64, device=dev)
        self.est_xy = torch.zeros((alloc, 2), dtype=torch.float64, device=dev)
        self.est_cov = torch.zeros((alloc, 3), dtype=torch.float64, device=dev)
        self.flags = torch.zeros(alloc, dtype=torch.int32, device=dev)
        self.ancestors = torch.zeros((alloc, P), dtype=torch.int32, device=dev)
        self.step_index = 0

    def _check_states(self, states):
        if states.shape[0] != self.num_states or states.shape[-1] != 6:
            raise _lib.MpccbfError(f"states must be ({self.num_states}, 6)")

    def init(self, states, init_xy=None, stream=None):
        """Start every filter at its neighbour's position in `states` (or at init_xy, pairs x 2);
        resets step_index. Returns (est_xy, est_cov)."""
        self._check_states(states)
        self.step_index = 0
        _lib.pf_init(self.params, states, self.nb_row_ptr, self.nb_col, self.num_pairs, self.particles,
                     self.weights, self.est_xy, self.est_cov, agent_first=self.agent_first,
                     num_agents=self.num_agents, init_xy=init_xy, flags=self.flags, step_index=0,
                     device=self.device, stream=stream)
        return self.est_xy, self.est_cov

    def step(self, states, input=None, stream=None):
        """One processFovUpdate of every filter against `states` (input: optional pairs x 2 motion
        input of the predict); advances step_index. Returns (est_xy, est_cov), the estimator's own
        tensors (the next step overwrites them)."""
        self._check_states(states)
        _lib.pf_step(self.params, states, self.nb_row_ptr, self.nb_col, self.num_pairs, self.particles,
                     self.weights, self.est_xy, self.est_cov, agent_first=self.agent_first,
                     num_agents=self.num_agents, input=input, flags=self.flags, ancestors=self.ancestors,
                     step_index=self.step_index, device=self.device, stream=stream)
        self.step_index += 1
        return self.est_xy, self.est_cov

"""Closed-loop safety monitor on the device (mpccbf_monitor_* / mpccbf_set_monitor in
include/mpccbf.h): scores snapshots of a swarm with the semantics of the reference's
collision_check.py as mpccbf.metrics restates them, without the trace leaving the device.

SafetyMonitor owns the device outputs; result_from_outputs turns their host copies into the answers
of metrics.instance_success (a pure function: no GPU, no library).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

KEY_ROW_BITS = 20     # first-collision key: (sample << 40) | (i << 20) | j
KEY_SAMPLE_SHIFT = 40
SHAPE_TYPES = {"circle": 0, "box": 1}


def decode_key(key: int):
    """(sample, i, j) of a first-collision key, or None for -1."""
    key = int(key)
    if key < 0:
        return None
    m = (1 << KEY_ROW_BITS) - 1
    return key >> KEY_SAMPLE_SHIFT, (key >> KEY_ROW_BITS) & m, key & m


def result_from_outputs(summary, reached_at, min_d2=None, hit_samples=None, unsafe_samples=None, *,
                        agent_first: int = 0, num_agents=None) -> dict:
    """The monitor's answers from host copies of its raw outputs (summary: 5 int64; the per-row
    arrays over the state table's rows; the agents are rows agent_first .. agent_first + num_agents,
    default all rows).

    instance_success, makespan, first_collision: the return values of metrics.instance_success on
    the same samples. The script walks the samples and stops at the first one before which every
    robot has reached its goal area: with R the last robot's arrival sample, a collision in a sample
    <= R fails the run ((False, inf, (sample, i, j))), a later one does not; a clean walk returns
    (True, R, None) when a sample follows R and (True, samples, None) otherwise (R is the last
    sample, or some robot never arrives)."""
    summary = np.asarray(summary, dtype=np.int64).reshape(-1)
    reached_at = np.asarray(reached_at, dtype=np.int64).reshape(-1)
    if num_agents is None:
        num_agents = reached_at.size - agent_first
    samples = int(summary[0])
    ra = reached_at[agent_first:agent_first + num_agents]
    all_reached = bool(np.all(ra >= 0))
    last_arrival = int(ra.max()) if (all_reached and ra.size) else -1  # (no agents: reached before sample 0)
    first = decode_key(summary[1])
    if first is not None and (not all_reached or first[0] <= last_arrival):
        ok, makespan, collision = False, float("inf"), first
    elif all_reached and last_arrival + 1 < samples:
        ok, makespan, collision = True, max(0, last_arrival), None
    else:
        ok, makespan, collision = True, samples, None
    d2 = float(np.asarray(summary[4:5]).view(np.float64)[0])
    out = {
        "instance_success": ok, "makespan": makespan, "first_collision": collision,
        "min_pair_distance_m": math.sqrt(d2),
        "goal_reached_frac": float(np.count_nonzero(ra >= 0)) / ra.size if ra.size else 1.0,
        "samples": samples, "first_collision_any": first,
        "colliding_pair_samples": int(summary[2]), "unsafe_pair_samples": int(summary[3]),
    }
    if hit_samples is not None:
        out["rows_hit"] = int(np.count_nonzero(np.asarray(hit_samples)))
    if unsafe_samples is not None:
        out["rows_unsafe"] = int(np.count_nonzero(np.asarray(unsafe_samples)))
    if min_d2 is not None and np.asarray(min_d2).size:
        out["row_min_distance_m"] = float(np.sqrt(np.min(np.asarray(min_d2, dtype=np.float64))))
    return out


class SafetyMonitor:
    """The device outputs of one monitor and the calls on them.

    rows: capacity of the per-row outputs (>= the rows of every state table scored). shape /
    shape_type: the script's collision shape ("box": half extents [cx, cy]; "circle": a radius).
    d_min: the CBF's safe distance. watch_radius: pairs farther apart are not seen (None: 3 d_min; it
    must cover d_min and the shape's reach). sample_log: rows of the optional per-sample log.
    max_samples: the most samples one device call scores (sizes the scratch; score() splits longer
    traces, and a context it is attached to scores at most int(h / Ts) per step).

    Outputs (device tensors): summary (5 int64), reached_at (rows int64), min_d2 (rows float64),
    hit_samples / unsafe_samples (rows int32), sample_log (sample_log x 3 int64, or None)."""

    def __init__(self, rows: int, shape=(0.2, 0.2), shape_type: str = "box", *, d_min: float,
                 goal_radius: float = 1.0, watch_radius=None, sample_log: int = 0, device: int = 0,
                 max_samples: int = 16):
        import torch
        if shape_type not in SHAPE_TYPES:
            raise ValueError(f"Unknown shape_type: {shape_type}")
        L = _lib.load()
        self.device = int(device)
        self.rows = int(rows)
        self.max_samples = int(max_samples)
        dev = torch.device("cuda", self.device)
        sh = [float(shape), 0.0] if shape_type == "circle" else [float(shape[0]), float(shape[1])]
        self.summary = torch.zeros(_lib.MONITOR_WORDS, dtype=torch.int64, device=dev)
        self.reached_at = torch.zeros(self.rows, dtype=torch.int64, device=dev)
        self.min_d2 = torch.zeros(self.rows, dtype=torch.float64, device=dev)
        self.hit_samples = torch.zeros(self.rows, dtype=torch.int32, device=dev)
        self.unsafe_samples = torch.zeros(self.rows, dtype=torch.int32, device=dev)
        self.sample_log = torch.zeros((int(sample_log), 3), dtype=torch.int64, device=dev) if sample_log > 0 else None
        nbytes = int(L.mpccbf_monitor_scratch_bytes(self.rows, self.max_samples))
        self.scratch = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=dev)
        self.struct = _lib.Monitor(
            shape_type=SHAPE_TYPES[shape_type], shape=(C.c_double * 2)(*sh), d_min=float(d_min),
            goal_radius=float(goal_radius), watch_radius=0.0 if watch_radius is None else float(watch_radius),
            rows=self.rows, summary=self.summary.data_ptr(), reached_at=self.reached_at.data_ptr(),
            min_d2=self.min_d2.data_ptr(), hit_samples=self.hit_samples.data_ptr(),
            unsafe_samples=self.unsafe_samples.data_ptr(),
            sample_log=None if self.sample_log is None else self.sample_log.data_ptr(),
            sample_log_rows=int(sample_log) if sample_log > 0 else 0, scratch=self.scratch.data_ptr(),
            scratch_bytes=int(self.scratch.numel()))
        self.agents = (0, self.rows)  # the agent range of the last score (result()'s default)
        self.reset()

    def reset(self, stream=None):
        """Initialise every output (mpccbf_monitor_reset): no samples, no collision, nobody arrived."""
        _lib._check(_lib.load().mpccbf_monitor_reset(C.byref(self.struct), self.device, _lib._stream(stream)))

    def score(self, states, goals=None, agent_first: int = 0, fixed_states=None, sample_first=None, stream=None):
        """Score a state table (n x 6: one sample) or a trace (n x ts x 6, the layout of
        Simulator's substeps and of a states.json array: ts samples) of the agents, rows agent_first
        .. agent_first + n of the table. fixed_states (num_states x 6): the table whose other rows
        take part in every sample as static rows. goals: n x 3, or None. sample_first: index of the
        first sample (None: continue after the samples scored so far). All device tensors
        (float64, contiguous)."""
        if states.dim() == 2:
            n, ts, strides = states.shape[0], 1, (6, 6)
        elif states.dim() == 3:
            n, ts, strides = states.shape[0], states.shape[1], (6, states.shape[1] * 6)
        else:
            raise _lib.MpccbfError("score takes a (n, 6) table or a (n, ts, 6) trace")
        if states.shape[-1] != 6:
            raise _lib.MpccbfError("a state has 6 entries")
        num_states = n + agent_first if fixed_states is None else fixed_states.shape[0]
        if goals is not None and (goals.dim() != 2 or goals.shape[0] != n or goals.shape[1] != 3):
            raise _lib.MpccbfError("goals must be (n, 3)")
        if fixed_states is not None and (fixed_states.dim() != 2 or fixed_states.shape[1] != 6):
            raise _lib.MpccbfError("fixed_states must be (num_states, 6)")
        fn, s, base = _lib.load().mpccbf_monitor_score, _lib._stream(stream), _lib._ptr(states) if n else None
        for s0 in range(0, max(ts, 1), self.max_samples):
            cnt = min(self.max_samples, ts - s0)
            _lib._check(fn(C.byref(self.struct), None if base is None else base + 8 * 6 * s0, cnt, strides[0],
                           strides[1], int(agent_first), n, _lib._ptr(fixed_states), int(num_states),
                           _lib._ptr(goals), -1 if sample_first is None else int(sample_first) + s0, self.device, s))
        self.agents = (int(agent_first), n)

    def raw(self) -> dict:
        """Host copies (numpy) of the outputs; waits for the device."""
        out = {k: getattr(self, k).cpu().numpy() for k in ("summary", "reached_at", "min_d2", "hit_samples",
                                                           "unsafe_samples")}
        out["sample_log"] = None if self.sample_log is None else self.sample_log.cpu().numpy()
        return out

    def result(self, agent_first=None, num_agents=None) -> dict:
        """result_from_outputs of the outputs as they stand (waits for the device); the agents
        default to those of the last score."""
        r = self.raw()
        if agent_first is None:
            agent_first, num_agents = self.agents if num_agents is None else (self.agents[0], num_agents)
        return result_from_outputs(r["summary"], r["reached_at"], r["min_d2"], r["hit_samples"], r["unsafe_samples"],
                                   agent_first=agent_first, num_agents=num_agents)

"""Inputs of test_gpu_param_space.py (GPU) and test_param_space_inputs.py (CPU): swarms off the
base configuration (moving reference trajectories, yaw motion, asymmetric limits, rings of
neighbours) and the CPU-side counts (statuses, live CBF rows, tight box rows) that say what each
input exercises. Everything is seeded; nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

import oracle_lib as O
from mpccbf import swarm

# per-channel limits that differ between x, y and yaw and are not symmetric about 0
ASYM = dict(v_min=[-1.0, -2.5, -1.0], v_max=[2.0, 1.5, 2.6],
            a_min=[-3.0, -5.0, -2.0], a_max=[5.0, 2.0, 3.0])


def crowded(n, scale, seed, v_range=0.5):
    """swarm.lattice_swarm with the positions times `scale`; each target keeps its original offset
    from its agent. Returns (states n x 6, targets n x 3)."""
    states, targets = swarm.lattice_swarm(n, seed=seed, v_range=v_range)
    off = targets - states[:, :3]
    states[:, :2] *= scale
    return states, states[:, :3] + off


def with_yaw(states, targets, seed, rate):
    """Copies with yaw U(-3, 3), yaw rate U(-rate, rate) and yaw target = yaw + U(-2.5, 2.5)."""
    rng = np.random.default_rng(seed)
    n = len(states)
    st, tg = states.copy(), targets.copy()
    st[:, 2] = rng.uniform(-3.0, 3.0, n)
    st[:, 5] = rng.uniform(-rate, rate, n)
    tg[:, 2] = st[:, 2] + rng.uniform(-2.5, 2.5, n)
    return st, tg


def moving_refs(states, targets, K, h, seed):
    """Reference trajectories n x 3K (sample-major, [k][channel]): per agent a and channel d,
    target_d + vel_d h k + 0.3 sin(0.7 k + d + a), vel ~ U(-1.5, 1.5)^3 — every channel moves."""
    rng = np.random.default_rng(seed)
    n = len(states)
    vel = rng.uniform(-1.5, 1.5, (n, 3))
    k = np.arange(K)[None, :, None]
    d = np.arange(3)[None, None, :]
    a = np.arange(n)[:, None, None]
    refs = targets[:, None, :] + vel[:, None, :] * h * k + 0.3 * np.sin(0.7 * k + d + a)
    return np.ascontiguousarray(refs.reshape(n, 3 * K))


def ring(n_ring, radius=2.02, v0=(0.2, 0.1)):
    """Agent 0 at the origin with velocity v0 and n_ring static robots on a half circle of
    `radius` around it; every other robot is a neighbour (the geometry of
    test_capacity_fallback_many_live_rows). Returns (states, targets, row_ptr, col)."""
    n = n_ring + 1
    states = np.zeros((n, 6))
    states[0, 3:5] = v0
    ang = np.linspace(0.05, np.pi - 0.05, n_ring)
    states[1:, 0] = radius * np.cos(ang)
    states[1:, 1] = radius * np.sin(ang)
    targets = np.zeros((n, 3))
    targets[:, 1] = -2.0
    targets[1:, :2] = states[1:, :2]
    rp, col = swarm.all_csr(n)
    return states, targets, rp, col


def oracle_batch(cfg, states, targets, rp, col, refs=None, cov=None):
    """The oracle's result of every agent (list of impc_optimize dicts)."""
    p = O.make_params(cfg)
    if refs is None:
        refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    return [O.impc_optimize(p, states, a, col[rp[a]:rp[a + 1]], refs[a], covs=cov)
            for a in range(len(rp) - 1)]


def status_mix(res):
    """{status tuple: number of agents} of an oracle batch."""
    mix = {}
    for r in res:
        key = tuple(int(s) for s in r["status"])
        mix[key] = mix.get(key, 0) + 1
    return mix


def attempted_unknown(res):
    """Agents whose oracle result holds an UNKNOWN for a QP that was attempted (the oracle's own
    solver gave no verdict): the first `attempted` entries of status."""
    return [i for i, r in enumerate(res) if O.UNKNOWN in list(r["status"][:r["attempted"]])]


def live_rows_it1(cfg, states, targets, rp, col, res=None):
    """Per agent, the iteration-1 CBF rows that the exact box filter keeps (b < max_u -a^T u): the
    egos are the oracle's iteration-0 curve at h k, k < cbf_horizon (0 rows when iteration 0 is
    not OPTIMAL: there is no iteration 1)."""
    p = O.make_params(cfg)
    if res is None:
        res = oracle_batch(cfg, states, targets, rp, col)
    amax, amin = np.array(cfg["a_max"]), np.array(cfg["a_min"])
    n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    out = np.zeros(len(rp) - 1, dtype=int)
    for i, r in enumerate(res):
        if r["status"][0] != O.OPTIMAL:
            continue
        x0 = r["x"][0][:n]
        for k in range(cfg["cbf_horizon"]):
            ego = np.concatenate([O.eval_curve(p, x0, cfg["h"] * k, 0), O.eval_curve(p, x0, cfg["h"] * k, 1)])
            for j in col[rp[i]:rp[i + 1]]:
                a, b = O.safety_cbf(ego, states[j], cfg["d_min"])
                out[i] += int(b < np.sum(np.maximum(-a * amin, -a * amax)))
    return out


def tight_box_agents(cfg, res, tol=1e-6):
    """Per channel, the number of agents whose last OPTIMAL curve has a velocity or acceleration
    sample (t = h k, k < k_hor) within tol of one of its four bounds."""
    p = O.make_params(cfg)
    n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    cnt = np.zeros(3, dtype=int)
    for r in res:
        ok = [it for it in range(cfg["impc_iter"]) if r["status"][it] == O.OPTIMAL]
        if not ok:
            continue
        x = r["x"][ok[-1]][:n]
        tight = np.zeros(3, dtype=bool)
        for k in range(cfg["k_hor"]):
            v = O.eval_curve(p, x, cfg["h"] * k, 1)
            a = O.eval_curve(p, x, cfg["h"] * k, 2)
            for d in range(3):
                tight[d] |= (abs(v[d] - cfg["v_min"][d]) <= tol or abs(v[d] - cfg["v_max"][d]) <= tol or
                             abs(a[d] - cfg["a_min"][d]) <= tol or abs(a[d] - cfg["a_max"][d]) <= tol)
        cnt += tight
    return cnt


def fov_swarm(n=64, seed=2, scale=0.7):
    """swarm.heading_swarm with the positions times `scale` (targets as generated)."""
    states, targets = swarm.heading_swarm(n, seed=seed)
    states[:, :2] *= scale
    return states, targets


def filter_edge(speeds=(0.30, 0.35, 0.35, 0.25), gap=2.05, far=12.0):
    """Four agents, each 'gap' from a static robot of its own (its only neighbour, the pairs 40 m
    apart), moving away from it at speeds[i] with its target 'far' beyond the robot: on the +x, -x,
    +y and -y side. The tracking cost asks for full acceleration back towards the robot, so the
    optimum sits on the pair's CBF row, whose bound b lies just below the filter's threshold
    max_u -a^T u: a filter that forms the threshold from another channel's or the other side's
    (narrower) acceleration bound drops a row that is active.
    Returns (states, targets, row_ptr, col); agents 0..3 move, 4..7 are the static robots."""
    dirs = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    states = np.zeros((8, 6))
    targets = np.zeros((8, 3))
    for i, d in enumerate(dirs):
        c = np.array([40.0 * i, 0.0])
        states[4 + i, :2] = c
        states[i, :2] = c + gap * d
        states[i, 3:5] = speeds[i] * d
        targets[i, :2] = c - far * d
        targets[4 + i, :2] = c
    rp = np.arange(9, dtype=np.int32)
    col = np.array([4, 5, 6, 7, 0, 1, 2, 3], dtype=np.int32)
    return states, targets, rp, col


def filter_edge_margins(cfg, states, targets, rp, col, res):
    """Per moving agent of filter_edge and IMPC iteration 0: (b, threshold, narrow, slack) — the
    CBF row's bound, the exact filter threshold max_u -a^T u, the largest threshold a filter would
    form from any other entry of a_min / a_max (or its negative) in place of the bound that
    matters, and the row's slack b + a^T u at the oracle's optimum (0: the row is active)."""
    p = O.make_params(cfg)
    n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    lim = sorted({abs(v) for v in cfg["a_min"] + cfg["a_max"]})
    out = []
    for i in range(4):
        a, b = O.safety_cbf(states[i], states[col[rp[i]]], cfg["d_min"])
        d = int(np.argmax(np.abs(a)))
        amin, amax = cfg["a_min"][d], cfg["a_max"][d]
        thr = max(-a[d] * amin, -a[d] * amax)
        used = abs(amin) if -a[d] * amin >= -a[d] * amax else abs(amax)
        narrow = max([abs(a[d]) * v for v in lim if v < used], default=0.0)
        u = O.eval_curve(p, res[i]["x"][0][:n], 0.0, 2)
        out.append((b, thr, narrow, b + float(a @ u)))
    return out

"""Seeded cases of the batched FoV particle filter (tests/test_pf_inputs.py pins them on the
reference alone; tests/test_gpu_pf.py runs them on the device).

A case is a dict: par (pf_ref.params), num_states, agent_first, rp / col (CSR over the observers
agent_first .. agent_first + num_agents - 1), steps, states(t) (the state table step t reads;
init reads states(0)), input (pairs x 2 or None) and init_xy (pairs x 2 or None)."""
import math

import numpy as np

import pf_ref

FOV = 2.0 * math.pi / 3.0  # base_config's fov_beta
RS = 6.0                   # and fov_Rs
PARTICLE_COUNTS = (2, 63, 64, 65, 100, 1024)


def _moving(states0, vel, dt=0.2):
    """states(t): constant planar / yaw velocity from states0, the yaw wrapped into (-pi, pi]."""
    states0, vel = np.array(states0, dtype=np.float64), np.array(vel, dtype=np.float64)

    def states(t):
        s = states0.copy()
        s[:, :3] += vel * dt * t
        s[:, 3:] = vel
        s[:, 2] = -((-s[:, 2] + math.pi) % (2.0 * math.pi) - math.pi)
        return s
    return states


def _csr(rows):
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([j for r in rows for j in r], dtype=np.int32)
    return rp, col


def shape_case(P, seed):
    """5 observers (rows 2 .. 6 of 12 states) with 0, 1, 9, 3 and 2 neighbours; random positions in
    a 10 m box, yaws over (-pi, pi] (one exactly pi), everyone drifting."""
    rng = np.random.default_rng(1000 + P)
    n = 12
    s0 = np.zeros((n, 6))
    s0[:, :2] = rng.uniform(-5.0, 5.0, (n, 2))
    s0[:, 2] = rng.uniform(-math.pi, math.pi, n)
    s0[4, 2] = math.pi
    vel = np.zeros((n, 3))
    vel[:, :2] = rng.uniform(-0.5, 0.5, (n, 2))
    vel[:, 2] = rng.uniform(-1.0, 1.0, n)
    first = 2
    rows = [[], [0], [j for j in range(n) if j != 4][:9], [11, 3, 7], [2, 10]]
    rp, col = _csr(rows)
    par = pf_ref.params(FOV, RS, num_particles=P, seed=seed)
    return dict(name=f"shape_P{P}", par=par, num_states=n, agent_first=first, rp=rp, col=col,
                steps=20 if P == 100 else 4, states=_moving(s0, vel), input=None, init_xy=None)


def scenario_case(seed):
    """One observer (row 3 of 6 states) at the origin looking along +x: neighbour 0 visible ahead,
    1 hidden behind it, 2 ahead but beyond Rs, 4 crossing the FoV edge outwards and 5 inwards over
    the steps. Non-diagonal W, init_cov and meas_cov, a non-zero input."""
    half = 0.5 * FOV
    s0 = np.zeros((6, 6))
    vel = np.zeros((6, 3))
    s0[0, :2] = (3.0, 0.5)
    s0[1, :2] = (-2.5, 0.3)
    s0[2, :2] = (7.5, -1.0)
    s0[4, :2] = (3.0 * math.cos(half - 0.25), 3.0 * math.sin(half - 0.25))
    vel[4, :2] = (-0.45, 0.6)
    s0[5, :2] = (2.0 * math.cos(-half - 0.3), 2.0 * math.sin(-half - 0.3))
    vel[5, :2] = (0.5, 0.35)
    vel[0, :2] = (0.1, -0.05)
    rp, col = _csr([[0, 1, 2, 4, 5]])
    par = pf_ref.params(FOV, RS, num_particles=100, init_cov=(0.8, 0.3, 0.5), process=(0.25, 0.05, -0.1, 0.2),
                        meas_cov=(0.05, 0.02, 0.08), weight_reduction=10.0, seed=seed)
    inp = np.array([[0.1, -0.05], [0.0, 0.0], [0.3, 0.2], [-0.45, 0.6], [0.5, 0.35]])
    return dict(name="scenarios", par=par, num_states=6, agent_first=3, rp=rp, col=col, steps=20,
                states=_moving(s0, vel), input=inp, init_xy=None)


def degenerate_case(seed):
    """The measured neighbour (visible, 3 m ahead) 100 m from every particle (init_xy), R = 0.05 I:
    every measurement weight underflows to 0. The second pair is an ordinary one."""
    s0 = np.zeros((3, 6))
    s0[1, :2] = (3.0, 0.0)
    s0[2, :2] = (2.0, 1.0)
    rp, col = _csr([[1, 2]])
    par = pf_ref.params(FOV, RS, num_particles=100, seed=seed)
    init_xy = np.array([[103.0, 0.0], [2.0, 1.0]])
    return dict(name="degenerate", par=par, num_states=3, agent_first=0, rp=rp, col=col, steps=2,
                states=_moving(s0, np.zeros((3, 3))), input=None, init_xy=init_xy)


# the seeds are chosen so that every case's decision margins stay >= 1e-10 over its steps
# (tests/test_pf_inputs.py); no case, pair or particle is left out of any comparison
def all_cases():
    return [shape_case(P, seed=11) for P in PARTICLE_COUNTS] + [scenario_case(seed=5), degenerate_case(seed=7)]


def run_reference(case):
    """init then `steps` free-running reference steps: (init dict, list of step dicts)."""
    c = case
    st = pf_ref.init(c["par"], c["states"](0), c["agent_first"], c["rp"], c["col"], init_xy=c["init_xy"])
    out, parts, wts = [], st["particles"], st["weights"]
    for t in range(c["steps"]):
        r = pf_ref.step(c["par"], c["states"](t), c["agent_first"], c["rp"], c["col"], parts, wts, t,
                        input=c["input"])
        out.append(r)
        parts, wts = r["particles"], r["weights"]
    return st, out

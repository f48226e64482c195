"""GPU: the batched FoV particle filter (mpccbf_pf_init / mpccbf_pf_step, csrc/kernels/pf_fov.hip)
against its numpy restatement (tests/pf_ref.py) on the committed cases (tests/pf_cases.py), the
FovEstimator's estimates into the batched FovControl QP, and the FovControlLoop against the
reference chain re-run on the device's own inputs of every step.

Tolerances: the device and numpy take the same discrete decisions on these cases
(tests/test_pf_inputs.py pins a decision margin >= 1e-10), so ancestors and flags compare exactly;
the continuous outputs differ through libm's last bits, FMA contraction and reordered FP64 sums of
<= 1024 terms."""
import math

import numpy as np
import pytest

import oracle_lib as O
import pf_cases
import pf_ref
from gpu_harness import require_gpu
from mpccbf import swarm

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in pf_cases.all_cases()}


@pytest.fixture(scope="module")
def reference():
    """init and the free-running reference steps of every case, computed once and left unchanged."""
    return {name: pf_cases.run_reference(c) for name, c in CASES.items()}


def _c_params(mpclib, par):
    p = mpclib.PfParams()
    p.num_particles = par["num_particles"]
    for name in ("init_cov", "process", "meas_cov"):
        for i, v in enumerate(par[name]):
            getattr(p, name)[i] = v
    p.dt, p.fov, p.Rs = par["dt"], par["fov"], par["Rs"]
    p.weight_reduction, p.seed = par["weight_reduction"], par["seed"]
    return p


class Dev:
    """A case's tensors on the device; init / step through the C ABI, results read back as numpy."""

    def __init__(self, mpclib, case, fill=0.0):
        torch = require_gpu()
        self.lib, self.c, self.torch = mpclib, case, torch
        self.dev = torch.device("cuda", 0)
        self.p = _c_params(mpclib, case["par"])
        n, P = int(case["rp"][-1]), case["par"]["num_particles"]
        self.n, self.P = n, P
        t = lambda v, dt=torch.float64: torch.tensor(np.ascontiguousarray(v), dtype=dt, device=self.dev)  # noqa: E731
        self.t = t
        self.rp, self.col = t(case["rp"], torch.int32), t(case["col"], torch.int32)
        self.particles = torch.full((n, 2, P), fill, dtype=torch.float64, device=self.dev)
        self.weights = torch.full((n, P), fill, dtype=torch.float64, device=self.dev)
        self.est_xy = torch.full((n, 2), fill, dtype=torch.float64, device=self.dev)
        self.est_cov = torch.full((n, 3), fill, dtype=torch.float64, device=self.dev)
        self.flags = torch.full((n,), -7, dtype=torch.int32, device=self.dev)
        self.ancestors = torch.full((n, P), -7, dtype=torch.int32, device=self.dev)
        self.input = None if case["input"] is None else t(case["input"])
        self.init_xy = None if case["init_xy"] is None else t(case["init_xy"])

    def _range(self, rows):
        """(agent_first, num_agents, row-pointer view, pairs) of the list rows [rows[0], rows[1])."""
        lo, hi = rows if rows else (0, len(self.c["rp"]) - 1)
        return (self.c["agent_first"] + lo, hi - lo, self.rp[lo:hi + 1],
                int(self.c["rp"][hi] - self.c["rp"][lo]))

    def init(self, rows=None):
        first, count, rp, pairs = self._range(rows)
        self.lib.pf_init(self.p, self.t(self.c["states"](0)), rp, self.col, pairs, self.particles, self.weights,
                         self.est_xy, self.est_cov, agent_first=first, num_agents=count, init_xy=self.init_xy,
                         flags=self.flags)

    def step(self, t, rows=None):
        first, count, rp, pairs = self._range(rows)
        self.lib.pf_step(self.p, self.t(self.c["states"](t)), rp, self.col, pairs, self.particles, self.weights,
                         self.est_xy, self.est_cov, agent_first=first, num_agents=count, input=self.input,
                         flags=self.flags, ancestors=self.ancestors, step_index=t)

    def read(self):
        self.torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("particles", "weights", "est_xy", "est_cov", "flags",
                                                             "ancestors")}


@pytest.mark.parametrize("name", list(CASES))
def test_init_matches_the_reference(mpclib, reference, name):
    d = Dev(mpclib, CASES[name], fill=math.nan)
    d.init()
    got, (ref, _) = d.read(), reference[name]
    np.testing.assert_allclose(got["particles"], ref["particles"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got["weights"], ref["weights"])
    np.testing.assert_array_equal(got["est_xy"], ref["est_xy"])
    np.testing.assert_array_equal(got["est_cov"], ref["est_cov"])
    np.testing.assert_array_equal(got["flags"], 0)


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_from_the_devices_own_state(mpclib, name):
    c = CASES[name]
    d = Dev(mpclib, c)
    d.init()
    before = d.read()
    d.step(0)
    got = d.read()
    ref = pf_ref.step(c["par"], c["states"](0), c["agent_first"], c["rp"], c["col"], before["particles"],
                      before["weights"], 0, input=c["input"])
    assert ref["margin"].min() >= 1e-10  # (the device's init differs from the reference's in the last bits)
    np.testing.assert_array_equal(got["ancestors"], ref["ancestors"])
    np.testing.assert_array_equal(got["flags"], ref["flags"])
    # the particles after the step are the pre-resampling particles gathered by the ancestors: the
    # reference's predict of the device's own particles to 1e-12, and copies of one ancestor are
    # the same bits
    anc = got["ancestors"].astype(np.int64)
    gathered = np.take_along_axis(ref["predicted"], anc[:, None, :].repeat(2, axis=1), axis=2)
    np.testing.assert_allclose(got["particles"], gathered, rtol=1e-12, atol=1e-12)
    for e in range(d.n):
        for axis in range(2):
            first_of = {}
            for i, a in enumerate(anc[e]):
                assert got["particles"][e, axis, i] == got["particles"][e, axis, first_of.setdefault(a, i)]
    np.testing.assert_allclose(got["weights"], ref["weights"], rtol=1e-10, atol=0.0)
    np.testing.assert_allclose(got["est_xy"], ref["est_xy"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["est_cov"], ref["est_cov"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_free_running_steps_match_the_reference(mpclib, reference, name):
    """Every case over all its steps (20 on the multi-step ones), the device from its own init."""
    c = CASES[name]
    d = Dev(mpclib, c)
    d.init()
    _, steps = reference[name]
    for t, ref in enumerate(steps):
        d.step(t)
        got = d.read()
        np.testing.assert_array_equal(got["ancestors"], ref["ancestors"], err_msg=f"step {t}")
        np.testing.assert_array_equal(got["flags"], ref["flags"], err_msg=f"step {t}")
        np.testing.assert_allclose(got["est_xy"], ref["est_xy"], rtol=1e-9, atol=1e-9, err_msg=f"step {t}")
        np.testing.assert_allclose(got["est_cov"], ref["est_cov"], rtol=1e-9, atol=1e-9, err_msg=f"step {t}")


def test_degenerate_weights_are_reset(mpclib):
    c = CASES["degenerate"]
    d = Dev(mpclib, c)
    d.init()
    d.step(0)
    got = d.read()
    assert got["flags"][0] == pf_ref.FLAG_MEASURED | pf_ref.FLAG_DEGENERATE
    np.testing.assert_array_equal(got["weights"][0], np.full(d.P, 1.0 / d.P))
    assert np.isfinite(got["est_xy"]).all() and np.isfinite(got["est_cov"]).all()
    assert got["flags"][1] == pf_ref.FLAG_MEASURED  # the ordinary pair next to it


def test_hidden_neighbour_keeps_the_reduced_weights(mpclib):
    """Pair 4 of the scenarios at step 0: hidden just outside the FoV edge, particles on both sides."""
    c = CASES["scenarios"]
    d = Dev(mpclib, c)
    d.init()
    before = d.read()
    d.step(0)
    got = d.read()
    e, par = 4, c["par"]
    assert got["flags"][e] & pf_ref.FLAG_MEASURED == 0 and got["flags"][e] & pf_ref.FLAG_DEGENERATE == 0
    ref = pf_ref.step(par, c["states"](0), c["agent_first"], c["rp"], c["col"], before["particles"],
                      before["weights"], 0, input=c["input"])
    ang, dist = pf_ref.fov_frame(c["states"](0)[c["agent_first"]], ref["predicted"][e, 0], ref["predicted"][e, 1])
    inside = (ang <= 0.5 * par["fov"]) & (dist <= par["Rs"])
    assert 0 < inside.sum() < d.P
    reduced = np.where(inside, before["weights"][e] / par["weight_reduction"], before["weights"][e])
    np.testing.assert_array_equal(got["weights"][e], reduced[got["ancestors"][e]])


def test_same_call_twice_is_bitwise_identical(mpclib):
    c = CASES["shape_P100"]
    runs = []
    for _ in range(2):
        d = Dev(mpclib, c)
        d.init()
        for t in range(3):
            d.step(t)
        runs.append(d.read())
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


def test_observers_split_over_two_calls(mpclib):
    """Observers split by agent_first (list rows 0 .. 1 and 2 .. 4, the second with a non-zero first
    row pointer) on shared buffers: bitwise the per-pair results of one call, and a call leaves the
    rows of pairs outside its range untouched."""
    c = CASES["shape_P65"]
    one = Dev(mpclib, c)
    one.init()
    one.step(0)
    whole = one.read()
    cut = int(c["rp"][2])
    assert 0 < cut < one.n
    two = Dev(mpclib, c, fill=-123.0)
    two.init(rows=(0, 2))
    part = two.read()
    for k in ("particles", "weights", "est_xy", "est_cov"):
        assert np.all(part[k][cut:] == -123.0), k
    assert np.all(part["flags"][cut:] == -7)
    two.init(rows=(2, 5))
    two.step(0, rows=(0, 2))
    part = two.read()
    assert np.all(part["ancestors"][cut:] == -7) and np.all(part["flags"][cut:] == 0)
    for k in ("particles", "weights", "est_xy", "est_cov"):
        np.testing.assert_array_equal(part[k][:cut], whole[k][:cut], err_msg=k)
    two.step(0, rows=(2, 5))
    part = two.read()
    for k in whole:
        np.testing.assert_array_equal(part[k], whole[k], err_msg=k)


def _slack_cfg(decay=0.5):
    return dict(swarm.fov_config(20), control_slack_mode=1, slack_cost=1000.0, slack_decay_rate=decay)


def test_estimates_feed_the_fov_controller(mpclib):
    """est_xy / est_cov of a stepped FovEstimator straight into fov_control_solve in slack mode,
    against the oracle on the same estimates (tolerances of tests/test_fov_control.py's slack test)."""
    torch = require_gpu()
    cfg = _slack_cfg()
    n = 64
    states, targets = swarm.heading_swarm(n, seed=5)
    rp, col = swarm.fov_csr(states, 8, cfg["fov_Rs"], cfg["fov_beta"])
    assert rp[-1] > n
    dev = torch.device("cuda", 0)
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    est = mpclib.FovEstimator(cfg, rp, col, n, seed=3)
    est.init(st)
    for _ in range(3):
        xy, cov = est.step(st)
    desired = np.zeros((n, 3))
    desired[:, :2] = 2.0 * (targets[:, :2] - states[:, :2])
    u = torch.empty((n, 3), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    obj = torch.empty(n, dtype=torch.float64, device=dev)
    mpclib.fov_control_solve(cfg, st, torch.tensor(desired, dtype=torch.float64, device=dev), est.nb_row_ptr, xy, u,
                             status=status, obj=obj, nb_cov=cov)
    torch.cuda.synchronize()
    u, status, obj, xy, cov = (v.cpu().numpy() for v in (u, status, obj, xy, cov))
    assert (est.flags.cpu().numpy() & pf_ref.FLAG_MEASURED).any()
    for a in range(n):
        stt, ur, objr = O.fov_control(cfg, states[a], desired[a], xy[rp[a]:rp[a + 1]], nb_cov=cov[rp[a]:rp[a + 1]])
        assert status[a] == stt, (a, status[a], stt)
        if stt == O.OPTIMAL:
            np.testing.assert_allclose(u[a], ur, atol=1e-5, rtol=1e-5)
            assert abs(obj[a] - objr) <= 1e-4 * max(1.0, abs(objr)), (a, obj[a], objr)
    assert np.all(status == O.OPTIMAL)


def _wrap(y):
    return y - 2 * math.pi if y > math.pi else (y + 2 * math.pi if y < -math.pi else y)


def test_fov_control_loop_against_the_reference_chain(mpclib):
    """3 robots, 30 steps, no noise; at every step the reference chain on the device's inputs of that
    step: pf_ref from the device's particle state, the FovControl oracle on the device's estimates,
    the double-integrator update and the yaw wrap. Robot 2 turns past +pi."""
    require_gpu()
    cfg = _slack_cfg(0.1)
    # a triangle whose robots face its inside, so each keeps the two others in view; robot 2 looks
    # along -x (yaw 3.05, turning at 0.8 rad/s) and its goal yaw -3.0 is closest as -3.0 + 2 pi
    states = np.array([[0.0, 1.0, -0.94, 0.0, 0.0, 0.0],
                       [0.0, -1.0, 0.94, 0.0, 0.0, 0.0],
                       [3.0, 0.0, 3.05, 0.0, 0.0, 0.8]])
    targets = np.array([[0.3, 0.8, -0.85], [0.3, -0.8, 0.85], [2.6, 0.1, -3.0]])
    loop = mpclib.FovControlLoop(cfg, states, targets, seed=4)
    est = loop.estimator
    par = pf_ref.params(cfg["fov_beta"], cfg["fov_Rs"], seed=4)
    rp, col, Ts = loop.rp, loop.col, cfg["h"]
    worst = dict(est=0.0, u=0.0, state=0.0)
    turned = False
    for t in range(30):
        s = loop.states.cpu().numpy()
        parts, wts = est.particles.cpu().numpy(), est.weights.cpu().numpy()
        new = loop.step().cpu().numpy()
        xy, cov = est.est_xy.cpu().numpy(), est.est_cov.cpu().numpy()
        ref = pf_ref.step(par, s, 0, rp, col, parts, wts, t)
        assert ref["margin"].min() >= 1e-10, (t, ref["margin"].min())
        np.testing.assert_array_equal(est.ancestors.cpu().numpy(), ref["ancestors"])
        np.testing.assert_array_equal(est.flags.cpu().numpy(), ref["flags"])
        np.testing.assert_allclose(xy, ref["est_xy"], rtol=1e-10, atol=1e-10, err_msg=f"step {t}")
        np.testing.assert_allclose(cov, ref["est_cov"], rtol=1e-10, atol=1e-10, err_msg=f"step {t}")
        worst["est"] = max(worst["est"], np.abs(xy - ref["est_xy"]).max(), np.abs(cov - ref["est_cov"]).max())
        status, u_dev = loop.status.cpu().numpy(), loop.applied_u.cpu().numpy()
        for i in range(3):
            cand = [targets[i, 2], targets[i, 2] + 2 * math.pi, targets[i, 2] - 2 * math.pi]
            off = [abs(cy - s[i, 2]) for cy in cand]
            goal = np.array([targets[i, 0], targets[i, 1], cand[int(np.argmin(off))]])
            desired = 1.0 * (goal - s[i, :3]) + (-s[i, 3:] * 2.0 * math.sqrt(1.0))
            stt, ur, _ = O.fov_control(cfg, s[i], desired, xy[rp[i]:rp[i + 1]], nb_cov=cov[rp[i]:rp[i + 1]])
            assert status[i] == stt, (t, i, status[i], stt)
            if stt != O.OPTIMAL:
                ur = np.zeros(3)
            nxt = O.apply_input(Ts, s[i], ur)
            turned |= i == 2 and abs(nxt[2]) > math.pi
            nxt[2] = _wrap(nxt[2])
            worst["u"] = max(worst["u"], np.abs(u_dev[i] - ur).max())
            worst["state"] = max(worst["state"], np.abs(new[i] - nxt).max())
            np.testing.assert_allclose(u_dev[i], ur, rtol=1e-6, atol=1e-6, err_msg=f"step {t} robot {i}")
            np.testing.assert_allclose(new[i], nxt, rtol=1e-6, atol=1e-6, err_msg=f"step {t} robot {i}")
        assert np.all(np.abs(new[:, 2]) <= math.pi)
    print("FovControlLoop vs the reference chain, largest differences:", worst)
    assert turned and loop.states[2, 2].item() < 0.0  # robot 2 went through +pi and was wrapped
    js = loop.to_json()
    assert js["dt"] == cfg["h"] and js["Ts"] == cfg["h"] and sorted(js["robots"]) == ["0", "1", "2"]
    for i in range(3):
        r = js["robots"][str(i)]
        assert sorted(r) == ["estimates_cov", "estimates_mean", "p_near_ellipse", "states"]
        assert len(r["states"]) == 30 and len(r["states"][0]) == 6
        others = sorted(str(j) for j in range(3) if j != i)
        for key, width in (("estimates_mean", 3), ("estimates_cov", 9), ("p_near_ellipse", 2)):
            assert sorted(r[key]) == others
            for j in others:
                assert len(r[key][j]) == 30 and len(r[key][j][0]) == width
    np.testing.assert_array_equal(np.array(js["robots"]["1"]["states"][-1]), loop.states.cpu().numpy()[1])

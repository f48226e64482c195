"""GPU: the closed-loop safety monitor (mpccbf_monitor_score, mpccbf_set_monitor).

The hand-built cases of monitor_cases.py go through the device and must give the raw outputs that
numpy and mpccbf.metrics give on the host (test_monitor_inputs.py pins what each case exercises):
every count, key and per-row array exactly; the smallest squared distances within rtol 1e-14, two
roundings of dx*dx + dy*dy with or without contraction. Attached to a context, the monitor scores a
closed loop as metrics.instance_success / min_pair_distance score its trace, and leaves the solve
bit for bit what it is unattached."""
import numpy as np
import pytest

import monitor_cases as M
from gpu_harness import require_gpu, to_device
from mpccbf import metrics, sim, swarm
from parity_rule import same_bits

pytestmark = pytest.mark.gpu

LOG_ROWS = 12
D2_RTOL = 1e-14
INT_KEYS = ("summary", "reached_at", "hit_samples", "unsafe_samples", "sample_log")


def _monitor(mpclib, c, rows=None, **kw):
    n = c["samples"].shape[1]
    return mpclib.SafetyMonitor(n if rows is None else rows, sample_log=LOG_ROWS, **c["monitor"], **kw)


def _device_inputs(c):
    """(agents' tensor, goals, fixed table): the agents as a state table (layout "table") or as a
    n x S x 6 trace (the substeps layout); the fixed rows as the table of sample 0."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    a0, na = c["agent_first"], c["num_agents"]
    ag = c["samples"][:, a0:a0 + na]
    agents = ag[0] if c["layout"] == "table" else np.transpose(ag, (1, 0, 2))
    goals = None if c["goals"] is None else torch.tensor(c["goals"], device=dev)
    fixed = torch.tensor(c["samples"][0], device=dev) if na < c["samples"].shape[1] else None
    return to_device(agents), goals, fixed


def _score(mpclib, c, per_call=None, rows=None):
    """Raw outputs after a reset and the case's samples in calls of per_call samples (None: one)."""
    torch = require_gpu()
    mon = _monitor(mpclib, c, rows=rows)
    agents, goals, fixed = _device_inputs(c)
    S = c["samples"].shape[0]
    if per_call is None:
        mon.score(agents, goals=goals, agent_first=c["agent_first"], fixed_states=fixed)
    else:
        for s in range(0, S, per_call):
            mon.score(agents[:, s:s + per_call].contiguous(), goals=goals, agent_first=c["agent_first"],
                      fixed_states=fixed)
    torch.cuda.synchronize()
    return mon.raw()


def _same_bits(a, b):
    same_bits(a, b, keys=INT_KEYS + ("min_d2",))


@pytest.mark.parametrize("name", list(M.CASES))
def test_case_outputs(mpclib, name):
    c, want = M.case(name)
    got = _score(mpclib, c)
    print(f"{name}: summary {got['summary'].tolist()}, want {want['summary'].tolist()}")
    # counts, keys, arrivals, per-row counts, the per-sample counts: exactly
    np.testing.assert_array_equal(got["summary"][:4], want["summary"][:4])
    for k in ("reached_at", "hit_samples", "unsafe_samples"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["sample_log"][:, :2], want["sample_log"][:, :2])
    # smallest squared distances: +inf where the host's is, else within two roundings
    for g, w in ((got["min_d2"], want["min_d2"]), (got["summary"][4:5].view(np.float64), want["summary"][4:5].view(np.float64)),
                 (got["sample_log"][:, 2].copy().view(np.float64), want["sample_log"][:, 2].copy().view(np.float64))):
        np.testing.assert_array_equal(np.isinf(g), np.isinf(w))
        np.testing.assert_allclose(g[np.isfinite(w)], w[np.isfinite(w)], rtol=D2_RTOL, atol=0.0)
    # a second run repeats bit for bit
    _same_bits(_score(mpclib, c), got)


def test_result_of_the_timing_cases(mpclib):
    for name in ("collision_before_arrival", "collision_at_arrival", "collision_after_arrival", "trace10"):
        c, _ = M.case(name)
        torch = require_gpu()
        mon = _monitor(mpclib, c)
        agents, goals, fixed = _device_inputs(c)
        mon.score(agents, goals=goals)
        torch.cuda.synchronize()
        r = mon.result()
        assert (r["instance_success"], r["makespan"], r["first_collision"]) == M.script_result(c), name


@pytest.mark.parametrize("name", ["trace10", "fixed_rows", "collision_at_arrival"])
def test_one_call_equals_one_call_per_sample(mpclib, name):
    c, _ = M.case(name)
    whole = _score(mpclib, c)
    _same_bits(_score(mpclib, c, per_call=1), whole)
    _same_bits(_score(mpclib, c, per_call=3), whole)


def test_rows_beyond_the_table_stay_untouched(mpclib):
    c, want = M.case("fixed_rows")
    got = _score(mpclib, c, rows=11)
    assert got["reached_at"][8:].tolist() == [-1] * 3 and np.isinf(got["min_d2"][8:]).all()
    assert got["hit_samples"][8:].tolist() == [0] * 3
    np.testing.assert_array_equal(got["hit_samples"][:8], want["hit_samples"])


def test_explicit_sample_first_and_reset(mpclib):
    torch = require_gpu()
    c, want = M.case("trace10")
    mon = _monitor(mpclib, c)
    agents, goals, _ = _device_inputs(c)
    mon.score(agents[:, 4:].contiguous(), goals=goals, sample_first=4)
    torch.cuda.synchronize()
    got = mon.raw()
    assert got["summary"][0] == 6
    np.testing.assert_array_equal(got["sample_log"][4:, :2], want["sample_log"][4:, :2])
    assert (got["sample_log"][:4] == [0, 0, M.INF_BITS]).all()
    assert got["summary"][1] >> 40 >= 4
    mon.reset()
    torch.cuda.synchronize()
    got = mon.raw()
    assert got["summary"].tolist() == [0, -1, 0, 0, M.INF_BITS]
    assert (got["reached_at"] == -1).all() and np.isinf(got["min_d2"]).all()
    assert not got["hit_samples"].any() and not got["unsafe_samples"].any()
    assert (got["sample_log"] == [0, 0, M.INF_BITS]).all()
    mon.score(agents, goals=goals)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mon.raw()["summary"], want["summary"])


# -------------------------------------------------------------------------------------------------
# attached to a context
# -------------------------------------------------------------------------------------------------
CROWD_N, CROWD_STEPS = 33, 12


def test_simulator_monitor_equals_the_host_metrics_on_the_trace(mpclib):
    """33 agents on the crowded lattice (0.6 x the spacing), 12 steps with sub-step records."""
    require_gpu()
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(CROWD_N, spacing_scale=0.6)
    s = sim.Simulator(cfg, states, targets, record=True, monitor=True)
    for _ in range(CROWD_STEPS):
        s.step()
    traj = metrics.trajectories_from_states_json(s.states_json())
    nsub = int(cfg["h"] / cfg["Ts"])
    assert traj.shape == (CROWD_N, CROWD_STEPS * nsub, 6)
    want = metrics.instance_success(traj, targets, 1.0, [0.2, 0.2], "box")
    dmin = metrics.min_pair_distance(traj)
    r = s.monitor.result()
    print(f"host: {want}, min distance {dmin!r}; monitor: {r}")
    assert r["samples"] == CROWD_STEPS * nsub
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == want
    assert r["min_pair_distance_m"] == dmin
    # the case is not a quiet one: the host finds a pair inside d_min, and so does the monitor
    assert dmin < cfg["d_min"], "no pair inside d_min: the crowded case checks nothing"
    p = traj[:, :, :2]
    d2 = ((p[:, None] - p[None]) ** 2).sum(axis=-1)
    iu = np.triu_indices(CROWD_N, k=1)
    inside = d2[iu] < cfg["d_min"] ** 2
    assert r["unsafe_pair_samples"] == int(inside.sum()) > 0
    raw = s.monitor.raw()
    full = d2 < cfg["d_min"] ** 2
    full[np.arange(CROWD_N), np.arange(CROWD_N)] = False
    np.testing.assert_array_equal(raw["unsafe_samples"], full.any(axis=1).sum(axis=1))
    reached = np.linalg.norm(p - targets[:, None, :2], axis=-1) <= 1.0
    first = np.where(reached.any(axis=1), reached.argmax(axis=1), -1)
    np.testing.assert_array_equal(raw["reached_at"], first)


GRID_N, GRID_STEPS = 64, 6


def _grid_swarm():
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(GRID_N, spacing_scale=0.6)
    return cfg, states, targets


def _run_steps(mpclib, attach, first=0, count=GRID_N):
    """GRID_STEPS grid-mode steps in one run_steps call as bench.py drives it (the loop form's options)."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg, states, targets = _grid_swarm()
    ctx = mpclib.Context(cfg)
    ctx.set_variant(4)  # the 16-lane kernel: the one with a loop form
    mon = None
    if attach:
        mon = mpclib.SafetyMonitor(GRID_N, d_min=cfg["d_min"], sample_log=GRID_STEPS)
        ctx.set_monitor(mon)
    a = torch.tensor(states, device=dev)
    b = torch.zeros_like(a)
    out = ctx.alloc_outputs(count)
    out["x"].fill_(float("nan"))
    traj_t = torch.full((count,), -1.0, dtype=torch.float64, device=dev)
    slog = torch.full((GRID_STEPS, count, 2), -7, dtype=torch.int32, device=dev)
    ilog = torch.full((GRID_STEPS, count, 2), -7, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, b, GRID_STEPS, targets=torch.tensor(targets[first:first + count], device=dev),
                      agent_first=first, num_agents=count, knn_k=8, knn_radius=3.0 * cfg["d_min"], x=out["x"],
                      obj=out["obj"], status=out["status"], iters=out["iters"], status_log=slog, iters_log=ilog,
                      traj_t=traj_t, pos_std=1e-3, vel_std=1e-2, noise_seed=5)
    torch.cuda.synchronize()
    res = dict(final=r["final"].cpu().numpy(), x=out["x"].cpu().numpy(), obj=out["obj"].cpu().numpy(),
               status=slog.cpu().numpy(), iters=ilog.cpu().numpy(), traj_t=traj_t.cpu().numpy(),
               form=ctx.launch_form, name=ctx.kernel_name)
    return res, (None if mon is None else mon.raw()), mon


def _solve_loop(mpclib, first=0, count=GRID_N):
    """The same steps as GRID_STEPS impc_solve calls with the monitor attached; returns the monitor's
    raw outputs and the trace of the per-step tables (rows x steps x 6)."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg, states, targets = _grid_swarm()
    ctx = mpclib.Context(cfg)
    ctx.set_variant(4)
    mon = mpclib.SafetyMonitor(GRID_N, d_min=cfg["d_min"], sample_log=GRID_STEPS)
    ctx.set_monitor(mon)
    cur = torch.tensor(states, device=dev)
    nxt = cur.clone()
    out = ctx.alloc_outputs(count)
    out["x"].fill_(float("nan"))
    traj_t = torch.full((count,), -1.0, dtype=torch.float64, device=dev)
    tg = torch.tensor(targets[first:first + count], device=dev)
    trace = []
    for s in range(GRID_STEPS):
        ctx.impc_solve(cur, targets=tg, agent_first=first, num_agents=count, knn_k=8, knn_radius=3.0 * cfg["d_min"],
                       x=out["x"], obj=out["obj"], status=out["status"], iters=out["iters"],
                       next_states=nxt[first:first + count], traj_t=traj_t, pos_std=1e-3, vel_std=1e-2, noise_seed=5,
                       step_index=s)
        trace.append(nxt.cpu().numpy().copy())
        cur, nxt = nxt, cur
        nxt.copy_(cur)  # (the rows outside the agent range carry over)
    torch.cuda.synchronize()
    return mon.raw(), np.stack(trace, axis=1), targets, cfg


def test_run_steps_is_untouched_by_the_monitor(mpclib):
    plain, _, _ = _run_steps(mpclib, attach=False)
    watched, raw, _ = _run_steps(mpclib, attach=True)
    assert plain["form"] == watched["form"] == "loop"
    assert plain["name"] == watched["name"]
    for k in ("final", "x", "obj", "status", "iters", "traj_t"):
        same_bits(watched[k], plain[k], what=k)
    assert not (watched["status"] == -7).any()
    assert raw["summary"][0] == GRID_STEPS


def test_run_steps_monitor_equals_the_host_metrics_and_the_solve_loop(mpclib):
    loop_raw, trace, targets, cfg = _solve_loop(mpclib)
    _, run_raw, mon = _run_steps(mpclib, attach=True)
    _same_bits(run_raw, loop_raw)
    want = metrics.instance_success(trace, targets, 1.0, [0.2, 0.2], "box")
    r = mon.result()
    print(f"host: {want}, monitor: {r}")
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == want
    assert r["min_pair_distance_m"] == metrics.min_pair_distance(trace)
    assert r["samples"] == GRID_STEPS


def test_run_steps_with_fixed_rows_equals_the_solve_loop(mpclib):
    loop_raw, trace, _, cfg = _solve_loop(mpclib, first=8, count=48)
    _, run_raw, _ = _run_steps(mpclib, attach=True, first=8, count=48)
    _same_bits(run_raw, loop_raw)
    assert (run_raw["reached_at"][:8] == -1).all() and (run_raw["reached_at"][56:] == -1).all()
    p = trace[:, :, :2]
    d2 = ((p[:, None] - p[None]) ** 2).sum(axis=-1)
    d2[np.arange(GRID_N), np.arange(GRID_N)] = np.inf
    np.testing.assert_array_equal(run_raw["min_d2"], np.where(d2.min(axis=(1, 2)) <= 36.0, d2.min(axis=(1, 2)), np.inf))


def test_detach_and_refusals(mpclib):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg, states, targets = _grid_swarm()
    ctx = mpclib.Context(cfg)
    mon = mpclib.SafetyMonitor(GRID_N, d_min=cfg["d_min"])
    ctx.set_monitor(mon)
    cur = torch.tensor(states, device=dev)
    out = ctx.alloc_outputs(GRID_N)
    tg = torch.tensor(targets, device=dev)
    kw = dict(targets=tg, knn_k=8, knn_radius=6.0, x=out["x"], status=out["status"])
    ctx.impc_solve(cur, next_states=out["next_states"], **kw)
    ctx.impc_solve(cur, **kw)  # (no next states: nothing to score)
    torch.cuda.synchronize()
    assert mon.raw()["summary"][0] == 1
    # a 2-rank communicator is refused while attached, before the rank joins the group
    comms = mpclib.Comm.local_group(2, 0)
    try:
        half = GRID_N // 2
        with pytest.raises(mpclib.MpccbfError, match="monitor"):
            ctx.run_steps(cur, torch.zeros_like(cur), 2, targets=tg[:half], agent_first=0, num_agents=half, knn_k=8,
                          knn_radius=6.0, comm=comms[0])
    finally:
        for cm in comms:
            cm.close()
    # a table with more rows than the monitor has
    small = mpclib.SafetyMonitor(GRID_N - 1, d_min=cfg["d_min"])
    ctx.set_monitor(small)
    with pytest.raises(mpclib.MpccbfError, match="monitor"):
        ctx.impc_solve(cur, next_states=out["next_states"], **kw)
    # detached: later calls score nothing
    ctx.set_monitor(None)
    ctx.impc_solve(cur, next_states=out["next_states"], **kw)
    torch.cuda.synchronize()
    assert mon.raw()["summary"][0] == 1 and small.raw()["summary"][0] == 0

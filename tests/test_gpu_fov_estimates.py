"""GPU: the FoV IMPC on each observer's own neighbour estimates (Context.set_fov_estimates /
set_fov_estimator; impc_fov_kernel<SLACK, true>) on the inputs of tests/fov_estimate_cases.py.

The reference is the unchanged oracle on a per-observer copy of the state table (oracle_reference
there): statuses equal, objectives within OBJ_TOL relative. "Bit for bit" is parity_rule.same_bits.
Every case stays at the base FoV configuration and at most 33 agents."""
import functools

import numpy as np
import pytest

import fov_estimate_cases as F
import oracle_lib as O
from mpccbf import swarm
from gpu_harness import Solver, require_gpu, same_bits, same_values, to_device, to_host
from parity_rule import check_parity

pytestmark = pytest.mark.gpu

EST_NAME = {"plain": "impc_fov_kernel<false,true>", "slack": "impc_fov_kernel<true,true>"}
OLD_NAME = {"plain": "impc_fov_kernel<false>", "slack": "impc_fov_kernel<true>"}
OUTS = ("x", "status", "obj", "iters", "next_states", "nb_out")


@functools.lru_cache(maxsize=None)
def _fans(ks):
    return F.fan_case(ks, lead_pairs=5, lead_rows=2)


@functools.lru_cache(maxsize=None)
def _oracle(kind, key, setting):
    """The oracle's (status, obj) of a case, computed once per session."""
    case = F.swarm_case(key) if kind == "swarm" else _fans(key)
    return F.oracle_batch(F.config(setting), case)


def _assert_matches_oracle(out, ref, what):
    """Statuses and objectives (the oracle batches here carry no curves)."""
    check_parity(to_host(out), ref, label=what, x=False)


@pytest.mark.parametrize("setting", ["plain", "slack"])
def test_true_positions_attached_are_the_unattached_solve(mpclib, setting):
    """Identity: estimates equal to the table's positions and covariances give the unattached solve
    bit for bit, through the estimate form; after a detach the old kernel runs again."""
    torch = require_gpu()
    c = dict(F.swarm_case(33))
    cov_table = F.random_spd(np.random.default_rng(3), 33)
    c["nb_xy"], c["nb_cov"] = c["states"][c["col"], :2], cov_table[c["col"]]
    s = Solver(mpclib, F.config(setting), c)
    cov = to_device(cov_table)
    plain = s.solve(cov=cov)
    assert s.ctx.kernel_name == OLD_NAME[setting]
    s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
    junk = torch.full_like(cov, 7.5)  # (batch.cov is ignored while attached)
    est = s.solve(cov=junk)
    assert s.ctx.kernel_name == EST_NAME[setting]
    same_bits(est, plain, keys=OUTS, what="attached")
    assert int((plain["status"] == O.OPTIMAL).sum()) > 33  # (the comparison is of solved QPs)
    s.ctx.set_fov_estimates(None)
    again = s.solve(cov=cov)
    assert s.ctx.kernel_name == OLD_NAME[setting]
    same_bits(again, plain, keys=OUTS, what="detached")


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("n", [17, 33])
def test_perturbed_estimates_match_the_oracle(mpclib, oracle, n, setting):
    """Parity: every observer plans from its own estimates (0.2 m off the true positions, random
    covariances). A kernel reading the state table misses by up to 2.5e-2 (n = 17) / 4.7e-3 (33):
    tests/test_fov_estimate_inputs.py."""
    s = Solver(mpclib, F.config(setting), F.swarm_case(n))
    s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
    out = s.solve()
    assert s.ctx.kernel_name == EST_NAME[setting]
    _assert_matches_oracle(out, _oracle("swarm", n, setting), f"swarm{n}/{setting}")
    nb = out["nb_out"].cpu().numpy()
    c = s.case
    for a in range(n):  # nb_col still names the neighbours
        lst = c["col"][c["rp"][a]:c["rp"][a + 1]]
        assert list(nb[a, :len(lst)]) == list(lst) and np.all(nb[a, len(lst):] == -1)


@pytest.mark.parametrize("setting", ["plain", "slack"])
def test_pair_offsets_and_caps(mpclib, oracle, setting):
    """Fans of different sizes in one batch (agent_first > 0, nb_row_ptr[0] > 0), a batch of one and
    every pinned fan size: each observer matches the oracle, so pair offsets are honoured. One
    neighbour over the cap reports what the unattached solve of the same lists reports."""
    cfg = F.config(setting)
    for ks in F.FAN_BATCHES[setting] + (F.FAN_KS[setting],):
        s = Solver(mpclib, cfg, _fans(ks))
        s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
        _assert_matches_oracle(s.solve(), _oracle("fans", ks, setting), f"fans{ks}/{setting}")
    over = F.FAN_OVER_CAP[setting]
    s = Solver(mpclib, cfg, _fans((2, over)))
    today = s.solve(cov=to_device(s.case["cov_table"]))
    s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
    est = s.solve()
    print("over the cap:", est["status"][1].tolist(), today["status"][1].tolist())
    assert s.torch.equal(est["status"][1], today["status"][1]), (est["status"], today["status"])
    assert s.torch.equal(est["iters"][1], today["iters"][1])
    # (the fan under the cap next to it is solved)
    assert int(est["status"][0, 0]) == O.OPTIMAL


def test_slack_order_is_per_pair(mpclib, oracle):
    """The slack weights follow the pair's own covariance: A and B swap the two covariances and
    differ 4.5-fold in the objective; unknown covariances give the list order, which is B's."""
    cfg = F.config(F.SLACK_ORDER)
    cases = F.slack_order_case()
    for name in ("A", "B"):
        s = Solver(mpclib, cfg, cases[name])
        s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
        ref = F.oracle_batch(cfg, cases[name])
        _assert_matches_oracle(s.solve(), ref, f"order/{name}")
    assert abs(F.PINS["order/A"]["obj"][0][0] - 3.27e4) < 50 and abs(F.PINS["order/B"]["obj"][0][0] - 7.28e3) < 5
    s = Solver(mpclib, cfg, cases["A"])
    s.ctx.set_fov_estimates(s.nb_xy, None)
    _assert_matches_oracle(s.solve(), F.oracle_batch(cfg, cases["B"]), "order/none")


@pytest.mark.parametrize("setting", ["plain", "slack"])
def test_guards(mpclib, setting):
    torch = require_gpu()
    c = F.swarm_case(33)
    s = Solver(mpclib, F.config(setting), c)
    # the collision controller has no estimates
    coll = mpclib.Context(swarm.config(15))
    with pytest.raises(mpclib.MpccbfError):
        coll.set_fov_estimates(s.nb_xy, s.nb_cov)
    s.ctx.set_fov_estimates(s.nb_xy, s.nb_cov)
    full = s.solve()
    # estimates belong to fixed pairs: no grid mode while attached
    with pytest.raises(mpclib.MpccbfError):
        s.solve(grid=True)
    # one pair short: the observer whose list reaches it reports ERROR and reads nothing there
    pairs, rp = int(c["rp"][-1]), c["rp"]
    last = max(a for a in range(33) if rp[a] < rp[a + 1])
    assert rp[last + 1] == pairs
    s.ctx.set_fov_estimates(s.nb_xy[:pairs - 1], s.nb_cov[:pairs - 1])
    short = s.solve()
    others = torch.tensor([a for a in range(33) if a != last], device=s.states.device)
    assert int(short["status"][last, 0]) == O.ERROR
    assert not bool((short["status"][others] == O.ERROR).any())
    same_values(short, full, keys=OUTS, what="one pair short", rows=others)
    # one non-finite estimate: its observer alone reports ERROR
    a = int(np.argmax(np.diff(rp)))
    bad_xy = s.nb_xy.clone()
    bad_xy[int(rp[a]) + 1, 1] = float("nan")
    s.ctx.set_fov_estimates(bad_xy, s.nb_cov)
    nan = s.solve()
    others = torch.tensor([b for b in range(33) if b != a], device=s.states.device)
    assert int(nan["status"][a, 0]) == O.ERROR
    same_values(nan, full, keys=OUTS, what="one NaN estimate", rows=others)
    s.ctx.set_fov_estimates(None)
    s.solve(grid=True)  # (detached: grid mode again)


def _loop_state(mpclib, cfg, c, seed):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    n = c["num_agents"]
    ctx = mpclib.Context(cfg)
    est = mpclib.FovEstimator(dict(cfg, pf_num_particles=100), c["rp"], c["col"], n, seed=seed)
    a = to_device(c["states"])
    est.init(a)
    out = ctx.alloc_outputs(n)
    out["x"].fill_(float("nan"))
    return dict(ctx=ctx, est=est, a=a, b=torch.empty_like(a), tg=to_device(c["targets"]),
                traj_t=torch.full((n,), -1.0, dtype=torch.float64, device=dev), out=out,
                slog=torch.full((5, n, 2), -7, dtype=torch.int32, device=dev),
                ilog=torch.full((5, n, 2), -7, dtype=torch.int32, device=dev))


NOISE = dict(pos_std=0.001, vel_std=0.01, noise_seed=20251015)


def _run_attached(mpclib, cfg, c, seed):
    torch = require_gpu()
    L = _loop_state(mpclib, cfg, c, seed)
    L["ctx"].set_fov_estimator(L["est"])
    o = L["out"]
    res = L["ctx"].run_steps(L["a"], L["b"], 5, targets=L["tg"], nb_row_ptr=L["est"].nb_row_ptr,
                             nb_col=L["est"].nb_col, x=o["x"], status=o["status"], obj=o["obj"], iters=o["iters"],
                             status_log=L["slog"], iters_log=L["ilog"], traj_t=L["traj_t"], step_index=0, **NOISE)
    torch.cuda.synchronize()
    assert L["est"].step_index == 5
    L["final"] = res["final"].clone()
    return L


def _run_python_loop(mpclib, cfg, c, seed):
    torch = require_gpu()
    L = _loop_state(mpclib, cfg, c, seed)
    est, o = L["est"], L["out"]
    L["ctx"].set_fov_estimates(est.est_xy, est.est_cov)
    cur, nxt = L["a"], L["b"]
    for s in range(5):
        est.step(cur)
        L["ctx"].impc_solve(cur, nb_row_ptr=est.nb_row_ptr, nb_col=est.nb_col, targets=L["tg"], x=o["x"],
                            status=L["slog"][s], obj=o["obj"], iters=L["ilog"][s], next_states=nxt,
                            traj_t=L["traj_t"], step_index=s, **NOISE)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    L["final"] = cur.clone()
    return L


@pytest.mark.parametrize("setting", ["plain", "slack"])
def test_filter_in_the_loop_is_the_python_loop(mpclib, setting):
    """run_steps with the estimator attached is est.step(states); impc_solve(...) step by step, bit
    for bit, and repeats bit for bit from the same seed."""
    torch = require_gpu()
    cfg, c = F.config(setting), F.swarm_case(33)
    runs = [_run_attached(mpclib, cfg, c, 11), _run_python_loop(mpclib, cfg, c, 11), _run_attached(mpclib, cfg, c, 11)]
    assert runs[0]["ctx"].kernel_name == EST_NAME[setting]
    ref = runs[0]
    # the loop did something: QPs were solved, filters measured their neighbours, states moved
    assert int((ref["slog"] == O.OPTIMAL).sum()) > 5 * 33 and int((ref["est"].flags & 1).sum()) > 0
    assert not torch.equal(ref["final"], ref["a"])
    for name, other in (("python loop", runs[1]), ("second run", runs[2])):
        for k in ("final", "slog", "ilog", "traj_t"):
            same_bits(other[k], ref[k], what=(name, k))
        same_bits(other["out"]["x"], ref["out"]["x"], what=(name, "x"))
        for k in ("est_xy", "est_cov", "particles", "weights", "flags"):
            same_bits(getattr(other["est"], k), getattr(ref["est"], k), what=(name, k))
    # the estimates are not the true positions: the filter, not the table, fed the planner
    true = ref["final"][torch.as_tensor(c["col"], device=ref["final"].device).long(), :2]
    assert float((ref["est"].est_xy[:len(c["col"])] - true).abs().max()) > 1e-3


def test_fov_impc_loop_records_the_example_json(mpclib):
    """FovImpcLoop: 8 robots, 10 steps, the example's slack setting, every robot tracking the robots
    it sees at the start; the record has the example's keys and shapes and no QP ends UNKNOWN or
    ERROR."""
    cfg = swarm.fov_config(20)
    del cfg["slack_mode"]  # (the loop's default: the example's slack setting)
    states, targets = swarm.heading_swarm(8)
    loop = mpclib.FovImpcLoop(cfg, states, targets, seed=5, pos_std=0.001, vel_std=0.01, noise_seed=20251015)
    assert loop.cfg["slack_mode"] == 1 and loop.cfg["slack_cost"] == 1000.0
    loop.run(10)
    assert loop.ctx.kernel_name == EST_NAME["slack"] and loop.estimator.step_index == 10
    st = np.array(loop.status_log)
    print(np.bincount(st.ravel(), minlength=7))
    assert not np.any((st == O.UNKNOWN) | (st == O.ERROR)), np.argwhere(st >= O.ERROR)
    assert np.count_nonzero(st == O.OPTIMAL) > 10 * 8
    rp, col = loop.rp, loop.col
    assert int(rp[-1]) >= 6 and np.diff(rp).max() >= 2  # (there are pairs to track)
    js = loop.to_json()
    nsub = int(cfg["h"] / cfg["Ts"])
    assert js["dt"] == cfg["h"] and js["Ts"] == cfg["Ts"] and set(js["robots"]) == {str(i) for i in range(8)}
    for i in range(8):
        r = js["robots"][str(i)]
        assert set(r) == {"states", "pred_curve", "estimates_mean", "estimates_cov"}
        others = {str(j) for j in col[rp[i]:rp[i + 1]]}  # keyed by the neighbour's id
        assert set(r["estimates_mean"]) == others and set(r["estimates_cov"]) == others
        assert all(np.array(r["estimates_mean"][j]).shape == (10, 3) for j in others)
        assert all(np.array(r["estimates_cov"][j]).shape == (10, 9) for j in others)
        assert np.array(r["states"]).shape == (10 * nsub, 6) and np.all(np.isfinite(np.array(r["states"])))
        assert len(r["pred_curve"]) == 10 and all(len(p) == 1 and np.array(p[0]).shape[1] == 3 for p in r["pred_curve"])

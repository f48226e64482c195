"""GPU status parity on closed-loop-evolved swarms of the bench workload (BASELINE config 3:
4096 agents, K = 15, 8 nearest within 3 d_min, the example's trajectory fallback and state noise),
and on captured regression cases.

The QPs the bench counts are the ones these states produce: from step ~14 on, agents that came
within d_min of a neighbour get INFEASIBLE QPs (ConnectivityIMPCCBF.cpp:199-211 then breaks out of
the IMPC loop), and iteration-1 QPs with two active neighbours need the phase-1 certificate. Every
agent whose status is not OPTIMAL, plus a seeded sample of 256 OPTIMAL ones, is re-solved by the
oracle on the same states and must agree: statuses equal, objectives within 1e-4.
"""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from gpu_harness import require_gpu, to_host
from mpccbf import swarm
from parity_rule import check_parity

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _check_agents(cfg, states, targets, agents, g_status, g_obj, g_x=None, cov=None, lists=None):
    """lists: per agent its neighbour list (default: the 8 nearest within 3 d_min)."""
    p = O.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    rp, col = swarm.knn_csr(states, 8, 3.0 * cfg["d_min"])
    ref = {}
    for a in agents:
        nb = lists[a] if lists is not None else col[rp[a]:rp[a + 1]]
        ref[int(a)] = O.impc_optimize(p, states, a, nb, refs[a], covs=cov)
    check_parity(dict(status=g_status, obj=g_obj, x=g_x), ref, agents, x=g_x is not None)


def test_regression_cases_match_oracle(mpclib):
    """Captured instances that once failed (tests/golden/regress_cases.json): agent 0 against its
    listed neighbours, the GPU's statuses / objectives / control points against the oracle."""
    torch = require_gpu()
    cases = json.load(open(os.path.join(HERE, "golden", "regress_cases.json")))["cases"]
    # (records beyond the oracle's reach are held by the penalty objective in test_gpu_fov_params.py)
    cases = [c for c in cases if c.get("reference") != "penalty"]
    dev = torch.device("cuda", 0)
    assert any(c.get("controller") == "fov_slack" for c in cases)
    assert any(c.get("controller") == "collision_slack" for c in cases)
    for case in cases:
        states = np.array(case["states"])
        n = len(states)
        cov = None
        if case.get("controller") == "fov_slack":  # FovBezierIMPCCBF in slack mode (config 5)
            cfg = swarm.fov_config(case["k_hor"], slack_mode=1, slack_cost=case["slack_cost"],
                                   slack_decay_rate=case["slack_decay_rate"])
            cov = np.tile(np.array(case["cov"]), (n, 1))
        elif case.get("controller") == "collision_slack":  # ConnectivityIMPCCBF in slack mode
            cfg = swarm.config(case["k_hor"], slack_mode=1, slack_cost=case["slack_cost"],
                               slack_decay_rate=case["slack_decay_rate"])
        else:
            cfg = swarm.config(case["k_hor"])
        targets = np.tile(np.array(case["target"]), (n, 1))
        rp = np.array([0, n - 1] + [n - 1] * (n - 1), np.int32)
        col = np.arange(1, n, dtype=np.int32)
        ctx = mpclib.Context(cfg)
        out = ctx.alloc_outputs(1)
        ctx.impc_solve(torch.tensor(states, device=dev), torch.tensor(rp, device=dev),
                       torch.tensor(col, device=dev), targets=torch.tensor(targets[:1], device=dev),
                       num_agents=1, cov=None if cov is None else torch.tensor(cov, device=dev), **out)
        torch.cuda.synchronize()
        g = to_host(out)
        _check_agents(cfg, states, targets, [0], g["status"], g["obj"], g["x"], cov=cov,
                      lists={0: np.arange(1, n, dtype=np.int32)})


@pytest.mark.parametrize("n,snaps,kernel", [
    (4096, (16, 20, 27), "impc_sep_kernel<1,1,false,256>"),
    # config 4's rank share: the default variant runs the one-agent-per-wave kernel, whose
    # deferrals (more active sides, the PDIP, phase 1) go to the capacity launch
    (1024, (16, 20, 27, 40), "impc_wide_kernel<256>")])
def test_bench_workload_statuses_match_oracle(mpclib, n, snaps, kernel):
    """Every non-OPTIMAL agent and a seeded sample of 256 OPTIMAL ones of the closed-loop-evolved
    swarm against the oracle, at the launch size of config 3 (the 16-lane kernel) and of config
    4's rank share (the default variant's one-agent-per-wave kernel)."""
    torch = require_gpu()
    cfg = swarm.config(15)
    states_h, targets_h = swarm.lattice_swarm(n)
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    tg = torch.tensor(targets_h, device=dev)
    out = ctx.alloc_outputs(n)
    traj_t = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    steps = max(snaps) + 3
    status_log = torch.empty((steps, n, 2), dtype=torch.int32, device=dev)
    iters_log = torch.empty((steps, n, 2), dtype=torch.int32, device=dev)
    cur = torch.tensor(states_h, device=dev)
    alt = torch.empty_like(cur)
    common = dict(targets=tg, knn_k=8, knn_radius=3.0 * cfg["d_min"], x=out["x"], obj=out["obj"],
                  traj_t=traj_t, pos_std=0.001, vel_std=0.01, noise_seed=20251015)
    s = 0
    saved = {}

    def advance(k):
        nonlocal s, cur, alt
        r = ctx.run_steps(cur, alt, k, status_log=status_log[s:s + k], iters_log=iters_log[s:s + k],
                          step_index=s, **common)
        if r["final"] is not cur:
            cur, alt = alt, cur
        s += k

    for b in list(snaps) + [steps]:
        if b > s:
            advance(b - s)
        if b < steps:
            st_in = cur.cpu().numpy().copy()
            advance(1)
            saved[b] = (st_in, out["obj"].cpu().numpy().copy())
    torch.cuda.synchronize()
    assert ctx.kernel_name == kernel, ctx.kernel_name
    slog = status_log.cpu().numpy()
    ilog = iters_log.cpu().numpy()
    attempted = ~((slog == 5) & (ilog == 0))
    # no capacity errors and no undecided QPs anywhere in the run
    assert not np.any((slog == 4) & attempted), "ERROR status in the bench workload"
    assert not np.any((slog == 5) & attempted), np.argwhere((slog == 5) & attempted)[:5]
    rng = np.random.default_rng(1234)
    for b in snaps:
        st_in, obj = saved[b]
        stat = slog[b]
        nonopt = np.nonzero(np.any(stat != 0, axis=1))[0]
        opt = np.nonzero(np.all(stat == 0, axis=1))[0]
        sample = rng.choice(opt, size=min(256, len(opt)), replace=False)
        assert len(nonopt) > 0 or b < 14, f"step {b}: expected infeasible agents in the transient"
        _check_agents(cfg, st_in, targets_h, np.concatenate([nonopt, sample]), stat, obj)

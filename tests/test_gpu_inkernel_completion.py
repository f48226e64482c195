"""GPU: the in-kernel completion of the 16-lane main launch (impc_sep_kernel<1,1,false,256>).

The kernel runs the lean pipeline (fast start + dual active set) inline and finishes the agents it
does not settle with an out-of-line call of the full pipeline in the same wave. The reference is the
two-launch lean path (mpccbf_options.lean: IMPC_SEP_LEAN + IMPC_QUEUE1), which hands the same agents
to a fallback launch that runs the same full pipeline on the same inputs.

Scenario: test_gpu_active_store.py's 64 agents, grid lists (8 nearest within 6 m), set_variant(4) (at
64 agents the default variant takes the one-agent-per-wave kernel), dual_as_steps=1: a QP that needs
a second active-set step has to take the completion, and then reports more than one step (the active
set's one plus the interior-point solver's), which is how the tests see from the outputs who went
through it. On the 0.45 x lattice (test_gpu_context_reuse.py's; CBF sides active, INFEASIBLE agents
included), not the 0.6 x one: at 0.6 x (and every seed / scale tried between 1.0 x and 0.5 x) no
agent settles iteration 0 and takes the completion in iteration 1, and the default seed has no wave
with exactly one group through the completion; at 0.45 x with the default seed 45 agents take it, in
2 waves alone and in 14 waves with others, agents 6 and 48 in iteration 1 only.

Bounds: statuses and step counts identical. Objectives, curves and states are the same arithmetic on
the same inputs but not the same code object — the completion is the full pipeline compiled as a
function with its rows in registers, the fallback launch the same source as a 64-thread kernel with
its rows in LDS, and how multiply-adds are contracted and ordered is the compiler's choice in each (measured: one
solve's objectives differ by up to 1.5e-14 relative, its control points by 5.2e-13, 10 closed-loop
steps' final states by 2.5e-12). They are held to 1e-7 relative, the suite's bound between two exact
solver paths (test_gpu_active_store.py).
"""
import functools

import numpy as np
import pytest

from gpu_harness import require_gpu, run_oracle, to_host
from mpccbf import swarm
from parity_rule import check_parity, check_routes_agree

pytestmark = pytest.mark.gpu

N, K, RADIUS, SCALE = 64, 8, 6.0, 0.45
SEP16 = 4
MAIN = "impc_sep_kernel<1,1,false,256>"
LEAN = "impc_sep_kernel<1,1,false,256,false,true>"
NOISE = dict(pos_std=1e-3, vel_std=1e-3, noise_seed=11)


def _scenario():
    states, targets = swarm.lattice_swarm(N, seed=swarm.SEED)
    states[:, :2] *= SCALE
    return states, targets


def _context(mpclib, lean):
    ctx = mpclib.Context(swarm.config(15), dual_as_steps=1, lean=lean)
    ctx.set_variant(SEP16)
    return ctx


@functools.lru_cache(maxsize=None)
def _solve(mpclib, lean):
    """One impc_solve of the scenario (computed once per path, never modified)."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    states, targets = _scenario()
    ctx = _context(mpclib, lean)
    out = ctx.alloc_outputs(N)
    out["nb_out"] = torch.full((N, 16), -7, dtype=torch.int32, device=dev)
    ctx.impc_solve(torch.tensor(states, device=dev), targets=torch.tensor(targets, device=dev), knn_k=K,
                   knn_radius=RADIUS, **out)
    torch.cuda.synchronize()
    assert ctx.kernel_name == (LEAN if lean else MAIN), ctx.kernel_name
    return to_host(out)


def test_one_solve_matches_the_two_launch_lean_path(mpclib):
    got, ref = _solve(mpclib, False), _solve(mpclib, True)
    went = (got["iters"] > 1).any(axis=1)
    per_wave = np.bincount(np.flatnonzero(went) // 4, minlength=N // 4)
    late = (got["status"][:, 0] == mpclib.OPTIMAL) & (got["iters"][:, 0] <= 1) & (got["iters"][:, 1] > 1)
    print(f"agents through the completion: {np.flatnonzero(went).tolist()}, waves with one: "
          f"{np.count_nonzero(per_wave == 1)}, with two or more: {np.count_nonzero(per_wave >= 2)}, "
          f"iteration 0 settled and iteration 1 not: {np.flatnonzero(late).tolist()}, statuses "
          f"{np.bincount(got['status'].ravel() + 1).tolist()}")
    np.testing.assert_array_equal(got["status"], ref["status"])
    np.testing.assert_array_equal(got["iters"], ref["iters"])
    np.testing.assert_array_equal(got["nb_out"], ref["nb_out"])
    for k in ("obj", "x", "next_states"):
        check_routes_agree(got[k], ref[k], k + " against the lean path")
    # the three situations of the hand-over
    assert np.any(per_wave == 1), "no wave with exactly one group through the completion"
    assert np.any(per_wave >= 2), "no wave with two or more groups through the completion"
    assert np.any(late), "no agent whose iteration 0 settled and whose iteration 1 took the completion"
    assert not np.all(went), "no agent the lean pipeline settled"
    # both against the oracle, on the lists the kernels built
    states, targets = _scenario()
    rp, col = swarm.knn_csr(states, K, RADIUS)
    for a in range(N):
        np.testing.assert_array_equal(got["nb_out"][a][got["nb_out"][a] >= 0], col[rp[a]:rp[a + 1]])
    cfg = swarm.config(15)
    agents = list(range(N))
    oracle = run_oracle(cfg, states, targets, rp, col, agents)
    for g in (got, ref):
        check_parity(g, oracle, agents)


def _loop(mpclib, lean, steps=10):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    states, targets = _scenario()
    ctx = _context(mpclib, lean)
    a = torch.tensor(states, device=dev)
    b = torch.empty_like(a)
    out = ctx.alloc_outputs(N)
    out["x"].fill_(float("nan"))
    traj_t = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    log = torch.full((steps, N, 2), -7, dtype=torch.int32, device=dev)
    ilog = torch.full((steps, N, 2), -7, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, b, steps, targets=torch.tensor(targets, device=dev), knn_k=K, knn_radius=RADIUS,
                      x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"], status_log=log,
                      iters_log=ilog, traj_t=traj_t, **NOISE)
    torch.cuda.synchronize()
    assert ctx.kernel_name == (LEAN if lean else MAIN), ctx.kernel_name
    return dict(final=r["final"].cpu().numpy(), x=out["x"].cpu().numpy(), obj=out["obj"].cpu().numpy(),
                traj_t=traj_t.cpu().numpy(), log=log.cpu().numpy(), ilog=ilog.cpu().numpy())


def test_closed_loop_matches_the_two_launch_lean_path(mpclib):
    """10 steps with noise and traj_t: a second table insert or a twice-advanced traj_t of a completed
    agent would change the following steps' neighbour lists or the kept curves' next states."""
    got, ref = _loop(mpclib, False), _loop(mpclib, True)
    went = (got["ilog"] > 1).any(axis=2)
    print(f"agents through the completion per step: {went.sum(axis=1).tolist()}")
    assert not np.any(got["log"] == -7)
    assert went[:-1].any(), "no agent took the completion before the last step: nothing to carry over"
    np.testing.assert_array_equal(got["log"], ref["log"])
    np.testing.assert_array_equal(got["ilog"], ref["ilog"])
    np.testing.assert_array_equal(got["traj_t"], ref["traj_t"])
    for k in ("final", "x", "obj"):
        check_routes_agree(got[k], ref[k], k + " against the lean path")

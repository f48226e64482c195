"""GPU: the loop form of the 16-lane main launch (FORM_LOOP) computes what the generic form computes.

Both forms are instantiations of one source in one library; the launch plan takes the loop form for
the closed-loop launch as the benchmark passes it and the generic form as soon as one optional
output is asked for. nb_out is such an output and changes no other: the same run_steps with and
without it must agree bit for bit — the forms differ in which tests are compiled, not in any
expression on a kept path — so every comparison here is torch.equal, step by step.

Swarm and starting curves: launch_form_cases.py (test_launch_form_inputs.py proves with the oracle
that it holds an agent without a neighbour, agents with active CBF rows in both iterations, and
INFEASIBLE agents with and without a stored curve to fall back to).
"""
import functools

import numpy as np
import pytest

import launch_form_cases as L
from gpu_harness import require_gpu, same_bits

pytestmark = pytest.mark.gpu

KEYS = ("states", "x", "obj", "status", "iters", "traj_t")


@functools.lru_cache(maxsize=None)
def _run(mpclib, shape, generic, calls, dual_as_steps=0):
    """The closed loop of L.STEPS steps in `calls` run_steps calls (a tuple of step counts; every
    call after the first continues the neighbour tables), as the loop form's launch or, with nb_out
    added, as the generic form's. Returns after every call a dict of clones: the state table, x, obj,
    status, iters, traj_t, and the calls' status / iteration logs."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    _, ns, first, count = next(s for s in L.SHAPES if s[0] == shape)
    cfg = L.config()
    states, targets = L.scenario(ns)
    x0, t0 = L.initial_curves(cfg, states, first, count)
    ctx = mpclib.Context(cfg, dual_as_steps=dual_as_steps)
    ctx.set_variant(L.SEP16)
    tables = [torch.tensor(states, device=dev), torch.zeros((ns, 6), dtype=torch.float64, device=dev)]
    out = ctx.alloc_outputs(count)
    out["x"].copy_(torch.tensor(x0, device=dev))
    traj_t = torch.tensor(t0, device=dev)
    tg = torch.tensor(targets[first:first + count], device=dev)
    extra = dict(nb_out=torch.full((count, 16), -7, dtype=torch.int32, device=dev)) if generic else {}
    snaps, step = [], 0
    for i, k in enumerate(calls):
        log = torch.full((k, count, 2), -7, dtype=torch.int32, device=dev)
        ilog = torch.full((k, count, 2), -7, dtype=torch.int32, device=dev)
        r = ctx.run_steps(tables[0], tables[1], k, targets=tg, agent_first=first, num_agents=count, knn_k=L.K,
                          knn_radius=L.RADIUS, x=out["x"], obj=out["obj"], status=out["status"], iters=out["iters"],
                          status_log=log, iters_log=ilog, traj_t=traj_t, step_index=step, continue_tables=i > 0,
                          **L.NOISE, **extra)
        torch.cuda.synchronize()
        assert ctx.kernel_name == L.MAIN, ctx.kernel_name
        assert ctx.launch_form == ("generic" if generic else "loop"), ctx.launch_form
        if r["final"] is not tables[0]:
            tables.reverse()
        step += k
        # (status / iters: the logs take their place in run_steps; the buffers stay as allocated)
        snaps.append(dict(states=tables[0].clone(), x=out["x"].clone(), obj=out["obj"].clone(), status=log,
                          iters=ilog, traj_t=traj_t.clone()))
    return snaps


def _same(got, ref):
    """Every snapshot bit for bit (NaN by bit pattern: x of an agent without a curve; INFEASIBLE
    objectives)."""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        same_bits(g, r, keys=KEYS, what=i)
        assert not bool((g["status"] == -7).any()), i


@pytest.mark.parametrize("shape", [s[0] for s in L.SHAPES])
def test_step_by_step_equals_the_generic_form(mpclib, shape):
    """Ten closed-loop steps with noise, one run_steps call per step (each continuing the tables):
    every output and the state table after every step."""
    calls = (1,) * L.STEPS
    got, ref = _run(mpclib, shape, False, calls), _run(mpclib, shape, True, calls)
    _same(got, ref)
    if shape in ("n64", "sub"):
        torch = require_gpu()
        st = torch.stack([g["status"][0] for g in got]).cpu().numpy()  # (steps, agents, 2)
        it = torch.stack([g["iters"][0] for g in got]).cpu().numpy()
        tt = got[0]["traj_t"].cpu().numpy()
        print(f"{shape}: statuses {[int(v) for v in np.bincount(st.ravel() + 1)]}, "
              f"agents with steps in both iterations at some step: {int(((it > 0).all(axis=2)).any(axis=0).sum())}")
        assert ((it > 0).all(axis=2)).any(), "no agent with active-set steps in both iterations"
        assert (st[0, :, 0] == mpclib.INFEASIBLE).any(), "no INFEASIBLE agent at step 0"
        assert (tt < 0).any() and (tt > 0).any(), "step 0: no agent still without a curve / none with one"


def test_one_call_and_a_continued_call_equal_the_generic_form(mpclib):
    """The same ten steps as one call, and as a first call of four steps and a continue_tables call
    of six: the logs of every step, and the same end as the step-by-step loop."""
    require_gpu()
    for calls in ((L.STEPS,), (4, L.STEPS - 4)):
        got, ref = _run(mpclib, "n64", False, calls), _run(mpclib, "n64", True, calls)
        _same(got, ref)
        end = _run(mpclib, "n64", False, (1,) * L.STEPS)[-1]
        same_bits(got[-1], end, keys=("states", "x", "obj", "traj_t"), what=calls)


def test_completion_from_the_loop_form(mpclib):
    """dual_as_steps = 1: a QP that needs a second active-set step takes impc_sep_complete, one
    function called the same way from both forms — identical statuses, step counts and values."""
    torch = require_gpu()
    calls = (1,) * L.STEPS
    got = _run(mpclib, "n64", False, calls, dual_as_steps=1)
    ref = _run(mpclib, "n64", True, calls, dual_as_steps=1)
    _same(got, ref)
    went = torch.stack([(g["iters"][0] > 1).any(dim=1) for g in got])
    print(f"agents through the completion per step: {went.sum(dim=1).tolist()}")
    assert bool(went[0].any()) and bool(went[1:].any()), "no agent took the completion"
    assert not bool(went.all()), "no agent the lean pipeline settled"

"""CPU: the launch plan's choice of the loop form (FORM_LOOP of the 16-lane main launch), and the
oracle's proof that the GPU test's swarm holds the situations it is meant to compare.

1. The qualifying launch — grid lists, targets, traj_t, every output of the closed loop, the next
   step's table, and none of the optional inputs / outputs — gets the new kernel id under the
   unchanged name. Each condition flipped on its own gives the id and the name the plan gives
   without any launch fact, i.e. today's.
2. On launch_form_cases.scenario() at step 0: an agent without a neighbour, an agent whose two IMPC
   iterations both have an active CBF row (so both dual active-set solves take steps), and agents
   whose first QP is INFEASIBLE with a stored curve (they fall back to it) and without (they hold).
"""
import numpy as np
import pytest

import launch_form_cases as L
from mpccbf import _lib as mlib
from mpccbf import swarm


def _plan(mpclib, launch, cfg=None, **kw):
    kw = dict(dict(variant=L.SEP16, num_agents=L.N, knn_k=L.K), **kw)
    return mpclib._lib.host_launch_plan(cfg or L.config(), launch=launch, **kw)


def test_the_qualifying_launch_takes_the_loop_form(mpclib):
    lib = mpclib._lib
    p = _plan(mpclib, lib.LOOP_LAUNCH)
    assert (p["kernel_id"], p["launch_form"], p["kernel_name"]) == (lib.IMPC_SEP_LOOP, "loop", L.MAIN)
    g = _plan(mpclib, {})
    assert (g["kernel_id"], g["launch_form"], g["kernel_name"]) == (lib.IMPC_SEP, "generic", L.MAIN)
    # the same launch shape and clock: the plan differs in the id and the form alone
    for k in ("block_size", "agents_per_block", "clock_waves", "store", "defers", "capacity_name"):
        assert p[k] == g[k] == mpclib._lib.host_launch_plan(L.config(), variant=L.SEP16, num_agents=L.N, knn_k=L.K)[k]
    # beyond the one-agent-per-wave kernel's range the default variant qualifies as well
    big = _plan(mpclib, lib.LOOP_LAUNCH, variant=0, num_agents=4096, wide_max=1024)
    assert (big["kernel_id"], big["launch_form"], big["kernel_name"]) == (lib.IMPC_SEP_LOOP, "loop", L.MAIN)


FLIPS = [(f, {f: not v}, {}, None) for f, v in sorted(mlib.LOOP_LAUNCH.items())]
FLIPS.remove(("targets", {"targets": False}, {}, None))
FLIPS += [
    ("refs", {"targets": False}, {}, None),  # (no targets: the reference-tail form)
    ("csr", {}, dict(csr=True), None),
    ("store", {}, dict(store=True), None),
    ("connectivity", {}, dict(connectivity=True), None),
    ("lean", {}, dict(lean=1), None),
    ("slack", {}, {}, dict(slack_mode=1)),
    ("wide 64", {}, dict(variant=0, num_agents=64, wide_max=1024), None),
    ("wide 1024", {}, dict(variant=0, num_agents=1024, wide_max=1024), None),
    ("wide variant", {}, dict(variant=5), None),
    ("dense", {}, dict(variant=3), None),
    ("fov", {}, {}, dict(cbf_mode=1, num_pieces=4, k_hor=20)),
]


@pytest.mark.parametrize("tag,flip,kw,over", FLIPS, ids=[f[0] for f in FLIPS])
def test_one_condition_flipped_falls_back_to_todays_kernel(mpclib, tag, flip, kw, over):
    lib = mpclib._lib
    cfg = swarm.config(over.pop("k_hor", 15), **over) if over else L.config()
    facts = dict(lib.LOOP_LAUNCH, **flip)
    got = _plan(mpclib, facts, cfg=cfg, **kw)
    today = _plan(mpclib, {}, cfg=cfg, **kw)  # (no fact given: never the loop form)
    plain = mpclib._lib.host_launch_plan(cfg, **dict(dict(variant=L.SEP16, num_agents=L.N, knn_k=L.K), **kw))
    assert got["launch_form"] == today["launch_form"] == "generic", tag
    assert got["kernel_id"] == today["kernel_id"] != lib.IMPC_SEP_LOOP, tag
    assert got["kernel_name"] == today["kernel_name"] == plain["kernel_name"], tag
    # the facts alone never leave the 16-lane kernel: only the launch's other properties do
    if not kw and not over:
        assert got["kernel_id"] == lib.IMPC_SEP and got["kernel_name"] == L.MAIN


def test_unknown_fact_is_refused(mpclib):
    with pytest.raises(ValueError):
        _plan(mpclib, {"stamps": True})


def test_the_swarm_holds_every_situation(mpclib, oracle):
    cfg = L.config()
    states, targets = L.scenario()
    rp, col = swarm.knn_csr(states, L.K, L.RADIUS)
    p = oracle.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    nnb = np.diff(rp)
    assert nnb[L.N - 1] == 0 and np.count_nonzero(nnb == 0) == 1, "one agent without a neighbour"
    none = np.zeros(0, np.int32)
    both, stored, hold = [], [], []
    for a in range(L.N):
        r = oracle.impc_optimize(p, states, a, col[rp[a]:rp[a + 1]], refs[a])
        if r["status"][0] == oracle.INFEASIBLE:
            (stored if L.has_stored_curve(a) else hold).append(a)
        elif list(r["status"]) == [oracle.OPTIMAL, oracle.OPTIMAL] and nnb[a] > 0:
            # a CBF row is active at an iteration's optimum exactly when leaving the rows out lowers
            # the optimum: the dual active set then takes at least one step in that iteration
            free = oracle.impc_optimize(p, states, a, none, refs[a])
            if all(r["obj"][it] > free["obj"][it] + 1e-6 * max(1.0, abs(free["obj"][it])) for it in range(2)):
                both.append(a)
    print(f"active CBF row in both iterations: {both}; INFEASIBLE with a stored curve: {stored}; without: {hold}")
    assert both and stored and hold
    # the sub-range holds them too, and the 15- and 17-agent tables at least the two fallbacks' kinds
    _, _, first, count = L.SHAPES[-1]
    inside = lambda v: [a for a in v if first <= a < first + count]  # noqa: E731
    assert inside(both) and inside(stored) and inside(hold)
    # the stored curves: constant at the agent's position, evaluation time 0
    x, t = L.initial_curves(cfg, states, 0, L.N)
    assert x.shape == (L.N, mpclib._lib.host_operators(cfg)["n"])
    assert np.all(t[::2] == 0.0) and np.all(t[1::2] == -1.0) and np.all(np.isnan(x[1::2])) and not np.any(np.isnan(x[::2]))
    curve = oracle.eval_curve(p, x[0], 0.05, 0)
    np.testing.assert_allclose(np.ravel(curve)[:2], states[0, :2], rtol=0, atol=1e-12)

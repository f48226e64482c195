"""GPU parity of the IMPC kernels off the base configuration: full reference trajectories
(mpccbf_batch.refs), cbf_horizon 1 .. 8, impc_iter 1 / 3 / 4, yaw motion with asymmetric per-channel
limits, and the exact-reduction options — each against the CPU oracle under the parity rule of
test_gpu_parity.py (statuses equal, objectives within 1e-4 relative, control points within 1e-5),
for every agent of every case. Every case asserts the kernel instantiation that ran.
The inputs' own properties (status mixes, live rows, tight box rows) are asserted on the CPU in
test_param_space_inputs.py."""
import numpy as np
import pytest

import oracle_lib as O
import param_space_cases as C
from mpccbf import swarm
from gpu_harness import fresh_outputs, require_gpu, run_gpu, run_oracle, to_host
from mpccbf._lib import MpccbfError
from parity_rule import check_parity, same_bits

pytestmark = pytest.mark.gpu

DENSE16, DENSE64 = "impc_kernel<6,16,4>", "impc_kernel<6,64,4>"
SEP, WIDE = "impc_sep_kernel<1,1,false,256>", "impc_wide_kernel<256>"
SLACK = "impc_sep_kernel<1,2,true,256>"
FOV = "impc_fov_kernel<false>"
# variant -> the instantiation for 64 agents of the separable controller (0: share-adaptive, one
# agent per wave at this count)
NAMES = {3: DENSE16, 4: SEP, 5: WIDE, 0: WIDE}

_refs = {}


def oracle_ref(key, cfg, st, tg, rp, col, refs=None):
    """The oracle's result of every agent, computed once per case and shared by the tests and
    variants that use it; every attempted QP has a verdict, so no agent is left out."""
    if key not in _refs:
        _refs[key] = run_oracle(cfg, st, tg, rp, col, list(range(len(rp) - 1)), refs=refs)
        assert C.attempted_unknown(_refs[key]) == [], key
    return _refs[key]


def check_variants(mpclib, torch, cfg, st, tg, rp, col, ref, names, refs=None, **opts):
    """Solve with every variant of `names` (variant -> expected kernel name) and compare all
    agents with the oracle."""
    agents = list(range(len(st)))
    for variant, name in names.items():
        ctx = mpclib.Context(cfg, **opts)
        if variant:
            ctx.set_variant(variant)
        g = run_gpu(ctx, st, tg, rp, col, torch, refs=refs)
        assert ctx.kernel_name == name, (variant, ctx.kernel_name)
        check_parity(g, ref, agents)


def lattice():
    st, tg = C.crowded(64, 0.45, 5)
    return (st, tg) + swarm.knn_csr(st, 8, 6.0)


def solve(ctx, torch, st, rp=None, col=None, **kw):
    """impc_solve on host arrays; returns the outputs as numpy."""
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.tensor(a, device=dev)  # noqa: E731
    n = kw.get("num_agents", len(st))
    out = ctx.alloc_outputs(n)
    ctx.impc_solve(t(st), t(rp), t(col), **{k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()},
                   **out)
    torch.cuda.synchronize()
    return to_host(out)


OUT_KEYS = ("status", "obj", "x", "iters", "next_states")


# ---- 1. reference trajectories ------------------------------------------------------------------

@pytest.mark.parametrize("spd_f", [1, 3, 8, 15])
def test_refs_match_oracle(mpclib, spd_f):
    """mpccbf_batch.refs (the reference-tail branch of agent_linear_term / agent_linear_term_lanes):
    nr = 3 spd_f = 3, 9, 24, 45 reference entries — below one 8-entry load chunk, not a multiple
    of 8, a multiple, and more than the 10 constant lanes of a 16-lane group take in two passes.
    The one-agent-per-wave kernel still applies at spd_f = 15 (hot operator prefix 1,952 <= 2,048
    doubles)."""
    torch = require_gpu()
    st, tg, rp, col = lattice()
    cfg = swarm.config(15, spd_f=spd_f)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    ref = oracle_ref(("refs", spd_f), cfg, st, tg, rp, col, refs)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, ref, NAMES, refs=refs)


def test_refs_fov_and_slack_match_oracle(mpclib):
    """refs through the FoV kernel (G = 64 lanes of the constant's striding) and the collision
    slack kernel, spd_f = 5 (nr = 15)."""
    torch = require_gpu()
    cfg = swarm.fov_config(20, spd_f=5)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    refs = C.moving_refs(st, tg, 20, cfg["h"], 7)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref("refs fov", cfg, st, tg, rp, col, refs),
                   {0: FOV}, refs=refs)
    cfg = swarm.config(15, spd_f=5, slack_mode=1)
    st, tg = C.crowded(64, 0.45, 21)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref("refs slack", cfg, st, tg, rp, col, refs),
                   {0: SLACK}, refs=refs)


@pytest.mark.parametrize("variant", [3, 4, 5])
def test_refs_of_replicated_target_equal_targets_call(mpclib, variant):
    """refs = the target replicated over the horizon is the targets= call's problem: the same
    statuses, objectives within 1e-10 relative (Qr r sums the entries Qt t holds pre-summed)."""
    torch = require_gpu()
    st, tg, rp, col = lattice()
    cfg = swarm.config(15)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    a = run_gpu(ctx, st, tg, rp, col, torch)
    b = run_gpu(ctx, st, tg, rp, col, torch, refs=swarm.refs_from_targets(tg, 15))
    assert ctx.kernel_name == NAMES[variant]
    np.testing.assert_array_equal(a["status"], b["status"])
    ok = a["status"] == O.OPTIMAL
    assert ok.sum() >= 98
    np.testing.assert_allclose(b["obj"][ok], a["obj"][ok], rtol=1e-10, atol=0)


@pytest.mark.parametrize("spd_f", [3, 8])
def test_refs_entries_before_the_tail_are_not_read(mpclib, spd_f):
    """Only the last spd_f samples of refs enter the cost: 1e6 in every earlier entry leaves every
    output bit-identical (collision layouts and the FoV kernel)."""
    torch = require_gpu()
    for fov in (False, True):
        if fov:
            cfg = swarm.fov_config(20, spd_f=spd_f)
            st, tg = C.fov_swarm()
            rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
        else:
            cfg = swarm.config(15, spd_f=spd_f)
            st, tg, rp, col = lattice()
        K = cfg["k_hor"]
        refs = C.moving_refs(st, tg, K, cfg["h"], 7)
        head = refs.copy()
        head[:, :3 * (K - spd_f)] = 1e6
        for variant in ((0,) if fov else (4, 5)):
            ctx = mpclib.Context(cfg)
            if variant:
                ctx.set_variant(variant)
            a = run_gpu(ctx, st, tg, rp, col, torch, refs=refs)
            b = run_gpu(ctx, st, tg, rp, col, torch, refs=head)
            assert ctx.kernel_name == (FOV if fov else NAMES[variant])
            assert np.count_nonzero(a["status"][:, 0] == O.OPTIMAL) >= 50
            same_bits(a, b, keys=OUT_KEYS)


@pytest.mark.parametrize("variant", [3, 4, 5])
def test_refs_are_indexed_by_the_batch_local_agent(mpclib, variant):
    """agent_first = 12, num_agents = 40 with a 40-row refs equals rows 12 .. 51 of the full solve
    bit for bit: row i of refs belongs to agent agent_first + i."""
    torch = require_gpu()
    st, tg, rp, col = lattice()
    cfg = swarm.config(15, spd_f=3)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    full = solve(ctx, torch, st, rp, col, refs=refs)
    # (the 40 rows lead a 64-row buffer whose other rows hold 1e6: a kernel indexing refs by the
    # global agent reads those, inside the buffer)
    buf = torch.full((64, 45), 1e6, dtype=torch.float64, device=torch.device("cuda", 0))
    buf[:40] = torch.tensor(refs[12:52], device=buf.device)
    part = solve(ctx, torch, st, rp[12:53].copy(), col, refs=buf[:40], agent_first=12, num_agents=40)
    assert ctx.kernel_name == NAMES[variant]
    assert np.count_nonzero(full["status"][12:52, 0] == O.OPTIMAL) >= 20
    same_bits({k: v[12:52] for k, v in full.items()}, part, keys=OUT_KEYS)


def _loop_with_refs(ctx, torch, st0, steps, **kw):
    """`steps` control steps issued one by one through impc_solve (grid neighbours), tables
    swapped by the caller; returns (final states, per-step statuses)."""
    a, b = st0.clone(), st0.clone()
    n = st0.shape[0]
    out = ctx.alloc_outputs(n)
    log = []
    for _ in range(steps):
        ctx.impc_solve(a, knn_k=8, knn_radius=6.0, x=out["x"], status=out["status"], obj=out["obj"],
                       iters=out["iters"], next_states=b, **kw)
        log.append(out["status"].clone())
        a, b = b, a
    torch.cuda.synchronize()
    return a.cpu().numpy(), torch.stack(log).cpu().numpy()


def test_run_steps_with_refs_matches_step_by_step(mpclib):
    """mpccbf_run_steps with refs over 3 steps == three impc_solve calls, bit for bit."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    st, tg, _, _ = lattice()
    cfg = swarm.config(15, spd_f=3)
    refs = torch.tensor(C.moving_refs(st, tg, 15, cfg["h"], 7), device=dev)
    st0 = torch.tensor(st, device=dev)
    ctx = mpclib.Context(cfg)
    ref_states, ref_log = _loop_with_refs(ctx, torch, st0, 3, refs=refs)
    a, b = st0.clone(), torch.empty_like(st0)
    out = ctx.alloc_outputs(64)
    log = torch.full((3, 64, 2), -9, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, b, 3, refs=refs, knn_k=8, knn_radius=6.0, x=out["x"], obj=out["obj"], status_log=log)
    torch.cuda.synchronize()
    assert ctx.kernel_name == WIDE
    same_bits(r["final"].cpu().numpy(), ref_states)
    same_bits(log.cpu().numpy(), ref_log)
    assert np.count_nonzero(ref_log[:, :, 0] == O.OPTIMAL) > 64


# ---- 2. CBF horizon -----------------------------------------------------------------------------

@pytest.mark.parametrize("cbf_h", [1, 3, 5, 8])
def test_cbf_horizon_lattice_matches_oracle(mpclib, cbf_h):
    """cbf_horizon 1 .. 8 (MAX_CBF_H) on the crowded lattice; at 8, iteration 1 of most agents is
    INFEASIBLE with up to 64 rows staged (certificate path). The operators' hot prefix grows by
    108 doubles per CBF sample: 2,024 at cbf_horizon = 5 still fits the one-agent-per-wave kernel's
    2,048, 2,348 at 8 does not — there the default falls back to the 16-lane kernel and variant 5
    (not a 16-lane variant) to the dense 64-lane instantiation."""
    torch = require_gpu()
    st, tg, rp, col = lattice()
    cfg = swarm.config(15, cbf_horizon=cbf_h)
    names = {4: SEP, 5: WIDE, 0: WIDE} if cbf_h < 8 else {4: SEP, 5: DENSE64, 0: SEP}
    ref = oracle_ref(("cbf_h", cbf_h), cfg, st, tg, rp, col)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, ref, names)


def test_cbf_horizon_3_grid_mode_equals_csr(mpclib):
    """Grid mode with 8 neighbours starts deferring at cbf_horizon = 3 (8 x 3 > 16 row slots,
    impc_launch_plan): the grid solve equals the CSR solve on the same lists."""
    torch = require_gpu()
    st, tg, rp, col = lattice()
    cfg = swarm.config(15, cbf_horizon=3)
    for variant in (4, 5):
        ctx = mpclib.Context(cfg)
        ctx.set_variant(variant)
        g_csr = solve(ctx, torch, st, rp, col, targets=tg)
        g = solve(ctx, torch, st, targets=tg, knn_k=8, knn_radius=6.0)
        assert ctx.kernel_name == NAMES[variant]
        np.testing.assert_array_equal(g["status"], g_csr["status"])
        ok = g["status"] == O.OPTIMAL
        np.testing.assert_allclose(g["obj"][ok], g_csr["obj"][ok], rtol=1e-10, atol=1e-9)
        check_parity(g, oracle_ref(("cbf_h", 3), cfg, st, tg, rp, col), list(range(64)))


@pytest.mark.parametrize("n_ring,cbf_h", [(12, 8), (20, 4), (40, 3)])
def test_ring_iteration1_rows_use_the_capacity_launch(mpclib, n_ring, cbf_h):
    """Agent 0 inside a ring of n_ring robots, all its neighbours: 53 / 72 / 120 live iteration-1
    CBF rows (test_param_space_inputs.py), beyond the 16 slots of the main kernels and within the
    capacity launch's 128: no ERROR, parity for every agent. (At cbf_horizon = 8 the operators do
    not fit the one-agent-per-wave kernel: the default is the 16-lane kernel, and variant 5 the
    dense 64-lane instantiation, which holds the rows itself.)"""
    torch = require_gpu()
    cfg = swarm.config(15, cbf_horizon=cbf_h)
    st, tg, rp, col = C.ring(n_ring)
    ref = oracle_ref(("ring", n_ring, cbf_h), cfg, st, tg, rp, col)
    assert list(ref[0]["status"]) == [O.OPTIMAL, O.OPTIMAL]
    for variant, name in (((4, SEP), (0, WIDE)) if cbf_h < 8 else ((0, SEP), (5, DENSE64))):
        ctx = mpclib.Context(cfg)
        ctx.set_variant(variant)
        g = run_gpu(ctx, st, tg, rp, col, torch)
        assert ctx.kernel_name == name
        assert not np.any(g["status"] == O.ERROR), np.argwhere(g["status"] == O.ERROR)[:5]
        check_parity(g, ref, list(range(n_ring + 1)))


def test_ring_beyond_the_capacity_launch_reports_error(mpclib):
    """40 ring neighbours at cbf_horizon = 5: 157 live iteration-1 rows on agent 0, more than the
    capacity launch's 128 (include/mpccbf.h: beyond that the QP reports ERROR). Agent 0:
    [OPTIMAL, ERROR], x the iteration-0 curve (the last OPTIMAL iteration's); every other agent as
    the oracle has it."""
    torch = require_gpu()
    cfg = swarm.config(15, cbf_horizon=5)
    st, tg, rp, col = C.ring(40)
    ref = oracle_ref(("ring", 40, 5), cfg, st, tg, rp, col)
    for variant, name in ((4, SEP), (0, WIDE)):
        ctx = mpclib.Context(cfg)
        ctx.set_variant(variant)
        g = run_gpu(ctx, st, tg, rp, col, torch)
        assert ctx.kernel_name == name
        assert list(g["status"][0]) == [O.OPTIMAL, O.ERROR], g["status"][0]
        ro = ref[0]["obj"][0]
        assert abs(g["obj"][0, 0] - ro) <= 1e-4 * max(1.0, abs(ro))
        assert np.max(np.abs(g["x"][0] - ref[0]["x"][0][:36])) <= 1e-5
        others = list(range(1, 41))
        check_parity({k: v[1:] for k, v in g.items()}, [ref[i] for i in others], list(range(40)))


def test_slack_mode_beyond_cbf_horizon_2_is_a_clean_error(mpclib):
    """Collision slack mode with cbf_horizon = 3 has no kernel (a neighbour's lane holds two
    samples' rows): the solve returns MPCCBF_ERR_CAPACITY (-3) with a message and launches
    nothing — the outputs keep their sentinel — and the library goes on working."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg = swarm.config(15, slack_mode=1, cbf_horizon=3)
    st, tg, rp, col = lattice()
    ctx = mpclib.Context(cfg)
    assert ctx.kernel_name == ""
    out = fresh_outputs(ctx, 64, fill=-77)
    with pytest.raises(MpccbfError) as e:
        ctx.impc_solve(torch.tensor(st, device=dev), torch.tensor(rp, device=dev), torch.tensor(col, device=dev),
                       targets=torch.tensor(tg, device=dev), **out)
    torch.cuda.synchronize()
    msg = str(e.value)
    assert msg.startswith("mpccbf error -3: ") and len(msg) > len("mpccbf error -3: "), msg
    for k, v in out.items():
        assert bool(torch.all(v == -77)), k
    ok = mpclib.Context(dict(cfg, cbf_horizon=2))
    g = run_gpu(ok, st, tg, rp, col, torch)
    assert ok.kernel_name == SLACK and np.all(g["status"][:, 0] == O.OPTIMAL)


def test_fov_slack_mode_beyond_cbf_horizon_2_is_refused_at_create(mpclib):
    """The FoV controller refuses slack_mode with cbf_horizon = 3 earlier still: mpccbf_create
    returns MPCCBF_ERR_INVALID_ARGUMENT (-1) with a message naming the limit, so there is no
    context to solve with (launch_impc_fov's own check is never reached)."""
    require_gpu()
    cfg = swarm.fov_config(20, slack_mode=1, slack_cost=1000.0, cbf_horizon=3)
    with pytest.raises(MpccbfError) as e:
        mpclib.Context(cfg)
    msg = str(e.value)
    assert msg.startswith("mpccbf error -1: ") and "cbf_horizon <= 2" in msg, msg
    assert mpclib.Context(dict(cfg, cbf_horizon=2)).kernel_name == "impc_fov_kernel<true>"


@pytest.mark.parametrize("cbf_h", [1, 3])
def test_fov_cbf_horizon_matches_oracle(mpclib, cbf_h):
    """FoV controller without slack at cbf_horizon 1 and 3, the full observed-neighbour lists (at
    most 3 observed neighbours here: 4 kinds x 3 x 3 rows stay within the kernel's rows)."""
    torch = require_gpu()
    cfg = swarm.fov_config(20, cbf_horizon=cbf_h)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref(("fov cbf_h", cbf_h), cfg, st, tg, rp, col),
                   {0: FOV})


# ---- 3. IMPC iterations -------------------------------------------------------------------------

def _cases_iter(impc_iter):
    st, tg, rp, col = lattice()
    yield "lattice", swarm.config(15, impc_iter=impc_iter), st, tg, rp, col, NAMES
    st, tg = C.crowded(64, 0.45, 21)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    yield "slack", swarm.config(15, impc_iter=impc_iter, slack_mode=1), st, tg, rp, col, {0: SLACK}
    cfg = swarm.fov_config(20, impc_iter=impc_iter)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    yield "fov", cfg, st, tg, rp, col, {0: FOV}


@pytest.mark.parametrize("impc_iter", [1, 3, 4])
def test_impc_iter_outputs_and_parity(mpclib, impc_iter):
    """impc_iter 1, 3 and 4 (outputs indexed ai * impc_iter + it; the one-agent-per-wave kernel
    writes iterations >= 2 as they finish): every entry of the n x impc_iter outputs is written,
    nothing past their end, parity with the oracle, x the last OPTIMAL iteration's curve."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    for tag, cfg, st, tg, rp, col, names in _cases_iter(impc_iter):
        ref = oracle_ref(("iter", tag, impc_iter), cfg, st, tg, rp, col)
        n = len(st)
        for variant, name in names.items():
            ctx = mpclib.Context(cfg)
            if variant:
                ctx.set_variant(variant)
            out, full = fresh_outputs(ctx, n, guard=8, fill=-77)
            assert out["status"].shape == (n, impc_iter) and out["obj"].shape == (n, impc_iter)
            ctx.impc_solve(torch.tensor(st, device=dev), torch.tensor(rp, device=dev), torch.tensor(col, device=dev),
                           targets=torch.tensor(tg, device=dev), **out)
            torch.cuda.synchronize()
            assert ctx.kernel_name == name, (tag, variant, ctx.kernel_name)
            g = to_host(full)
            for k, v in g.items():
                assert np.all(v[n:] == -77), (tag, variant, k)  # the guard rows
                assert not np.any(v[:n] == -77), (tag, variant, k, np.argwhere(v[:n] == -77)[:4])
            check_parity({k: v[:n] for k, v in g.items()}, ref, list(range(n)))


def test_run_steps_impc_iter_3_matches_step_by_step(mpclib):
    """3 native closed-loop steps with impc_iter = 3 and a status_log (count x impc_iter per
    step) == the step-by-step loop, bit for bit."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    st, tg, _, _ = lattice()
    cfg = swarm.config(15, impc_iter=3)
    st0, tgd = torch.tensor(st, device=dev), torch.tensor(tg, device=dev)
    ctx = mpclib.Context(cfg)
    ref_states, ref_log = _loop_with_refs(ctx, torch, st0, 3, targets=tgd)
    a, b = st0.clone(), torch.empty_like(st0)
    out = ctx.alloc_outputs(64)
    log = torch.full((3 + 1, 64, 3), -9, dtype=torch.int32, device=dev)
    ilog = torch.full((3 + 1, 64, 3), -9, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, b, 3, targets=tgd, knn_k=8, knn_radius=6.0, x=out["x"], obj=out["obj"],
                      status_log=log[:3], iters_log=ilog[:3])
    torch.cuda.synchronize()
    assert ctx.kernel_name == WIDE
    same_bits(r["final"].cpu().numpy(), ref_states)
    lg = log.cpu().numpy()
    same_bits(lg[:3], ref_log)
    assert np.all(lg[3] == -9) and np.all(ilog.cpu().numpy()[3] == -9)  # nothing past 3 steps' logs
    assert not np.any(ilog.cpu().numpy()[:3] == -9)
    assert np.count_nonzero(np.all(ref_log == O.OPTIMAL, axis=2)) > 64


# ---- 4. yaw channel and asymmetric limits -------------------------------------------------------

def _yaw_case(rate):
    st, tg = C.crowded(64, 0.55, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    st, tg = C.with_yaw(st, tg, 11, rate)
    return st, tg, rp, col


@pytest.mark.parametrize("rate", [0.9, 2.4])
def test_yaw_and_asymmetric_limits_match_oracle(mpclib, rate):
    """Yaw, yaw rate and yaw target nonzero with limits that differ per channel and per side
    (ASYM). rate 0.9: all OPTIMAL, 27 / 14 / 20 agents with a tight box row in x / y / yaw.
    rate 2.4: 24 agents' yaw rate lies below v_min[2], infeasible by the constant rows of the yaw
    channel alone, 40 OPTIMAL. All layouts and collision slack mode."""
    torch = require_gpu()
    st, tg, rp, col = _yaw_case(rate)
    cfg = swarm.config(15, **C.ASYM)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref(("yaw", rate), cfg, st, tg, rp, col), NAMES)
    cfg = swarm.config(15, slack_mode=1, **C.ASYM)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref(("yaw slack", rate), cfg, st, tg, rp, col),
                   {0: SLACK})


def test_cbf_filter_uses_each_channels_own_bound(mpclib):
    """filter_edge: four agents whose optimum lies on a CBF row with b just below the filter's
    threshold max_u -a^T u, on the a_min[0], a_max[0], a_min[1] and a_max[1] side in turn
    (test_param_space_inputs.py). A filter that formed the threshold from another channel's or the
    other side's narrower bound would drop the row and return another curve. (A wider wrong bound
    only keeps more rows, which changes no result: the collision rows' yaw coefficient is 0, so
    which bound channel 2 reads cannot show.)"""
    torch = require_gpu()
    st, tg, rp, col = C.filter_edge()
    cfg = swarm.config(15, **C.ASYM)
    ref = oracle_ref("filter edge", cfg, st, tg, rp, col)
    assert all(list(r["status"]) == [O.OPTIMAL, O.OPTIMAL] for r in ref)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, ref, NAMES)
    cfg = swarm.config(15, slack_mode=1, **C.ASYM)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref("filter edge slack", cfg, st, tg, rp, col),
                   {0: SLACK})


def test_fov_asymmetric_limits_match_oracle(mpclib):
    torch = require_gpu()
    cfg = swarm.fov_config(20, **C.ASYM)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    check_variants(mpclib, torch, cfg, st, tg, rp, col, oracle_ref("fov asym", cfg, st, tg, rp, col), {0: FOV})


# ---- 5. combined --------------------------------------------------------------------------------

def test_combined_case_matches_oracle(mpclib):
    """ASYM limits, cbf_horizon = 3, impc_iter = 3, spd_f = 5, moving refs and yaw (rate 2.4) at
    once: 39 x all OPTIMAL, 24 x INFEASIBLE, 1 x (OPTIMAL, INFEASIBLE, -)."""
    torch = require_gpu()
    st, tg, rp, col = _yaw_case(2.4)
    cfg = swarm.config(15, cbf_horizon=3, impc_iter=3, spd_f=5, **C.ASYM)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    ref = oracle_ref("combined", cfg, st, tg, rp, col, refs)
    check_variants(mpclib, torch, cfg, st, tg, rp, col, ref, {4: SEP, 5: WIDE, 0: WIDE}, refs=refs)


# ---- 6. exact-reduction options -----------------------------------------------------------------

def _reduction_case(mpclib, torch, k_hor, name, variant=0, **opts):
    st, tg = C.crowded(64, 0.5, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    cfg = swarm.config(k_hor)
    ref = oracle_ref(("opt", k_hor), cfg, st, tg, rp, col)
    base = run_gpu(mpclib.Context(cfg), st, tg, rp, col, torch)
    ctx = mpclib.Context(cfg, **opts)
    if variant:
        ctx.set_variant(variant)
    g = run_gpu(ctx, st, tg, rp, col, torch)
    assert ctx.kernel_name == name, ctx.kernel_name
    np.testing.assert_array_equal(g["status"], base["status"])
    ok = base["status"] == O.OPTIMAL
    assert ok.sum() >= 120
    err = np.abs(g["obj"][ok] - base["obj"][ok]) / np.maximum(1.0, np.abs(base["obj"][ok]))
    assert err.max() <= 1e-8, err.max()
    check_parity(g, ref, list(range(64)))


@pytest.mark.parametrize("k_hor,name", [(10, DENSE16), (15, DENSE64)])
def test_keep_redundant_changes_no_result(mpclib, k_hor, name):
    """mpccbf_options.keep_redundant: every box row kept (57 rows at k_hor = 10, 87 at 15 — more
    than 16 per channel, so the dense layouts run). With caller lists the default variant takes
    impc_kernel<6,64,4> at both (at 57 rows the 16-lane instantiation has 7 CBF row slots and no
    capacity launch). `name` is what variant 3 runs: impc_kernel<6,16,4> below 64 rows (these
    inputs' at most 4 live rows fit its 7 slots), impc_kernel<6,64,4> from 64 on. Each: same
    statuses as the default context, objectives within 1e-8 relative, parity with the oracle."""
    _reduction_case(mpclib, require_gpu(), k_hor, DENSE64, keep_redundant=True)
    _reduction_case(mpclib, require_gpu(), k_hor, name, variant=3, keep_redundant=True)


@pytest.mark.parametrize("k_hor", [10, 15])
def test_no_cbf_filter_changes_no_result(mpclib, k_hor):
    """mpccbf_options.no_cbf_filter: every CBF row staged (8 neighbours x 2 samples = the 16 slots
    at most); the rows the filter drops are implied by the box rows, so nothing changes."""
    _reduction_case(mpclib, require_gpu(), k_hor, WIDE, no_cbf_filter=True)

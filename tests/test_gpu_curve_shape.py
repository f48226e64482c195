"""GPU parity of the IMPC kernels over the horizon k_hor and the curve's shape (num_pieces,
num_control_points, continuity_upto_degree, piece_max_parameter) — each case of
curve_shape_cases.py against the CPU oracle under the parity rule of test_gpu_parity.py (statuses
equal, objectives within 1e-4 relative, control points within 1e-5, every agent), with the kernel
instantiation asserted for every variant that runs, and next_states against the Bernstein evaluation
(numpy) of the device's own control points at t = h. The dense-layout capacity cases (more CBF rows
than the 16-lane instantiation's 64 - m slots) and the shapes no kernel takes are at the end.
The inputs' own properties are asserted on the CPU in test_curve_shape_inputs.py."""
import numpy as np
import pytest

import curve_shape_cases as S
import oracle_lib as O
import param_space_cases as P
from mpccbf import swarm
from gpu_harness import fresh_outputs, require_gpu, run_gpu, to_host
from mpccbf._lib import MpccbfError
from parity_rule import check_parity, same_bits

pytestmark = pytest.mark.gpu

_refs = {}


def oracle_ref(c):
    """The oracle's result of every agent of a case, computed once; every attempted QP has a
    verdict, so no agent is left out."""
    key = (c.cfg["k_hor"], tuple(sorted((k, str(v)) for k, v in c.cfg.items())), str(c.swarm))
    if key not in _refs:
        _refs[key] = S.oracle_batch(c.cfg, *S.inputs(c))
        assert P.attempted_unknown(_refs[key]) == [], c.name
    return _refs[key]


def check_next_states(cfg, st, g):
    """next_states = the device's own curve at t = h (position and velocity; numpy Bernstein
    evaluation, the tolerance of test_next_state_is_curve_at_h), or the current state where the
    agent has no curve (x is NaN)."""
    have = np.any(g["status"] == O.OPTIMAL, axis=1)
    for a in range(len(st)):
        if have[a]:
            np.testing.assert_allclose(g["next_states"][a], S.curve_state(cfg, g["x"][a], cfg["h"]), rtol=0,
                                       atol=1e-9, err_msg=str(a))
        else:
            assert np.all(np.isnan(g["x"][a]))
            np.testing.assert_array_equal(g["next_states"][a], st[a])
    return int(have.sum())


def check_case(mpclib, torch, c):
    """Solve the case with every variant of its names and hold each to the oracle."""
    st, tg, rp, col = S.inputs(c)
    ref = oracle_ref(c)
    out = {}
    for variant, name in c.names.items():
        ctx = mpclib.Context(c.cfg, **c.opts)
        if variant:
            ctx.set_variant(variant)
        g = run_gpu(ctx, st, tg, rp, col, torch)
        assert ctx.kernel_name == name, (c.name, variant, ctx.kernel_name)
        assert g["x"].shape == (len(st), c.sizes[2])
        eo, ex = check_parity(g, ref, list(range(len(st))), label=f"{c.name} variant {variant}")
        print(f"\nCURVE_SHAPE {c.name} variant {variant} {ctx.kernel_name} obj_err {eo:.3e} x_err {ex:.3e} "
              f"errors {int(np.count_nonzero(g['status'] == O.ERROR))}")
        assert check_next_states(c.cfg, st, g) >= 1
        out[variant] = g
    return out


# ---- horizon ------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", S.HORIZON, ids=[c.name for c in S.HORIZON])
def test_horizon_matches_oracle(mpclib, c):
    """k_hor 1 .. 16 on the base curve, variants 0 / 3 / 4 / 5: 3 .. 51 box rows; up to k_hor = 15
    the separable kernels (one to 16 rows per channel and lane group); at 16, the base
    configuration's own horizon, 17 rows per channel: the dense layouts, the 64-lane instantiation
    by default and the 16-lane one for variant 3."""
    check_case(mpclib, require_gpu(), c)


@pytest.mark.parametrize("c", S.BEYOND16, ids=[c.name for c in S.BEYOND16])
def test_horizon_beyond_16_matches_oracle(mpclib, c):
    """Four pieces, k_hor 17 / 20 / 21: 54, 63 and 66 box rows (from 64 on every variant runs the
    64-lane instantiation)."""
    check_case(mpclib, require_gpu(), c)


@pytest.mark.parametrize("c", S.SLACK_CASES, ids=[c.name for c in S.SLACK_CASES])
def test_slack_mode_horizon_matches_oracle(mpclib, c):
    """Slack mode at k_hor 2 and 16 and, on four pieces, 21 (22 box rows per channel: two row
    slots per lane): every QP OPTIMAL, the oracle's objective (slack cost included) and curve.
    (k_hor = 16 is the case that showed the oracle's polish keeping an inconsistent active set:
    agent 45's curve 3.2e-3 from the device's, which an independent KKT solve confirmed to 5e-10;
    DESIGN.md section 5. With the polish corrected the worst control-point error here is ~1e-9.)"""
    g = check_case(mpclib, require_gpu(), c)[0]
    assert np.all(g["status"] == O.OPTIMAL)


@pytest.mark.parametrize("c", S.FOV_CASES, ids=[c.name for c in S.FOV_CASES])
def test_fov_horizon_matches_oracle(mpclib, c):
    """FoV controller at k_hor 2 / 6 / 12 / 21 (9 .. 75 box rows) and in slack mode at 12."""
    g = check_case(mpclib, require_gpu(), c)[0]
    assert np.all(g["status"] == O.OPTIMAL)


# ---- curve shape --------------------------------------------------------------------------------

@pytest.mark.parametrize("c", S.SHAPES, ids=[c.name for c in S.SHAPES])
def test_curve_shape_matches_oracle(mpclib, c):
    """One piece (n = 12); two pieces of three control points (n = 18, the run-time control-point
    count); pieces of 0.37 (samples off the piece boundaries); five, six and ten pieces (the
    one-agent-per-wave kernel's LDS stage holds the operators of five, not of six; the piece lookup
    beyond eight pieces)."""
    check_case(mpclib, require_gpu(), c)


def test_continuity_degree_4_is_bit_identical_to_degree_3(mpclib):
    """continuity_upto_degree = 4 on cubic pieces gives the operators of degree 3
    (test_curve_shape_inputs.py): every output equals the base context's bit for bit."""
    torch = require_gpu()
    st, tg, rp, col = S.lattice()
    for variant, name in S.SEPARABLE.items():
        res = []
        for cfg in (swarm.config(15), swarm.config(15, continuity_upto_degree=4)):
            ctx = mpclib.Context(cfg)
            ctx.set_variant(variant)
            res.append(run_gpu(ctx, st, tg, rp, col, torch))
            assert ctx.kernel_name == name
        assert np.count_nonzero(res[0]["status"][:, 0] == O.OPTIMAL) == 50
        same_bits(*res, keys=("status", "obj", "x", "iters", "next_states"))


def test_fov_five_control_points_matches_oracle(mpclib):
    """FoV controller on three pieces of five control points (nz = 15, n = 45, 69 box rows): the
    kernel reads the control-point count at run time (five Voronoi rows per neighbour, the curve
    evaluation's loop) and the piece count only through the operators, so the shape is taken and
    must match the oracle — never a wrong curve under an OPTIMAL status."""
    g = check_case(mpclib, require_gpu(), S.FOV_C5)[0]
    assert np.all(g["status"] == O.OPTIMAL)


# ---- shapes no kernel takes ---------------------------------------------------------------------

@pytest.mark.parametrize("c", S.REFUSED, ids=[c.name for c in S.REFUSED])
def test_shapes_without_a_kernel_are_a_clean_error(mpclib, c):
    """Reduced dimensions other than 6 (collision) and 15 (FoV): the solve returns
    MPCCBF_ERR_CAPACITY (-3) with a message and launches nothing — the outputs keep their sentinel
    — whatever the variant, and the library goes on working."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    st, tg, rp, col = S.inputs(c)
    for variant in (0, 3, 4, 5):
        ctx = mpclib.Context(c.cfg)
        if variant:
            ctx.set_variant(variant)
        assert ctx.nz == c.sizes[1] and ctx.n == c.sizes[2]
        if c.names is not None:
            assert ctx.kernel_name == ""
        out = fresh_outputs(ctx, len(st), fill=-77)
        with pytest.raises(MpccbfError) as e:
            ctx.impc_solve(torch.tensor(st, device=dev), torch.tensor(rp, device=dev), torch.tensor(col, device=dev),
                           targets=torch.tensor(tg, device=dev), **out)
        torch.cuda.synchronize()
        msg = str(e.value)
        assert msg.startswith("mpccbf error -3: ") and "no kernel instantiation" in msg, msg
        for k, v in out.items():
            assert bool(torch.all(v == -77)), k
    base = S.FOV_CASES[2] if c.swarm == "fov" else S.HORIZON[-2]
    g = run_gpu(mpclib.Context(base.cfg), *S.inputs(base), torch)
    assert np.count_nonzero(g["status"][:, 0] == O.OPTIMAL) >= 50


# ---- stored-curve evaluation --------------------------------------------------------------------

def test_stored_curve_with_three_control_points_is_followed_across_the_piece_boundary(mpclib):
    """Closed-loop semantics (traj_t) on two pieces of three control points, 0.75 each: a first
    solve stores every feasible agent's curve; then every agent's velocity leaves the box (no QP is
    feasible), so each falls back to its stored curve at traj_t + h, with traj_t set before, at and
    beyond the piece boundary and at the curve's end. next_states, the ten sub-step records and
    traj_t equal the numpy evaluation of the stored control points; x is left as stored."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    c = S.SHAPES[2]
    assert c.name == "c3K16"
    cfg = c.cfg
    st, tg, rp, col = S.inputs(c)
    n, nsub = len(st), int(round(cfg["h"] / cfg["Ts"]))
    tend = cfg["num_pieces"] * cfg["piece_max_parameter"]
    step = cfg["Ts"] * int(cfg["h"] / cfg["Ts"])  # the advance of a control step (the last sub-step's time)
    t_set = np.array([0.1, 0.66, 0.68, 0.7, 0.72, 0.74, 0.75, 1.3, 1.45, 1.5])[np.arange(n) % 10]
    bad = st.copy()
    bad[:, 3] = 2.5
    t = lambda a, dt=None: torch.tensor(a, device=dev, dtype=dt)  # noqa: E731
    for variant, name in c.names.items():
        ctx = mpclib.Context(cfg)
        if variant:
            ctx.set_variant(variant)
        out = ctx.alloc_outputs(n)
        traj_t = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        sub = torch.zeros((n, nsub, 6), dtype=torch.float64, device=dev)
        kw = dict(nb_row_ptr=t(rp), nb_col=t(col), targets=t(tg), traj_t=traj_t, substeps=sub, **out)
        ctx.impc_solve(t(st), **kw)
        torch.cuda.synchronize()
        assert ctx.kernel_name == name
        x0 = out["x"].cpu().numpy().copy()
        fresh = np.any(out["status"].cpu().numpy() == O.OPTIMAL, axis=1)
        assert fresh.sum() == 48
        tt = traj_t.cpu().numpy()
        assert np.all(tt[fresh] == cfg["h"]) and np.all(tt[~fresh] == -1.0)
        # the fresh curves' own sub-steps (this step's solution, run-time control-point count)
        s1, nx1 = sub.cpu().numpy(), out["next_states"].cpu().numpy()
        for a in np.flatnonzero(fresh):
            for k in range(nsub - 1):
                np.testing.assert_allclose(s1[a, k], S.curve_state(cfg, x0[a], cfg["Ts"] * (k + 1)), rtol=0, atol=1e-9)
            np.testing.assert_allclose(nx1[a], S.curve_state(cfg, x0[a], cfg["h"]), rtol=0, atol=1e-9)
            np.testing.assert_array_equal(s1[a, nsub - 1], nx1[a])
        # fall back to the stored curves
        traj_t.copy_(t(np.where(fresh, t_set, -1.0)))
        ctx.impc_solve(t(bad), **kw)
        torch.cuda.synchronize()
        status = out["status"].cpu().numpy()
        assert np.all(status[:, 0] == O.INFEASIBLE)
        x1, s2, nx2, t2 = out["x"].cpu().numpy(), sub.cpu().numpy(), out["next_states"].cpu().numpy(), traj_t.cpu().numpy()
        np.testing.assert_array_equal(x1[fresh], x0[fresh])
        crossed = 0
        for a in np.flatnonzero(fresh):
            tn = min(t_set[a] + step, tend)
            assert t2[a] == tn
            np.testing.assert_allclose(nx2[a], S.curve_state(cfg, x0[a], tn), rtol=0, atol=1e-9, err_msg=str(a))
            for k in range(1, nsub):
                exp = S.curve_state(cfg, x0[a], min(t_set[a] + cfg["Ts"] * k, tend))
                np.testing.assert_allclose(s2[a, k - 1], exp, rtol=0, atol=1e-9, err_msg=str((a, k)))
            crossed += int(t_set[a] < 0.75 < tn)
        assert crossed >= 10
        # agents without a stored curve hold their position at zero velocity
        hold = np.flatnonzero(~fresh)
        np.testing.assert_array_equal(nx2[hold, :3], bad[hold, :3])
        assert np.all(nx2[hold, 3:] == 0.0) and np.all(t2[hold] == -1.0)


# ---- dense-layout capacity ----------------------------------------------------------------------

@pytest.mark.parametrize("c", S.CAPACITY, ids=[c.name for c in S.CAPACITY])
def test_default_context_holds_the_rows_the_16_lane_layout_cannot(mpclib, c):
    """Configurations whose box rows leave impc_kernel<6,16,4> 1 or 13 CBF row slots, on inputs
    with agents beyond them (4 live rows; 16 staged rows without the filter; 24 and 55 on the
    ring's agent 0): the default context runs impc_kernel<6,64,4>, reports no ERROR and matches the
    oracle for every agent."""
    torch = require_gpu()
    g = check_case(mpclib, torch, c)[0]
    assert not np.any(g["status"] == O.ERROR), np.argwhere(g["status"] == O.ERROR)[:5]
    if c.opts:  # the exact-reduction options change no status of the default context
        base = run_gpu(mpclib.Context(c.cfg), *S.inputs(c), torch)
        np.testing.assert_array_equal(g["status"], base["status"])
    if c.swarm != "lattice":
        assert list(g["status"][0]) == [O.OPTIMAL, O.OPTIMAL]


def test_forced_16_lane_layout_reports_error_beyond_its_slots(mpclib):
    """Variant 3 asks for impc_kernel<6,16,4>: at k_hor = 16 (51 box rows) it has 13 CBF row slots
    and no capacity launch (include/mpccbf.h). The ring's agent 0 has 24 live iteration-1 rows:
    [OPTIMAL, ERROR], x the iteration-0 curve (the last OPTIMAL iteration's); every other agent as
    the oracle has it."""
    torch = require_gpu()
    c = S.FORCED16
    st, tg, rp, col = S.inputs(c)
    ref = oracle_ref(c)
    ctx = mpclib.Context(c.cfg)
    ctx.set_variant(3)
    g = run_gpu(ctx, st, tg, rp, col, torch)
    assert ctx.kernel_name == S.DENSE16
    assert list(g["status"][0]) == [O.OPTIMAL, O.ERROR], g["status"][0]
    # agent 0 by the rule over its iteration 0 alone (the oracle has no capacity: its iteration 1 is OPTIMAL)
    first = dict(status=ref[0]["status"][:1], obj=ref[0]["obj"][:1], x=ref[0]["x"][:1])
    check_parity(dict(status=g["status"][:, :1], obj=g["obj"][:, :1], x=g["x"]), [first], [0])
    np.testing.assert_allclose(g["next_states"][0], S.curve_state(c.cfg, g["x"][0], c.cfg["h"]), rtol=0, atol=1e-9)
    check_parity({k: v[1:] for k, v in g.items()}, ref[1:], list(range(12)))


def test_default_variant_on_grid_lists(mpclib):
    """Grid lists at k_hor = 16: with 6 nearest neighbours (12 rows at most against 13 slots) the
    default context keeps impc_kernel<6,16,4>, with 8 it runs impc_kernel<6,64,4>; both equal the
    caller-list solve on the same lists and report the kernel that ran."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg = S.config(16)
    st, tg = P.crowded(64, 0.45, 5)
    for k, name in ((6, S.DENSE16), (8, S.DENSE64)):
        rp, col = swarm.knn_csr(st, k, 6.0)
        ctx = mpclib.Context(cfg)
        out = ctx.alloc_outputs(64)
        ctx.impc_solve(torch.tensor(st, device=dev), targets=torch.tensor(tg, device=dev), knn_k=k, knn_radius=6.0,
                       **out)
        torch.cuda.synchronize()
        assert ctx.kernel_name == name
        g = to_host(out)
        g_csr = run_gpu(ctx, st, tg, rp, col, torch)
        assert ctx.kernel_name == S.DENSE64
        np.testing.assert_array_equal(g["status"], g_csr["status"])
        assert not np.any(g["status"] == O.ERROR)
        ok = g["status"] == O.OPTIMAL
        assert ok.sum() >= 80
        err = np.abs(g["obj"][ok] - g_csr["obj"][ok]) / np.maximum(1.0, np.abs(g_csr["obj"][ok]))
        assert err.max() <= 1e-8, err.max()

"""GPU: the batched IMPC with connectivity-maintenance rows (Context.set_connectivity,
mpccbf_set_connectivity) against the CPU reference built from the oracle (conn_impc_ref.py) on the
seeded teams of conn_impc_cases.py: parity where the lambda2 row binds, where CLF rows bind and
where the added rows make the QP INFEASIBLE; team shapes across the wave and block boundaries;
options; detach; the closed loop (run_steps, ranks, the simulator)."""
import threading

import numpy as np
import pytest

import conn_impc_cases as Cs
import conn_impc_ref as R
import oracle_lib as O
from gpu_harness import fresh_outputs, require_gpu, to_device, to_host
from mpccbf import swarm
from parity_rule import ROUTE_REL, check_parity, same_bits, worse

pytestmark = pytest.mark.gpu

L2_TOL = 1e-10
ROW_TOL = 1e-8   # added rows at the device's x, scaled by 1 + |bound|


def _solve(torch, ctx, states, targets, rp, col, agent_first=0, num_agents=None):
    n = len(states) - agent_first if num_agents is None else num_agents
    out = fresh_outputs(ctx, n, fill=0)
    sl = slice(agent_first, agent_first + n)
    ctx.impc_solve(to_device(states), to_device(rp[agent_first:agent_first + n + 1]), to_device(col),
                   targets=to_device(targets[sl]), agent_first=agent_first,
                   num_agents=n, x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"],
                   next_states=out["next_states"])
    torch.cuda.synchronize()
    return to_host(out)


def _attach(torch, ctx, team_ptr, **kw):
    dev = torch.device("cuda", 0)
    l2 = torch.full((max(len(team_ptr) - 1, 1),), -1.0, dtype=torch.float64, device=dev)
    fd = torch.zeros((max(int(team_ptr[-1] - team_ptr[0]), 1),), dtype=torch.float64, device=dev)
    ctx.set_connectivity(team_ptr, kw.pop("d_max", Cs.D_MAX), lambda2=l2, fiedler=fd, **kw)
    return l2, fd


def _compare(got, ref, rows, first=0, label=""):
    """The parity rule on the device outputs (rows first .. of the batch) against the reference
    results of `rows`, and every added row of the reference at the device's x within ROW_TOL
    scaled, asserted per agent. Returns the measured maxima (objective relative, x, row excess)."""
    worst_obj, worst_x = check_parity(got, ref, rows, first=first, label=label)
    worst_row = -np.inf
    for i in rows:
        r = ref[i]
        ok = [it for it in range(len(r["status"])) if r["status"][it] == O.OPTIMAL]
        if ok:
            e = R.row_excess(r["rows"][ok[-1]], got["x"][i - first])
            worst_row = worse(worst_row, e)
            assert e <= ROW_TOL, (label, i, e)
    print(f"{label}: largest scaled added-row excess {worst_row:.3e}")
    return dict(obj=worst_obj, x=worst_x, row=worst_row)


@pytest.fixture(scope="module")
def cases():
    return Cs.cases()


@pytest.fixture(scope="module")
def solved(mpclib, cases):
    """The cases batch solved once with connectivity attached (shared by the tests below)."""
    torch = require_gpu()
    ctx = mpclib.Context(cases["cfg"])
    l2, fd = _attach(torch, ctx, cases["team_ptr"])
    got = _solve(torch, ctx, cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    name = ctx.kernel_name
    return dict(got=got, l2=l2.cpu().numpy(), fiedler=fd.cpu().numpy(), kernel=name, ctx=ctx)


def test_parity_on_the_cases(cases, solved):
    """Statuses of both iterations identical, objective within 1e-4 max(1, |ref|), x within 1e-5,
    lambda2 within 1e-10 max(1, |lambda2|), every added row of the reference satisfied at the
    device's x to 1e-8 scaled — on agents where the connectivity row binds, where CLF rows bind and
    where the added rows make the QP INFEASIBLE."""
    assert "conn" in solved["kernel"], solved["kernel"]
    keep = np.nonzero(cases["keep"])[0]
    kinds = [cases["kind"][i] for i in keep]
    assert min(kinds.count("conn"), kinds.count("clf"), kinds.count("infeasible")) >= 6
    _compare(solved["got"], cases["ref"], keep, label="cases")
    for t, (l2, ev, _) in enumerate(cases["spectra"]):
        assert abs(solved["l2"][t] - l2) <= L2_TOL * max(1.0, abs(l2)), (t, solved["l2"][t], l2)
        r0, r1 = int(cases["team_ptr"][t]), int(cases["team_ptr"][t + 1])
        v = solved["fiedler"][r0:r1]
        if r1 - r0 >= 2:  # the unit Fiedler vector up to its sign
            assert abs(abs(float(v @ ev)) - 1.0) <= 1e-9 and abs(float(v @ v) - 1.0) <= 1e-12, (t, v, ev)
    # the added rows change results: agents differ from a solve without them
    free = cases["free"]
    changed = [i for i in keep if list(free[i]["status"]) != list(cases["ref"][i]["status"])]
    assert len(changed) >= 6


SHAPE_SIZES = (3, 2, 5, 8, 1, 16, 4, 17)  # offsets 0 3 5 10 18 19 35 39 56: teams straddle rows 4, 8, 12, 16, 32, 48


@pytest.fixture(scope="module")
def shapes():
    cfg = Cs.config()
    st, tg, tp = swarm.team_swarm(SHAPE_SIZES, 2.55, seed=21, shape="ring", speed=(0.2, 0.8), gap=40.0)
    rp, col = swarm.team_csr(tp)
    rows = [i for i in range(int(tp[7]))]  # every team but the 17
    ref = Cs.reference(cfg, st, tg, tp, rp, col, rows=rows)
    up = Cs.reference(cfg, st, tg, tp, rp, col, rows=rows, shift=Cs.SHIFT)
    dn = Cs.reference(cfg, st, tg, tp, rp, col, rows=rows, shift=-Cs.SHIFT)
    keep = [i for i in rows if list(ref[i]["status"]) == list(up[i]["status"]) == list(dn[i]["status"])]
    return dict(cfg=cfg, states=st, targets=tg, team_ptr=tp, rp=rp, col=col, ref=ref, keep=keep, rows=rows)


def test_team_shapes(mpclib, shapes):
    """Teams of 2, 3, 4, 5, 8, 16, 1 and 17 in one batch across the 4-agent wave and 16-agent block
    boundaries: parity for teams up to 16, ERROR for the team of 17 alone (NaN lambda2), the team
    of 1 as without connectivity, and an agent range that cuts through teams."""
    torch = require_gpu()
    s = shapes
    tp = s["team_ptr"]
    assert len(s["keep"]) >= 0.95 * len(s["rows"])
    ctx = mpclib.Context(s["cfg"])
    # (the solve without connectivity in the layout the connectivity launch has, 16 lanes per agent:
    # the one-agent-per-wave kernel this batch size would take sums the objective's terms, which are
    # ~1e3 times the objective here, in another order — 4e-9 relative on the MI355X)
    ctx.set_variant(4)
    plain = _solve(torch, ctx, s["states"], s["targets"], s["rp"], s["col"])
    l2, _ = _attach(torch, ctx, tp)
    got = _solve(torch, ctx, s["states"], s["targets"], s["rp"], s["col"])
    _compare(got, s["ref"], s["keep"], label="shapes")
    l2 = l2.cpu().numpy()
    big = slice(int(tp[7]), int(tp[8]))
    assert np.all(got["status"][big, 0] == O.ERROR) and np.all(got["status"][big, 1] == O.UNKNOWN)
    assert np.all(got["status"][:int(tp[7])] != O.ERROR)
    assert np.isnan(l2[7]) and np.all(np.isfinite(l2[:7]))
    for t in range(7):
        ref_l2 = R.team_spectrum(s["states"], int(tp[t]), int(tp[t + 1] - tp[t]), Cs.D_MAX)[0]
        assert abs(l2[t] - ref_l2) <= L2_TOL * max(1.0, abs(ref_l2)), (t, l2[t], ref_l2)
    one = int(tp[4])  # the team of 1: as a solve without connectivity
    assert list(got["status"][one]) == list(plain["status"][one])
    np.testing.assert_allclose(got["obj"][one], plain["obj"][one], rtol=1e-9, atol=0.0)
    # agents 7 .. 36 only: the range starts inside the team of 5 and ends inside the team of 4
    part = _solve(torch, ctx, s["states"], s["targets"], s["rp"], s["col"], agent_first=7, num_agents=30)
    for k in ("status", "obj", "x", "next_states"):
        np.testing.assert_array_equal(part[k], got[k][7:37])


def test_no_cbf_filter_agrees(mpclib, cases, solved):
    torch = require_gpu()
    ctx = mpclib.Context(cases["cfg"], no_cbf_filter=True)
    _attach(torch, ctx, cases["team_ptr"])
    got = _solve(torch, ctx, cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    base = solved["got"]
    keep = np.nonzero(cases["keep"])[0]
    np.testing.assert_array_equal(got["status"][keep], base["status"][keep])
    ok = base["status"][keep] == O.OPTIMAL
    err = np.abs(got["obj"][keep][ok] - base["obj"][keep][ok]) / np.maximum(1.0, np.abs(base["obj"][keep][ok]))
    has = np.any(ok, axis=1)
    dx = np.abs(got["x"][keep][has] - base["x"][keep][has])
    print(f"no_cbf_filter: max objective difference {err.max():.3e} (relative), max |dx| {dx.max():.3e}")
    assert err.max() <= ROUTE_REL and dx.max() <= ROUTE_REL


def test_lambda2_switch_flips_the_mode(mpclib, cases):
    """lambda2_switch 0.15: the teams with 0.1 < lambda2 <= 0.15 take the CLF rows instead."""
    torch = require_gpu()
    tp = cases["team_ptr"]
    flipped = [t for t, (l2, _, _) in enumerate(cases["spectra"]) if 0.1 < l2 <= 0.15]
    assert flipped and all(abs(cases["spectra"][t][0] - 0.15) >= 1e-6 for t in range(len(tp) - 1))
    rows = [i for t in flipped for i in range(int(tp[t]), int(tp[t + 1]))]
    a = (cases["cfg"], cases["states"], cases["targets"], tp, cases["row_ptr"], cases["col"])
    ref = Cs.reference(*a, l2_switch=0.15, rows=rows)
    up = Cs.reference(*a, l2_switch=0.15, rows=rows, shift=Cs.SHIFT)
    dn = Cs.reference(*a, l2_switch=0.15, rows=rows, shift=-Cs.SHIFT)
    keep = [i for i in rows if list(ref[i]["status"]) == list(up[i]["status"]) == list(dn[i]["status"])]
    assert len(keep) >= 0.95 * len(rows) and not any(ref[i]["conn_mode"] for i in rows)
    assert all(cases["ref"][i]["conn_mode"] for i in rows)
    ctx = mpclib.Context(cases["cfg"])
    _attach(torch, ctx, tp, lambda2_switch=0.15)
    got = _solve(torch, ctx, cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    _compare(got, ref, keep, label="lambda2_switch 0.15")


@pytest.mark.parametrize("over", [dict(cbf_horizon=1), dict(cbf_horizon=3), dict(impc_iter=1)],
                         ids=["cbf_h1", "cbf_h3", "impc_iter1"])
def test_parity_off_the_default_horizon(mpclib, over):
    """cbf_horizon 1 and 3 (teams up to 6) and impc_iter 1 on the first two groups of the cases."""
    torch = require_gpu()
    cfg = Cs.config(**over)
    st, tg, tp = Cs.build(Cs.GROUPS[:3])
    rp, col = swarm.team_csr(tp)
    ref = Cs.reference(cfg, st, tg, tp, rp, col)
    up = Cs.reference(cfg, st, tg, tp, rp, col, shift=Cs.SHIFT)
    dn = Cs.reference(cfg, st, tg, tp, rp, col, shift=-Cs.SHIFT)
    keep = [i for i in ref if list(ref[i]["status"]) == list(up[i]["status"]) == list(dn[i]["status"])]
    assert len(keep) >= 0.95 * len(ref)
    ctx = mpclib.Context(cfg)
    _attach(torch, ctx, tp)
    got = _solve(torch, ctx, st, tg, rp, col)
    _compare(got, ref, keep, label=str(over))


def test_detach_restores_the_plain_solve(mpclib, cases):
    torch = require_gpu()
    ctx = mpclib.Context(cases["cfg"])
    a = (cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    first = _solve(torch, ctx, *a)
    name = ctx.kernel_name
    _attach(torch, ctx, cases["team_ptr"])
    mid = _solve(torch, ctx, *a)
    assert ctx.kernel_name != name
    ctx.set_connectivity(None)
    third = _solve(torch, ctx, *a)
    assert ctx.kernel_name == name
    for k in first:
        np.testing.assert_array_equal(first[k], third[k])
    assert not np.array_equal(first["status"], mid["status"])


def test_refusals_that_need_a_context(mpclib, cases):
    """Slack mode, the FoV controller and d_max <= d_min are refused at attach time with
    MPCCBF_ERR_INVALID_ARGUMENT (-1); the cap audit refuses while connectivity is attached; a team
    offset beyond the state table is refused at the solve."""
    torch = require_gpu()
    tp = cases["team_ptr"]
    for cfg, what in ((Cs.config(slack_mode=1), "slack mode"), (swarm.fov_config(), "FoV")):
        with pytest.raises(mpclib.MpccbfError, match=r"error -1: connectivity: .*" + what):
            mpclib.Context(cfg).set_connectivity(tp, Cs.D_MAX)
    ctx = mpclib.Context(cases["cfg"])
    for bad in (cases["cfg"]["d_min"], 1.0):
        with pytest.raises(mpclib.MpccbfError, match="error -1: connectivity: d_max must exceed d_min"):
            ctx.set_connectivity(tp, bad)
    _attach(torch, ctx, tp)
    dev = torch.device("cuda", 0)
    got = _solve(torch, ctx, cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    with pytest.raises(mpclib.MpccbfError, match="error -1: cap audit: not supported while connectivity is attached"):
        ctx.audit_neighbors(torch.tensor(cases["states"], device=dev), x=torch.tensor(got["x"], device=dev),
                            status=torch.tensor(got["status"], device=dev),
                            targets=torch.tensor(cases["targets"], device=dev),
                            nb_row_ptr=torch.tensor(cases["row_ptr"], device=dev),
                            nb_col=torch.tensor(cases["col"], device=dev))
    with pytest.raises(mpclib.MpccbfError, match="error -1: connectivity: team_ptr ends at row"):
        _solve(torch, ctx, cases["states"][:10], cases["targets"][:10], cases["row_ptr"][:11], cases["col"])


def _run_steps(torch, mpclib, cfg, states, targets, tp, rp, col, steps, nranks=1):
    """run_steps over `steps` closed-loop steps on nranks in-process ranks: per rank (final table,
    status log, lambda2 of the last step)."""
    dev = torch.device("cuda", 0)
    n = len(states)
    per = n // nranks
    comms = mpclib.Comm.local_group(nranks, 0) if nranks > 1 else [None]
    results, errors = [None] * nranks, []

    def rank_main(r):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                ctx = mpclib.Context(cfg)
                l2, _ = _attach(torch, ctx, tp)
                a = torch.tensor(states, device=dev)
                b = torch.empty_like(a)
                slog = torch.empty((steps, per, cfg["impc_iter"]), dtype=torch.int32, device=dev)
                res = ctx.run_steps(a, b, steps, targets=to_device(targets[r * per:(r + 1) * per]),
                                    agent_first=r * per, num_agents=per,
                                    nb_row_ptr=to_device(rp[r * per:(r + 1) * per + 1]),
                                    nb_col=torch.tensor(col, device=dev), status_log=slog, comm=comms[r], stream=stream)
                stream.synchronize()
                results[r] = (res["final"].cpu().numpy(), slog.cpu().numpy(), l2.cpu().numpy())
        except Exception as e:  # surfaced in the main thread
            errors.append(e)

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    for c in comms:
        if c is not None:
            c.close()
    assert not errors, errors
    return results


def test_run_steps_equals_single_solves(mpclib, cases):
    """run_steps over 10 steps equals ten impc_solve calls, each from the previous one's next
    states, bit for bit; and two in-process ranks with a team across the rank boundary equal one."""
    torch = require_gpu()
    cfg, tp, rp, col = cases["cfg"], cases["team_ptr"], cases["row_ptr"], cases["col"]
    states, targets = cases["states"], cases["targets"]
    steps = 10
    final, slog, l2 = _run_steps(torch, mpclib, cfg, states, targets, tp, rp, col, steps)[0]
    ctx = mpclib.Context(cfg)
    l2s, _ = _attach(torch, ctx, tp)
    cur = states.copy()
    for s in range(steps):
        got = _solve(torch, ctx, cur, targets, rp, col)
        same_bits(got["status"], slog[s])
        cur = got["next_states"]
    same_bits(cur, final)
    same_bits(l2s.cpu().numpy(), l2)
    assert not np.array_equal(final, states)
    # 58 agents as 2 ranks x 29: rows 27 .. 30 are one team, across the boundary
    assert len(states) == 58 and any(tp[t] < 29 < tp[t + 1] for t in range(len(tp) - 1))
    for r, (f2, s2, l22) in enumerate(_run_steps(torch, mpclib, cfg, states, targets, tp, rp, col, steps, nranks=2)):
        same_bits(f2, final)
        same_bits(s2, slog[:, r * 29:(r + 1) * 29])


def test_three_jacobi_steps_match_the_reference_loop(mpclib):
    torch = require_gpu()
    cfg = Cs.config()
    st, tg, tp = Cs.loop_teams()
    rp, col = swarm.team_csr(tp)
    trace, stats, stable = Cs.closed_loop(cfg, st, tg, tp, rp, col, 3)
    assert stable
    final, slog, _ = _run_steps(torch, mpclib, cfg, st, tg, tp, rp, col, 3)[0]
    np.testing.assert_array_equal(slog, stats)
    err = float(np.max(np.abs(final - trace[-1])))
    print(f"3 Jacobi steps: max |state - reference| {err:.3e}")
    assert err <= 1e-8


def test_simulator_logs_lambda2(mpclib):
    """Simulator(teams=..., d_max=...): the logged lambda2 of every step equals the oracle's
    lambda2 of the states that step planned from (knn lists: the device neighbour grid)."""
    torch = require_gpu()
    from mpccbf.sim import Simulator
    cfg = Cs.config()
    st, tg, tp = Cs.loop_teams()
    sim = Simulator(cfg, st, tg, knn_k=8, knn_radius=6.0, teams=tp, d_max=Cs.D_MAX, record=False)
    tables = []
    for _ in range(4):
        tables.append(sim.states.cpu().numpy().copy())
        sim.step()
    assert len(sim.lambda2_log) == 4
    for s, table in enumerate(tables):
        for t in range(len(tp) - 1):
            ref = O.lambda2(table[int(tp[t]):int(tp[t + 1]), :2], Cs.D_MAX)[0]
            assert abs(sim.lambda2_log[s][t] - ref) <= L2_TOL * max(1.0, abs(ref)), (s, t, sim.lambda2_log[s][t], ref)
    assert not np.allclose(sim.lambda2_log[0], sim.lambda2_log[-1])


def test_active_store_gets_zero_records_while_attached(mpclib, cases):
    """The connectivity launch has no store instantiation: an attached active-set store gets zero
    records for the agents it solves (the rule for kernels without the store), and records again
    after the detach."""
    torch = require_gpu()
    ctx = mpclib.Context(cases["cfg"])
    store = ctx.alloc_active_store(len(cases["states"]))
    store.fill_(7)
    ctx.set_active_store(store)
    _attach(torch, ctx, cases["team_ptr"])
    a = (cases["states"], cases["targets"], cases["row_ptr"], cases["col"])
    _solve(torch, ctx, *a)
    assert int(torch.count_nonzero(store)) == 0
    ctx.set_connectivity(None)
    _solve(torch, ctx, *a)
    assert int(torch.count_nonzero(store)) > 0

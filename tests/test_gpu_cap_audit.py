"""GPU: the neighbour-cap audit (mpccbf_cap_audit_run, Context.audit_neighbors) on the separable
collision controller.

Scenario: swarm.lattice_swarm on the 0.45 x lattice (a crowd: neighbours inside d_min), config
K = 15, the k nearest within 6 m. tests/test_cap_audit.py confirms on the CPU oracle that at k = 1
and k = 2 rows are dropped live and violated, and that every decision the audit makes there (row
live or not, violated or not) has a margin of >= 1e-3, so the equalities below do not hang on
rounding.

Bounds: counts and live neighbours equal; scaled excesses within 1e-9 (1 + |excess|) of the numpy
restatement on the GPU's own solutions (the same arithmetic: FP64 rounding of a cubic Bezier and a
20-flop row); statuses equal and objectives / solutions within 1e-7 relative between a certified
capped solve and the all-others solve, the project's bound between two exact solver paths
(DESIGN.md section 4).
"""
import functools

import numpy as np
import pytest

import cap_audit_ref as R
from mpccbf import swarm
from mpccbf.sim import Simulator
from gpu_harness import require_gpu, same_bits, to_device
from parity_rule import ROUTE_REL, check_routes_agree

pytestmark = pytest.mark.gpu

RADIUS = 6.0
SEP16, WIDE = 4, 5
OPTIMAL, INFEASIBLE = 0, 3


def _np(t):
    return t.cpu().numpy()


def _solve(mpclib, n, k=None, variant=0, csr=None, first=0, count=None, ctx=None, states=None):
    """One IMPC step of agents first .. first + count - 1 of the n-agent scenario: grid mode with
    the k nearest (nb_out kept), or csr = (row_ptr, col) of the whole swarm. Returns the context,
    the device tensors and the keyword arguments audit_neighbors needs for that batch."""
    torch = require_gpu()
    cfg, st, targets = R.scenario(n)
    if states is not None:
        st = states
    count = n - first if count is None else count
    dev = torch.device("cuda", 0)
    ctx = ctx or mpclib.Context(cfg)
    ctx.set_variant(variant)
    a = torch.tensor(st, device=dev)
    tg = torch.tensor(targets[first:first + count], device=dev)
    out = ctx.alloc_outputs(count)
    if csr is None:
        nb_out = torch.full((count, 16), -7, dtype=torch.int32, device=dev)
        lists = dict(knn_k=k, knn_radius=RADIUS)
        ctx.impc_solve(a, targets=tg, agent_first=first, num_agents=count, x=out["x"], status=out["status"],
                       obj=out["obj"], iters=out["iters"], nb_out=nb_out, **lists)
        lists["nb_out"] = nb_out
    else:
        rp, col = csr
        lists = dict(nb_row_ptr=to_device(rp[first:first + count + 1]),
                     nb_col=to_device(col))
        ctx.impc_solve(a, targets=tg, agent_first=first, num_agents=count, x=out["x"], status=out["status"],
                       obj=out["obj"], iters=out["iters"], **lists)
    torch.cuda.synchronize()
    akw = dict(x=out["x"], status=out["status"], targets=tg, agent_first=first, num_agents=count, **lists)
    return dict(ctx=ctx, cfg=cfg, states_np=st, states=a, targets=tg, out=out, akw=akw, kernel=ctx.kernel_name)


@functools.lru_cache(maxsize=None)
def _grid_audit(mpclib, n, k, variant=0):
    """Grid-mode solve of the whole n-agent scenario and its audit (computed once, never modified):
    host arrays."""
    s = _solve(mpclib, n, k, variant)
    res = s["ctx"].audit_neighbors(s["states"], live_nb=True, x0=True, **s["akw"])
    require_gpu().cuda.synchronize()
    r = {key: _np(v) for key, v in res.items()}
    r.update(status=_np(s["out"]["status"]), obj=_np(s["out"]["obj"]), x=_np(s["out"]["x"]),
             nb_out=_np(s["akw"]["nb_out"]), states=s["states_np"], cfg=s["cfg"], kernel=s["kernel"])
    return r


def _lists_of(nb_out):
    return [row[:np.argmax(row < 0)] if (row < 0).any() else row for row in nb_out]


@pytest.mark.parametrize("n", [64, 70, 257])
def test_kernel_matches_the_numpy_restatement(mpclib, oracle, n):
    """One LDS tile (64, 70: a ragged one) and two (257: the second holds one row), k = 1 in grid
    mode: every count, the live neighbours and the excesses against the audit restated in numpy on
    the GPU's own x0, x, status and nb_out with the oracle's safety_cbf / eval_curve."""
    g = _grid_audit(mpclib, n, 1)
    lists = _lists_of(g["nb_out"])
    assert all(len(l) <= 1 for l in lists)
    ref = R.audit(oracle, g["cfg"], g["states"], lists, g["status"], g["x0"], g["x"])
    c, rc = g["counts"], ref["counts"]
    print(f"n = {n} ({g['kernel']}): live / violated totals "
          f"{[int(np.clip(c[:, w], 0, None).sum()) for w in range(4)]}, "
          f"agents with a violated row {np.count_nonzero(c[:, 1] > 0)} / {np.count_nonzero(c[:, 3] > 0)}, "
          f"certified {np.count_nonzero(c[:, 7] & 1)} / {np.count_nonzero(c[:, 7] & 2)}, "
          f"min |b - bmax| margin {ref['bmargin']:.3e}")
    for w in (0, 1, 2, 3, 6, 7):
        np.testing.assert_array_equal(c[:, w], rc[:, w], err_msg=f"counts word {w}")
    np.testing.assert_array_equal(g["live_nb"], ref["live_nb"])
    ex, rex = g["excess"], ref["excess"]
    np.testing.assert_array_equal(np.isnan(ex), np.isnan(rex))
    ok = ~np.isnan(rex)
    err = np.abs(ex[ok] - rex[ok]) / (1.0 + np.abs(rex[ok]))
    print(f"scaled excess: max error {err.max():.3e} over {ok.sum()} values, range "
          f"[{rex[ok].min():.3e}, {rex[ok].max():.3e}]")
    assert err.max() <= 1e-9
    for it in range(2):  # the winner may differ only where the reference's top two are within 1e-9
        diff = c[:, 4 + it] != rc[:, 4 + it]
        assert not np.any(diff & ~(ref["gap"][:, it] <= 1e-9)), np.nonzero(diff)[0]
    # x0 is NaN exactly where iteration 0 was not OPTIMAL
    np.testing.assert_array_equal(np.isnan(g["x0"]).all(axis=1), g["status"][:, 0] != OPTIMAL)
    np.testing.assert_array_equal(np.isnan(g["x0"]).any(axis=1), g["status"][:, 0] != OPTIMAL)
    assert np.count_nonzero(c[:, 1] > 0) >= 1 and np.count_nonzero(c[:, 3] > 0) >= 1, "vacuous: nothing violated"


@functools.lru_cache(maxsize=None)
def _all_others(mpclib, variant):
    s = _solve(mpclib, 64, csr=swarm.all_csr(64), variant=variant)
    return dict(status=_np(s["out"]["status"]), obj=_np(s["out"]["obj"]), x=_np(s["out"]["x"]))


@pytest.mark.parametrize("variant", [SEP16, WIDE])
@pytest.mark.parametrize("k", [1, 2])
def test_certificate_means_what_it_says(mpclib, k, variant):
    """A certified agent's capped solve is the all-others solve (statuses equal, objectives and x
    within 1e-7 relative); an agent with a violated iteration-0 row has an all-others iteration 0
    that is not OPTIMAL or strictly more expensive."""
    g = _grid_audit(mpclib, 64, k, variant)
    full = _all_others(mpclib, variant)
    c, st, obj = g["counts"], g["status"], g["obj"]
    bit0, bit1 = (c[:, 7] & 1) != 0, (c[:, 7] & 2) != 0
    viol0 = c[:, 1] > 0
    print(f"k = {k}, variant {variant} ({g['kernel']}): bit 0 on {bit0.sum()}, bit 1 on {bit1.sum()}, "
          f"violated iteration-0 row on {viol0.sum()} agents")
    assert not np.any(bit1 & ~bit0)
    np.testing.assert_array_equal(st[bit0, 0], full["status"][bit0, 0])
    o = bit0 & (st[:, 0] == OPTIMAL)
    check_routes_agree(obj[o, 0], full["obj"][o, 0], "certified agents: objective, iteration 0")
    np.testing.assert_array_equal(st[bit1], full["status"][bit1])
    o1 = bit1 & (st[:, 1] == OPTIMAL)
    check_routes_agree(obj[o1, 1], full["obj"][o1, 1], "certified agents: objective, iteration 1")
    hasx = bit1 & (st == OPTIMAL).any(axis=1)
    check_routes_agree(g["x"][hasx], full["x"][hasx], "certified agents: x")
    np.testing.assert_array_equal(np.isnan(g["x"][bit1]), np.isnan(full["x"][bit1]))
    # the flagged agents: the capped optimum breaks a row of the all-others QP, whose optimum is
    # therefore strictly more expensive (a relaxation's optimum that is infeasible for the full QP)
    fo, fs = full["obj"][viol0, 0], full["status"][viol0, 0]
    worse = (fs != OPTIMAL) | ((fo - obj[viol0, 0]) > ROUTE_REL * np.maximum(1.0, np.abs(obj[viol0, 0])))
    print(f"flagged agents: all-others iteration 0 not OPTIMAL on {np.count_nonzero(fs != OPTIMAL)}, smallest "
          f"relative objective increase {np.min(((fo - obj[viol0, 0]) / np.maximum(1.0, np.abs(obj[viol0, 0])))[fs == OPTIMAL], initial=np.inf):.3e}")
    assert worse.all(), np.nonzero(viol0)[0][~worse]
    assert bit0.sum() >= 40
    assert viol0.sum() >= (10 if k == 1 else 1)


def test_complete_lists_are_never_flagged(mpclib):
    """k = 8 on the same lattice keeps every live row: no live or violated count, and both bits
    for every agent whose statuses are OPTIMAL or INFEASIBLE."""
    g = _grid_audit(mpclib, 64, 8)
    c, st = g["counts"], g["status"]
    assert np.all(c[:, :4] <= 0), c[:, :4]
    assert np.all(c[:, 0] == 0) and np.all(c[:, 1] == 0)
    np.testing.assert_array_equal(c[:, 4:6], -1)
    assert np.isnan(g["excess"]).all() and np.all(g["live_nb"] == -1)
    np.testing.assert_array_equal(c[:, 6], 63 - (g["nb_out"] >= 0).sum(axis=1))
    settled = np.isin(st[:, 0], (OPTIMAL, INFEASIBLE)) & ((st[:, 0] != OPTIMAL) | np.isin(st[:, 1], (OPTIMAL, INFEASIBLE)))
    assert settled.sum() >= 32
    np.testing.assert_array_equal(c[settled, 7], 3)
    np.testing.assert_array_equal(c[~settled, 7] & 2, 0)


def test_csr_lists_and_a_partial_batch(mpclib):
    torch = require_gpu()
    g = _grid_audit(mpclib, 64, 1)
    rp, col = swarm.knn_csr(g["states"], 1, RADIUS)
    s = _solve(mpclib, 64, csr=(rp, col), first=16, count=32)
    res = s["ctx"].audit_neighbors(s["states"], live_nb=True, **s["akw"])
    np.testing.assert_array_equal(_np(s["out"]["status"]), g["status"][16:48])
    np.testing.assert_array_equal(_np(res["counts"]), g["counts"][16:48])
    np.testing.assert_array_equal(_np(res["live_nb"]), g["live_nb"][16:48])
    err = np.abs(_np(res["excess"]) - g["excess"][16:48])
    assert np.nanmax(err) <= 1e-6  # (two solves of the same QPs; the decisions have 1e-3 margins)

    # a list given in descending order with a duplicated entry audits like the sorted unique list
    g2 = _grid_audit(mpclib, 64, 2)
    rp2, col2 = swarm.knn_csr(g2["states"], 2, RADIUS)
    rows = [col2[rp2[a]:rp2[a + 1]] for a in range(64)]
    odd = [np.concatenate([r[::-1], r[:1]]) for r in rows]
    assert any(len(r) == 2 for r in rows)
    orp = np.zeros(65, dtype=np.int32)
    orp[1:] = np.cumsum([len(r) for r in odd])
    dev = s["states"].device
    s2 = _solve(mpclib, 64, csr=(rp2, col2))
    plain = s2["ctx"].audit_neighbors(s2["states"], live_nb=True, **s2["akw"])
    akw = dict(s2["akw"], nb_row_ptr=torch.tensor(orp, device=dev),
               nb_col=torch.tensor(np.concatenate(odd).astype(np.int32), device=dev))
    got = s2["ctx"].audit_neighbors(s2["states"], live_nb=True, **akw)
    np.testing.assert_array_equal(_np(got["counts"]), _np(plain["counts"]))
    np.testing.assert_array_equal(_np(got["live_nb"]), _np(plain["live_nb"]))
    np.testing.assert_array_equal(_np(plain["counts"]), g2["counts"])

    # a single state: nothing to drop
    one = _solve(mpclib, 64, k=1, states=g["states"][:1], count=1)
    r1 = one["ctx"].audit_neighbors(one["states"], live_nb=True, **one["akw"])
    c1 = _np(r1["counts"])[0]
    assert list(_np(one["akw"]["nb_out"])[0]) == [-1] * 16
    assert list(_np(one["out"]["status"])[0]) == [OPTIMAL, OPTIMAL]
    assert list(c1) == [0, 0, 0, 0, -1, -1, 0, 3]
    assert list(_np(r1["live_nb"])[0]) == [-1] * 8


def test_audit_leaves_the_callers_data_alone(mpclib):
    torch = require_gpu()
    cfg, states, targets = R.scenario(64)
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    a = torch.tensor(states, device=dev)
    tg = torch.tensor(targets, device=dev)
    out = ctx.alloc_outputs(64)
    out["x"].fill_(float("nan"))
    traj_t = torch.full((64,), -1.0, dtype=torch.float64, device=dev)
    nb_out = torch.full((64, 16), -1, dtype=torch.int32, device=dev)
    store = ctx.alloc_active_store(64)
    ctx.set_active_store(store)
    ctx.impc_solve(a, targets=tg, x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"],
                   next_states=out["next_states"], traj_t=traj_t, nb_out=nb_out, knn_k=1, knn_radius=RADIUS)
    torch.cuda.synchronize()
    keep = dict(out, traj_t=traj_t, store=store, nb_out=nb_out, states=a)
    before = {k: _np(v).copy() for k, v in keep.items()}
    assert np.count_nonzero(before["store"]) > 0
    res = ctx.audit_neighbors(a, x=out["x"], status=out["status"], targets=tg, nb_out=nb_out, knn_k=1,
                              knn_radius=RADIUS)
    torch.cuda.synchronize()
    assert np.count_nonzero(_np(res["counts"])[:, 1] > 0) >= 10
    same_bits(keep, before, what="after the audit")  # (NaN patterns included)
    # the audit of a solve with a store attached is the audit of the plain solve
    np.testing.assert_array_equal(_np(res["counts"]), _grid_audit(mpclib, 64, 1)["counts"])


def test_simulator_with_audit_reproduces_the_plain_run(mpclib):
    cfg, states, targets = R.scenario(64)
    kw = dict(knn_k=1, knn_radius=RADIUS, pos_std=1e-3, vel_std=1e-3, noise_seed=5)
    runs = []
    for audit in (False, True):
        sim = Simulator(cfg, states, targets, audit=audit, **kw)
        for _ in range(6):
            sim.step()
        runs.append(sim)
    plain, aud = runs
    np.testing.assert_array_equal(np.array(plain.status_log), np.array(aud.status_log))
    assert _np(plain.states).tobytes() == _np(aud.states).tobytes()
    assert plain.states_json() == aud.states_json()
    assert plain.audit_log == [] and plain.audit_counts is None
    assert len(aud.audit_log) == 6 and tuple(aud.audit_counts.shape) == (64, 8)
    assert aud.audit_log[-1] == mpclib.audit_summary(aud.audit_counts)
    assert aud.audit_log[0]["violated0"] >= 10 and aud.audit_log[0]["agents"] == 64
    print("per-step uncertified agents:", [s["uncertified"] for s in aud.audit_log])


def test_continued_run_after_an_audit_equals_the_run_without(mpclib):
    """The audit's own launch ends a continue_tables rotation like any mpccbf_impc_solve: the next
    mpccbf_run_steps rebuilds its table, and its results are those of the run without the audit."""
    torch = require_gpu()
    cfg, states, targets = R.scenario(64)
    dev = torch.device("cuda", 0)
    finals, logs = [], []
    for with_audit in (False, True):
        s = _solve(mpclib, 64, 1)  # (a solved batch on other buffers, for the audit call)
        ctx = s["ctx"]
        a = torch.tensor(states, device=dev)
        b = torch.empty_like(a)
        tg = torch.tensor(targets, device=dev)
        log = torch.zeros((2, 64, 2), dtype=torch.int32, device=dev)
        r = ctx.run_steps(a, b, 2, targets=tg, knn_k=8, knn_radius=RADIUS)
        assert r["final"] is a
        if with_audit:
            ctx.audit_neighbors(s["states"], **s["akw"])
        r = ctx.run_steps(a, b, 2, targets=tg, knn_k=8, knn_radius=RADIUS, status_log=log, step_index=2,
                          continue_tables=True)
        torch.cuda.synchronize()
        finals.append(_np(r["final"]).copy())
        logs.append(_np(log).copy())
    assert finals[0].tobytes() == finals[1].tobytes()
    np.testing.assert_array_equal(logs[0], logs[1])


def test_device_side_argument_and_capacity_errors(mpclib):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    s = _solve(mpclib, 64, 1)
    ctx, akw = s["ctx"], s["akw"]
    Err = mpclib.MpccbfError
    for variant in (1, 3):  # the dense layouts
        ctx.set_variant(variant)
        with pytest.raises(Err, match="cap audit: the separable layouts only"):
            ctx.audit_neighbors(s["states"], **akw)
    ctx.set_variant(0)
    # zero agents is fine
    res = ctx.audit_neighbors(s["states"], **dict(akw, num_agents=0))
    assert tuple(res["counts"].shape) == (0, 8)
    # a state table beyond the membership bitmap's capacity
    big = torch.zeros((65537, 6), dtype=torch.float64, device=dev)
    with pytest.raises(Err, match=r"mpccbf error -3: cap audit: num_states \(65537\) > 65536"):
        ctx.audit_neighbors(big, **akw)
    # grid mode needs the query of the solve
    with pytest.raises(Err, match="grid neighbours need knn_k >= 1"):
        ctx.audit_neighbors(s["states"], **dict(akw, knn_k=0))
    # the context still audits after the errors
    res = ctx.audit_neighbors(s["states"], **akw)
    np.testing.assert_array_equal(_np(res["counts"]), _grid_audit(mpclib, 64, 1)["counts"])
    for cfg, what in ((swarm.config(15, slack_mode=1), "slack mode is not supported"),
                      (swarm.fov_config(), "the FoV controller is not supported"),
                      (swarm.config(15, impc_iter=3), "impc_iter > 2 is not supported")):
        c2 = mpclib.Context(cfg)
        with pytest.raises(Err, match="mpccbf error -1: cap audit: " + what):
            c2.audit_neighbors(s["states"], **akw)
        c2.close()


def test_simulator_rejects_what_the_audit_does_not_support(mpclib):
    require_gpu()
    cfg, states, targets = R.scenario(16)
    with pytest.raises(ValueError, match="jacobi"):
        Simulator(cfg, states, targets, audit=True, order="gauss_seidel")
    with pytest.raises(ValueError, match="collision controller without slack"):
        Simulator(swarm.config(15, slack_mode=1), states, targets, audit=True)
    with pytest.raises(ValueError, match="collision controller without slack"):
        Simulator(swarm.fov_config(), states, targets, audit=True)


def test_non_finite_data_audits_as_no_live_row_and_no_bits(mpclib):
    """A NaN state: the agent itself and every agent that lists it audit as no live row and no
    bits; where it is a dropped neighbour its rows are not live; every other agent's counts are
    those of the finite swarm. (CSR lists from the finite positions, k = 1.)"""
    g = _grid_audit(mpclib, 64, 1)
    rp, col = swarm.knn_csr(g["states"], 1, RADIUS)
    lists = [col[rp[a]:rp[a + 1]] for a in range(64)]
    # an agent that somebody lists and that is a live dropped neighbour of somebody else
    listed = {int(j) for l in lists for j in l}
    live = {int(j) for j in g["live_nb"].ravel() if j >= 0}
    nan = min(listed & live)
    st = g["states"].copy()
    st[nan, 0] = np.nan
    s = _solve(mpclib, 64, csr=(rp, col), states=st)
    res = s["ctx"].audit_neighbors(s["states"], live_nb=True, **s["akw"])
    c, ln, status = _np(res["counts"]), _np(res["live_nb"]), _np(s["out"]["status"])
    hit = [nan] + [a for a in range(64) if nan in lists[a]]
    assert len(hit) >= 2
    for a in hit:
        assert status[a, 0] not in (OPTIMAL, INFEASIBLE), (a, status[a])
        assert list(c[a, :6]) == [0, 0, -1, -1, -1, -1] and c[a, 7] == 0, (a, c[a])
        assert list(ln[a]) == [-1] * 8
        assert np.isnan(_np(res["excess"])[a]).all()
    np.testing.assert_array_equal(c[:, 6], g["counts"][:, 6])
    dropped_live = [a for a in range(64) if nan in g["live_nb"][a]]
    assert dropped_live and not set(dropped_live) & set(hit)
    for a in dropped_live:  # its rows are gone, nothing else changed
        assert nan not in ln[a]
        assert c[a, 0] <= g["counts"][a, 0] and c[a, 2] <= g["counts"][a, 2]
        assert c[a, 0] + max(c[a, 2], 0) < g["counts"][a, 0] + max(g["counts"][a, 2], 0)
    rest = [a for a in range(64) if a not in hit and a not in dropped_live]
    np.testing.assert_array_equal(c[rest], g["counts"][rest])
    np.testing.assert_array_equal(ln[rest], g["live_nb"][rest])

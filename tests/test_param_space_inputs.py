"""The inputs of test_gpu_param_space.py, checked on the CPU oracle alone: each has the property
its GPU test relies on (the status mix, no QP without a verdict, tight box rows in every channel,
live iteration-1 CBF rows of the rings within / beyond the 128-row capacity), so those conditions
hold wherever the GPU tests run."""
import numpy as np
import pytest

import oracle_lib as O
import param_space_cases as C
from mpccbf import swarm

OK, INF, UNK = O.OPTIMAL, O.INFEASIBLE, O.UNKNOWN


def _check(res, mix):
    assert C.attempted_unknown(res) == []  # every attempted QP has a verdict: no agent is left out
    assert C.status_mix(res) == mix


@pytest.fixture(scope="module")
def lattice():
    st, tg = C.crowded(64, 0.45, 5)
    return (st, tg) + swarm.knn_csr(st, 8, 6.0)


@pytest.mark.parametrize("spd_f", [1, 3, 8, 15])
def test_refs_lattice_mix(oracle, lattice, spd_f):
    st, tg, rp, col = lattice
    cfg = swarm.config(15, spd_f=spd_f)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    assert refs.shape == (64, 45)
    # every channel of the tail moves, per agent (a constant tail would hide a wrong sample index)
    tail = refs.reshape(64, 15, 3)[:, 15 - max(spd_f, 2):]
    assert np.all(np.ptp(tail, axis=1) > 1e-3)
    _check(C.oracle_batch(cfg, st, tg, rp, col, refs=refs), {(OK, OK): 49, (INF, UNK): 14, (OK, INF): 1})


def test_refs_fov_and_slack_all_optimal(oracle):
    cfg = swarm.fov_config(20, spd_f=5)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    _check(C.oracle_batch(cfg, st, tg, rp, col, refs=C.moving_refs(st, tg, 20, cfg["h"], 7)), {(OK, OK): 64})
    cfg = swarm.config(15, spd_f=5, slack_mode=1)
    st, tg = C.crowded(64, 0.45, 21)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    _check(C.oracle_batch(cfg, st, tg, rp, col, refs=C.moving_refs(st, tg, 15, cfg["h"], 7)), {(OK, OK): 64})


@pytest.mark.parametrize("cbf_h,mix", [
    (1, {(OK, OK): 50, (INF, UNK): 14}),
    (3, {(OK, OK): 46, (OK, INF): 4, (INF, UNK): 14}),
    (5, {(OK, OK): 31, (OK, INF): 19, (INF, UNK): 14}),
    (8, {(OK, OK): 12, (OK, INF): 38, (INF, UNK): 14}),
])
def test_cbf_horizon_lattice_mix(oracle, lattice, cbf_h, mix):
    st, tg, rp, col = lattice
    _check(C.oracle_batch(swarm.config(15, cbf_horizon=cbf_h), st, tg, rp, col), mix)


@pytest.mark.parametrize("cbf_h,mix", [(1, {(OK, OK): 64}), (3, {(OK, OK): 63, (OK, INF): 1})])
def test_cbf_horizon_fov_mix(oracle, cbf_h, mix):
    cfg = swarm.fov_config(20, cbf_horizon=cbf_h)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    _check(C.oracle_batch(cfg, st, tg, rp, col), mix)


@pytest.mark.parametrize("n_ring,cbf_h,live0", [(12, 8, 53), (20, 4, 72), (40, 3, 120), (40, 5, 157)])
def test_ring_live_rows(oracle, n_ring, cbf_h, live0):
    """Agent 0's live iteration-1 rows: beyond the 16 slots of the default kernels and within the
    capacity launch's 128 (the first three), beyond the 128 (the last). Agent 0 is OPTIMAL in both
    iterations; the ring robots are infeasible."""
    cfg = swarm.config(15, cbf_horizon=cbf_h)
    st, tg, rp, col = C.ring(n_ring)
    res = C.oracle_batch(cfg, st, tg, rp, col)
    _check(res, {(OK, OK): 1, (INF, UNK): n_ring})
    assert list(res[0]["status"]) == [OK, OK]
    live = C.live_rows_it1(cfg, st, tg, rp, col, res)
    assert live[0] == live0
    assert (16 < live[0] <= 128) if live0 <= 128 else live[0] > 128
    assert np.all(live[1:] == 0)


@pytest.mark.parametrize("impc_iter,mix", [
    (1, {(OK,): 50, (INF,): 14}),
    (3, {(OK, OK, OK): 49, (INF, UNK, UNK): 14, (OK, INF, UNK): 1}),
    (4, {(OK, OK, OK, OK): 49, (INF, UNK, UNK, UNK): 14, (OK, INF, UNK, UNK): 1}),
])
def test_impc_iter_lattice_mix(oracle, lattice, impc_iter, mix):
    st, tg, rp, col = lattice
    _check(C.oracle_batch(swarm.config(15, impc_iter=impc_iter), st, tg, rp, col), mix)


def test_impc_iter_slack_and_fov_all_optimal(oracle):
    st, tg = C.crowded(64, 0.45, 21)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    _check(C.oracle_batch(swarm.config(15, impc_iter=3, slack_mode=1), st, tg, rp, col), {(OK, OK, OK): 64})
    cfg = swarm.fov_config(20, impc_iter=3)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    _check(C.oracle_batch(cfg, st, tg, rp, col), {(OK, OK, OK): 64})


@pytest.mark.parametrize("slack", [0, 1])
def test_yaw_asym_main_case_tight_rows(oracle, slack):
    """All OPTIMAL, and at least 10 agents per channel (x, y, yaw) end on a box bound, so a kernel
    that reads another channel's bound, or the wrong side's, changes many optima."""
    cfg = swarm.config(15, slack_mode=slack, **C.ASYM)
    st, tg = C.crowded(64, 0.55, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    st, tg = C.with_yaw(st, tg, 11, 0.9)
    res = C.oracle_batch(cfg, st, tg, rp, col)
    _check(res, {(OK, OK): 64})
    tight = C.tight_box_agents(cfg, res)
    assert list(tight) == [27, 14, 20]
    assert np.all(tight >= 10)


def test_yaw_asym_mixed_feasibility(oracle):
    """rate 2.4: the infeasible agents are exactly those whose yaw rate lies outside
    [v_min[2], v_max[2]] = [-1, 2.6] (their planar velocities are within the x / y limits)."""
    cfg = swarm.config(15, **C.ASYM)
    st, tg = C.crowded(64, 0.55, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    st, tg = C.with_yaw(st, tg, 11, 2.4)
    res = C.oracle_batch(cfg, st, tg, rp, col)
    _check(res, {(OK, OK): 40, (INF, UNK): 24})
    bad = [i for i, r in enumerate(res) if r["status"][0] == INF]
    assert bad == [i for i in range(64) if st[i, 5] < -1.0]
    assert np.all(np.abs(st[:, 3:5]) <= 0.5)


def test_fov_asym_all_optimal(oracle):
    cfg = swarm.fov_config(20, **C.ASYM)
    st, tg = C.fov_swarm()
    rp, col = swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])
    res = C.oracle_batch(cfg, st, tg, rp, col)
    _check(res, {(OK, OK): 64})
    assert np.all(C.tight_box_agents(cfg, res)[:2] >= 10)


def test_combined_case_mix(oracle):
    cfg = swarm.config(15, cbf_horizon=3, impc_iter=3, spd_f=5, **C.ASYM)
    st, tg = C.crowded(64, 0.55, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    st, tg = C.with_yaw(st, tg, 11, 2.4)
    refs = C.moving_refs(st, tg, 15, cfg["h"], 7)
    _check(C.oracle_batch(cfg, st, tg, rp, col, refs=refs),
           {(OK, OK, OK): 39, (INF, UNK, UNK): 24, (OK, INF, UNK): 1})


@pytest.mark.parametrize("k_hor", [10, 15])
def test_reduction_options_input_mix(oracle, k_hor):
    st, tg = C.crowded(64, 0.5, 5)
    rp, col = swarm.knn_csr(st, 8, 6.0)
    _check(C.oracle_batch(swarm.config(k_hor), st, tg, rp, col), {(OK, OK): 62, (INF, UNK): 2})


def test_asym_operators_keep_the_separable_layout(mpclib):
    """With ASYM at k_hor = 15 the host operators still have nz = 6 and 16 box rows per channel
    (48 shared rows), the layout of the separable and one-agent-per-wave kernels."""
    from mpccbf import _lib
    for cfg in (swarm.config(15), swarm.config(15, **C.ASYM)):
        o = _lib.host_operators(cfg)
        assert (o["nz"], o["m"], o["mc"]) == (6, 48, 3)


@pytest.mark.parametrize("slack", [0, 1])
def test_filter_edge_rows_are_active_below_the_threshold(oracle, slack):
    """filter_edge with ASYM: all OPTIMAL; each moving agent's iteration-0 CBF row is active at the
    optimum (slack 0) with its bound b inside [narrow, threshold): the exact filter keeps it, a
    filter reading any narrower entry of a_min / a_max for that channel and side would drop it.
    (Agent 3's side is a_max[1] = 2, the narrowest entry: no narrower one exists.)"""
    cfg = swarm.config(15, slack_mode=slack, **C.ASYM)
    st, tg, rp, col = C.filter_edge()
    res = C.oracle_batch(cfg, st, tg, rp, col)
    _check(res, {(OK, OK): 8})
    m = C.filter_edge_margins(cfg, st, tg, rp, col, res)
    assert [round(v[2], 3) for v in m] == [8.2, 12.3, 12.3, 0.0]
    for b, thr, narrow, row_slack in m:
        assert narrow + 0.5 < b < thr - 0.5
        if not slack:
            assert abs(row_slack) <= 1e-9

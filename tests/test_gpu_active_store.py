"""GPU: the active-set store (mpccbf_set_active_store) on the separable collision controller, in
both layouts (set_variant(4): 16 lanes per agent; set_variant(5): one agent per wave).

The feature checks itself: a warm start is a list of the QP's own sides, accepted only when their
equality QP has multipliers of the right signs, and the optimum of a strictly convex QP is unique —
so a run with a store must return the statuses and solutions of the run without one, whatever the
store holds. Bounds: statuses identical; objectives and final states within 1e-7 relative, the
project's bound between two exact solver paths (wide vs 16-lane).

Scenario: 64 agents of swarm.lattice_swarm on the crowded 0.6 x lattice, 8 nearest within 6 m,
closed loop with state noise. tests/test_active_store.py confirms on the CPU oracle that its first
step already has agents with >= 3 active inequality rows in iteration 0 (so >= 3 active-set
steps); here the cold runs assert iteration-0 solves of >= 3 steps, so nothing passes vacuously.
On the 0.6 x lattice the active sides are box sides almost throughout (measured: 5 CBF keys
exported in 30 steps x 64 agents), so the CBF keys' path — the staged rows' keys, the mapping by
neighbour — would go untested: the warm = cold, cross-layout and exported-set tests also run on
the 0.45 x lattice of test_gpu_context_reuse.py (29-34 CBF keys per step in its first steps,
INFEASIBLE agents included), where they assert that CBF keys were read.
"""
import functools

import numpy as np
import pytest

from gpu_harness import require_gpu, to_device
from mpccbf import swarm
from parity_rule import check_routes_agree, same_bits

pytestmark = pytest.mark.gpu

N, K, RADIUS, STEPS = 64, 8, 6.0, 25
SEP16, WIDE = 4, 5
NOISE = dict(pos_std=1e-3, vel_std=1e-3, noise_seed=11)
INT_MIN = -2 ** 31


def _scenario(seed=swarm.SEED, scale=0.6):
    states, targets = swarm.lattice_swarm(N, seed=seed)
    states[:, :2] *= scale
    return states, targets


def _loop(mpclib, schedule, store0=None, min_steps=1, inject=None, seed=swarm.SEED, scale=0.6):
    """Closed loop, one mpccbf_run_steps call per step (so every step's objectives can be read),
    step t on layout schedule[t]. store0: None = no store, else the store's initial contents
    (N x 8). inject(t, store): rewrites the store before step t. Returns per-step status / obj /
    iters, the state table and the store as each step read them, the final store and the final
    states (host arrays)."""
    torch = require_gpu()
    cfg = swarm.config(15)
    states, targets = _scenario(seed, scale)
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    a = torch.tensor(states, device=dev)
    b = torch.empty_like(a)
    tg = torch.tensor(targets, device=dev)
    out = ctx.alloc_outputs(N)
    out["x"].fill_(float("nan"))
    traj_t = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    store = None
    if store0 is not None:
        store = to_device(np.asarray(store0, dtype=np.int32))
        ctx.set_active_store(store, min_steps)
    res = dict(status=[], obj=[], iters=[], read=[], tables=[], kernels=set())
    for t, variant in enumerate(schedule):
        ctx.set_variant(variant)
        if inject is not None:
            inject(t, store)
        if store is not None:
            res["read"].append(store.cpu().numpy())
        res["tables"].append(a.cpu().numpy())
        r = ctx.run_steps(a, b, 1, targets=tg, knn_k=K, knn_radius=RADIUS, x=out["x"], status=out["status"],
                          obj=out["obj"], iters=out["iters"], traj_t=traj_t, step_index=t, **NOISE)
        torch.cuda.synchronize()
        res["kernels"].add(ctx.kernel_name)
        if r["final"] is b:
            a, b = b, a
        for k in ("status", "obj", "iters"):
            res[k].append(out[k].cpu().numpy())
    for k in ("status", "obj", "iters", "read", "tables"):
        res[k] = np.array(res[k])
    res["final"] = a.cpu().numpy()
    res["store"] = None if store is None else store.cpu().numpy()
    return res


@functools.lru_cache(maxsize=None)
def _cold(mpclib, schedule, scale=0.6):
    """The run without a store (computed once per layout schedule and lattice, never modified)."""
    r = _loop(mpclib, schedule, scale=scale)
    it0 = r["iters"][:, :, 0]
    print(f"cold {schedule[0]}..{schedule[-1]} at {scale}: max iteration-0 steps {it0.max()}, "
          f"solves with >= 3 steps {np.count_nonzero(it0 >= 3)}, kernels {sorted(r['kernels'])}")
    assert it0.max() >= 3, "the scenario has no iteration-0 solve of >= 3 steps: nothing to warm-start"
    assert not any("store" in k for k in r["kernels"]), r["kernels"]
    return r


def _same_results(got, ref, what):
    """Test 1's criteria: statuses identical, objectives and final states within 1e-7 relative."""
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=what)
    check_routes_agree(got["obj"], ref["obj"], what + ": objective")
    assert np.all(np.isfinite(ref["final"])), what
    check_routes_agree(got["final"], ref["final"], what + ": final state")
    print(f"{what}: iters differ at {np.count_nonzero(got['iters'] != ref['iters'])} of {ref['iters'].size}, "
          f"solver steps {got['iters'].sum()} vs cold {ref['iters'].sum()}")


# ---- 1. warm = cold ---------------------------------------------------------------------------

def _cbf_keys_read(run):
    """CBF keys (negative, among a record's first k keys) in the stores the steps read."""
    read = run["read"]
    live = np.arange(5)[None, None, :] < read[:, :, :1]
    return int(np.count_nonzero((read[:, :, 1:6] < 0) & live))


@pytest.mark.parametrize("scale", [0.6, 0.45])
@pytest.mark.parametrize("variant", [SEP16, WIDE])
def test_warm_run_equals_cold_run(mpclib, variant, scale):
    schedule = (variant,) * STEPS
    cold = _cold(mpclib, schedule, scale)
    warm = _loop(mpclib, schedule, store0=np.zeros((N, 8)), min_steps=1, scale=scale)
    assert all("store" in k for k in warm["kernels"]), warm["kernels"]  # the store kernels ran
    _same_results(warm, cold, f"warm vs cold, variant {variant}, lattice {scale}")
    # the warm path ran: records with sides were read, and some solve took other steps than cold
    assert np.any(warm["read"][1:, :, 0] > 0)
    assert np.any(warm["iters"] != cold["iters"])
    print(f"CBF keys read: {_cbf_keys_read(warm)}")
    if scale == 0.45:
        assert _cbf_keys_read(warm) >= 20
    # export only (min_steps < 0): never warm-started, so even the iteration counts are the cold run's
    export = _loop(mpclib, schedule[:8], store0=np.zeros((N, 8)), min_steps=-1, scale=scale)
    np.testing.assert_array_equal(export["iters"], cold["iters"][:8])
    np.testing.assert_array_equal(export["status"], cold["status"][:8])
    np.testing.assert_array_equal(export["obj"], cold["obj"][:8])
    assert np.any(export["store"][:, 0] > 0)


# ---- 2. exported sets are the active constraints ------------------------------------------------

@pytest.mark.parametrize("variant", [SEP16, WIDE])
def test_exported_sets_are_the_active_constraints(mpclib, variant):
    torch = require_gpu()
    cfg = swarm.config(15)
    # the evolved table: on the 0.45 x lattice (CBF sides active), the closed loop's table whose step
    # exported the most CBF sides, from an export-only run (= the cold run)
    export = _loop(mpclib, (variant,) * 12, store0=np.zeros((N, 8)), min_steps=-1, scale=0.45)
    written = np.concatenate([export["read"][1:], export["store"][None]])  # step t's records
    n_neg = [sum(int(np.count_nonzero(r[1:1 + r[0]] < 0)) for r in w) for w in written]
    t_best = int(np.argmax(n_neg[2:])) + 2  # (not the lattice itself: at least two steps in)
    evolved = export["tables"][t_best]
    print(f"variant {variant}: CBF sides exported per step {n_neg}, table of step {t_best}")
    _, targets = _scenario(scale=0.45)
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    store = ctx.alloc_active_store(N)
    ctx.set_active_store(store, 1)  # (a zero store: every solve starts cold)
    st = torch.tensor(evolved, device=dev)
    out = ctx.alloc_outputs(N)
    nb_out = torch.full((N, 16), -7, dtype=torch.int32, device=dev)
    ctx.impc_solve(st, targets=torch.tensor(targets, device=dev), knn_k=K, knn_radius=RADIUS, x=out["x"],
                   status=out["status"], obj=out["obj"], iters=out["iters"], nb_out=nb_out)
    torch.cuda.synchronize()
    rec, status, iters = store.cpu().numpy(), out["status"].cpu().numpy(), out["iters"].cpu().numpy()
    x, nbs = out["x"].cpu().numpy(), nb_out.cpu().numpy()
    ops = mpclib._lib.host_operators(cfg)
    G, Gs, lo, hi = ops["G"], ops["Gs"], ops["lo"], ops["hi"]
    # rows of G per channel, in order (the header's box-key rule)
    chan_rows = [[i for i in range(ops["m"]) if np.any(G[i, 2 * d:2 * d + 2] != 0.0)] for d in range(3)]
    assert sorted(sum(chan_rows, [])) == list(range(ops["m"]))
    n_box = n_cbf = n_zero = 0
    worst = 0.0
    for a in range(N):
        opt = [it for it in range(2) if status[a, it] == mpclib.OPTIMAL]
        k = rec[a, 0]
        assert 0 <= k <= 5, (a, rec[a])
        if not opt:
            assert not rec[a].any(), (a, rec[a], status[a])
            continue
        last = opt[-1]
        # fast start: the unconstrained minimiser holds every row, no side is active (an iteration 1
        # of 0 steps after an iteration 0 with steps confirmed the set handed over: not a fast start)
        if iters[a, :last + 1].sum() == 0:
            assert k == 0, (a, rec[a], iters[a])
        if not rec[a].any():  # (an empty set found in 0 steps, or an optimum without an exact set)
            n_zero += iters[a, last] > 0
            continue
        assert rec[a, 7] == last, (a, rec[a], status[a])
        # steps: the solve's own, plus the sides iteration 0 handed to iteration 1 (none in iteration 0:
        # the store was empty)
        if last == 0:
            assert rec[a, 6] == iters[a, 0], (a, rec[a], iters[a])
        else:
            assert iters[a, 1] <= rec[a, 6] <= iters[a, 1] + 5, (a, rec[a], iters[a])
        assert not rec[a, 1 + k:6].any(), (a, rec[a])
        sides = mpclib.decode_active_sides(rec[a])
        assert len(set(sides)) == k, (a, sides)
        y = np.linalg.lstsq(ops["Z"], x[a] - ops["Xs"] @ evolved[a], rcond=None)[0]
        for s in sides:
            if s[0] == "cbf":
                n_cbf += 1
                assert s[1] in nbs[a][nbs[a] >= 0], (a, s, nbs[a])
                assert s[2] < (1 if last == 0 else cfg["cbf_horizon"]), (a, s)
            else:
                n_box += 1
                _, d, r, up = s
                assert r < len(chan_rows[d]), (a, s)
                i = chan_rows[d][r]
                bound = (hi[i] if up else lo[i]) - Gs[i] @ evolved[a]
                res = abs(G[i] @ y - bound) / (1.0 + abs(bound))
                worst = max(worst, res)
                assert res <= 1e-8, (a, s, res)
    print(f"variant {variant}: {np.count_nonzero(rec[:, 0] > 0)} agents with sides, {n_box} box sides "
          f"(worst scaled residual {worst:.2e}), {n_cbf} CBF sides, max k {rec[:, 0].max()}, "
          f"{n_zero} optima after > 0 steps without a record")
    assert n_box > 0 and n_cbf > 0 and rec[:, 0].max() >= 2


# ---- 3. stale and hostile records ---------------------------------------------------------------

def _hostile_records(kmax):
    """Keys that name non-neighbours, huge and out-of-range values, inert and out-of-range rows,
    both sides of one row and duplicates, next to a few rows the operators have, under a steps word
    that passes any threshold. Records hold 1 .. kmax keys, kmax the most the layout's solver takes
    (16-lane 5, wide 4: a longer record starts cold before any key is looked at, the k_7 case), so
    every key reaches the layout's range checks, neighbour comparison and duplicate filter."""
    rec = np.zeros((N, 8), dtype=np.int64)
    for a in range(N):
        far = (a + N // 2) % N  # across the lattice: never among the 8 nearest within 6 m
        pool = [-(1 + far * 8), -(1 + (2 ** 27) * 8 + 7), INT_MIN, -1 - 8 * a, 1000, 96, 95, 94, 2 ** 31 - 1,
                62, 63, 30, 30, 7, 42]
        rec[a, 0] = 1 + a % kmax
        rec[a, 1:6] = [pool[(a + j) % len(pool)] for j in range(5)]
        rec[a, 6] = 2 ** 30
        rec[a, 7] = a % 3
    return rec.astype(np.int32)


@pytest.mark.parametrize("variant", [SEP16, WIDE])
@pytest.mark.parametrize("kind", ["other_swarm", "hostile_keys", "k_7"])
def test_stale_and_hostile_records_are_harmless(mpclib, variant, kind):
    steps = 12
    schedule = (variant,) * steps
    cold = _cold(mpclib, (variant,) * STEPS)
    cold = {k: (v[:steps] if k != "final" else None) for k, v in cold.items() if k in ("status", "obj", "iters", "final")}
    if kind == "other_swarm":
        other = _loop(mpclib, schedule, store0=np.zeros((N, 8)), min_steps=1, seed=swarm.SEED + 1)["store"]
        assert np.any(other[:, 0] > 0)
        got = _loop(mpclib, schedule, store0=other, min_steps=1)
    else:
        bad = _hostile_records(5 if variant == SEP16 else 4)
        if kind == "k_7":
            bad[:, 0] = 7
        torch = require_gpu()
        bad_dev = torch.tensor(bad, device=torch.device("cuda", 0))
        # (re-written before every step: each step's solve reads the hostile records, not its own)
        got = _loop(mpclib, schedule, store0=bad, min_steps=1, inject=lambda t, store: store.copy_(bad_dev))
    np.testing.assert_array_equal(got["status"], cold["status"], err_msg=kind)
    check_routes_agree(got["obj"], cold["obj"], f"{kind}, variant {variant}: objective")
    print(f"iters differ at {np.count_nonzero(got['iters'] != cold['iters'])} of {cold['iters'].size}")
    if kind == "k_7":  # more sides than any solver holds: every solve started cold
        np.testing.assert_array_equal(got["iters"], cold["iters"])
    else:  # the records reached the mapping: some solve took other steps than the cold run's
        assert np.any(got["iters"] != cold["iters"]), kind


# ---- 4. cross-layout ----------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [0.6, 0.45])
@pytest.mark.parametrize("first,second", [(SEP16, WIDE), (WIDE, SEP16)])
def test_records_cross_layouts(mpclib, first, second, scale):
    """Records written by one layout start the other layout's solves: the layout changes after 12
    steps on one context and one store."""
    cut = 12
    schedule = (first,) * cut + (second,) * (STEPS - cut)
    cold = _cold(mpclib, schedule, scale)
    warm = _loop(mpclib, schedule, store0=np.zeros((N, 8)), min_steps=1, scale=scale)
    assert len(warm["kernels"]) == 2 and all("store" in k for k in warm["kernels"]), warm["kernels"]
    _same_results(warm, cold, f"layout {first} -> {second}, lattice {scale}")
    assert np.any(warm["read"][cut][:, 0] > 0)  # the other layout's records, as the first step after the cut read them
    assert np.any(warm["iters"][cut] != cold["iters"][cut])  # and they started its solves


# ---- 5. kernels without the store ----------------------------------------------------------------

@pytest.mark.parametrize("mode", ["slack", "fov"])
def test_unsupported_kernels_ignore_the_store(mpclib, mode):
    """Slack mode and the FoV controller never read the store and zero their agents' records:
    outputs bit-identical to a context without a store."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    if mode == "slack":
        cfg = swarm.config(15, slack_mode=1)
        states, targets = _scenario()
    else:
        cfg = swarm.fov_config()
        states, targets = swarm.heading_swarm(N)
        states[:, :2] *= 0.6
        targets[:, :2] *= 0.6
    first, count = 8, 48  # (rows outside the batch keep their contents)
    res = []
    for with_store in (False, True):
        ctx = mpclib.Context(cfg)
        store = None
        if with_store:
            store = torch.full((N, 8), 3, dtype=torch.int32, device=dev)
            ctx.set_active_store(store, 1)
        out = ctx.alloc_outputs(count)
        nxt = torch.empty((count, 6), dtype=torch.float64, device=dev)
        ctx.impc_solve(torch.tensor(states, device=dev), targets=torch.tensor(targets[first:first + count], device=dev),
                       agent_first=first, num_agents=count, knn_k=K, knn_radius=RADIUS, x=out["x"],
                       status=out["status"], obj=out["obj"], iters=out["iters"], next_states=nxt)
        torch.cuda.synchronize()
        assert "store" not in ctx.kernel_name, ctx.kernel_name
        res.append({k: out[k].cpu().numpy() for k in ("x", "status", "obj", "iters")} | {"next": nxt.cpu().numpy()})
        if with_store:
            s = store.cpu().numpy()
            assert not s[first:first + count].any()
            assert np.all(s[:first] == 3) and np.all(s[first + count:] == 3)
    same_bits(res[1], res[0], what=mode)
    assert np.any(res[0]["status"] == mpclib.OPTIMAL)


# ---- 6. run_steps split in two calls --------------------------------------------------------------

@pytest.mark.parametrize("variant", [SEP16, WIDE])
def test_split_run_steps_with_store_matches_one_call(mpclib, variant):
    torch = require_gpu()
    cfg = swarm.config(15)
    states, targets = _scenario()
    dev = torch.device("cuda", 0)
    total, cut = 14, 6

    def run(parts):
        ctx = mpclib.Context(cfg)
        ctx.set_variant(variant)
        store = ctx.alloc_active_store(N)
        ctx.set_active_store(store, 1)
        a = torch.tensor(states, device=dev)
        b = torch.empty_like(a)
        out = ctx.alloc_outputs(N)
        log = torch.full((total, N, 2), -7, dtype=torch.int32, device=dev)
        ilog = torch.full((total, N, 2), -7, dtype=torch.int32, device=dev)
        done = 0
        for n in parts:
            r = ctx.run_steps(a, b, n, targets=torch.tensor(targets, device=dev), knn_k=K, knn_radius=RADIUS,
                              x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"],
                              status_log=log[done:], iters_log=ilog[done:], step_index=done,
                              continue_tables=done > 0)
            if r["final"] is b:
                a, b = b, a
            done += n
        torch.cuda.synchronize()
        return dict(final=a.cpu().numpy(), store=store.cpu().numpy(), log=log.cpu().numpy(), ilog=ilog.cpu().numpy(),
                    x=out["x"].cpu().numpy(), obj=out["obj"].cpu().numpy())

    one, two = run([total]), run([cut, total - cut])
    assert not np.any(one["log"] == -7) and np.any(one["store"][:, 0] > 0)
    for k in one:
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)


# ---- the rows check and the Python checks ---------------------------------------------------------

def test_store_argument_checks(mpclib):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg = swarm.config(15)
    states, targets = _scenario()
    ctx = mpclib.Context(cfg)
    small = ctx.alloc_active_store(N - 1)
    assert small.shape == (N - 1, 8) and small.dtype == torch.int32 and not small.any()
    ctx.set_active_store(small)
    out = ctx.alloc_outputs(N)
    solve = lambda: ctx.impc_solve(torch.tensor(states, device=dev), targets=torch.tensor(targets, device=dev),  # noqa: E731
                                   knn_k=K, knn_radius=RADIUS, x=out["x"], status=out["status"])
    with pytest.raises(mpclib.MpccbfError, match=r"active store: rows \(63\) < num_states \(64\)"):
        solve()
    ctx.set_active_store(None)  # detached: the same call runs
    solve()
    torch.cuda.synchronize()
    assert not small.any()
    for bad in (torch.zeros((N, 8), dtype=torch.int32), torch.zeros((N, 8), dtype=torch.int64, device=dev),
                torch.zeros((N, 7), dtype=torch.int32, device=dev), torch.zeros((N * 8,), dtype=torch.int32, device=dev),
                torch.zeros((N, 16), dtype=torch.int32, device=dev)[:, ::2], np.zeros((N, 8), dtype=np.int32)):
        with pytest.raises(mpclib.MpccbfError):
            ctx.set_active_store(bad)


def test_simulator_warm_flag(mpclib):
    """Simulator(warm=True) attaches a store; its statuses are those of warm=False."""
    from mpccbf.sim import Simulator
    require_gpu()
    cfg = swarm.config(15)
    states, targets = _scenario()
    runs = []
    for warm in (False, True):
        sim = Simulator(cfg, states, targets, record=False, warm=warm)
        for _ in range(6):
            sim.step()
        runs.append(sim)
    assert runs[0].active_store is None and runs[1].active_store is not None
    assert np.any(runs[1].active_store.cpu().numpy()[:, 0] > 0)
    np.testing.assert_array_equal(np.array(runs[0].status_log), np.array(runs[1].status_log))
    a, b = runs[0].states.cpu().numpy(), runs[1].states.cpu().numpy()
    assert np.all(np.isfinite(a))
    check_routes_agree(b, a, "warm against cold states")

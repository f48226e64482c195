"""GPU: what a long-lived mpccbf Context carries from one call to the next.

The other GPU tests compare single calls and single closed loops with the oracle, nearly always
on a fresh Context. A context that serves a whole run (bench.py, mpccbf/sim.py, the
qpcpp::HIPSolver adapter) also holds the grid-mode neighbour tables with their continuation
record, the two alternating deferral queues, scratch that grows on demand, and the layout variant
with the last launch size. These tests reuse one context across calls and hold it to the result
of the same call on a fresh one:

(a) a continue_tables call after a call that rewrote the recorded state table rebuilds;
(b) the FoV kernels through a continuation (3 + 4 + 5 steps == 12 steps);
(c) seeded call sequences on one context == every call alone on a fresh context, bit for bit;
(d) agent counts at the tail of a wave / block against the oracle, rows past num_agents untouched;
(e) a PreparedRun's timing arrays survive its next call;
(f) solve_stride times the solves it names, and timing of any kind changes no result.

Bit equality is the bar in (a)-(c): both sides run the same kernel, launch size and inputs, every
agent is solved independently of the deferral queue's order, and the suite already holds the
kernels to run-to-run and rank-split bit identity (test_fov_closed_loop_is_deterministic,
test_gpu_multirank.py).
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_harness import _manual_loop, fresh_outputs, require_gpu, run_oracle, to_device, to_host
from mpccbf import swarm
from parity_rule import check_parity, same_bits

pytestmark = pytest.mark.gpu

K, RADIUS = 8, 6.0
WIDE, SEP = "impc_wide_kernel<256>", "impc_sep_kernel<1,1,false,256>"
OUT_KEYS = ("x", "status", "obj", "iters")


def _csr_device(torch, dev, rp, col, first=0, count=None):
    """Device CSR lists of agents [first, first + count) (row_ptr[0] may be nonzero)."""
    count = len(rp) - 1 - first if count is None else count
    return dict(nb_row_ptr=to_device(rp[first:first + count + 1]),
                nb_col=to_device(col))


# ---- (a) continuation after a foreign write ----------------------------------------------------

def _moved_rows(before, after):
    return np.count_nonzero(np.max(np.abs(before - after), axis=1) > 1e-6)


def _foreign_write_sequence(mpclib, torch, cfg, st0, refill, tg, first, count, interlude, cont):
    """3 grid steps, the interlude (which rewrites the table the 3 steps ended in and ends in that
    same table; zero_step: the caller copies `refill` into it), 4 grid steps with
    continue_tables=cont; one fresh context. Returns the final states, the last call's status log
    and the table before / after the interlude (host)."""
    dev = st0.device
    ctx = mpclib.Context(cfg)
    out = ctx.alloc_outputs(count)
    grid = dict(targets=tg, agent_first=first, num_agents=count, knn_k=K, knn_radius=RADIUS)
    a, b = st0.clone(), torch.empty_like(st0)
    r = ctx.run_steps(a, b, 3, x=out["x"], obj=out["obj"], **grid)
    tab = r["final"]  # the table the continuation record names
    alt = a if tab is b else b
    torch.cuda.synchronize()
    before = tab.cpu().numpy()
    if interlude == "zero_step":
        tab.copy_(refill)
        r = ctx.run_steps(tab, alt, 0, x=out["x"], obj=out["obj"], **grid)
        assert r["final"] is tab
    else:
        rp, col = swarm.knn_csr(before, K, RADIUS)
        csr = dict(targets=tg, agent_first=first, num_agents=count, **_csr_device(torch, dev, rp, col, first, count))
        if interlude == "csr_run":
            r = ctx.run_steps(tab, alt, 2, x=out["x"], obj=out["obj"], **csr)
            assert r["final"] is tab
        else:  # csr_solve: two single steps ping-pong through next_states, back into the table
            alt.copy_(tab)  # (rows outside the batch carry over)
            ctx.impc_solve(tab, next_states=alt[first:first + count], x=out["x"], obj=out["obj"], **csr)
            ctx.impc_solve(alt, next_states=tab[first:first + count], x=out["x"], obj=out["obj"], **csr)
    torch.cuda.synchronize()
    after = tab.cpu().numpy()
    log = torch.full((4, count, 2), -7, dtype=torch.int32, device=dev)
    r = ctx.run_steps(tab, alt, 4, x=out["x"], obj=out["obj"], status_log=log, step_index=5,
                      continue_tables=cont, **grid)
    torch.cuda.synchronize()
    return r["final"].cpu().numpy(), log.cpu().numpy(), before, after


@pytest.mark.parametrize("interlude", ["csr_run", "csr_solve", "zero_step"])
@pytest.mark.parametrize("first,count", [(0, 256), (12, 244)])
def test_continuation_after_foreign_write_rebuilds(mpclib, first, count, interlude):
    """mpccbf_run::continue_tables after a call that rewrote the recorded state table at the same
    address — a 2-step CSR-mode run_steps, two CSR-mode impc_solve calls that ping-pong back into
    it, or a zero-step run_steps after the caller refilled it: the continuing call must rebuild the
    neighbour table (it holds copies of the neighbours' states), so it equals the identical
    sequence with continue_tables=False, bit for bit. Precondition checked on the host: the
    interlude moved at least a quarter of the table's rows by more than 1e-6 — otherwise a stale
    table would go unseen.
    zero_step refills the table with the same swarm at lattice scale 0.45, not with the initial
    states themselves: on the initial 0.6 lattice hardly a CBF row is active at the first step's
    optimum (oracle: solved with and without neighbours, every agent's curve agrees to 3.2e-6,
    within its solver tolerance; at 0.45, 169 of 256 curves or statuses change), so a stale
    neighbour table changed no result and that refill passed on the library without the fix (0 of
    256 final rows differed). With the 0.45 refill 165 / 156 of 256 final rows differed there, and
    17 of 256 in each of the other two cases."""
    torch = require_gpu()
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(256, seed=6)
    states[:, :2] *= 0.6
    crowded = states.copy()
    crowded[:, :2] *= 0.75  # lattice scale 0.45
    dev = torch.device("cuda", 0)
    st0, refill = torch.tensor(states, device=dev), torch.tensor(crowded, device=dev)
    tg = torch.tensor(targets[first:first + count], device=dev)
    args = (mpclib, torch, cfg, st0, refill, tg, first, count, interlude)
    ref, ref_log, _, _ = _foreign_write_sequence(*args, False)
    got, got_log, before, after = _foreign_write_sequence(*args, True)
    moved = _moved_rows(before, after)
    print(f"foreign write {interlude} ({first}, {count}): {moved} of 256 rows moved, "
          f"{np.count_nonzero(np.any(got != ref, axis=1))} final rows differ")
    assert moved >= 64, moved
    assert not np.any(ref_log == -7)
    if interlude == "zero_step":  # the last call starts from the refilled table: 4 steps one by one
        loop, loop_status = _manual_loop(mpclib.Context(cfg), refill, tg, 4, first, count, torch)
        same_bits(ref, loop)
        same_bits(ref_log[-1], loop_status)
    same_bits(got, ref)
    same_bits(got_log, ref_log)


# ---- (b) FoV continuation ----------------------------------------------------------------------

@pytest.mark.parametrize("slack", [False, True])
def test_fov_run_steps_continuation_matches_one_call(mpclib, slack):
    """test_run_steps_continuation_matches_one_call's scheme for the FoV kernels
    (impc_fov_kernel<false|true>, which bench.py runs through a continuation): 3 + 4 + 5 steps in
    three calls, continuing, and with a grid-mode impc_solve between the second and third call
    (which then rebuilds), == 12 steps in one call: bit-identical states and statuses."""
    torch = require_gpu()
    over = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.5) if slack else {}
    cfg = swarm.fov_config(20, **over)
    n = 256
    states, targets = swarm.heading_swarm(n)
    dev = torch.device("cuda", 0)
    st0 = torch.tensor(states, device=dev)
    cov = torch.tensor(np.tile([0.1, 0.0, 0.1], (n, 1)), device=dev) if slack else None
    common = dict(targets=torch.tensor(targets, device=dev), knn_k=K, knn_radius=cfg["fov_Rs"], cov=cov)
    ctx = mpclib.Context(cfg)
    assert ctx.kernel_name == ("impc_fov_kernel<true>" if slack else "impc_fov_kernel<false>")
    out = ctx.alloc_outputs(n)
    a, b = st0.clone(), torch.empty_like(st0)
    log1 = torch.full((12, n, 2), -7, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, b, 12, x=out["x"], obj=out["obj"], status_log=log1, **common)
    torch.cuda.synchronize()
    ref, ref_log = r["final"].cpu().numpy(), log1.cpu().numpy()
    assert not np.any(ref_log == -7) and np.any(ref_log == O.OPTIMAL)
    assert _moved_rows(states, ref) >= n // 2
    for mode in ("continue", "interrupted"):
        c = mpclib.Context(cfg)
        o = c.alloc_outputs(n)
        a, b = st0.clone(), torch.empty_like(st0)
        log2 = torch.full((12, n, 2), -7, dtype=torch.int32, device=dev)
        s = 0
        for k in (3, 4, 5):
            if mode == "interrupted" and s == 7:  # a grid-mode solve between the calls
                c.impc_solve(a, **common)
            r = c.run_steps(a, b, k, x=o["x"], obj=o["obj"], status_log=log2[s:s + k], step_index=s,
                            continue_tables=s > 0, **common)
            if r["final"] is not a:
                a, b = b, a
            s += k
        torch.cuda.synchronize()
        same_bits(a.cpu().numpy(), ref, what=mode)
        same_bits(log2.cpu().numpy(), ref_log, what=mode)


# ---- (c) call sequences on one context ---------------------------------------------------------

def _op(n, nb, scale, kind="solve", variant=None, stream=False, first=0, count=None, seed=0):
    return dict(n=n, nb=nb, scale=scale, kind=kind, variant=variant, stream=stream, first=first,
                count=n - first if count is None else count, seed=seed)


# State-table sizes 64 -> 1025 -> 17 -> 36 -> 1024 -> 1 -> 64: the grid scratch and the deferral
# queues grow and then serve smaller batches; the default variant crosses wide_max (1,024 on
# MI355X) in both directions. variant: set_variant before the operation (None: left as it is).
COLLISION_OPS = [
    _op(64, "grid", 0.42, variant=0, seed=1),                   # wide kernel, deferrals
    _op(64, "knn", 1.0, seed=2),
    _op(1025, "grid", 0.42, kind="run3", seed=3),               # variant 0 beyond wide_max: 16-lane kernel
    _op(1025, "knn", 0.42, seed=4),                             # 16-lane kernel with the deferral queue
    _op(1025, "grid", 1.0, variant=5, seed=5),                  # wide kernel at any count
    _op(17, "grid", 0.42, variant=0, stream=True, seed=6),      # smaller batch on the grown buffers
    _op(17, "knn", 0.42, kind="run3", variant=4, seed=7),
    _op(36, "all", 0.42, variant=0, seed=8),                    # the 128-slot capacity launch
    _op(1024, "grid", 0.42, kind="run3", variant=4, seed=9),
    _op(1024, "grid", 0.42, variant=0, stream=True, seed=10),   # wide kernel at exactly wide_max
    _op(1024, "knn", 1.0, seed=11),
    _op(1024, "grid", 0.42, kind="run3", first=100, count=613, stream=True, seed=12),
    _op(1, "grid", 1.0, seed=13),
    _op(1, "knn", 1.0, kind="run3", variant=5, seed=14),
    _op(64, "grid", 0.42, kind="run3", variant=0, first=5, count=50, seed=15),
    _op(64, "all", 1.0, variant=4, seed=16),
]

FOV_OPS = [
    _op(64, "grid", 1.0, seed=21),
    _op(300, "fov", 0.6, seed=22),
    _op(17, "grid", 0.6, kind="run3", seed=23),
    _op(300, "grid", 0.6, kind="run3", stream=True, first=30, count=200, seed=24),
    _op(1, "grid", 1.0, seed=25),
    _op(64, "fov", 0.6, kind="run3", seed=26),
    _op(300, "grid", 1.0, stream=True, seed=27),
]


def _op_inputs(cfg, op):
    """Host inputs of one operation (seeded): states, the batch's targets, CSR lists or None."""
    fov = cfg["cbf_mode"] == 1
    states, targets = (swarm.heading_swarm if fov else swarm.lattice_swarm)(op["n"], seed=100 + op["seed"])
    states[:, :2] *= op["scale"]
    if fov:
        targets[:, :2] *= op["scale"]
    lists = None
    if op["nb"] == "knn":
        lists = swarm.knn_csr(states, K, RADIUS)
    elif op["nb"] == "fov":
        lists = swarm.fov_csr(states, K, cfg["fov_Rs"], cfg["fov_beta"])
    elif op["nb"] == "all":
        lists = swarm.all_csr(op["n"])
    cov = np.tile([0.1, 0.0, 0.1], (op["n"], 1)) if fov and cfg["slack_mode"] else None
    return states, targets[op["first"]:op["first"] + op["count"]], lists, cov


def _run_op(ctx, cfg, op, inputs, torch):
    """One operation on ctx; every output and the written state table on the host."""
    dev = torch.device("cuda", 0)
    states, targets, lists, cov = inputs
    first, count = op["first"], op["count"]
    st = torch.tensor(states, device=dev)
    kw = dict(targets=torch.tensor(targets, device=dev), agent_first=first, num_agents=count,
              cov=None if cov is None else torch.tensor(cov, device=dev))
    if lists is None:
        kw.update(knn_k=K, knn_radius=cfg["fov_Rs"] if cfg["cbf_mode"] == 1 else RADIUS)
    else:
        kw.update(_csr_device(torch, dev, lists[0], lists[1], first, count))
    out = {k: v for k, v in fresh_outputs(ctx, count).items() if k in OUT_KEYS}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev) if op["stream"] else None
    if op["kind"] == "run3":
        alt = torch.full_like(st, float("nan"))
        r = ctx.run_steps(st, alt, 3, stream=stream, **kw, **out)
        torch.cuda.synchronize()
        nxt = r["final"]
    else:
        nxt = torch.full((count, 6), float("nan"), dtype=torch.float64, device=dev)
        ctx.impc_solve(st, next_states=nxt, stream=stream, **kw, **out)
        torch.cuda.synchronize()
    res = to_host(out)
    res["next"] = nxt.cpu().numpy()
    return res


def _run_sequence(mpclib, torch, cfg, ops):
    """ops in order on one Context, and each alone on a fresh Context: compared bit for bit.
    Returns the kernel names that ran and every operation's result."""
    reused = mpclib.Context(cfg)
    variant = 0
    names, results = [], []
    for i, op in enumerate(ops):
        inputs = _op_inputs(cfg, op)
        if op["variant"] is not None and op["variant"] != variant:
            variant = op["variant"]
            reused.set_variant(variant)
        got = _run_op(reused, cfg, op, inputs, torch)
        names.append(reused.kernel_name)
        fresh = mpclib.Context(cfg)
        fresh.set_variant(variant)
        ref = _run_op(fresh, cfg, op, inputs, torch)
        assert fresh.kernel_name == names[-1], (i, fresh.kernel_name, names[-1])
        fresh.close()
        assert not np.any(ref["status"] == -7), (i, op)
        same_bits(got, ref, keys=OUT_KEYS + ("next",), what=f"operation {i} {op}")
        results.append(got)
    return names, results


def test_collision_call_sequence_matches_fresh_contexts(mpclib):
    """16 seeded operations on one collision-controller Context — state tables of 64, 1025, 17,
    36, 1024, 1 and 64 agents; grid mode, CSR kNN lists and all-neighbours CSR; lattice scales 0.42
    (deferrals to phase 1 and the PDIP, INFEASIBLE agents) and 1.0; set_variant 0, 4 and 5 between
    them; 3-step run_steps next to single impc_solve calls, part ranges, non-default streams —
    each give x, status, obj, iters and the next states of the same operation alone on a fresh
    Context, bit for bit: nothing the context carries (grown grid scratch, deferral queues and their
    parity, continuation record, variant and last launch size) leaks into a result."""
    torch = require_gpu()
    cfg = swarm.config(15)
    assert len(COLLISION_OPS) >= 12 and sum(op["stream"] for op in COLLISION_OPS) >= 2
    names, results = _run_sequence(mpclib, torch, cfg, COLLISION_OPS)
    assert WIDE in names and SEP in names, names
    # the default variant on both sides of wide_max
    assert names[2] == SEP and names[9] == WIDE, names
    status = np.concatenate([r["status"].ravel() for r in results])
    iters = np.concatenate([r["iters"].ravel() for r in results])
    assert np.any((status != O.OPTIMAL) & (status != -7))
    assert np.any(status == O.INFEASIBLE)
    assert np.any((status == O.OPTIMAL) & (iters > 0))


@pytest.mark.parametrize("slack", [False, True])
def test_fov_call_sequence_matches_fresh_contexts(mpclib, slack):
    """The same for a FoV Context (impc_fov_kernel<false|true>): grid and CSR calls, single solves
    and 3-step runs, tables of 64, 300, 17 and 1 agents, mixed on one context."""
    torch = require_gpu()
    over = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.5) if slack else {}
    cfg = swarm.fov_config(20, **over)
    names, results = _run_sequence(mpclib, torch, cfg, FOV_OPS)
    assert set(names) == {"impc_fov_kernel<true>" if slack else "impc_fov_kernel<false>"}, names
    status = np.concatenate([r["status"].ravel() for r in results])
    assert np.any(status == O.OPTIMAL)


# ---- (d) small agent counts against the oracle, guarded tails ----------------------------------

SMALL_N = (1, 2, 3, 5, 15, 16, 17, 63, 65)
SMALL_SCALES = (0.55, 0.45)
GUARD = 7


@functools.lru_cache(maxsize=None)
def _small_case(n, scale):
    """Inputs and oracle results of one (n, scale), computed once and shared (read only)."""
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(n, seed=11)
    states[:, :2] *= scale
    rp, col = swarm.knn_csr(states, K, RADIUS)
    ref = run_oracle(cfg, states, targets, rp, col, list(range(n)))
    return states, targets, rp, col, ref


@pytest.fixture(scope="module")
def small_sweep(mpclib):
    """Every (variant, mode, scale, n) of the sweep solved once, one Context per variant, every
    output and the next-state table allocated for n + 7 agents and filled with a sentinel."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    cfg = swarm.config(15)
    res = {}
    for variant in (0, 4, 5):
        ctx = mpclib.Context(cfg)
        ctx.set_variant(variant)
        for scale in SMALL_SCALES:
            for n in SMALL_N:
                states, targets, rp, col, _ = _small_case(n, scale)
                st, tg = torch.tensor(states, device=dev), torch.tensor(targets, device=dev)
                for mode in ("csr", "grid"):
                    out = fresh_outputs(ctx, n + GUARD)
                    nb = _csr_device(torch, dev, rp, col) if mode == "csr" else dict(knn_k=K, knn_radius=RADIUS)
                    ctx.impc_solve(st, targets=tg, num_agents=n, **nb, **out)
                    torch.cuda.synchronize()
                    res[variant, mode, scale, n] = (to_host(out), ctx.kernel_name)
    return res


@pytest.mark.parametrize("mode", ["csr", "grid"])
@pytest.mark.parametrize("variant", [0, 4, 5])
def test_small_agent_counts_match_oracle_with_guarded_tails(small_sweep, variant, mode):
    """Agent counts at the tail of a wave or block — 1, 2, 3, 5 (the one-agent-per-wave kernel runs
    4 agents per 256-thread block), 15, 16, 17, 63, 65 (the 16-lane kernel 16 per block) — for the
    layout variants 0, 4 and 5, CSR kNN lists and grid mode, on lattice_swarm(n, seed=11) at scale
    0.55 (every QP OPTIMAL) and 0.45 (INFEASIBLE agents from n = 15 on): every agent against the
    oracle at the project's parity tolerances (statuses equal, objective 1e-4, control points
    1e-5), and the 7 rows after num_agents of every output and of the next-state table keep their
    sentinel."""
    cfg = swarm.config(15)
    for scale in SMALL_SCALES:
        for n in SMALL_N:
            g, name = small_sweep[variant, mode, scale, n]
            assert name == (SEP if variant == 4 else WIDE), (variant, n, name)
            ref = _small_case(n, scale)[4]
            check_parity({k: v[:n] for k, v in g.items()}, ref, list(range(n)))
            for k, v in g.items():
                tail = v[n:]
                assert tail.shape[0] == GUARD
                untouched = np.isnan(tail) if v.dtype == np.float64 else tail == -7
                assert np.all(untouched), (variant, mode, scale, n, k, tail)
            assert not np.any(g["status"][:n] == -7) and not np.any(np.isnan(g["next_states"][:n]))


def test_small_agent_counts_cover_hard_qps(small_sweep):
    """The sweep is not all fast starts: at scale 0.45 every n >= 15 has an INFEASIBLE agent
    (oracle and GPU), and over the whole sweep at least 20 OPTIMAL QPs took solver steps on the
    GPU (iters > 0; measured on MI355X with scales 0.55 and 0.45: 2,916)."""
    for n in SMALL_N:
        ref = _small_case(n, 0.55)[4]
        assert all(list(r["status"]) == [O.OPTIMAL, O.OPTIMAL] for r in ref), n
        if n >= 15:
            ref = _small_case(n, 0.45)[4]
            assert any(r["status"][0] == O.INFEASIBLE or r["status"][1] == O.INFEASIBLE for r in ref), n
    hard = 0
    for (variant, mode, scale, n), (g, _) in small_sweep.items():
        st, it = g["status"][:n], g["iters"][:n]
        if scale == 0.45 and n >= 15:
            assert np.any(st == O.INFEASIBLE), (variant, mode, n)
        hard += np.count_nonzero((st == O.OPTIMAL) & (it > 0))
    print(f"small-count sweep: {hard} OPTIMAL QPs with iters > 0")
    assert hard >= 20, hard


# ---- (e) PreparedRun reuse ---------------------------------------------------------------------

def test_prepared_run_timings_survive_the_next_call(mpclib):
    """PreparedRun.__call__ hands out step_ms and solve_ms as copies: the library overwrites its
    host buffers at the next call, which must not change (or alias) an earlier result."""
    torch = require_gpu()
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(64, seed=6)
    states[:, :2] *= 0.6
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    a = torch.tensor(states, device=dev)
    run = ctx.prepare_run_steps(a, torch.empty_like(a), 3, targets=torch.tensor(targets, device=dev),
                                knn_k=K, knn_radius=RADIUS, timing=True)
    r1 = run()
    kept = {k: r1[k].copy() for k in ("step_ms", "solve_ms")}
    assert kept["step_ms"].shape == (3,) and np.all(kept["step_ms"] > 0) and np.all(kept["solve_ms"] > 0)
    r2 = run()
    for k in ("step_ms", "solve_ms"):
        assert not np.shares_memory(r1[k], r2[k]), k
        np.testing.assert_array_equal(r1[k], kept[k], err_msg=k)
        assert np.all(r2[k] > 0), k


# ---- (f) solve_stride --------------------------------------------------------------------------

def _timed_run(mpclib, torch, **timing):
    """5 grid steps of the base collision config at 64 agents on a fresh context; the call's
    result, and the final table, the status log and x on the host."""
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(64, seed=6)
    states[:, :2] *= 0.6
    dev = torch.device("cuda", 0)
    ctx = mpclib.Context(cfg)
    out = ctx.alloc_outputs(64)
    a = torch.tensor(states, device=dev)
    log = torch.full((5, 64, 2), -7, dtype=torch.int32, device=dev)
    r = ctx.run_steps(a, torch.empty_like(a), 5, targets=torch.tensor(targets, device=dev), knn_k=K,
                      knn_radius=RADIUS, x=out["x"], status_log=log, **timing)
    torch.cuda.synchronize()
    return r, (r["final"].cpu().numpy(), log.cpu().numpy(), out["x"].cpu().numpy())


def test_solve_stride_times_every_other_solve_and_changes_no_result(mpclib):
    """mpccbf_run::solve_stride = 2 over 5 steps: step_ms has its 5 positive entries, solve_ms the
    3 of steps 0, 2 and 4 (the untimed steps' -1 dropped), each positive and no longer than its
    step (the margin of test_run_steps_matches_step_by_step); solve_stride = 1 times all 5. Which
    events a call records changes nothing it computes: the final table, the status log and x of
    both timed runs equal those of an untimed run, bit for bit."""
    torch = require_gpu()
    _, plain = _timed_run(mpclib, torch, timing=False)
    assert not np.any(plain[1] == -7)
    every, got1 = _timed_run(mpclib, torch, timing=True, solve_stride=1)
    other, got2 = _timed_run(mpclib, torch, timing=True, solve_stride=2)
    print(f"solve_stride 1: step_ms {every['step_ms']} solve_ms {every['solve_ms']}\n"
          f"solve_stride 2: step_ms {other['step_ms']} solve_ms {other['solve_ms']}")
    assert every["step_ms"].shape == (5,) and every["solve_ms"].shape == (5,)
    assert np.all(every["step_ms"] > 0) and np.all(every["solve_ms"] > 0)
    assert np.all(every["solve_ms"] <= every["step_ms"] + 1e-3)
    assert other["step_ms"].shape == (5,) and np.all(other["step_ms"] > 0)
    assert other["solve_ms"].shape == (3,) and np.all(other["solve_ms"] > 0)
    assert np.all(other["solve_ms"] <= other["step_ms"][[0, 2, 4]] + 1e-3)
    for got in (got1, got2):
        for g, p, name in zip(got, plain, ("final table", "status log", "x")):
            same_bits(g, p, what=name)

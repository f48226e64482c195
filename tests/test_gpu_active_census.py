"""GPU: parity by active-set size. The collision IMPC kernels on QPs whose optimum has exactly 0 .. 6
active sides (active_census_cases.py; each claim proved on the CPU by test_active_census_inputs.py),
on both sides of the caps where the solve changes route:

  16 lanes per agent (set_variant(4)): the dual active set's factor holds DK = 5 sides
  (pdip_sep.hpp); a sixth gives up (`if (k == DK) return 0;`) to the interior-point solver and its
  active-set finish. One agent per wave (set_variant(5)): WK = 4 (impc_wide.hpp); a fifth side hands
  the agent to the capacity launch. The step limit (dual_as_steps) takes the same hand-over.

Every launch solves SOLVED = 63 agents of a 64-row table with explicit lists, so the last wave of
every layout is partly filled. Rules: parity with the oracle (parity_rule.check_parity: OBJ_TOL,
X_TOL) on every row, nothing left out; bit identity of a row's outputs wherever it sits in the batch
(same_bits); ROUTE_REL between two device routes to the same QP; 1e-8 scaled residual for an
exported box side (test_gpu_active_store.py)."""
import functools

import numpy as np
import pytest

import active_census_cases as A
from gpu_harness import fresh_outputs, require_gpu, to_device, to_host
from parity_rule import ROUTE_REL, check_parity, check_routes_agree, same_bits

pytestmark = pytest.mark.gpu

DENSE16, DENSE64 = "impc_kernel<6,16,4>", "impc_kernel<6,64,4>"
SEP, WIDE = "impc_sep_kernel<1,1,false,256>", "impc_wide_kernel<256>"
SEP_LEAN = "impc_sep_kernel<1,1,false,256,false,true>"
SEP_STORE, WIDE_STORE = "impc_sep_store_kernel<1,256,false>", "impc_wide_store_kernel<256>"
SEP16, WIDE64 = 4, 5
# tag -> (variant, options, the kernel of 63 agents with caller lists). The one-agent-per-wave layout
# has no interior-point path: with the active set switched off (dual_as_steps < 0) the launch plan
# takes the dense 64-lane kernel for it, by design (test_launch_plan.py).
OPTION_SETS = {
    "v0": (0, {}, WIDE), "v3": (3, {}, DENSE16), "v4": (SEP16, {}, SEP), "v5": (WIDE64, {}, WIDE),
    "v4/steps1": (SEP16, dict(dual_as_steps=1), SEP), "v4/pdip": (SEP16, dict(dual_as_steps=-1), SEP),
    "v5/steps1": (WIDE64, dict(dual_as_steps=1), WIDE), "v5/pdip": (WIDE64, dict(dual_as_steps=-1), DENSE64),
    "v4/lean": (SEP16, dict(lean=True), SEP_LEAN), "v5/lean": (WIDE64, dict(lean=True), WIDE),
    "v4/nofilter": (SEP16, dict(no_cbf_filter=True), SEP),
}
for _steps in (3, 4, 5, 6):  # the step limit on the boundary (test c)
    OPTION_SETS[f"v4/steps{_steps}"] = (SEP16, dict(dual_as_steps=_steps), SEP)
    OPTION_SETS[f"v5/steps{_steps}"] = (WIDE64, dict(dual_as_steps=_steps), WIDE)
PARITY_SETS = ["v0", "v3", "v4", "v5", "v4/steps1", "v4/pdip", "v5/steps1", "v5/pdip", "v4/lean", "v5/lean",
               "v4/nofilter"]
OUT_KEYS = ("status", "obj", "x", "next_states", "iters")
N = A.SOLVED


@functools.lru_cache(maxsize=None)
def _contexts(mpclib, config, tag, store):
    """One context per configuration, option set and store mode (None: no store; else min_steps)."""
    variant, opts, _ = OPTION_SETS[tag]
    ctx = mpclib.Context(A.CONFIGS[config], **opts)
    if variant:
        ctx.set_variant(variant)
    rec = None
    if store is not None:
        rec = ctx.alloc_active_store(A.ROWS)
        ctx.set_active_store(rec, store)
    return ctx, rec


@functools.lru_cache(maxsize=None)
def _solve(mpclib, config, tag, order, store=None):
    """One impc_solve of the first N rows of batch(order, config) (computed once, never modified):
    the outputs as host arrays, "rec" (the store after the solve) with a store."""
    torch = require_gpu()
    b = A.batch(order, config)
    ctx, rec = _contexts(mpclib, config, tag, store)
    if rec is not None:
        rec.zero_()
    out = fresh_outputs(ctx, N)
    ctx.impc_solve(to_device(b["states"]), to_device(b["rp"][:N + 1], torch.int32), to_device(b["col"], torch.int32),
                   targets=to_device(b["targets"]), agent_first=0, num_agents=N, **out)
    torch.cuda.synchronize()
    want = OPTION_SETS[tag][2]
    if store is not None:
        want = {SEP: SEP_STORE, WIDE: WIDE_STORE}[want]
    assert ctx.kernel_name == want, (config, tag, ctx.kernel_name, want)  # the layout that was asked for
    got = to_host(out)
    if rec is not None:
        got["rec"] = rec.cpu().numpy()
    return got


def _perms(config):
    return A.permutations(config)


def _oracle_rows(config, order):
    ref = A.reference(config)
    return [ref[o] for o in order[:N]]


# ---- a + d. parity at every k, wherever the row sits ------------------------------------------------

@pytest.mark.parametrize("tag", PARITY_SETS)
@pytest.mark.parametrize("config", sorted(A.CONFIGS))
def test_parity_at_every_k_and_placement(mpclib, config, tag):
    """Every row of every permutation against the oracle (no row left out: the CPU test proved every
    status stable), and every row's outputs bit-identical across the four permutations — each
    cap-crossing case sits once in each 16-lane group of a wave and once in the last, partly filled
    wave, among wave-mates that take 0 steps."""
    perms = _perms(config)
    worst = [0.0, 0.0]
    first = None
    for p, order in enumerate(perms):
        got = _solve(mpclib, config, tag, order)
        eo, ex = check_parity(got, _oracle_rows(config, order), label=f"{config}/{tag}/perm{p}")
        worst = [max(worst[0], eo), max(worst[1], ex)]
        by_old = {o: i for i, o in enumerate(order[:N])}  # old row -> this permutation's row
        if first is None:
            first = (got, by_old)
            continue
        common = sorted(set(by_old) & set(first[1]))
        rows_a, rows_b = [by_old[o] for o in common], [first[1][o] for o in common]
        same_bits({k: got[k][rows_a] for k in OUT_KEYS}, {k: first[0][k][rows_b] for k in OUT_KEYS},
                  what=f"{config}/{tag}: permutation {p} against permutation 0")
    print(f"{config}/{tag}: worst objective error {worst[0]:.3e} (<= 1e-4), worst |dx| {worst[1]:.3e} (<= 1e-5)")


# ---- b. the route each k takes ------------------------------------------------------------------

def _census_new_rows(config, order):
    """Per new row: the census of both iterations with the CBF sides' neighbours as new row indices."""
    cens, b = A.batch_census(config), A.batch(order, config)
    out = []
    for o in order[:N]:
        out.append([{(s if s[0] == "box" else ("cbf", int(b["row_of"][s[1]]), s[2])) for s in m["active"]}
                    for m in cens[o]])
    return out


def _check_record(mpclib, config, order, got, a, want, tag):
    """Row a's record equals the census `want` of the last iteration; returns the worst scaled
    residual of its box sides at the device's own solution."""
    rec = got["rec"][a]
    if not want and not rec.any():  # (an empty set found in 0 steps: the fast start writes no record)
        return 0.0
    assert rec[0] == len(want) and rec[7] == 1, (tag, a, rec, want)
    assert not rec[1 + rec[0]:6].any(), (tag, a, rec)
    sides = mpclib.decode_active_sides(rec)
    assert len(sides) == len(set(sides)) and set(sides) == want, (tag, a, sides, want)
    b = A.batch(order, config)
    y = A.reduced(b["cfg"], b["states"][a], got["x"][a])
    worst = 0.0
    for key, g, bound in A.sides(b["cfg"], b["states"], a, [], 1, got["x"][a]):
        if key in want:
            res = abs(g @ y - bound) / (1.0 + abs(bound))
            worst = max(worst, res)
            assert res <= 1e-8, (tag, a, key, res)
    return worst


@pytest.mark.parametrize("config", sorted(A.CONFIGS))
def test_route_by_active_set_size(mpclib, config):
    """Export-only store (min_steps -1: never warm-started), one solve per layout and permutation.
    16-lane: up to DK = 5 sides the record is the census; at 6 the dual active set has given up, and
    the record is all zero — warm_count() sets act[POL_K] = -1 before every solve (impc_sep.hpp:491),
    only a converged sep_dual_as writes a set there (pdip_sep.hpp save_sides), and as_word_sep returns
    0 for every word of a set with k < 0 (active_store.hpp:80, called at impc_sep.hpp:782).
    Wide: up to WK = 4 the record is the census; 5 and 6 are handed over and agree with the 16-lane
    layout's result, and where the hand-over writes a record, it is the census."""
    perms = _perms(config)
    names = A.layout(config)[0]
    worst_box = worst_route = 0.0
    table = []
    seen16, seen_wide, handed = set(), set(), set()  # active-set sizes met: in-kernel, handed over
    for p, order in enumerate(perms):
        g4 = _solve(mpclib, config, "v4", order, store=-1)
        g5 = _solve(mpclib, config, "v5", order, store=-1)
        ref = _oracle_rows(config, order)
        for g, tag in ((g4, "v4 store"), (g5, "v5 store")):
            check_parity(g, ref, label=f"{config}/{tag}/perm{p}")
        # export only: the results are those of the kernels without a store
        for tag, g in (("v4", g4), ("v5", g5)):
            plain = _solve(mpclib, config, tag, order)
            np.testing.assert_array_equal(g["status"], plain["status"])
            check_routes_agree(g["obj"], plain["obj"], f"{config}/{tag}: store kernel against plain, objective")
        cens = _census_new_rows(config, order)
        ego = A.batch(order, config)["ego"]
        case_of = {r: n for n, r in ego.items()}
        for a in range(N):
            k0, k1 = len(cens[a][0]), len(cens[a][1])
            want = cens[a][1]
            assert list(g4["status"][a]) == [0, 0] and list(g5["status"][a]) == [0, 0]
            # 16 lanes per agent
            if k1 <= 5:
                worst_box = max(worst_box, _check_record(mpclib, config, order, g4, a, want, "v4"))
                seen16.add(k1)
            else:
                assert not g4["rec"][a].any(), (a, g4["rec"][a])
                seen16.add(6)
            if k0 == 6:
                assert g4["iters"][a, 0] >= 6, (a, g4["iters"][a])
            # one agent per wave
            if k1 <= 4:
                worst_box = max(worst_box, _check_record(mpclib, config, order, g5, a, want, "v5"))
                seen_wide.add(k1)
            else:
                if g5["rec"][a].any():
                    worst_box = max(worst_box, _check_record(mpclib, config, order, g5, a, want, "v5 handed over"))
                handed.add(k1)
            if max(k0, k1) >= 5:
                for key in ("obj", "x", "next_states"):
                    worst_route = max(worst_route, check_routes_agree(g5[key][a], g4[key][a],
                                                                      f"{config}/row {a}: wide against 16-lane, {key}"))
            if p == 0 and a in case_of:
                table.append((case_of[a], (k0, k1), g4["iters"][a].tolist(), int(g4["rec"][a, 0]), bool(g4["rec"][a].any()),
                              g5["iters"][a].tolist(), int(g5["rec"][a, 0]), bool(g5["rec"][a].any())))
    print(f"\n{'case':<14}{'k (it 0, 1)':<13}{'16-lane iters':<15}{'rec k':<7}{'wide iters':<13}{'rec k':<6}")
    for name, k, i4, r4, any4, i5, r5, any5 in sorted(table, key=lambda t: (t[1][1], t[0])):
        print(f"{name:<14}{str(k):<13}{str(i4):<15}{(str(r4) if any4 else 'zero'):<7}{str(i5):<13}"
              f"{(str(r5) if any5 else 'zero'):<6}")
    print(f"{config}: worst scaled residual of an exported box side {worst_box:.2e} (<= 1e-8), worst relative "
          f"difference wide / 16-lane at k >= 5 {worst_route:.2e} (<= {ROUTE_REL})")
    # nothing vacuous: every size on both sides of each cap was met
    if config == "base":
        assert seen16 == set(range(7)) and seen_wide == set(range(5)) and handed == {5, 6}, (seen16, seen_wide, handed)
        assert len(names) >= 30
    else:
        assert {4, 5, 6} <= seen16 and 4 in seen_wide and handed == {5, 6}, (seen16, seen_wide, handed)


# ---- c. the step limit on the boundary ----------------------------------------------------------

@pytest.mark.parametrize("variant", [SEP16, WIDE64])
@pytest.mark.parametrize("name", ["box_4", "cbf1_4", "box_5", "cbf1_5"])
def test_step_limit_on_the_boundary(mpclib, name, variant):
    """dual_as_steps = k - 1, k, k + 1 for a case with k active sides in iteration 0 (a cold active
    set needs k steps at least): parity on the whole batch at all three, and at k + 1 the case's
    result is the default options' result."""
    order = _perms("base")[0]
    a = A.batch(order)["ego"][name]
    k = A.FOUND[name][4][0]
    ref = _oracle_rows("base", order)
    v = "v4" if variant == SEP16 else "v5"
    default = _solve(mpclib, "base", v, order)
    for steps in (k - 1, k, k + 1):
        got = _solve(mpclib, "base", f"{v}/steps{steps}", order)
        check_parity(got, ref, label=f"{v}, dual_as_steps {steps} ({name}: k = {k})")
        print(f"{name} on {v} with dual_as_steps {steps}: iters {got['iters'][a].tolist()} "
              f"(default options {default['iters'][a].tolist()})")
    np.testing.assert_array_equal(got["status"][a], default["status"][a])
    for key in ("obj", "x", "next_states"):
        check_routes_agree(got[key][a], default[key][a], f"{name} on {v}: dual_as_steps {k + 1} against default, {key}")


# ---- e. warm start at the cap ---------------------------------------------------------------------

def _run(mpclib, variant, steps, with_store):
    torch = require_gpu()
    order = _perms("base")[0]
    b = A.batch(order)
    ctx = mpclib.Context(b["cfg"])
    ctx.set_variant(variant)
    rec = None
    if with_store:
        rec = ctx.alloc_active_store(A.ROWS)
        ctx.set_active_store(rec, 1)
    t0 = to_device(b["states"])
    t1 = t0.clone()  # (row 63, never solved, carries over)
    out = fresh_outputs(ctx, N)
    log = torch.full((steps, N, 2), -7, dtype=torch.int32, device=t0.device)
    ilog = torch.full((steps, N, 2), -7, dtype=torch.int32, device=t0.device)
    r = ctx.run_steps(t0, t1, steps, targets=to_device(b["targets"]), agent_first=0, num_agents=N,
                      nb_row_ptr=to_device(b["rp"][:N + 1], torch.int32), nb_col=to_device(b["col"], torch.int32),
                      x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"], status_log=log,
                      iters_log=ilog)
    torch.cuda.synchronize()
    assert ("store" in ctx.kernel_name) == with_store, ctx.kernel_name
    return dict(final=r["final"].cpu().numpy()[:N], obj=out["obj"].cpu().numpy(), log=log.cpu().numpy(),
                ilog=ilog.cpu().numpy(), rec=None if rec is None else rec.cpu().numpy())


@pytest.mark.parametrize("variant", [SEP16, WIDE64])
def test_warm_start_at_the_cap(mpclib, variant):
    """3 closed-loop steps of the batch (box_5, box_6, cbf1_6 and the rest) with a store that
    warm-starts every solve (min_steps 1) against the run without one: a full record (k = 5 =
    AS_KEYS) and a set that does not fit (k = 6: no record) are both harmless — statuses identical,
    objectives and final states within ROUTE_REL (test_gpu_active_store._same_results' rule)."""
    cold, warm = _run(mpclib, variant, 3, False), _run(mpclib, variant, 3, True)
    assert not np.any(cold["log"] == -7) and not np.any(warm["log"] == -7)
    np.testing.assert_array_equal(warm["log"], cold["log"])
    check_routes_agree(warm["obj"], cold["obj"], f"variant {variant}: warm against cold, objective")
    assert np.all(np.isfinite(cold["final"]))
    check_routes_agree(warm["final"], cold["final"], f"variant {variant}: warm against cold, final state")
    ego = A.batch(_perms("base")[0])["ego"]
    for name in ("box_5", "box_6", "cbf1_6"):
        a = ego[name]
        print(f"{name} on variant {variant}: cold iters {cold['ilog'][:, a].tolist()}, warm {warm['ilog'][:, a].tolist()}, "
              f"record {warm['rec'][a].tolist()}")
    # the warm path ran: records with sides were written and read, and some solve took other steps
    assert np.any(warm["rec"][:, 0] > 0) and np.any(warm["ilog"] != cold["ilog"])
    if variant == SEP16:
        assert np.any(warm["rec"][:, 0] == 5), "no full record (k = 5 = AS_KEYS) was written"

"""GPU: parity by feasibility margin. The collision IMPC kernels on QPs whose minimal uniform row
violation t* was chosen (feasibility_cases.py; every level proved on the CPU by
test_feasibility_inputs.py): feasible with an interior 1e-3, 1e-5 and 3e-6 wide, infeasible by 3e-6 and
8e-6 (below the dual active set's 10 feas_tol certificate rule: phase 1 decides), 1.2e-5 (just above
it), 1e-3 and 1e-1 — on each of the four routes to INFEASIBLE (constant rows, a single CBF row, the
certificate, phase 1).

Every launch solves SOLVED = 127 agents of a 128-row table with explicit lists, so the last wave of
every layout is partly filled, and asserts the kernel it meant to run. Rules: parity with the oracle
(parity_rule.check_parity: OBJ_TOL, X_TOL) on every row, nothing left out; bit identity of a row's
outputs wherever it sits in the batch (same_bits); ROUTE_REL between two device routes to the same
QP; the exported t* within a factor T_RATIO of the LP's."""
import functools

import numpy as np
import pytest

import feasibility_cases as F
import oracle_lib as O
from gpu_harness import fresh_outputs, require_gpu, to_device, to_host
from parity_rule import ROUTE_REL, X_TOL, check_parity, check_routes_agree, same_bits
from test_gpu_active_census import OPTION_SETS as CENSUS_SETS, PARITY_SETS as CENSUS_PARITY

pytestmark = pytest.mark.gpu

SLACK_KERNEL = "impc_sep_kernel<1,2,true,256>"  # test_gpu_parity.test_slack_mode_matches_oracle
OPTION_SETS = {tag: CENSUS_SETS[tag] for tag in CENSUS_PARITY}
OPTION_SETS["slack"] = (0, {}, SLACK_KERNEL)
# (configuration, option set): the census's parity sets on both tables, the slack configuration on
# its default variant
LAUNCHES = [(c, t) for c in ("asym", "base") for t in CENSUS_PARITY] + [("slack", "slack")]
OUT_KEYS = ("status", "obj", "x", "next_states", "iters", "primal_res", "dual_res")
N = F.SOLVED
# The exported t* (primal_res of an INFEASIBLE iteration) over the LP's: the certificate exports a
# lower bound and phase 1 an upper one, and the outputs do not say which ran, so the rule is
# two-sided. Measured on an MI355X over 1276 finite values: 0.520852 (pair_skew_m3e-6's iteration 1
# wherever the dual active set runs first: its certificate's lower bound of a t* of 4.6) to 1.051809
# (pair_skew_p3e-6 on the dense 16-lane layout: phase 1's early exit); at the levels +3e-6 .. +1.2e-5
# alone 0.999304 to 1.051809. T_RATIO is twice the worst ratio either way, 2 x 1 / 0.520852.
T_RATIO = 3.84


def _sets(config):
    return [t for c, t in LAUNCHES if c == config]


@functools.lru_cache(maxsize=None)
def _context(mpclib, config, tag):
    variant, opts, _ = OPTION_SETS[tag]
    ctx = mpclib.Context(F.CONFIGS[config], **opts)
    if variant:
        ctx.set_variant(variant)
    return ctx


@functools.lru_cache(maxsize=None)
def _solve(mpclib, config, tag, order):
    """One impc_solve of the first N rows of batch(order, config) with every output requested
    (computed once, never modified): the outputs as host arrays."""
    torch = require_gpu()
    b = F.batch(order, config)
    ctx = _context(mpclib, config, tag)
    out = fresh_outputs(ctx, N)
    assert out["primal_res"] is not None and out["dual_res"] is not None
    ctx.impc_solve(to_device(b["states"]), to_device(b["rp"][:N + 1], torch.int32), to_device(b["col"], torch.int32),
                   targets=to_device(b["targets"]), agent_first=0, num_agents=N, **out)
    torch.cuda.synchronize()
    assert ctx.kernel_name == OPTION_SETS[tag][2], (config, tag, ctx.kernel_name)  # the layout that was asked for
    return to_host(out)


def _perms(config):
    return F.permutations(F.TABLE_OF[config])


def _oracle_rows(config, order):
    ref = F.reference(config)
    return [ref[o] for o in order[:N]]


def _egos(config, order):
    """(name, spec, new row, old row) of every ego among the solved rows."""
    b = F.batch(order, config)
    old = F.batch(F.IDENTITY, config)["ego"]
    return [(n, F.FOUND[n], a, old[n]) for n, a in sorted(b["ego"].items()) if a < N]


# ---- a + b. parity at every level, wherever the row sits ---------------------------------------------

@pytest.mark.parametrize("config,tag", LAUNCHES)
def test_parity_at_every_level_and_placement(mpclib, config, tag):
    """Every row of every permutation against the oracle — the statuses at the levels are the point
    — and every row's outputs, residuals included, bit-identical across the four permutations: each
    ego sits once in each 16-lane group of a wave, the pair egos at +3e-6 .. +1.2e-5 once in the last,
    partly filled wave."""
    perms = _perms(config)
    first = None
    per_level = {}
    for p, order in enumerate(perms):
        got = _solve(mpclib, config, tag, order)
        ref = _oracle_rows(config, order)
        check_parity(got, ref, label=f"{config}/{tag}/perm{p}")
        for name, spec, a, _ in _egos(config, order):
            w = per_level.setdefault(spec[2], [0.0, 0.0, 0])
            w[2] += 1
            for it in range(2):
                if ref[a]["status"][it] == O.OPTIMAL:
                    w[0] = max(w[0], abs(got["obj"][a, it] - ref[a]["obj"][it]) / max(1.0, abs(ref[a]["obj"][it])))
                    last = it
            if ref[a]["status"][0] == O.OPTIMAL:
                w[1] = max(w[1], float(np.max(np.abs(got["x"][a] - ref[a]["x"][last][:got["x"].shape[1]]))))
        by_old = {o: i for i, o in enumerate(order[:N])}  # old row -> this permutation's row
        if first is None:
            first = (got, by_old)
            continue
        common = sorted(set(by_old) & set(first[1]))
        rows_a, rows_b = [by_old[o] for o in common], [first[1][o] for o in common]
        same_bits({k: got[k][rows_a] for k in OUT_KEYS}, {k: first[0][k][rows_b] for k in OUT_KEYS},
                  what=f"{config}/{tag}: permutation {p} against permutation 0")
    for level in sorted(per_level):
        eo, ex, cnt = per_level[level]
        print(f"{config}/{tag} level {level:+.1e}: {cnt} ego solves, worst objective error {eo:.3e} (<= 1e-4), "
              f"worst |dx| {ex:.3e} (<= 1e-5)")


# ---- c. what a row without a curve returns ---------------------------------------------------------

@pytest.mark.parametrize("config,tag", LAUNCHES)
def test_rows_without_a_curve(mpclib, config, tag):
    """include/mpccbf.h: no OPTIMAL iteration — x all NaN, obj NaN, next_states the input state, bit
    for bit; [OPTIMAL, INFEASIBLE] — obj[1] NaN, x iteration 0's (check_parity) and next_states that
    curve at t = h. The curve's tolerance is X_TOL on the control points, so X_TOL on a position (a
    Bezier point is a convex combination) and 12 X_TOL on a velocity (a cubic piece 0.5 s long:
    3 / 0.5 times a difference of two control points)."""
    cfg = F.CONFIGS[config]
    p = O.make_params(cfg)
    none = kept = 0
    for order in _perms(config):
        got, ref, b = _solve(mpclib, config, tag, order), _oracle_rows(config, order), F.batch(order, config)
        for a in range(N):
            st = [int(s) for s in ref[a]["status"]]
            assert [int(s) for s in got["status"][a]] == st
            if O.OPTIMAL not in st:
                assert np.all(np.isnan(got["x"][a])) and np.all(np.isnan(got["obj"][a])), (config, tag, a)
                same_bits(got["next_states"][a], b["states"][a], what=f"{config}/{tag} row {a}: next_states of a row without a curve")
                none += 1
            elif st == [O.OPTIMAL, O.INFEASIBLE]:
                assert np.isfinite(got["obj"][a, 0]) and np.isnan(got["obj"][a, 1]), (config, tag, a, got["obj"][a])
                x0 = ref[a]["x"][0]
                want = np.concatenate([O.eval_curve(p, x0, cfg["h"], 0), O.eval_curve(p, x0, cfg["h"], 1)])
                err = np.abs(got["next_states"][a] - want)
                assert err[:3].max() <= X_TOL and err[3:].max() <= 12.0 * X_TOL, (config, tag, a, err)
                kept += 1
    print(f"{config}/{tag}: {none} solves without a curve, {kept} that kept iteration 0's")
    assert none >= (4 * 12 if config == "slack" else 4) and (kept >= 4 or config == "slack")


# ---- d. the exported t* ------------------------------------------------------------------------------

def _tstar_rows(mpclib, config, tag, order):
    """Per INFEASIBLE iteration of an ego: (family, level, iteration, exported value, the LP's t*)."""
    got, lps = _solve(mpclib, config, tag, order), F.batch_tstar(F.TABLE_OF[config])
    out = []
    for name, spec, a, _ in _egos(config, order):
        for it in range(2):
            if got["status"][a, it] == O.INFEASIBLE:
                out.append((spec[1], spec[2], it, float(got["primal_res"][a, it]), lps[name][it]["t"]))
                assert np.isnan(got["dual_res"][a, it]), (config, tag, name, it)
    return out


@pytest.mark.parametrize("config", ["asym", "base", "slack"])
def test_exported_tstar(mpclib, config):
    """primal_res of an INFEASIBLE iteration is t* (finite, > feas_tol) or NaN (include/mpccbf.h).
    Every finite value is > feas_tol and within [1 / T_RATIO, T_RATIO] of the LP's t*; which rows
    export NaN is printed per option set (it is the same under every permutation: the bit identity
    of test_parity_at_every_level_and_placement)."""
    lo, hi, finite = np.inf, 0.0, 0
    for tag in _sets(config):
        rows = [r for order in _perms(config) for r in _tstar_rows(mpclib, config, tag, order)]
        table = {}
        for family, level, it, val, t in rows:
            key = (family, level, it)
            ent = table.setdefault(key, [np.inf, 0.0, 0, 0])
            if np.isnan(val):
                ent[3] += 1
                continue
            assert t > F.FEAS_TOL and val > F.FEAS_TOL, (config, tag, key, val, t)
            ent[0], ent[1], ent[2] = min(ent[0], val / t), max(ent[1], val / t), ent[2] + 1
        for key in sorted(table):
            r0, r1, cnt, nan = table[key]
            ratio = f"primal_res / t* in [{r0:.6f}, {r1:.6f}] ({cnt} values)" if cnt else "no finite value"
            print(f"{config}/{tag} {key[0]} at {key[1]:+.1e}, iteration {key[2]}: {ratio}, {nan} NaN")
            if cnt:
                lo, hi, finite = min(lo, r0), max(hi, r1), finite + cnt
                assert 1.0 / T_RATIO <= r0 and r1 <= T_RATIO, (config, tag, key, r0, r1)
    print(f"{config}: exported t* over the LP's in [{lo:.6f}, {hi:.6f}] over {finite} finite values (T_RATIO {T_RATIO})")
    assert finite > 0 or config == "slack"  # (slack: only the velocity cases are INFEASIBLE, by the constant rows)


# ---- e. routes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["asym", "base"])
def test_routes_agree(mpclib, config):
    """The lean launch (fast start and dual active set in the main kernel, the rest deferred) against
    the full one on both layouts: statuses identical, objectives, curves and next states within
    ROUTE_REL; and the statuses identical across every option set of the configuration."""
    for p, order in enumerate(_perms(config)):
        base = _solve(mpclib, config, _sets(config)[0], order)
        for tag in _sets(config)[1:]:
            np.testing.assert_array_equal(_solve(mpclib, config, tag, order)["status"], base["status"], err_msg=f"{config}/{tag}/perm{p}")
        for v in ("v4", "v5"):
            full, lean = _solve(mpclib, config, v, order), _solve(mpclib, config, v + "/lean", order)
            np.testing.assert_array_equal(lean["status"], full["status"])
            for key in ("obj", "x", "next_states"):
                check_routes_agree(lean[key], full[key], f"{config}/perm{p}: {v}/lean against {v}, {key}")


@pytest.mark.parametrize("config", ["asym", "base"])
def test_lean_step_counts(mpclib, config):
    """`iters` identical between the lean launch and the full one on both layouts, on every row. The
    QPs that only phase 1 can decide — pair_* and iter1_pair at +3e-6 and +8e-6, below the
    certificate's 10 feas_tol — are the ones at stake: the in-kernel completion and the fallback
    launch are two code objects of one source (test_gpu_inkernel_completion.py), phase 1 starts from
    the failed solve's last iterate and stops as soon as its decision is settled, and the two took 7
    and 9, 7 and 8, 8 and 7 phase-1 steps to the same t* (the trace build's split; active-set and PDIP
    steps identical). While the 16-lane kernel added those steps to `iters`, against include/mpccbf.h
    ("phase-1 steps not included"), this test failed on exactly these rows, [13, 0] against [15, 0]."""
    differ = []
    for p, order in enumerate(_perms(config)):
        who = {a: n for n, _, a, _ in _egos(config, order)}
        for v in ("v4", "v5"):
            full, lean = _solve(mpclib, config, v, order), _solve(mpclib, config, v + "/lean", order)
            for a in np.flatnonzero((lean["iters"] != full["iters"]).any(axis=1)):
                print(f"{config}/perm{p} row {a} ({who.get(a, 'no case')}): statuses {full['status'][a].tolist()}, iters "
                      f"{v} {full['iters'][a].tolist()}, {v}/lean {lean['iters'][a].tolist()}")
                differ.append((v, p, int(a), who.get(a)))
    assert not differ, differ

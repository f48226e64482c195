"""GPU: the formation-control rollouts (mpccbf_formation_rollout, mpccbf.FormationRollouts) against
the unchanged oracle, teacher-forced: every decision of a recorded run is repeated by the oracle on
the table that decision planned from, rebuilt from the run's own trace
(formation_rollout_cases.check_decisions; free-running comparison amplifies last-digit differences
through the CBF rows and is no test). Then the order witness, the shape edges, bit-for-bit
independence of split, place in the batch and optional outputs, the summary against mpccbf.metrics,
and the example's JSON record."""
import numpy as np
import pytest

import formation_rollout_cases as F
import oracle_lib as O
from gpu_harness import to_device, to_host
from mpccbf import metrics
from parity_rule import same_bits

pytestmark = pytest.mark.gpu

RECORDS = ("trace", "cbf_u", "desired_u", "status", "lambda2", "iters")
WIDTH = dict(trace=(6,), cbf_u=(3,), desired_u=(3,), status=(), lambda2=(), iters=())
SUMMARY = ("arrival_sample", "first_collision", "min_d2", "fail_count")
FILL = -12345  # the records' fill: what a run must overwrite, and what it must leave where it writes nothing


def run_raw(mpclib, cfg, team_ptr, states, targets, seeds, steps, step_first=0, records=RECORDS, summary=None,
            summary_keys=SUMMARY, steps_per_launch=0, pos_std=F.EDGE_NOISE["pos_std"], vel_std=F.EDGE_NOISE["vel_std"],
            shape_half=(0.2, 0.2), goal_radius=1.0):
    """One mpccbf_formation_rollout call on fresh device tensors through the thin binding (no host
    checks of the team sizes): host copies of the states after it, of the chosen records (filled with
    FILL before) and of the summary (summary: host arrays to continue from, None = initialised).
    records / summary_keys: the optional outputs the call is given; the others are NULL."""
    import torch
    dev = torch.device("cuda", 0)
    team_ptr = np.ascontiguousarray(team_ptr, dtype=np.int32)
    n, teams = int(team_ptr[-1]), len(team_ptr) - 1
    t = lambda a, dt=None: to_device(np.asarray(a, dtype=dt))  # noqa: E731
    d_states = t(states, np.float64)
    rec = {k: torch.full((steps, n) + WIDTH[k], FILL, dtype=torch.int32 if k in ("status", "iters") else torch.float64,
                         device=dev) for k in records}
    if summary is None:
        summary = dict(arrival_sample=np.full(n, -1, np.int32), first_collision=np.full((teams, 3), -1, np.int32),
                       min_d2=np.full(teams, np.inf), fail_count=np.zeros(teams, np.int32))
    summ = {k: t(summary[k]) for k in summary_keys}
    seed_bits = np.array([int(s) & ((1 << 64) - 1) for s in seeds], dtype=np.uint64).view(np.int64)
    mpclib.formation_rollout(cfg, t(team_ptr), d_states, t(targets, np.float64), t(seed_bits), steps, step_first,
                             Ts=cfg["Ts"], pos_std=pos_std, vel_std=vel_std, shape_half=shape_half,
                             goal_radius=goal_radius, steps_per_launch=steps_per_launch, **rec, **summ)
    torch.cuda.synchronize()
    out = to_host(rec)
    out.update(to_host(summ))
    out["states"] = d_states.cpu().numpy()
    return out


def team_rec(rec, r0, r1):
    return {k: rec[k][:, r0:r1] for k in RECORDS if k in rec}


def check_batch(cfg, states, targets, team_ptr, seeds, rec, step_first=0, skip=(), **noise):
    """check_decisions over every team of a batch (but `skip`): the mismatches, and the decisions seen."""
    noise = {**F.EDGE_NOISE, **noise}
    bad, seen = [], 0
    for t in range(len(team_ptr) - 1):
        r0, r1 = int(team_ptr[t]), int(team_ptr[t + 1])
        if t in skip or r1 == r0:
            continue
        got = F.check_decisions(cfg, states[r0:r1], targets[r0:r1], seeds[t], team_rec(rec, r0, r1), cfg["Ts"],
                                noise["pos_std"], noise["vel_std"], step_first=step_first)
        bad += [f"team {t} (n={r1 - r0}) {m}" for m in got]
        seen += (r1 - r0) * len(rec["trace"])
    return bad, seen


# ---- the parity batch, run once per slack mode -------------------------------------------------
@pytest.fixture(scope="module")
def parity_runs(mpclib):
    """slack -> list of (FormationRollouts after PARITY_STEPS steps, its records, the group of
    formation_rollout_cases.parity_groups it must be)."""
    import torch
    runs = {}
    for slack in (False, True):
        objs = mpclib.FormationRollouts.from_instances(F.PARITY_NAMES, [F.PARITY_SEED], preprocess="own", slack=slack)
        groups = F.parity_groups(slack)
        assert [names for _, names in objs] == [g["names"] for g in groups]
        out = []
        for (obj, _), g in zip(objs, groups):
            obj.run(F.PARITY_STEPS)
            torch.cuda.synchronize()
            out.append((obj, obj.records(), g))
        runs[slack] = out
    return runs


@pytest.mark.parametrize("slack", [False, True], ids=["plain", "slack"])
def test_decision_parity(parity_runs, slack):
    """1. Every decision of the 8 instances over 30 steps: status, branch, lambda2, u on OPTIMAL
    decisions, desired_u and the next state. None is left out."""
    bad, seen = [], 0
    for obj, rec, g in parity_runs[slack]:
        assert obj.cfg == g["cfg"] and (obj.pos_std, obj.vel_std) == (g["pos_std"], g["vel_std"])
        for t, (name, states, targets) in enumerate(g["teams"]):
            r0, r1 = int(obj.team_ptr_host[t]), int(obj.team_ptr_host[t + 1])
            assert r1 - r0 == len(states)
            got = F.check_decisions(g["cfg"], states, targets, F.PARITY_SEED, team_rec(rec, r0, r1), g["cfg"]["Ts"],
                                    g["pos_std"], g["vel_std"])
            bad += [f"{name}: {m}" for m in got]
            seen += len(states) * F.PARITY_STEPS
    print(f"slack={slack}: {seen} decisions, {len(bad)} mismatches")
    assert seen == 38 * F.PARITY_STEPS
    assert not bad, f"{len(bad)} mismatches, the first: " + "; ".join(bad[:5])


def test_parity_run_holds_what_it_is_there_to_see(parity_runs):
    """OPTIMAL and INFEASIBLE decisions, both branches and the zero-control fallback are in the GPU's
    own run (the CPU pin shows them in the oracle's)."""
    st = np.concatenate([rec["status"].ravel() for s in (False, True) for _, rec, _ in parity_runs[s]])
    l2 = np.concatenate([rec["lambda2"].ravel() for s in (False, True) for _, rec, _ in parity_runs[s]])
    u = np.concatenate([rec["cbf_u"].reshape(-1, 3) for s in (False, True) for _, rec, _ in parity_runs[s]])
    assert np.any(st == O.OPTIMAL) and np.any(st == O.INFEASIBLE)
    assert np.any(l2 > F.L2_SWITCH) and np.any(l2 <= F.L2_SWITCH)
    assert np.any(st != O.OPTIMAL) and np.all(u[st != O.OPTIMAL] == 0.0)


def test_order_witness(parity_runs):
    """2. The same check with every table taken wholly from the sample before (Jacobi) fails on
    5r/circle: the teacher-forced check cannot pass on the wrong order."""
    for obj, rec, g in parity_runs[False]:
        if "5r/circle" not in g["names"]:
            continue
        t = g["names"].index("5r/circle")
        _, states, targets = g["teams"][t]
        r0, r1 = int(obj.team_ptr_host[t]), int(obj.team_ptr_host[t + 1])
        args = (g["cfg"], states, targets, F.PARITY_SEED, team_rec(rec, r0, r1), g["cfg"]["Ts"], g["pos_std"], g["vel_std"])
        assert F.check_decisions(*args) == []
        wrong = F.check_decisions(*args, order="jacobi")
        print(f"jacobi tables: {len(wrong)} mismatches over {5 * F.PARITY_STEPS} decisions")
        assert len(wrong) >= 1
        return
    raise AssertionError("5r/circle is not in the batch")


def test_from_instances_on_the_base_config(mpclib):
    """preprocess="base" (the reference's run semantics) is uniform: one object, team t = instance
    t // seeds with noise key t % seeds, the base config's parameters, the instances' noise and box:
    every team's records equal, bit for bit, a call on that instance alone with that seed, and the seeds
    tell the copies of an instance apart.
    (Not a decision check against the oracle: at step 0 robot 0 of 5r/circle on the base config the
    desired control is exactly the velocity row's bound (u_x = -2 = k (target - pos) with v_min = -2), a
    solution without strict complementarity, where the interior-point method of the shared per-robot
    solve returns -1.99995872, 4.1e-5 off at tolerance 1e-9; the parity tests' 1e-5 does not hold
    there, for this kernel as for mpccbf_connectivity_control_solve, whose answer on that table is
    compared at the end: DESIGN section 2, row f9.)"""
    import torch
    from mpccbf import instances
    names, seeds = ["2r/line", "5r/circle"], [5, 6, 7]
    (obj, group), = mpclib.FormationRollouts.from_instances(names, seeds, preprocess="base")
    assert group == names
    assert obj.num_teams == 6 and obj.team_ptr_host.tolist() == [0, 2, 4, 6, 11, 16, 21]
    assert (obj.cfg["d_min"], obj.cfg["d_max"], obj.cfg["control_slack_mode"]) == (2.0, 4.0, 0)
    assert obj.cfg["v_max"][:2] == [2.0, 2.0] and (obj.pos_std, obj.vel_std) == (0.001, 0.01)
    obj.run(3)
    torch.cuda.synchronize()
    rec = obj.records()
    for t in range(6):
        _, states, targets, shape, kind, noise = instances.instance(names[t // 3], preprocess="base")
        r0, r1 = int(obj.team_ptr_host[t]), int(obj.team_ptr_host[t + 1])
        alone = run_raw(mpclib, obj.cfg, [0, r1 - r0], states, targets, [seeds[t % 3]], 3, shape_half=shape[:2], **noise)
        for k in RECORDS:
            same_bits(alone[k], rec[k][:, r0:r1], what=(t, k))
    assert rec["trace"][:, 0:2].tobytes() != rec["trace"][:, 2:4].tobytes()
    assert len(obj.results()) == 6
    # that first decision of 5r/circle is the batched controller's own answer on the same table
    _, states, targets, _, _, _ = instances.instance("5r/circle", preprocess="base")
    dev = torch.device("cuda", 0)
    ud = np.array([F.desired_control(states[i], targets[i]) for i in range(5)])
    u = torch.empty((5, 3), dtype=torch.float64, device=dev)
    mpclib.connectivity_control_solve(obj.cfg, torch.tensor([0, 5], dtype=torch.int32, device=dev),
                                      torch.tensor(states, device=dev), torch.tensor(ud, device=dev), u)
    torch.cuda.synchronize()
    r0 = int(obj.team_ptr_host[3])
    assert np.allclose(u.cpu().numpy()[0], rec["cbf_u"][0, r0], rtol=0.0, atol=1e-9)


# ---- 3. shape edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [False, True], ids=["plain", "slack"])
def test_team_sizes_1_2_15_16(mpclib, slack):
    cfg = F.edge_cfg(slack)
    states, targets, team_ptr, seeds = F.edge_batch([1, 2, 15, 16])
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 2)
    bad, seen = check_batch(cfg, states, targets, team_ptr, seeds, rec)
    assert seen == 2 * 34
    assert not bad, f"{len(bad)} mismatches, the first: " + "; ".join(bad[:5])
    for k in RECORDS:
        assert not np.any(rec[k] == FILL), k


@pytest.mark.parametrize("slack", [False, True], ids=["plain", "slack"])
def test_capacity_teams_on_the_connectivity_row(mpclib, slack):
    """15 and 16 robots on a lattice 1.0 apart: lambda2 1.6, so every decision takes the connectivity
    row, whose gradient and Hessian terms are summed over a full 16-lane group."""
    cfg = F.edge_cfg(slack)
    states, targets, team_ptr, seeds = F.dense_batch()
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 2)
    assert np.all(rec["lambda2"] > 1.0) and np.all(rec["status"] == O.OPTIMAL)
    bad, seen = check_batch(cfg, states, targets, team_ptr, seeds, rec)
    assert seen == 2 * 31
    assert not bad, f"{len(bad)} mismatches, the first: " + "; ".join(bad[:5])


def test_oversize_and_empty_teams(mpclib):
    """A team of 17 among solvable ones reports ERROR alone, with NaN cbf_u / lambda2, its states
    untouched and its trace rows copies of them; an empty team writes nothing."""
    cfg = F.edge_cfg()
    sizes = [3, 17, 2, 0, 4]
    states, targets, team_ptr, seeds = F.edge_batch(sizes)
    steps = 3
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, steps)
    bad, seen = check_batch(cfg, states, targets, team_ptr, seeds, rec, skip=(1,))
    assert seen == steps * 9 and not bad, bad[:5]
    r0, r1 = int(team_ptr[1]), int(team_ptr[2])
    assert np.all(rec["status"][:, r0:r1] == O.ERROR) and np.all(rec["iters"][:, r0:r1] == 0)
    assert np.all(np.isnan(rec["cbf_u"][:, r0:r1])) and np.all(np.isnan(rec["lambda2"][:, r0:r1]))
    same_bits(rec["states"][r0:r1], states[r0:r1])
    for s in range(steps):
        same_bits(rec["trace"][s, r0:r1], states[r0:r1])
        want = np.array([F.desired_control(states[i], targets[i]) for i in range(r0, r1)])
        assert np.allclose(rec["desired_u"][s, r0:r1], want, rtol=1e-12, atol=1e-12)
    others = np.ones(team_ptr[-1], dtype=bool)
    others[r0:r1] = False
    assert not np.any(rec["status"][:, others] == O.ERROR)
    assert rec["fail_count"].tolist()[1] == 17 * steps
    # the empty team: no rows to write, its summary as initialised
    assert rec["first_collision"][3].tolist() == [-1, -1, -1] and rec["min_d2"][3] == np.inf
    assert rec["fail_count"][3] == 0
    assert not np.any(rec["trace"][:, others] == FILL)


@pytest.mark.parametrize("teams", [1, 33, 300])
def test_batch_sizes(mpclib, teams):
    cfg = F.edge_cfg(teams == 33)
    sizes = [(1, 2, 3, 5, 8, 4)[t % 6] for t in range(teams)]
    states, targets, team_ptr, seeds = F.edge_batch(sizes, seed=teams)
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 2)
    bad, seen = check_batch(cfg, states, targets, team_ptr, seeds, rec)
    assert seen == 2 * int(team_ptr[-1])
    assert not bad, f"{len(bad)} mismatches, the first: " + "; ".join(bad[:5])


def test_zero_steps_and_one_step(mpclib):
    cfg = F.edge_cfg()
    states, targets, team_ptr, seeds = F.edge_batch([3, 5])
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 0)
    same_bits(rec["states"], states)
    assert np.all(rec["arrival_sample"] == -1) and np.all(rec["first_collision"] == -1)
    assert np.all(rec["min_d2"] == np.inf) and np.all(rec["fail_count"] == 0)
    assert all(rec[k].shape[0] == 0 for k in RECORDS)
    rec = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 1)
    bad, seen = check_batch(cfg, states, targets, team_ptr, seeds, rec)
    assert seen == 8 and not bad, bad[:5]
    same_bits(rec["states"], rec["trace"][0])
    assert np.all(np.isfinite(rec["min_d2"]))


# ---- 4. independence, bit for bit --------------------------------------------------------------
INDEP_SIZES = [(2, 3, 5, 8, 1, 16, 4)[t % 7] for t in range(33)]
INDEP_STEPS = 20
ALL = RECORDS + SUMMARY + ("states",)


@pytest.fixture(scope="module")
def indep(mpclib):
    cfg = F.edge_cfg(True)
    states, targets, team_ptr, seeds = F.edge_batch(INDEP_SIZES, seed=4)
    base = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, INDEP_STEPS)
    return cfg, states, targets, team_ptr, seeds, base


def test_split_and_chained_calls_change_nothing(mpclib, indep):
    cfg, states, targets, team_ptr, seeds, base = indep
    assert not np.any(base["trace"] == FILL)
    again = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, INDEP_STEPS)
    same_bits(base, again, ALL)
    for per in (1, 7, 32):  # (32: one launch)
        got = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, INDEP_STEPS, steps_per_launch=per)
        same_bits(base, got, ALL, what=per)
    a = run_raw(mpclib, cfg, team_ptr, states, targets, seeds, 12)
    b = run_raw(mpclib, cfg, team_ptr, a["states"], targets, seeds, 8, step_first=12,
                summary={k: a[k] for k in SUMMARY})
    chained = {k: np.concatenate([a[k], b[k]]) for k in RECORDS}
    chained.update({k: b[k] for k in SUMMARY + ("states",)})
    same_bits(base, chained, ALL)


def test_a_team_alone_equals_the_team_in_a_batch(mpclib, indep):
    cfg, states, targets, team_ptr, seeds, base = indep
    t = 17
    r0, r1 = int(team_ptr[t]), int(team_ptr[t + 1])
    assert r1 - r0 == INDEP_SIZES[17] >= 2
    alone = run_raw(mpclib, cfg, [0, r1 - r0], states[r0:r1], targets[r0:r1], [seeds[t]], INDEP_STEPS)
    for k in RECORDS:
        same_bits(alone[k], base[k][:, r0:r1], what=k)
    same_bits(alone["states"], base["states"][r0:r1])
    assert alone["arrival_sample"].tolist() == base["arrival_sample"][r0:r1].tolist()
    for k in ("first_collision", "min_d2", "fail_count"):
        same_bits(alone[k][0], base[k][t], what=k)
    # another seed is another run
    other = run_raw(mpclib, cfg, [0, r1 - r0], states[r0:r1], targets[r0:r1], [seeds[t] + 1], INDEP_STEPS)
    assert other["trace"].tobytes() != alone["trace"].tobytes()


@pytest.mark.parametrize("slack", [False, True], ids=["plain", "slack"])
def test_optional_outputs_change_nothing(mpclib, slack):
    """Every optional output — the six records and the four summary arrays — absent, alone and all
    together, on a batch with a team of 17 among solvable ones: the states and every output that is
    present are bit for bit those of the call with all of them."""
    cfg = F.edge_cfg(slack)
    states, targets, team_ptr, seeds = F.edge_batch([3, 17, 2, 8, 16, 1], seed=9)
    steps = 5
    run = lambda rec, summ: run_raw(mpclib, cfg, team_ptr, states, targets, seeds, steps, records=rec,  # noqa: E731
                                    summary_keys=summ)
    base = run(RECORDS, SUMMARY)
    assert not np.any(base["trace"] == FILL) and base["fail_count"][1] == 17 * steps
    cases = [(RECORDS, ()), ((), SUMMARY), ((), ())]
    cases += [((k,), SUMMARY) for k in RECORDS] + [((k,), ()) for k in RECORDS]
    cases += [((), (k,)) for k in SUMMARY] + [(RECORDS, (k,)) for k in SUMMARY]
    for rec, summ in cases:
        got = run(rec, summ)
        assert set(got) == set(rec) | set(summ) | {"states"}
        same_bits(base, got, tuple(rec) + tuple(summ) + ("states",), what=(rec, summ))


# ---- 5. summary --------------------------------------------------------------------------------
def test_summary_of_the_parity_batch(parity_runs):
    """results() against metrics.instance_success / min_pair_distance on the same run's trace."""
    for slack in (False, True):
        for obj, rec, g in parity_runs[slack]:
            res = obj.results()
            for t, (name, _, targets) in enumerate(g["teams"]):
                r0, r1 = int(obj.team_ptr_host[t]), int(obj.team_ptr_host[t + 1])
                traj = rec["trace"][:, r0:r1].transpose(1, 0, 2)
                ok, span, first = metrics.instance_success(traj, targets, obj.goal_radius, list(obj.shape_half), "box")
                r = res[t]
                assert (r["instance_success"], r["makespan"], r["first_collision"]) == (ok, span, first), (name, slack)
                assert r["min_pair_distance_m"] == metrics.min_pair_distance(traj), (name, slack)
                assert r["fail_count"] == int(np.count_nonzero(rec["status"][:, r0:r1] != O.OPTIMAL)), (name, slack)


def test_summary_of_hand_built_teams(mpclib):
    import torch
    cfg, shape_half, goal_radius, teams = F.summary_teams()
    team_ptr = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in teams])])
    obj = mpclib.FormationRollouts(cfg, team_ptr, np.concatenate([s for _, s, _ in teams]),
                                   np.concatenate([g for _, _, g in teams]), shape_half=shape_half,
                                   goal_radius=goal_radius)
    obj.run(5).run(3)  # (the summary chains over calls)
    torch.cuda.synchronize()
    rec, res = obj.records(), obj.results()
    raw_first = obj.first_collision.cpu().numpy()
    for t, (name, _, targets) in enumerate(teams):
        r0, r1 = int(team_ptr[t]), int(team_ptr[t + 1])
        traj = rec["trace"][:, r0:r1].transpose(1, 0, 2)
        ok, span, first = metrics.instance_success(traj, targets, goal_radius, list(shape_half), "box")
        r = res[t]
        assert (r["instance_success"], r["makespan"], r["first_collision"]) == (ok, span, first), name
        assert r["min_pair_distance_m"] == metrics.min_pair_distance(traj), name
        assert np.all(rec["status"][:, r0:r1] == O.INFEASIBLE) and np.all(rec["cbf_u"][:, r0:r1] == 0.0), name
        assert r["fail_count"] == 2 * 8, name
    by = {name: res[t] for t, (name, _, _) in enumerate(teams)}
    assert by["head_on"]["instance_success"] is False and by["head_on"]["first_collision"] == (0, 0, 1)
    assert by["arrive_then_collide"]["instance_success"] is True and by["arrive_then_collide"]["makespan"] == 0
    assert raw_first[1].tolist() == [2, 0, 1]  # the later collision is seen, and does not fail the run
    assert by["same_sample"]["instance_success"] is False and by["same_sample"]["first_collision"] == (0, 0, 1)
    assert obj.arrival_sample.cpu().numpy().tolist() == [-1, -1, 0, 0, 0, 0]


# ---- 6. JSON -----------------------------------------------------------------------------------
def test_to_json_is_the_examples_record(parity_runs):
    import json
    obj, rec, g = parity_runs[False][0]
    t = 1
    n = len(g["teams"][t][1])
    js = json.loads(json.dumps(obj.to_json(t, records=rec)))
    assert set(js) == {"dt", "Ts", "robots"} and js["dt"] == js["Ts"] == g["cfg"]["Ts"]
    assert sorted(js["robots"]) == sorted(str(i) for i in range(n))
    for i in range(n):
        assert set(js["robots"][str(i)]) == {"states", "desired_u", "cbf_u"}
        assert [len(js["robots"][str(i)][k]) for k in ("states", "desired_u", "cbf_u")] == [F.PARITY_STEPS] * 3
        assert len(js["robots"][str(i)]["states"][0]) == 6 and len(js["robots"][str(i)]["cbf_u"][0]) == 3
    r0 = int(obj.team_ptr_host[t])
    back = metrics.trajectories_from_states_json(js)
    same_bits(back, rec["trace"][:, r0:r0 + n].transpose(1, 0, 2))

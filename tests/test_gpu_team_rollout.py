"""GPU: the MPC-CBF team rollouts (mpccbf_team_rollout, mpccbf.TeamRollouts).

1. bit for bit the per-robot-launch simulator (Simulator(order="gauss_seidel", neighbours="all")),
   whose launches are impc_kernel<6,64,4>, the kernel whose agent body the rollout shares;
2. the unchanged oracle, teacher-forced (oracle_lib.closed_loop_gauss_seidel(..., inputs=) with the
   rule of test_gpu_reference_instances.py), on the parity batch and on a team at k_hor = 10;
3. the order witness and what the parity batch holds;
4. the shape edges; 5. bit-for-bit independence of the split into launches and calls, of the place in
   the batch and of the optional outputs; 6. the summary against mpccbf.metrics."""
import numpy as np
import pytest

import oracle_lib as O
import team_rollout_cases as T
from gpu_harness import require_gpu, same_bits, to_device, to_host
from mpccbf import metrics, sim

pytestmark = pytest.mark.gpu

RECORDS = ("status", "obj", "iters", "x", "traj_t0", "substeps", "trace")
SUMMARY = ("arrival_sample", "first_collision", "min_d2", "fail_count")
CARRIED = ("states", "x_keep", "traj_t")
FILL = -12345  # the records' fill: what a run must overwrite, and what it must leave where it writes nothing


def run_raw(mpclib, ctx, team_ptr, states, targets, seeds, steps, step_first=0, records=RECORDS, summary=None,
            summary_keys=SUMMARY, carry=None, steps_per_launch=0, alloc_steps=None, shape_half=(0.2, 0.2),
            goal_radius=1.0, **noise):
    """One mpccbf_team_rollout call on fresh device tensors through the thin binding (no host checks
    of the team sizes): host copies of what it carries (states, x_keep, traj_t; carry: host arrays
    (x_keep, traj_t) to continue from), of the chosen records (filled with FILL before) and of the
    summary (summary: host arrays to continue from, None = initialised)."""
    import torch
    from mpccbf import _lib
    dev = torch.device("cuda", 0)
    noise = {**T.EDGE_NOISE, **noise}
    team_ptr = np.ascontiguousarray(team_ptr, dtype=np.int32)
    n, teams = int(team_ptr[-1]), len(team_ptr) - 1
    nsub = int(ctx.cfg["h"] / ctx.cfg["Ts"])
    width = dict(status=(ctx.impc_iter,), obj=(ctx.impc_iter,), iters=(ctx.impc_iter,), x=(ctx.n,), traj_t0=(),
                 substeps=(nsub, 6), trace=(6,))
    t = lambda a, dt=None: to_device(np.asarray(a, dtype=dt))  # noqa: E731
    rows = steps if alloc_steps is None else alloc_steps
    rec = {k: torch.full((rows, n) + width[k], FILL, dtype=torch.int32 if k in ("status", "iters") else torch.float64,
                         device=dev) for k in records}
    if summary is None:
        summary = dict(arrival_sample=np.full(n, -1, np.int32), first_collision=np.full((teams, 3), -1, np.int32),
                       min_d2=np.full(teams, np.inf), fail_count=np.zeros(teams, np.int32))
    summ = {k: t(summary[k]) for k in summary_keys}
    d_states = t(states, np.float64)
    x_keep = t(np.full((n, ctx.n), np.nan) if carry is None else carry[0], np.float64)
    traj_t = t(np.full(n, -1.0) if carry is None else carry[1], np.float64)
    seed_bits = np.array([int(s) & ((1 << 64) - 1) for s in seeds], dtype=np.uint64).view(np.int64)
    _lib.team_rollout(ctx, t(team_ptr), d_states, t(targets, np.float64), t(seed_bits), x_keep, traj_t, steps,
                      step_first, shape_half=shape_half, goal_radius=goal_radius, steps_per_launch=steps_per_launch,
                      **noise, **rec, **summ)
    torch.cuda.synchronize()
    out = to_host(rec)
    out.update(to_host(summ))
    out.update(states=d_states.cpu().numpy(), x_keep=x_keep.cpu().numpy(), traj_t=traj_t.cpu().numpy())
    return out


@pytest.fixture(scope="module")
def base_ctx(mpclib):
    require_gpu()
    return mpclib.Context(T.base_cfg())


# ---- 1. bit for bit the per-robot-launch simulator ---------------------------------------------
BITS_STEPS = max(steps for _, steps in T.BITS_CASES)


@pytest.fixture(scope="module")
def sim_runs(mpclib):
    """name -> the simulator's run of BITS_STEPS steps: per step the states after it, the sub-steps,
    status, obj, iters, the kept x, traj_t before and after; its states.json; its kernel."""
    require_gpu()
    runs = {}
    for name, _ in T.BITS_CASES:
        cfg, states, targets, shape, kind, noise = T.instance(name)
        s = sim.Simulator(cfg, states, targets, order="gauss_seidel", neighbours="all", noise_seed=T.BITS_SEED, **noise)
        log = {k: [] for k in ("trace", "substeps", "status", "obj", "iters", "x", "traj_t0", "traj_t")}
        for _ in range(BITS_STEPS):
            log["traj_t0"].append(s.traj_t.cpu().numpy().copy())
            s.step()
            log["trace"].append(s.states.cpu().numpy().copy())
            log["substeps"].append(s.substeps.cpu().numpy().copy())
            for k in ("status", "obj", "iters", "x"):
                log[k].append(s.out[k].cpu().numpy().copy())
            log["traj_t"].append(s.traj_t.cpu().numpy().copy())
        runs[name] = dict(log={k: np.array(v) for k, v in log.items()}, json=s.states_json(),
                          kernel=s.ctx.kernel_name)
    return runs


def json_head(js, steps, nsub):
    """A states.json cut to its first `steps` steps."""
    return {"dt": js["dt"], "Ts": js["Ts"],
            "robots": {i: {"pred_curve": r["pred_curve"][:steps], "states": r["states"][:steps * nsub]}
                       for i, r in js["robots"].items()}}


def check_against_simulator(obj, rec, team, ref, steps, name):
    """Team `team` of a rollout of `steps` steps against the simulator's first `steps` steps."""
    r0, r1 = int(obj.team_ptr_host[team]), int(obj.team_ptr_host[team + 1])
    assert len(rec["trace"]) == steps
    same_bits({k: rec[k][:, r0:r1] for k in RECORDS}, {k: ref["log"][k][:steps] for k in RECORDS}, what=name)
    same_bits(obj.traj_t.cpu().numpy()[r0:r1], ref["log"]["traj_t"][steps - 1], what=f"{name} traj_t")
    same_bits(obj.states.cpu().numpy()[r0:r1], ref["log"]["trace"][steps - 1], what=f"{name} states")
    assert obj.to_json(team, rec) == json_head(ref["json"], steps, obj.nsub), name


@pytest.mark.parametrize("name,steps", T.BITS_CASES, ids=[n for n, _ in T.BITS_CASES])
def test_one_instance_is_the_simulator_bit_for_bit(mpclib, sim_runs, name, steps):
    """1. An instance as a batch of its own: states after every step, sub-steps, status, obj, iters,
    the kept x and traj_t carry the simulator's bits, and the JSON record is the simulator's."""
    import torch
    ref = sim_runs[name]
    assert ref["kernel"] == "impc_kernel<6,64,4>"  # what is compared: the dense 64 x 4 per-robot launch
    obj = mpclib.TeamRollouts.from_instances([name], [T.BITS_SEED])
    obj.run(steps)
    torch.cuda.synchronize()
    check_against_simulator(obj, obj.records(), 0, ref, steps, name)
    st = ref["log"]["status"][:steps, :, 0]
    if name in T.INSIDE_DMIN:  # every QP INFEASIBLE: the hold-position path with accumulated noise
        assert np.all(st == O.INFEASIBLE) and np.all(np.isnan(obj.x_keep.cpu().numpy()))
    elif name in ("2r/circle", "5r/circle"):  # kept curves continue past the OPTIMAL -> INFEASIBLE transition
        tr = np.argwhere((st[:-1] == O.OPTIMAL) & (st[1:] == O.INFEASIBLE))
        assert len(tr) > 0 and np.any(ref["log"]["traj_t0"][:steps][st != O.OPTIMAL] > 0.0)


def test_four_instances_in_one_batch_are_the_simulator_bit_for_bit(mpclib, sim_runs):
    """1. All four in one batch: each team is still its own simulator run."""
    import torch
    names = [n for n, _ in T.BITS_CASES]
    assert all(sim_runs[n]["kernel"] == "impc_kernel<6,64,4>" for n in names)
    obj = mpclib.TeamRollouts.from_instances(names, [T.BITS_SEED])
    obj.run(BITS_STEPS)
    torch.cuda.synchronize()
    rec = obj.records()
    for team, name in enumerate(names):
        check_against_simulator(obj, rec, team, sim_runs[name], BITS_STEPS, name)


# ---- 2. oracle parity, teacher-forced ----------------------------------------------------------
@pytest.fixture(scope="module")
def parity_run(mpclib):
    """The parity batch after PARITY_STEPS steps in one launch sequence, and its records."""
    import torch
    require_gpu()
    obj = mpclib.TeamRollouts.from_instances(T.PARITY_NAMES, [T.PARITY_SEED])
    assert np.diff(obj.team_ptr_host).tolist() == list(T.PARITY_ROBOTS)
    obj.run(T.PARITY_STEPS)
    torch.cuda.synchronize()
    return obj, obj.records()


def team_trace(obj, rec, team):
    """steps + 1 x n x 6: the team's initial states, then its table after every step."""
    r0, r1 = int(obj.team_ptr_host[team]), int(obj.team_ptr_host[team + 1])
    return np.concatenate([obj.states0[None, r0:r1], rec["trace"][:, r0:r1]]), r0, r1


@pytest.mark.parametrize("team", range(len(T.PARITY_NAMES)), ids=list(T.PARITY_NAMES))
def test_oracle_parity_teacher_forced(parity_run, team):
    """2. Every update of the team against the oracle on the table it planned from."""
    obj, rec = parity_run
    name = T.PARITY_NAMES[team]
    cfg, states, targets, shape, kind, noise = T.instance(name)
    trace, r0, r1 = team_trace(obj, rec, team)
    loose, updates = T.check_oracle_parity(cfg, states, targets, trace, rec["status"][:, r0:r1], rec["obj"][:, r0:r1],
                                           T.PARITY_SEED, noise["pos_std"], noise["vel_std"], label=name)
    print(f"{name}: {updates} updates, {loose} beyond 1e-8")
    assert updates == (T.PARITY_STEPS + 1) * T.PARITY_ROBOTS[team]


def test_oracle_parity_at_k_hor_10(mpclib):
    """2. One seeded 4-robot team at k_hor = 10: the same kernel on a K <= 15 configuration."""
    import torch
    require_gpu()
    cfg = T.base_cfg(k_hor=10)
    states, targets, team_ptr, seeds = T.edge_batch(list(T.KHOR10_SIZES))
    obj = mpclib.TeamRollouts(cfg, team_ptr, states, targets, seeds=seeds, **T.EDGE_NOISE)
    obj.run(6)
    torch.cuda.synchronize()
    rec = obj.records()
    trace, r0, r1 = team_trace(obj, rec, 0)
    loose, updates = T.check_oracle_parity(cfg, states, targets, trace, rec["status"], rec["obj"], seeds[0],
                                           T.EDGE_NOISE["pos_std"], T.EDGE_NOISE["vel_std"], label="k_hor 10")
    assert updates == 7 * 4 and np.any(rec["status"][:, :, 0] == O.OPTIMAL)


# ---- 3. the order witness ----------------------------------------------------------------------
def test_parity_check_sees_the_order(parity_run):
    """3. The same run read as if every robot had planned from the previous sample's whole table
    (Jacobi) disagrees beyond 1e-6 on decisions of robots i > 0 — and only there: robot 0's table is
    the same in both orders. Read in its own order the witness' loop agrees everywhere."""
    obj, rec = parity_run
    team = T.PARITY_NAMES.index(T.WITNESS)
    cfg, states, targets, shape, kind, noise = T.instance(T.WITNESS)
    trace, r0, r1 = team_trace(obj, rec, team)
    args = (cfg, states, targets, trace, T.PARITY_SEED, noise["pos_std"], noise["vel_std"])
    bad = T.order_mismatches(*args, order="jacobi")
    print(f"{T.WITNESS} read as Jacobi: {len(bad)} of {T.PARITY_STEPS * 5} updates differ, first {bad[:3]}")
    assert any(i > 0 for _, i, _ in bad)
    assert not T.order_mismatches(*args, order="gauss_seidel")


def test_parity_batch_holds_what_it_is_there_to_see(parity_run):
    """3. An INFEASIBLE decision, a decision that kept an old curve, and a robot that never had one."""
    obj, rec = parity_run
    st0 = rec["status"][:, :, 0]
    assert np.any(st0 == O.OPTIMAL) and np.any(st0 == O.INFEASIBLE)
    assert np.any((st0 != O.OPTIMAL) & (rec["traj_t0"] >= 0.0))                     # continued on the kept curve
    never = np.all(st0 != O.OPTIMAL, axis=0)
    assert np.any(never) and np.all(np.isnan(obj.x_keep.cpu().numpy()[never]))      # held position throughout
    assert np.all(obj.traj_t.cpu().numpy()[never] == -1.0)
    assert not np.any(st0 == O.ERROR)


# ---- 4. shapes ---------------------------------------------------------------------------------
def test_team_sizes_1_2_15_16_against_the_oracle(mpclib):
    """4. Teams of 1, 2, 15 and 16 robots on lattices above d_min, 3 steps, every update checked."""
    import torch
    require_gpu()
    cfg = T.base_cfg()
    states, targets, team_ptr, seeds = T.edge_batch(list(T.SHAPE_SIZES))
    obj = mpclib.TeamRollouts(cfg, team_ptr, states, targets, seeds=seeds, **T.EDGE_NOISE)
    obj.run(3)
    torch.cuda.synchronize()
    rec = obj.records()
    assert not np.any(rec["status"] == O.ERROR) and np.any(rec["status"][:, :, 0] == O.OPTIMAL)
    for team, n in enumerate(T.SHAPE_SIZES):
        trace, r0, r1 = team_trace(obj, rec, team)
        T.check_oracle_parity(cfg, states[r0:r1], targets[r0:r1], trace, rec["status"][:, r0:r1], rec["obj"][:, r0:r1],
                              seeds[team], T.EDGE_NOISE["pos_std"], T.EDGE_NOISE["vel_std"], label=f"team of {n}")


def test_oversize_and_empty_teams_among_solvable_ones(mpclib, base_ctx):
    """4. A team of 17 takes no step (ERROR, states stay, rows copy them, fail_count counts them all),
    an empty team writes nothing, and their neighbours in the batch are bit for bit what they are
    without them."""
    steps, sizes = 3, [3, 17, 0, 2]
    states, targets, team_ptr, seeds = T.edge_batch(sizes)
    got = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, steps)
    big = slice(int(team_ptr[1]), int(team_ptr[2]))
    assert np.all(got["status"][:, big, 0] == O.ERROR) and np.all(got["status"][:, big, 1:] == O.UNKNOWN)
    assert np.all(np.isnan(got["obj"][:, big])) and np.all(got["iters"][:, big] == 0)
    same_bits(got["states"][big], states[big], what="the oversize team's states stay")
    for s in range(steps):
        same_bits(got["trace"][s, big], states[big], what="its trace rows copy them")
        for k in range(got["substeps"].shape[2]):
            same_bits(got["substeps"][s, big, k], states[big], what="its sub-step rows copy them")
    assert np.all(np.isnan(got["x"][:, big])) and np.all(got["traj_t0"][:, big] == -1.0)
    assert got["fail_count"].tolist()[1:3] == [17 * steps, 0]
    assert got["first_collision"][1:3].tolist() == [[-1] * 3] * 2 and np.all(np.isinf(got["min_d2"][1:3]))
    assert np.all(got["arrival_sample"][big] == -1)
    # the solvable teams alone, with their own seeds
    keep = [0, 3]
    rows = np.concatenate([np.arange(team_ptr[t], team_ptr[t + 1]) for t in keep])
    alone = run_raw(mpclib, base_ctx, [0, 3, 5], states[rows], targets[rows], [seeds[t] for t in keep], steps)
    for k in RECORDS:
        same_bits(got[k][:, rows], alone[k], what=k)
    for k in CARRIED + ("arrival_sample",):
        same_bits(got[k][rows], alone[k], what=k)
    for k in ("first_collision", "min_d2", "fail_count"):
        same_bits(got[k][keep], alone[k], what=k)
    assert np.any(alone["status"][:, :, 0] == O.OPTIMAL) and not np.any(alone["status"] == FILL)


@pytest.fixture(scope="module")
def small_batches(mpclib, base_ctx):
    out = {}
    for teams in T.BATCH_COUNTS:
        states, targets, team_ptr, seeds = T.small_batch(teams)
        out[teams] = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 2)
    return out


@pytest.mark.parametrize("teams", T.BATCH_COUNTS)
def test_batch_sizes(small_batches, teams):
    """4. Batches of 1, 33 and 300 teams of 2 - 3 robots: every decision is taken and written, and a
    team is the same team in every batch that holds it."""
    got, big = small_batches[teams], small_batches[max(T.BATCH_COUNTS)]
    n = len(got["states"])
    assert n == int(T.small_batch(teams)[2][-1])
    for k in RECORDS:
        assert not np.any(got[k] == FILL), k
        same_bits(got[k], big[k][:, :n], what=k)
    assert not np.any(got["status"] == O.ERROR) and np.any(got["status"][:, :, 0] == O.OPTIMAL)
    assert np.all(got["fail_count"] == np.add.reduceat(np.count_nonzero(got["status"][:, :, 0] != O.OPTIMAL, axis=0),
                                                       T.small_batch(teams)[2][:-1]))
    for k in CARRIED + ("arrival_sample",):
        same_bits(got[k], big[k][:n], what=k)
    for k in ("first_collision", "min_d2", "fail_count"):
        same_bits(got[k], big[k][:teams], what=k)


def test_zero_steps_write_nothing_and_one_step_is_the_first_of_two(mpclib, base_ctx, small_batches):
    """4. 0 steps: no output is touched. 1 step: the first step of the 2-step run."""
    states, targets, team_ptr, seeds = T.small_batch(1)
    none = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 0, alloc_steps=1)
    for k in RECORDS:
        assert np.all(none[k] == FILL), k
    same_bits(none["states"], states)
    assert np.all(np.isnan(none["x_keep"])) and np.all(none["traj_t"] == -1.0)
    assert np.all(none["arrival_sample"] == -1) and np.all(none["first_collision"] == -1)
    assert np.all(np.isinf(none["min_d2"])) and np.all(none["fail_count"] == 0)
    one, two = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 1), small_batches[1]
    for k in RECORDS:
        same_bits(one[k], two[k][:1], what=k)
    same_bits(one["states"], two["trace"][0])


def test_nan_state_is_an_error_of_its_team_alone(mpclib, base_ctx):
    """4. A NaN in one robot's state: that robot reports ERROR and holds (no curve, the NaN stays);
    the other teams are bit for bit what they are without it."""
    states, targets, team_ptr, seeds = T.small_batch(3)
    clean = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 2)
    bad = states.copy()
    r = int(team_ptr[1])  # the first robot of team 1
    bad[r, 0] = np.nan
    got = run_raw(mpclib, base_ctx, team_ptr, bad, targets, seeds, 2)
    assert np.all(got["status"][:, r, 0] == O.ERROR) and np.all(got["status"][:, r, 1:] == O.UNKNOWN)
    assert np.isnan(got["states"][r, 0]) and np.all(np.isnan(got["x_keep"][r])) and got["traj_t"][r] == -1.0
    assert np.all(np.abs(got["states"][r, 1:3] - states[r, 1:3]) < 0.05)  # held: only the position noise moved it
    assert got["fail_count"][1] >= 2
    others = np.concatenate([np.arange(team_ptr[0], team_ptr[1]), np.arange(team_ptr[2], team_ptr[3])])
    for k in RECORDS:
        same_bits(got[k][:, others], clean[k][:, others], what=k)
    for k in CARRIED + ("arrival_sample",):
        same_bits(got[k][others], clean[k][others], what=k)
    for k in ("first_collision", "min_d2", "fail_count"):
        same_bits(got[k][[0, 2]], clean[k][[0, 2]], what=k)


# ---- 5. bit for bit under every decomposition --------------------------------------------------
@pytest.fixture(scope="module")
def nine_steps(mpclib, base_ctx):
    """Three teams, 9 steps, one launch: what every decomposition must reproduce."""
    states, targets, team_ptr, seeds = T.small_batch(3)
    return (states, targets, team_ptr, seeds), run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 9,
                                                      steps_per_launch=9)


ALL_KEYS = RECORDS + SUMMARY + CARRIED


@pytest.mark.parametrize("per_launch", [1, 3, 0], ids=["1", "3", "default"])
def test_split_into_launches(mpclib, base_ctx, nine_steps, per_launch):
    """5. steps_per_launch 1, 3 and the default against all nine steps in one launch."""
    (states, targets, team_ptr, seeds), whole = nine_steps
    got = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 9, steps_per_launch=per_launch)
    same_bits(got, whole, keys=ALL_KEYS, what=f"steps_per_launch {per_launch}")


def test_split_into_calls(mpclib, base_ctx, nine_steps):
    """5. Four steps, then five from step 4 on the carried state and summary, against nine; and
    TeamRollouts.run(4).run(5) keeps the absolute step."""
    import torch
    (states, targets, team_ptr, seeds), whole = nine_steps
    a = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 4)
    b = run_raw(mpclib, base_ctx, team_ptr, a["states"], targets, seeds, 5, step_first=4,
                carry=(a["x_keep"], a["traj_t"]), summary={k: a[k] for k in SUMMARY})
    for k in RECORDS:
        same_bits(np.concatenate([a[k], b[k]]), whole[k], what=k)
    same_bits(b, whole, keys=SUMMARY + CARRIED, what="run(4); run(5)")
    obj = mpclib.TeamRollouts(T.base_cfg(), team_ptr, states, targets, seeds=seeds, **T.EDGE_NOISE)
    obj.run(4).run(5)
    torch.cuda.synchronize()
    assert obj.steps == 9
    same_bits(obj.records(), whole, keys=RECORDS, what="TeamRollouts.run(4).run(5)")
    same_bits(to_host({k: getattr(obj, k) for k in SUMMARY + CARRIED}), whole, keys=SUMMARY + CARRIED)


def test_place_in_the_batch(mpclib, base_ctx, nine_steps):
    """5. Team 1 alone, and first and last among other teams, with its own seed."""
    (states, targets, team_ptr, seeds), whole = nine_steps
    r0, r1 = int(team_ptr[1]), int(team_ptr[2])
    alone = run_raw(mpclib, base_ctx, [0, r1 - r0], states[r0:r1], targets[r0:r1], [seeds[1]], 9)
    os_, ot, op, _ = T.edge_batch([3, 2], seed=77)
    for place in ("first", "last"):
        parts = [(states[r0:r1], targets[r0:r1]), (os_, ot)]
        sizes, sd = [r1 - r0, 3, 2], [seeds[1], 9001, 9002]
        if place == "last":
            parts, sizes, sd = parts[::-1], [3, 2, r1 - r0], [9001, 9002, seeds[1]]
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        got = run_raw(mpclib, base_ctx, ptr, np.concatenate([p[0] for p in parts]),
                      np.concatenate([p[1] for p in parts]), sd, 9)
        t = 0 if place == "first" else 2
        rows = slice(int(ptr[t]), int(ptr[t + 1]))
        for src, what in ((alone, "alone"), ({k: (whole[k][:, r0:r1] if k in RECORDS else whole[k][r0:r1])
                                              for k in RECORDS + CARRIED + ("arrival_sample",)}, "second of three")):
            for k in RECORDS:
                same_bits(got[k][:, rows], src[k], what=f"{place} / {what}: {k}")
            for k in CARRIED + ("arrival_sample",):
                same_bits(got[k][rows], src[k], what=f"{place} / {what}: {k}")
        for k in ("first_collision", "min_d2", "fail_count"):
            same_bits(got[k][t], alone[k][0], what=k)
            same_bits(got[k][t], whole[k][1], what=k)


CHOICES = [()] + [(k,) for k in RECORDS] + [RECORDS]
SUMMARY_CHOICES = [()] + [(k,) for k in SUMMARY]


@pytest.mark.parametrize("records", CHOICES, ids=["none"] + list(RECORDS) + ["all"])
def test_every_choice_of_records(mpclib, base_ctx, nine_steps, records):
    """5. What is computed does not depend on what is recorded (without `substeps` the sub-steps go
    through the context's work rows)."""
    (states, targets, team_ptr, seeds), whole = nine_steps
    got = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 9, records=records)
    same_bits(got, whole, keys=tuple(records) + SUMMARY + CARRIED, what=f"records {records}")


@pytest.mark.parametrize("keys", SUMMARY_CHOICES, ids=["none"] + list(SUMMARY))
def test_every_choice_of_summary(mpclib, base_ctx, nine_steps, keys):
    (states, targets, team_ptr, seeds), whole = nine_steps
    got = run_raw(mpclib, base_ctx, team_ptr, states, targets, seeds, 9, records=("trace",), summary_keys=keys)
    same_bits(got, whole, keys=("trace",) + tuple(keys) + CARRIED, what=f"summary {keys}")


# ---- 6. the summary ----------------------------------------------------------------------------
def json_metrics(obj, rec, team, targets, shape_half, goal_radius):
    traj = metrics.trajectories_from_states_json(obj.to_json(team, rec))
    ok, span, first = metrics.instance_success(traj, targets, goal_radius, list(shape_half), "box")
    r0, r1 = int(obj.team_ptr_host[team]), int(obj.team_ptr_host[team + 1])
    fails = int(np.count_nonzero(rec["status"][:, r0:r1, 0] != O.OPTIMAL))
    return dict(instance_success=ok, makespan=span, first_collision=first,
                min_pair_distance_m=metrics.min_pair_distance(traj), fail_count=fails)


def test_results_are_the_metrics_of_the_runs_own_trace(parity_run):
    """6. .results() against metrics.instance_success, min_pair_distance and the count of decisions
    without an OPTIMAL iteration on the run's own record, for every team of the parity batch."""
    obj, rec = parity_run
    res = obj.results()
    assert len(res) == len(T.PARITY_NAMES)
    for team, name in enumerate(T.PARITY_NAMES):
        cfg, states, targets, shape, kind, noise = T.instance(name)
        assert res[team] == json_metrics(obj, rec, team, targets, obj.shape_half, obj.goal_radius), name
    assert any(r["first_collision"] is not None for r in res) or any(r["fail_count"] > 0 for r in res)


def test_hand_built_summary_teams(mpclib):
    """6. The four hand-built pairs: the stated answers, and the metrics of the run's own trace."""
    import torch
    require_gpu()
    shape_half, goal_radius, steps, teams = T.summary_teams()
    cfg = T.base_cfg()
    ptr = np.arange(len(teams) + 1) * 2
    obj = mpclib.TeamRollouts(cfg, ptr, np.concatenate([t[1] for t in teams]), np.concatenate([t[2] for t in teams]),
                              shape_half=shape_half, goal_radius=goal_radius)
    obj.run(steps)
    torch.cuda.synchronize()
    rec, res = obj.records(), obj.results()
    samples = steps * obj.nsub
    for team, (name, states, targets, (ok, first, arrived)) in enumerate(teams):
        got = res[team]
        assert got == json_metrics(obj, rec, team, targets, shape_half, goal_radius), name
        assert (got["instance_success"], got["first_collision"]) == (ok, first), (name, got)
        arr = obj.arrival_sample.cpu().numpy()[2 * team:2 * team + 2]
        assert (arr.tolist() == [0, 0]) if arrived else np.all(arr == -1), (name, arr)
        if ok:
            assert got["makespan"] == (0 if arrived else samples), (name, got)
        if first is not None:  # inside d_min: every QP INFEASIBLE, both hold their position exactly
            assert got["fail_count"] == 2 * steps
            same_bits(rec["trace"][-1, 2 * team:2 * team + 2, :2], states[:, :2], what=name)

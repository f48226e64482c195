"""CPU: what mpccbf_formation_rollout refuses (on the host, before any device call, so no GPU is
needed), the host program that drives the same rules, the header's declarations, the binding, and
FormationRollouts' own host-side checks and summary arithmetic."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mpccbf import _lib, formation, metrics

INVALID = -1  # MPCCBF_ERR_INVALID_ARGUMENT
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")
CHECK = os.path.join(REPO, "mpc-cbf_amd", "build", "formation_args_check")

KEEP = dict(team_ptr=np.array([0, 2], np.int32), states=np.zeros((2, 6)), targets=np.zeros((2, 3)),
            team_seed=np.array([7], np.uint64))


def _params(**over):
    p = _lib.ConnControlParams(d_min=0.8, d_max=3.0, slack_mode=0, slack_cost=1e5, slack_decay_rate=0.1)
    for d in range(3):
        p.v_min[d], p.v_max[d] = -1.0, 1.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _formation(**over):
    f = _lib.FormationParams(Ts=0.01, spring_constant=0.5, pos_std=0.001, vel_std=0.01, goal_radius=1.0,
                             steps_per_launch=0)
    f.shape_half[0] = f.shape_half[1] = 0.2
    for k, v in over.items():
        if k == "shape_half":
            f.shape_half[0], f.shape_half[1] = v
        else:
            setattr(f, k, v)
    return f


def _batch(**over):
    """A well-formed batch over host memory: only ever handed to calls that must refuse it or that
    enqueue nothing."""
    b = _lib.FormationBatch(num_teams=1, team_ptr=KEEP["team_ptr"].ctypes.data, states=KEEP["states"].ctypes.data,
                            targets=KEEP["targets"].ctypes.data, team_seed=KEEP["team_seed"].ctypes.data,
                            step_first=0, num_steps=3)
    for k, v in over.items():
        setattr(b, k, v)
    return b


def _call(mpclib, p, f, b):
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return mpclib.load().mpccbf_formation_rollout(ref(p), ref(f), ref(b), 0, None)


BAD = [
    ("null_params", lambda: (None, _formation(), _batch())),
    ("null_formation", lambda: (_params(), None, _batch())),
    ("null_batch", lambda: (_params(), _formation(), None)),
    ("null_team_ptr", lambda: (_params(), _formation(), _batch(team_ptr=None))),
    ("null_states", lambda: (_params(), _formation(), _batch(states=None))),
    ("null_targets", lambda: (_params(), _formation(), _batch(targets=None))),
    ("null_team_seed", lambda: (_params(), _formation(), _batch(team_seed=None))),
    ("num_teams_negative", lambda: (_params(), _formation(), _batch(num_teams=-1))),
    ("num_steps_negative", lambda: (_params(), _formation(), _batch(num_steps=-1))),
    ("step_first_negative", lambda: (_params(), _formation(), _batch(step_first=-1))),
    ("samples_beyond_int32", lambda: (_params(), _formation(), _batch(step_first=(1 << 31) - 3))),
    ("Ts_nan", lambda: (_params(), _formation(Ts=math.nan), _batch())),
    ("Ts_inf", lambda: (_params(), _formation(Ts=math.inf), _batch())),
    ("Ts_zero", lambda: (_params(), _formation(Ts=0.0), _batch())),
    ("steps_per_launch_negative", lambda: (_params(), _formation(steps_per_launch=-1), _batch())),
    ("pos_std_negative", lambda: (_params(), _formation(pos_std=-1e-3), _batch())),
    ("vel_std_nan", lambda: (_params(), _formation(vel_std=math.nan), _batch())),
    ("spring_negative", lambda: (_params(), _formation(spring_constant=-0.5), _batch())),
    ("box_zero_extent", lambda: (_params(), _formation(shape_half=(0.2, 0.0)), _batch())),
    ("goal_radius_negative", lambda: (_params(), _formation(goal_radius=-1.0), _batch())),
    ("d_min_zero", lambda: (_params(d_min=0.0), _formation(), _batch())),
    ("slack_without_cost", lambda: (_params(slack_mode=1, slack_cost=0.0), _formation(), _batch())),
    ("slack_decay_above_one", lambda: (_params(slack_mode=1, slack_decay_rate=1.5), _formation(), _batch())),
]


@pytest.mark.parametrize("name,make", BAD, ids=[b[0] for b in BAD])
def test_bad_calls_are_refused(mpclib, name, make):
    assert _call(mpclib, *make()) == INVALID
    msg = mpclib.load().mpccbf_last_error().decode()
    assert msg.startswith("formation rollout:"), msg


def test_nothing_to_run_is_a_successful_no_op(mpclib):
    assert _call(mpclib, _params(), _formation(), _batch(num_steps=0)) == 0
    assert _call(mpclib, _params(), _formation(), _batch(num_teams=0)) == 0
    # nothing is read from a batch with nothing to run
    assert _call(mpclib, _params(), _formation(), _batch(num_steps=0, states=None, team_seed=None)) == 0
    assert KEEP["states"].tolist() == np.zeros((2, 6)).tolist()


def test_args_program():
    """The same rules and the launch split from a plain C++ program (no HIP, no library)."""
    assert os.path.exists(CHECK), "make -C mpc-cbf_amd builds build/formation_args_check"
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"formation_args_check: (\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 800, r.stdout


def test_header_declares_and_library_exports_the_rollout(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_FORMATION_ROLLOUT\s+1\b", text)
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", text)
    m = re.search(r"#define\s+MPCCBF_FORMATION_STEPS_PER_LAUNCH\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.FORMATION_STEPS_PER_LAUNCH

    def fields_of(struct):
        m = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", text, re.S)
        assert m, struct
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for f in (re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()):
            kind = f.rsplit(" ", 1)[0]
            out += [(kind, n.strip()) for n in f.rsplit(" ", 1)[1].split(",")] if "," not in kind else \
                [(f.split(" ", 1)[0], n.strip()) for n in f.split(" ", 1)[1].split(",")]
        return out

    fp = fields_of("mpccbf_formation_params")
    assert [n.split("[")[0] for _, n in fp] == [f[0] for f in _lib.FormationParams._fields_]
    fb = fields_of("mpccbf_formation_batch")
    assert [n.lstrip("*") for _, n in fb] == [f[0] for f in _lib.FormationBatch._fields_]
    assert [n for _, n in fb] == ["num_teams", "team_ptr", "states", "targets", "team_seed", "step_first", "num_steps",
                                  "trace", "cbf_u", "desired_u", "status", "lambda2", "iters", "arrival_sample",
                                  "first_collision", "min_d2", "fail_count"]
    assert C.sizeof(_lib.FormationParams) == 64 and C.sizeof(_lib.FormationBatch) == 136
    L = mpclib.load()
    assert L.mpccbf_abi_version() == 12
    assert hasattr(L, "mpccbf_formation_rollout") and "mpccbf_formation_rollout" in _lib.EXPORTED
    for name in ("FormationRollouts", "formation", "formation_rollout"):
        assert hasattr(mpclib, name), name


def test_team_sizes_are_checked_on_the_host():
    """Before any device call: a GPU is not needed to be told that a team does not fit."""
    import formation_rollout_cases as F
    cfg = F.edge_cfg()
    for sizes, bad, n in (([3, 17, 2], 1, 17), ([2, 0, 4], 1, 0)):
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        with pytest.raises(ValueError, match=f"team {bad} has {n} robots"):
            formation.FormationRollouts(cfg, ptr, np.zeros((ptr[-1], 6)), np.zeros((ptr[-1], 3)))
    with pytest.raises(ValueError, match="seeds: one per team"):
        formation.FormationRollouts(cfg, [0, 2], np.zeros((2, 6)), np.zeros((2, 3)), seeds=[1, 2])
    with pytest.raises(ValueError, match="states must be"):
        formation.FormationRollouts(cfg, [0, 2], np.zeros((3, 6)), np.zeros((2, 3)))


def _walk(arrivals, collision, samples):
    """A two-robot trace scored by metrics.instance_success: robot i enters its goal area at sample
    arrivals[i] (-1: never) and stays, and the boxes overlap at sample `collision` only (None: never).
    y tells arrived (0.3) from not (0.0) against goals at y = 1.25 with radius 1 (0.95 < 1 < 1.25, with
    room for the x offsets below), so the boxes (half extent 0.2: offsets below 0.4 overlap) always
    overlap in y; x decides: 0.5 apart, 0.2 at the collision."""
    goals = np.array([[0.0, 1.25, 0.0], [0.5, 1.25, 0.0]])
    traj = np.zeros((2, samples, 6))
    for i, a in enumerate(arrivals):
        traj[i, :, 0] = goals[i, 0]
        traj[i, :, 1] = [0.3 if (a >= 0 and t >= a) else 0.0 for t in range(samples)]
    if collision is not None:
        traj[1, collision, 0] = 0.2
    return metrics.instance_success(traj, goals, 1.0, [0.2, 0.2], "box")


def test_results_from_summary_is_the_scripts_walk():
    """results_from_summary against metrics.instance_success over every small case: the arrivals of
    two robots, one collision sample, the run's length."""
    cases = 0
    for samples in (1, 2, 4):
        for a0 in range(-1, samples):
            for a1 in range(-1, samples):
                for col in [None] + list(range(samples)):
                    ok, span, first = _walk([a0, a1], col, samples)
                    fc = [-1, -1, -1] if col is None else [col, 0, 1]
                    r = formation.results_from_summary([0, 2], [a0, a1], [fc], [4.0], [3], samples)[0]
                    assert (r["instance_success"], r["makespan"], r["first_collision"]) == (ok, span, first), \
                        (samples, a0, a1, col)
                    assert r["min_pair_distance_m"] == 2.0 and r["fail_count"] == 3
                    cases += 1
    assert cases == 2 * 4 + 3 * 9 + 5 * 25

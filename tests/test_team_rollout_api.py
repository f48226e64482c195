"""CPU: the header's declarations of mpccbf_team_rollout and the binding that mirrors them, the host
program that drives the call's refusals and accepted edges (csrc/host/team_rollout_args.hpp, no
device), and what mpccbf.TeamRollouts refuses on the host before a context is created."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import team_rollout_cases as T
from mpccbf import _lib, team_rollout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")
SOURCE = os.path.join(REPO, "tools", "team_rollout_args_check.cpp")
HOST_INC = os.path.join(REPO, "mpc-cbf_amd", "csrc", "host")


def test_header_declares_and_library_exports_the_rollout(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_TEAM_ROLLOUT\s+1\b", text)
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", text)
    m = re.search(r"#define\s+MPCCBF_TEAM_STEPS_PER_LAUNCH\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.TEAM_STEPS_PER_LAUNCH >= 1
    assert re.search(r"int\s+mpccbf_team_rollout\(mpccbf_ctx\*\s*ctx,\s*const\s+mpccbf_team_rollout_params\*\s*p,\s*"
                     r"const\s+mpccbf_team_batch\*\s*b,\s*void\*\s*hip_stream\);", text)

    def names_of(struct):
        m = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", text, re.S)
        assert m, struct
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for f in (re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()):
            head, rest = f.split(",")[0], f.split(",")[1:]
            out += [head.rsplit(" ", 1)[1].lstrip("*").split("[")[0]] + [n.strip().lstrip("*").split("[")[0] for n in rest]
        return out

    assert names_of("mpccbf_team_rollout_params") == [f[0] for f in _lib.TeamRolloutParams._fields_] == \
        ["pos_std", "vel_std", "shape_half", "goal_radius", "steps_per_launch"]
    assert names_of("mpccbf_team_batch") == [f[0] for f in _lib.TeamBatch._fields_] == \
        ["num_teams", "team_ptr", "states", "targets", "team_seed", "step_first", "num_steps", "x_keep", "traj_t",
         "status", "obj", "iters", "x", "traj_t0", "substeps", "trace", "arrival_sample", "first_collision", "min_d2",
         "fail_count"]
    assert C.sizeof(_lib.TeamRolloutParams) == 48 and C.sizeof(_lib.TeamBatch) == 160
    L = mpclib.load()
    assert L.mpccbf_abi_version() == 12
    assert hasattr(L, "mpccbf_team_rollout") and "mpccbf_team_rollout" in _lib.EXPORTED
    assert mpclib.TeamRollouts is team_rollout.TeamRollouts and mpclib.team_rollout is team_rollout
    # the summary goes through the formation rollout's scoring, imported, not restated
    from mpccbf import formation
    assert team_rollout.results_from_summary is formation.results_from_summary


def test_args_program(tmp_path):
    """tools/team_rollout_args_check.cpp compiles with plain g++ (no HIP, no library), runs and
    passes: every refusal of the call and the accepted edges (0 teams, 0 steps, step_first +
    num_steps = 2^31 - 1), and the launch split."""
    exe = str(tmp_path / "team_rollout_args_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", HOST_INC, SOURCE, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"team_rollout_args_check: (\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 3000, r.stdout
    # the program names each listed refusal and accepted edge
    src = open(SOURCE).read()
    for what in ("a FoV context: refused", "slack mode: refused", "a reduced dimension other than 6: refused",
                 "256 shared rows: refused", "15 * cbf_horizon against 256 - m", "connectivity rows attached: refused",
                 "a multi-rank communicator: refused", "NULL parameters: refused", "NULL batch: refused",
                 "a missing required pointer: refused", "num_teams < 0: refused",
                 "a negative or non-finite parameter: refused", "step_first + num_steps = 2^31: refused",
                 "0 teams: accepted", "0 steps: accepted", "step_first + num_steps = 2^31 - 1: accepted"):
        assert f'"{what}"' in src, what


def test_configuration_errors_are_raised_on_the_host():
    """Before a context is created: no GPU is needed to be told that a team does not fit or that the
    configuration is out of scope."""
    cfg = T.base_cfg()
    for sizes, bad, n in (([3, 17, 2], 1, 17), ([2, 0, 4], 1, 0)):
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        with pytest.raises(ValueError, match=f"team {bad} has {n} robots: teams of 1 .. 16"):
            team_rollout.TeamRollouts(cfg, ptr, np.zeros((ptr[-1], 6)), np.zeros((ptr[-1], 3)))
    two = ([0, 2], np.zeros((2, 6)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="slack mode is not supported"):
        team_rollout.TeamRollouts(T.base_cfg(slack_mode=1), *two)
    with pytest.raises(ValueError, match="FoV controller"):
        team_rollout.TeamRollouts(T.base_cfg(cbf_mode=1), *two)
    with pytest.raises(ValueError, match="seeds: one per team"):
        team_rollout.TeamRollouts(cfg, *two, seeds=[1, 2])
    with pytest.raises(ValueError, match="states must be"):
        team_rollout.TeamRollouts(cfg, [0, 2], np.zeros((3, 6)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="record: unknown"):
        team_rollout.TeamRollouts(cfg, *two, record=("trace", "lambda2"))
    # the instances' own parameters are slack mode: out of scope, told as such
    with pytest.raises(ValueError, match="slack mode is not supported"):
        team_rollout.TeamRollouts.from_instances(["3r/line3"], [1], preprocess="own")

"""CPU: the IMPC launch plan (csrc/kernels/launch_plan.hpp) and the operator packing, no GPU.

1. Over a grid of hand-filled operators the plan gives the answers of the selection functions it
   replaced (recorded at the parent commit by tools/launch_plan_grid.cpp -DPARENT into
   tests/golden/launch_plan_parent.txt): kernel name, clock waves, store, defer, capacity launch.
2. For real configurations (mpccbf_host_launch_plan) the names are the literals the GPU tests
   assert after their solves, and the packed buffer keeps its invariants."""
import os
import subprocess

import numpy as np
import pytest

from mpccbf import swarm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "mpc-cbf_amd", "build", "launch_plan_grid")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plan_parent.txt")

DENSE16, DENSE64 = "impc_kernel<6,16,4>", "impc_kernel<6,64,4>"
SEP, WIDE = "impc_sep_kernel<1,1,false,256>", "impc_wide_kernel<256>"
SEP_STORE, WIDE_STORE = "impc_sep_store_kernel<1,256,false>", "impc_wide_store_kernel<256>"
SLACK, SLACK32 = "impc_sep_kernel<1,2,true,256>", "impc_sep_kernel<2,2,true,128>"
FOV, FOV_SLACK = "impc_fov_kernel<false>", "impc_fov_kernel<true>"


def decode(text):
    """{point label: [token per combination]} of a launch_plan_grid output."""
    tokens, points = {}, {}
    for ln in text.splitlines():
        kind, key, rest = ln.split(" ", 2)
        if kind == "T":
            tokens[key] = rest
        else:
            points[key] = [tokens[rest[i:i + 2]] for i in range(0, len(rest), 2)]
    return points


def test_plan_equals_the_parents_selection_functions():
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} not built (make -C mpc-cbf_amd)")
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60, check=True).stdout
    want, got = decode(open(GOLDEN).read()), decode(out)
    # 6 bases x 31 single-field variations; 6 variants x 4 counts x store x csr x knn_k, + 4 with connectivity
    assert len(want) == 186 and all(len(v) == 196 for v in want.values())
    assert list(got) == list(want)
    for label, toks in want.items():
        diff = [(i, t, g) for i, (t, g) in enumerate(zip(toks, got[label])) if t != g]
        assert not diff and len(got[label]) == len(toks), (label, diff[:3])


# configuration -> variant -> the name the GPU tests assert for 64 agents (test_gpu_param_space.py
# NAMES / SLACK / FOV and the cbf_horizon = 8 names, test_gpu_parity.py), without / with a store
COLLISION = {0: WIDE, 3: DENSE16, 4: SEP, 5: WIDE}
CASES = [
    ("base", swarm.config(15), COLLISION),
    ("spd_f 15", swarm.config(15, spd_f=15), COLLISION),
    ("cbf_horizon 8", swarm.config(15, cbf_horizon=8), {0: SEP, 3: DENSE16, 4: SEP, 5: DENSE64}),
    ("slack", swarm.config(15, slack_mode=1), dict.fromkeys((0, 3, 4, 5), SLACK)),
    ("slack cbf_horizon 3", swarm.config(15, slack_mode=1, cbf_horizon=3), dict.fromkeys((0, 3, 4, 5), "")),
    ("slack K 16", swarm.config(16, slack_mode=1), dict.fromkeys((0, 3, 4, 5), SLACK32)),
    ("fov", swarm.fov_config(20), dict.fromkeys((0, 3, 4, 5), FOV)),
    ("fov slack", swarm.fov_config(20, slack_mode=1, slack_cost=1000.0), dict.fromkeys((0, 3, 4, 5), FOV_SLACK)),
]
WITH_STORE = {WIDE: WIDE_STORE, SEP: SEP_STORE}

_ops = {}


def host_ops(mpclib, tag, cfg):
    if tag not in _ops:
        _ops[tag] = mpclib._lib.host_operators(cfg)
    return _ops[tag]


@pytest.mark.parametrize("tag,cfg,names", CASES, ids=[c[0] for c in CASES])
def test_real_configurations(mpclib, tag, cfg, names):
    plan = mpclib._lib.host_launch_plan
    for variant, name in names.items():
        for store in (False, True):
            p = plan(cfg, variant=variant, num_agents=64, csr=True, store=store, wide_max=1024, with_buffer=True)
            want = WITH_STORE.get(name, name) if store else name
            assert p["kernel_name"] == want, (tag, variant, store, p["kernel_name"])
            assert bool(p["store"]) == (store and "store" in want)
            # packing: every operator starts inside the buffer (whose last element is padding)
            assert p["total"] == len(p["buf"]) and 0 <= p["hot"] < p["total"]
            assert all(0 <= o < p["total"] for o in p["offsets"]), p["offsets"]
            # the one-agent-per-wave kernel exactly where its LDS stage holds the hot operators
            if cfg.get("cbf_mode", 0) == 0 and not cfg.get("slack_mode", 0) and variant == 5:
                assert ("wide" in p["kernel_name"]) == (p["hot"] <= p["wide_capacity"]), p["hot"]
            if "wide" in p["kernel_name"]:
                assert 0 < p["hot"] <= p["wide_capacity"] == 2048
            # separable layout: channel d's box rows in their order of G (row f in slot f / 16, lane
            # f % 16, i.e. consecutive), every row after them inert: g = 0 in [-1, 1]
            if p["sep"]:
                sb, rpd = p["sep_sb"], p["sep_rows_per_dim"]
                assert sb == (rpd + 15) // 16 and p["o_Gsep"] + 3 * sb * 16 * 10 <= p["total"]
                rows = p["buf"][p["o_Gsep"]:p["o_Gsep"] + 3 * sb * 16 * 10].reshape(3, sb * 16, 10)
                ops = host_ops(mpclib, tag, cfg)
                assert ops["nz"] == 6
                counts = []
                for d in range(3):
                    mine = np.flatnonzero(np.any(ops["G"][:, 2 * d:2 * d + 2] != 0.0, axis=1))
                    counts.append(len(mine))
                    np.testing.assert_array_equal(rows[d, :len(mine), 0:2], ops["G"][mine, 2 * d:2 * d + 2])
                    np.testing.assert_array_equal(rows[d, :len(mine), 2:8], ops["Gs"][mine])
                    np.testing.assert_array_equal(rows[d, :len(mine), 8], ops["lo"][mine])
                    np.testing.assert_array_equal(rows[d, :len(mine), 9], ops["hi"][mine])
                    inert = rows[d, len(mine):]
                    assert len(inert) > 0 or sb == 1, counts  # (K = 16: two slots per lane, the second mostly inert)
                    assert np.all(inert[:, :8] == 0.0) and np.all(inert[:, 8] == -1.0) and np.all(inert[:, 9] == 1.0)
                assert max(counts) == rpd and sum(counts) == ops["m"]
            else:
                assert cfg.get("cbf_mode", 0) == 1

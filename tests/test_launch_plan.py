"""CPU: the IMPC launch plan (csrc/kernels/launch_plan.hpp) and the operator packing, no GPU.

1. Over a grid of hand-filled operators the plan gives the answers of the selection functions it
   replaced (recorded at the parent commit by tools/launch_plan_grid.cpp -DPARENT into
   tests/golden/launch_plan_parent.txt): kernel name, clock waves, store, defer, capacity launch —
   except where the default variant's dense-layout slot rule moves a
   combination from the 16-lane to the 64-lane instantiation, which the test computes itself.
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
    # One rule has changed since the fixture was recorded: the default variant takes the dense
    # 16-lane instantiation (64 - m CBF row slots, no capacity launch) only when no agent can exceed
    # its slots — grid lists with knn_k x cbf_h <= 64 - m — and the 64-lane one otherwise. The
    # combinations that move are computed here from that rule and the grid's own operators
    # (tools/launch_plan_grid.cpp: m and cbf_h of the base, one field varied per point); for them
    # the parent's token holds with the kernel name alone replaced; every other one is the parent's.
    base_m = {"sep15": 48, "slack16": 48, "slack32": 51, "dense6": 48, "fov": 60, "fovslack": 60}
    combos = [(variant, n, store, csr, knn) for variant in range(6) for n in (0, 5, 1024, 1025)
              for store in (0, 1) for csr in (0, 1) for knn in (8, 9)]
    moved = {}
    for label, toks in want.items():
        base, field = label.split("/")
        name, value = field.split("=")
        m = int(value) if name == "m" else base_m[base]
        cbf_h = int(value) if name == "cbf_h" else 2
        assert len(got[label]) == len(toks) == len(combos) + 4
        for i, (t, g) in enumerate(zip(toks, got[label])):
            expect = t
            if i < len(combos):  # (the last four: connectivity attached)
                variant, _, _, csr, knn = combos[i]
                if variant == 0 and t.startswith(DENSE16 + "|") and (csr or knn * cbf_h > 64 - m):
                    assert m < 64
                    expect = DENSE64 + t[len(DENSE16):]
                    moved.setdefault(label, []).append(i)
            assert g == expect, (label, i, t, g)
    # the moved set: caller lists at every dense point; grid lists where knn_k x cbf_h exceeds the
    # slots (9 x 2 > 16 at m = 48, 8 x 3 > 16, 8 x 2 > 1 at m = 63) and not where it does not
    assert moved and all(b in ("sep15", "dense6") for b in {k.split("/")[0] for k in moved})
    grid16 = [i for i, c in enumerate(combos) if c[0] == 0 and not c[3] and c[4] == 8]
    assert not set(grid16) & set(moved["dense6/lean=0"]) and set(grid16) <= set(moved["dense6/m=63"])
    assert set(grid16) <= set(moved["dense6/cbf_h=3"])
    assert len(moved["dense6/lean=0"]) == 4 * 2 * 3  # counts x store x (csr 8, csr 9, grid 9)
    # the separable kernels' answers (the benchmarked paths) are all the parent's
    for label, toks in want.items():
        for i, t in enumerate(toks):
            if "sep" in t.split("|")[0] or "wide" in t.split("|")[0]:
                assert got[label][i] == t


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

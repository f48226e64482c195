"""Inputs of test_gpu_curve_shape.py (GPU) and test_curve_shape_inputs.py (CPU): the horizon k_hor
and the four curve parameters (num_pieces, num_control_points, continuity_upto_degree,
piece_max_parameter) off the base configuration, on the swarms of param_space_cases. Each case
names its configuration, its swarm, the kernel every variant it runs must report, and the host
operators' sizes; the CPU test pins those and the oracle's status mix, so a GPU pass means what
the case says. Nothing here touches a GPU."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import param_space_cases as P
from mpccbf import swarm

DENSE16, DENSE64 = "impc_kernel<6,16,4>", "impc_kernel<6,64,4>"
SEP, WIDE = "impc_sep_kernel<1,1,false,256>", "impc_wide_kernel<256>"
SLACK, SLACK32 = "impc_sep_kernel<1,2,true,256>", "impc_sep_kernel<2,2,true,128>"
FOV, FOV_SLACK = "impc_fov_kernel<false>", "impc_fov_kernel<true>"

# the four variants of the collision controller where the separable kernels apply (k_hor <= 15 on
# the base curve: at most 16 box rows per channel), 64 agents
SEPARABLE = {0: WIDE, 3: DENSE16, 4: SEP, 5: WIDE}
# more than 16 box rows per channel, fewer than 64 in all, caller lists: the default and the
# separable variants take the dense 64-lane instantiation, variant 3 the 16-lane one it asks for
DENSE = {0: DENSE64, 3: DENSE16, 4: DENSE64, 5: DENSE64}

# name: the case's id; cfg; swarm: "lattice" | "fov" | ("ring", n_ring); names: variant -> kernel;
# sizes: (m, nz, n) of the host operators; opts: mpccbf_options of the context
Case = namedtuple("Case", "name cfg swarm names sizes opts")


def config(k_hor, **over):
    """swarm.config with spd_f = min(8, K) and cbf_horizon = min(2, K) unless given."""
    kw = dict(spd_f=min(8, k_hor), cbf_horizon=min(2, k_hor))
    kw.update(over)
    return swarm.config(k_hor, **kw)


def fov_config(k_hor, **over):
    kw = dict(cbf_mode=1, num_pieces=4)
    kw.update(over)
    return config(k_hor, **kw)


def case(name, cfg, names, sizes, swarm_="lattice", **opts):
    return Case(name, cfg, swarm_, names, sizes, opts)


C3 = dict(num_pieces=2, num_control_points=3, continuity_upto_degree=1, piece_max_parameter=0.75)

HORIZON = [case(f"K{k}", config(k), SEPARABLE, (m, 6, 36))
           for k, m in ((1, 3), (2, 9), (3, 12), (8, 27), (11, 36), (14, 45))]
HORIZON.append(case("K16", config(16), DENSE, (51, 6, 36)))

# four pieces; m = 54, 63 and 66 (the first m >= 64: every variant runs the 64-lane instantiation).
# Variant 3 at K = 17 keeps the 16-lane layout's 10 slots (at most 5 live rows here); at K = 20 its
# single slot is what the capacity cases are about
BEYOND16 = [
    case("K17p4", config(17, num_pieces=4), {0: DENSE64, 3: DENSE16}, (54, 6, 48)),
    case("K20p4", config(20, num_pieces=4), {0: DENSE64}, (63, 6, 48)),
    case("K21p4", config(21, num_pieces=4), {0: DENSE64, 3: DENSE64}, (66, 6, 48)),
]

SLACK_CASES = [
    case("slackK2", config(2, slack_mode=1), {0: SLACK}, (9, 6, 36)),
    case("slackK16", config(16, slack_mode=1), {0: SLACK32}, (51, 6, 36)),
    case("slackK21p4", config(21, num_pieces=4, slack_mode=1), {0: SLACK32}, (66, 6, 48)),
]

FOV_CASES = [
    case("fovK2", fov_config(2), {0: FOV}, (9, 15, 48), "fov"),
    case("fovK6", fov_config(6), {0: FOV}, (21, 15, 48), "fov"),
    case("fovK12", fov_config(12), {0: FOV}, (45, 15, 48), "fov"),
    case("fovK21", fov_config(21), {0: FOV}, (75, 15, 48), "fov"),
    case("fovK12slack", fov_config(12, slack_mode=1, slack_cost=1000.0), {0: FOV_SLACK}, (45, 15, 48), "fov"),
]
# five control points per piece in three pieces: nz = 15 as with the base FoV curve, n = 45
FOV_C5 = case("fovK12c5", fov_config(12, num_pieces=3, num_control_points=5, continuity_upto_degree=4),
              {0: FOV}, (69, 15, 45), "fov")

# the operators' hot prefix (the one-agent-per-wave kernel stages up to 2,048 doubles of it) grows
# with the pieces: 1,990 at five, 2,135 at six — there the default falls back to the 16-lane kernel
# and variant 5 (not a 16-lane variant) to the dense 64-lane instantiation
NO_WIDE = {0: SEP, 3: DENSE16, 4: SEP, 5: DENSE64}
SHAPES = [
    case("p1", config(15, num_pieces=1, piece_max_parameter=1.5), SEPARABLE, (48, 6, 12)),
    case("c3K8", config(8, **C3), SEPARABLE, (16, 6, 18)),
    case("c3K16", config(16, **C3), SEPARABLE, (18, 6, 18)),
    case("T037", config(12, piece_max_parameter=0.37), SEPARABLE, (39, 6, 36)),
    case("p5", config(15, num_pieces=5, piece_max_parameter=0.3), SEPARABLE, (48, 6, 60)),
    case("p6", config(15, num_pieces=6, piece_max_parameter=0.25), NO_WIDE, (48, 6, 72)),
    case("p10", config(15, num_pieces=10, piece_max_parameter=0.15), NO_WIDE, (48, 6, 120)),
]
HOT = {"p5": 1990, "p6": 2135}

# no kernel takes these reduced dimensions: nz = 12 and nz = 9 (collision), nz = 18 (FoV)
REFUSED = [
    case("cont2", config(15, continuity_upto_degree=2), dict.fromkeys((0, 3, 4, 5), ""), (54, 12, 36)),
    case("c5cont4", config(15, num_control_points=5, continuity_upto_degree=4), dict.fromkeys((0, 3, 4, 5), ""),
         (87, 9, 45)),
    case("fovp5", fov_config(20, num_pieces=5), None, (72, 18, 60), "fov"),
]

# dense-layout capacity: configurations whose box rows leave the 16-lane instantiation fewer CBF row
# slots (64 - m) than some agent stages; the default variant must run the 64-lane one
CAPACITY = [
    case("capK20p4", config(20, num_pieces=4), {0: DENSE64}, (63, 6, 48)),
    case("capK16nofilter", config(16), {0: DENSE64}, (51, 6, 36), no_cbf_filter=True),
    case("capK11keep", config(11), {0: DENSE64}, (63, 6, 36), keep_redundant=True),
    case("capK16ring", config(16, cbf_horizon=2), {0: DENSE64}, (51, 6, 36), ("ring", 12)),
    case("capK16ring8", config(16, cbf_horizon=8), {0: DENSE64}, (51, 6, 36), ("ring", 12)),
]
# the forced 16-lane layout on the ring: agent 0's 24 live rows against 13 slots
FORCED16 = case("forcedK16ring", config(16, cbf_horizon=2), {3: DENSE16}, (51, 6, 36), ("ring", 12))
# the range edge: 15 h = 10 x 0.15 passes swarm.validate, and the curve's own parameter range
# (the accumulated 0.15s) ends just below the last sample
RANGE_EDGE = dict(k_hor=16, num_pieces=10, piece_max_parameter=0.15)


def lattice():
    st, tg = P.crowded(64, 0.45, 5)
    return (st, tg) + swarm.knn_csr(st, 8, 6.0)


def fov_inputs(cfg, scale=0.7):
    st, tg = P.fov_swarm(scale=scale)
    return (st, tg) + swarm.fov_csr(st, 8, cfg["fov_Rs"], cfg["fov_beta"])


def inputs(c):
    """(states, targets, row_ptr, col) of a case."""
    if c.swarm == "lattice":
        return lattice()
    if c.swarm == "fov":
        return fov_inputs(c.cfg)
    return P.ring(c.swarm[1])


# ---- the curve in numpy (SingleParameterPiecewiseCurve::eval restated as in
# tests/golden/make_golden.py: lower_bound piece lookup, local parameter clamped to the piece) ----

def bernstein(deg, T, t, d):
    """Derivative d of the degree-deg Bernstein basis on [0, T] at t (monomial expansion)."""
    out = np.zeros(deg + 1)
    for i in range(deg + 1):
        acc = 0.0
        for j in range(deg + 1 - d):
            if j + d >= i:
                acc += (math.comb(deg - i, j + d - i) * (1.0 / T) ** (j + d) * math.perm(j + d, d)
                        * t ** j * (1 if (j + d - i) % 2 == 0 else -1))
        out[i] = acc * math.comb(deg, i)
    return out


def curve_state(cfg, x, t):
    """(position, velocity) in (x, y, yaw) at parameter t of the curve with control points x
    (piece-major, then channel, then control point)."""
    npc, ncp, T = cfg["num_pieces"], cfg["num_control_points"], cfg["piece_max_parameter"]
    cum = np.zeros(npc)
    acc = 0.0
    for i in range(npc):
        acc += T
        cum[i] = acc
    i = min(int(np.searchsorted(cum, t, side="left")), npc - 1)
    local = min(max(t if i == 0 else t - cum[i - 1], 0.0), T)
    cp = np.asarray(x, dtype=np.float64).reshape(npc, 3, ncp)[i]
    return np.concatenate([cp @ bernstein(ncp - 1, T, local, 0), cp @ bernstein(ncp - 1, T, local, 1)])


def oracle_batch(cfg, states, targets, rp, col, threads=8):
    """param_space_cases.oracle_batch with the agents spread over a few threads (every call into
    the oracle is independent and leaves the interpreter lock; the results are the serial ones)."""
    from concurrent.futures import ThreadPoolExecutor

    import oracle_lib as O
    p = O.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    one = lambda a: O.impc_optimize(p, states, a, col[rp[a]:rp[a + 1]], refs[a])  # noqa: E731
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(one, range(len(rp) - 1)))


def moved_by_neighbours(cfg, states, targets, rp, col, res, tol=1e-6):
    """Agents whose result differs from the one they get planning alone (empty lists): a different
    status, or a last curve further than tol away — some row of a neighbour is active at their
    optimum. The FoV cases' measure of live rows (all of them are OPTIMAL)."""
    n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    none = np.zeros(len(rp), dtype=np.int32), np.zeros(0, dtype=np.int32)
    alone = oracle_batch(cfg, states, targets, *none)
    return [i for i, (a, b) in enumerate(zip(res, alone))
            if list(a["status"]) != list(b["status"]) or
            (a["status"][-1] == 0 and np.max(np.abs(a["x"][-1][:n] - b["x"][-1][:n])) > tol)]

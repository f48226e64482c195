"""Inputs of test_gpu_monitor.py (GPU) and test_monitor_inputs.py (CPU): hand-built sample arrays for
the safety monitor (mpccbf_monitor_score) with their expected outputs from mpccbf.metrics and plain
numpy. Coordinates are small dyadic numbers unless a case says otherwise, so that every product and
sum is exact in any arithmetic and a decision on the CPU is the decision on the device.

A case is a dict: samples (S x N x 6, every row of the table in every sample), agent_first /
num_agents (the rows whose states move; the others are fixed rows), goals (num_agents x 3 or None),
monitor (keyword arguments of mpccbf.SafetyMonitor) and layout ("table": one sample as a state table,
"trace": the agents as n x S x 6, the substeps layout). Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

import exact_geometry_cases as G
from mpccbf import metrics
from mpccbf.monitor import result_from_outputs

INF_BITS = 0x7FF0000000000000
CELL_MARGIN = G.CELL_MARGIN


def table_size(n: int) -> int:
    """hash_table_size of kernels/neighbors.hip (what mpccbf_monitor_table_size returns)."""
    t = 1024
    while t < 2 * n:
        t <<= 1
    return t


def watch_of(mon: dict) -> float:
    w = mon.get("watch_radius")
    return 3.0 * mon["d_min"] if w is None else w


def cell_of(x: float, watch: float) -> int:
    return G.library_cell(x, watch)


def bits(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).view(np.int64)


# -------------------------------------------------------------------------------------------------
# the device outputs, restated in numpy (all pairs, no hash)
# -------------------------------------------------------------------------------------------------
def pair_tests(p, mon):
    """For one sample's positions p (N x 2): the strict upper triangle's (i, j), squared distance,
    within the watch radius, collision and inside-d_min flags."""
    n = len(p)
    iu, ju = np.triu_indices(n, k=1)
    dx, dy = p[ju, 0] - p[iu, 0], p[ju, 1] - p[iu, 1]
    d2 = dx * dx + dy * dy
    w = watch_of(mon)
    seen = d2 <= w * w
    if mon.get("shape_type", "box") == "box":
        hit = metrics.collision_check(p[iu, 0], p[iu, 1], p[ju, 0], p[ju, 1], list(mon["shape"]), "box")
    else:
        r = float(mon["shape"])
        hit = d2 <= (2 * r) * (2 * r)
    inside = d2 < mon["d_min"] * mon["d_min"]
    return iu, ju, d2, seen, hit & seen, inside & seen


def model_outputs(case, sample_log_rows=0, rows=None) -> dict:
    """The monitor's raw outputs after a reset and one score of the case."""
    S, N = case["samples"].shape[:2]
    rows = N if rows is None else rows
    mon = case["monitor"]
    a0, na = case["agent_first"], case["num_agents"]
    summary = np.array([S, -1, 0, 0, INF_BITS], dtype=np.int64)
    reached = np.full(rows, -1, dtype=np.int64)
    min_d2 = np.full(rows, np.inf)
    hits = np.zeros(rows, dtype=np.int32)
    unsafe = np.zeros(rows, dtype=np.int32)
    log = np.zeros((sample_log_rows, 3), dtype=np.int64)
    log[:, 2] = INF_BITS
    gr = mon.get("goal_radius", 1.0)
    best = np.inf
    for s in range(S):
        p = case["samples"][s, :, :2]
        iu, ju, d2, seen, hit, inside = pair_tests(p, mon)
        for arr, flag in ((hits, hit), (unsafe, inside)):
            on = np.zeros(N, dtype=bool)
            on[iu[flag]] = True
            on[ju[flag]] = True
            arr[:N] += on
        for i, j, d in zip(iu[seen], ju[seen], d2[seen]):
            min_d2[i] = min(min_d2[i], d)
            min_d2[j] = min(min_d2[j], d)
        smin = d2[seen].min() if seen.any() else np.inf
        best = min(best, smin)
        summary[2] += int(hit.sum())
        summary[3] += int(inside.sum())
        if hit.any() and summary[1] < 0:
            k = int(np.argmax(hit))  # (i, j) ascending: the script's order
            summary[1] = (s << 40) | (int(iu[k]) << 20) | int(ju[k])
        if s < sample_log_rows:
            log[s] = (int(hit.sum()), int(inside.sum()), int(bits(smin)))
        if case["goals"] is not None:
            g = case["goals"]
            dx, dy = p[a0:a0 + na, 0] - g[:, 0], p[a0:a0 + na, 1] - g[:, 1]
            inside_goal = dx * dx + dy * dy <= gr * gr
            r = reached[a0:a0 + na]
            r[inside_goal & (r < 0)] = s
    summary[4] = int(bits(best))
    return dict(summary=summary, reached_at=reached, min_d2=min_d2, hit_samples=hits, unsafe_samples=unsafe,
                sample_log=log)


def model_result(case) -> dict:
    o = model_outputs(case)
    return result_from_outputs(o["summary"], o["reached_at"], o["min_d2"], o["hit_samples"], o["unsafe_samples"],
                               agent_first=case["agent_first"], num_agents=case["num_agents"])


def script_result(case):
    """metrics.instance_success on the case's samples (every row a robot; cases with goals for all)."""
    assert case["agent_first"] == 0 and case["num_agents"] == case["samples"].shape[1]
    mon = case["monitor"]
    traj = np.transpose(case["samples"], (1, 0, 2))
    shape = list(mon["shape"]) if mon.get("shape_type", "box") == "box" else float(mon["shape"])
    return metrics.instance_success(traj, case["goals"], mon.get("goal_radius", 1.0), shape,
                                    mon.get("shape_type", "box"))


# -------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------
BOX = dict(shape=(0.25, 0.25), shape_type="box")  # corner = centre - 0.125, extent 0.5: all dyadic


def _case(xy, *, monitor, goals=None, agent_first=0, num_agents=None, layout=None):
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim == 2:
        xy = xy[None]
    S, N = xy.shape[:2]
    samples = np.zeros((S, N, 6))
    samples[:, :, :2] = xy
    samples[:, :, 2] = 0.125  # (the monitor reads x and y only)
    samples[:, :, 3] = -7.0
    num_agents = N - agent_first if num_agents is None else num_agents
    if goals is not None:
        g = np.zeros((num_agents, 3))
        g[:, :2] = np.asarray(goals, dtype=np.float64)
        goals = g
    return dict(samples=samples, agent_first=agent_first, num_agents=num_agents, goals=goals, monitor=dict(monitor),
                layout=layout or ("table" if S == 1 else "trace"))


def rows_1():
    return _case([[1.5, -2.0]], monitor=dict(BOX, d_min=1.0), goals=[[1.5, -1.0]])


def rows_2():
    """Two overlapping boxes inside d_min."""
    return _case([[0.0, 0.0], [0.25, 0.125]], monitor=dict(BOX, d_min=1.0), goals=[[5.0, 5.0], [0.25, 0.125]])


def _lattice(nx, ny, spacing, x0=0.0, y0=0.0):
    g = np.arange(nx * ny)
    return np.stack([x0 + spacing * (g % nx), y0 + spacing * (g // nx)], axis=1)


def rows_65():
    """13 x 5 lattice at spacing 1.0 around the origin with d_min 1.25 (axis neighbours inside it,
    diagonal ones not) and one row moved onto its neighbour's box."""
    xy = _lattice(13, 5, 1.0, -6.0, -2.0)
    xy[40] = xy[39] + [0.375, 0.25]
    return _case(xy, monitor=dict(BOX, d_min=1.25, watch_radius=2.0))


def rows_300():
    """20 x 15 lattice at spacing 0.75: more than one block of the query launch; two hits."""
    xy = _lattice(20, 15, 0.75, -7.0, -5.0)
    xy[299] = xy[0] + [0.25, 0.0]
    xy[150] = xy[151] + [0.0, -0.375]
    return _case(xy, monitor=dict(BOX, d_min=1.0))


CROWD = 70


def crowded_cell():
    """70 rows at one position (more than the 64 slots of the IMPC grid's buckets) and 5 apart."""
    xy = np.concatenate([np.tile([[0.5, -0.25]], (CROWD, 1)), _lattice(5, 1, 2.0, 8.0, 8.0)])
    return _case(xy, monitor=dict(BOX, d_min=1.0))


SHARED_WATCH = G.SHARED_QUERY[1]


def far_cell_with_bucket(cell, mask):
    """A cell at least 8 cells from `cell` on both axes with the same bucket."""
    h = G.cell_hash(cell[0], cell[1], mask)
    for cx in range(cell[0] + 8, cell[0] + 400):
        for cy in range(cell[1] + 8, cell[1] + 400):
            if G.cell_hash(cx, cy, mask) == h:
                return cx, cy
    raise AssertionError("no far cell shares the bucket")


def shared_bucket():
    """exact_geometry_cases.shared_bucket (its centre cell's 3 x 3 block reaches two buckets twice),
    and a second cluster in a distant cell that shares the first cluster's centre bucket: a bucket
    read twice, or a foreign cell's rows taken for neighbours, shows in the counts."""
    a = G.shared_bucket()[0][:, :2]
    mask = table_size(2 * len(a)) - 1
    far = far_cell_with_bucket(G.SHARED_CELL, mask)
    edge = SHARED_WATCH * (1.0 + CELL_MARGIN)
    b = a - a.min(axis=0) + [far[0] * edge + 0.5, far[1] * edge + 0.5]
    return _case(np.concatenate([a, b]), monitor=dict(BOX, d_min=2.5, watch_radius=SHARED_WATCH))


EDGE_WATCH = 4.0


def cell_edges():
    """Rows exactly on cell edges (multiples of the cell edge 4 (1 + 2^-20), negative ones included),
    each with a partner 0.375 to its left whose box overlaps it, on the other side of the edge."""
    edge = EDGE_WATCH * (1.0 + CELL_MARGIN)
    k = np.arange(-2, 3)
    a = np.stack(np.meshgrid(k * edge, k * edge), axis=-1).reshape(-1, 2)
    return _case(np.concatenate([a, a - [0.375, 0.0]]), monitor=dict(BOX, d_min=1.0, watch_radius=EDGE_WATCH))


def negative_lattice():
    """exact_geometry_cases.tie_lattice: 12 x 12 at spacing 2 from -12 to +10, d_min 2.5."""
    return _case(G.tie_lattice()[0][:, :2], monitor=dict(BOX, d_min=2.5, watch_radius=4.0))


def box_threshold():
    """Pairs of boxes (half 0.25: width 0.5) exactly touching along x and along y (no hit: the
    script's comparisons are strict) and one ulp inside (hit), far from each other."""
    inside = np.nextafter(0.5, 0.0)
    xy = [[0.0, 0.0], [0.5, 0.0],        # touching in x
          [10.0, 0.0], [10.0, 0.5],      # touching in y
          [0.0, 30.0], [inside, 30.0],   # one ulp inside in x (the lower row at 0: the corner
          [40.0, 0.0], [40.25, inside],  # one ulp inside in y   arithmetic stays exact)
          [0.0, 20.0], [-0.5, 20.5]]     # touching at a corner
    return _case(xy, monitor=dict(BOX, d_min=0.75, watch_radius=2.0))


def circle_pairs():
    """Circle shape, radius 0.25: centres 0.5 apart (hit: inclusive), 0.625 apart (no hit)."""
    xy = [[0.0, 0.0], [0.0, 0.5], [10.0, 0.0], [10.375, 0.5]]
    return _case(xy, monitor=dict(shape=0.25, shape_type="circle", d_min=0.75, watch_radius=2.0))


def watch_edge():
    """Rows 0 and 1 exactly watch_radius = 5 apart (3-4-5: seen, min d2 = 25); row 2 a hair more than
    5 from row 0 and 10 from row 1 (sees nobody: min d2 stays +inf)."""
    xy = [[0.0, 0.0], [3.0, 4.0], [-3.0, -4.0 - 2.0 ** -50]]
    return _case(xy, monitor=dict(BOX, d_min=2.0, watch_radius=5.0))


def goal_exact():
    """Goal radius 1.25: agent 0 at offset (0.75, 1.0) from its goal, distance exactly 1.25 (reached:
    inclusive, every product exact); agent 1 one ulp farther in y (not reached)."""
    goals = [[4.0, -2.0], [-8.0, 16.0]]
    xy = [[4.75, -1.0], [-8.0 + 0.75, 16.0 + 1.0 + 2.0 ** -48]]
    return _case(xy, monitor=dict(BOX, d_min=1.0, goal_radius=1.25), goals=goals)


def first_order():
    """Pairs (2, 3), (1, 5) and (1, 4) collide in the same sample: the script meets (1, 4) first."""
    xy = [[0.0, 0.0], [4.0, 0.0], [8.0, 0.0], [8.25, 0.0], [4.25, 0.0], [3.75, 0.125], [12.0, 0.0]]
    return _case(xy, monitor=dict(BOX, d_min=1.0))


def _timing(collide_at):
    """Two robots closing in on goals 4 apart, the last arriving in sample 3 of 6; they pass through
    each other's box in sample `collide_at` only (a detour of robot 1)."""
    S = 6
    xy = np.zeros((S, 2, 2))
    xy[:, 0, 0] = [-4.0, -3.0, -2.0, -2.0, -2.0, -2.0]   # goal (-2, 0): inside radius 1 from sample 1
    xy[:, 1, 0] = [6.0, 5.0, 4.0, 3.0, 2.5, 2.0]         # goal (2, 0): inside radius 1 from sample 3
    xy[collide_at, 1] = xy[collide_at, 0] + [0.25, 0.125]
    if collide_at == 3:
        xy[3, 0] = [1.5, 0.0]  # (robot 1 still arrives in sample 3: the collision happens at its goal)
        xy[3, 1] = [1.75, 0.125]
    return _case(xy, monitor=dict(BOX, d_min=1.0), goals=[[-2.0, 0.0], [2.0, 0.0]])


def collision_before_arrival():
    return _timing(2)


def collision_at_arrival():
    return _timing(3)


def collision_after_arrival():
    return _timing(5)


def fixed_rows():
    """8 rows, agents 3 .. 5, S = 4: agent 4 walks onto fixed row 6; fixed rows 0 and 1 overlap in every
    sample; agent 3 reaches its goal in sample 2, agent 5 starts on its goal, agent 4 never arrives."""
    S = 4
    xy = np.zeros((S, 8, 2))
    xy[:, 0] = [0.0, 0.0]
    xy[:, 1] = [0.25, 0.25]
    xy[:, 2] = [-6.0, 3.0]
    xy[:, 6] = [6.0, 6.0]
    xy[:, 7] = [-9.0, -9.0]
    for s in range(S):
        xy[s, 3] = [10.0 - 2.0 * s, -4.0]
        xy[s, 4] = [6.0, 3.0 + s]
        xy[s, 5] = [-3.0, -3.0]
    return _case(xy, monitor=dict(BOX, d_min=1.5), goals=[[6.5, -4.0], [30.0, 30.0], [-3.0, -3.5]], agent_first=3,
                 num_agents=3)


def trace10():
    """33 robots on a 0.75 lattice contracting towards its centre over 10 samples (steps of 1/16 of
    the offset): pairs inside d_min from the start, boxes overlapping towards the end."""
    base = _lattice(11, 3, 0.75, -3.75, -0.75)
    xy = np.stack([base * (1.0 - s / 16.0) for s in range(10)])
    return _case(xy, monitor=dict(BOX, d_min=1.0), goals=base * 0.5)


CASES = {f.__name__: f for f in (
    rows_1, rows_2, rows_65, rows_300, crowded_cell, shared_bucket, cell_edges, negative_lattice, box_threshold,
    circle_pairs, watch_edge, goal_exact, first_order, collision_before_arrival, collision_at_arrival,
    collision_after_arrival, fixed_rows, trace10)}

_BUILT = {}


def case(name):
    """The case and its expected raw outputs (with a 12-row sample log), built once."""
    if name not in _BUILT:
        c = CASES[name]()
        _BUILT[name] = (c, model_outputs(c, sample_log_rows=12))
    return _BUILT[name]


# -------------------------------------------------------------------------------------------------
# seeded random small traces (result_from_outputs against the script)
# -------------------------------------------------------------------------------------------------
def random_trace(seed):
    """A few robots walking on a 1/8 grid from random starts to random goals (straight lines,
    rounded to the grid), arriving at different times, some never; every squared distance is exact."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 6))
    S = int(rng.integers(1, 13))
    start = rng.integers(-24, 25, size=(n, 2)) / 8.0
    goal = rng.integers(-24, 25, size=(n, 2)) / 8.0
    if seed % 4 == 0:
        goal = start + rng.integers(-6, 7, size=(n, 2)) / 8.0  # (everybody starts near its goal)
    dur = rng.integers(1, 16, size=n)
    xy = np.zeros((S, n, 2))
    for s in range(S):
        f = np.minimum(1.0, s / dur)[:, None]
        xy[s] = np.round((start + (goal - start) * f) * 8.0) / 8.0
    return _case(xy, monitor=dict(BOX, d_min=1.0), goals=goal, layout="trace")

"""Inputs of test_gpu_exact_geometry.py (GPU) and test_exact_geometry_inputs.py (CPU): swarms whose
coordinates are small integers times a power of two, so that every squared distance is exact in
any arithmetic (with or without FMA contraction) and a tie on the CPU is a tie on the device:
exact ties that the k-nearest cut falls into, neighbours at exactly the radius, agents on cell
edges and at negative coordinates, coincident agents, a 3 x 3 cell block that reaches one hash
bucket twice, and neighbour lists that give identical or linearly dependent CBF rows.

The neighbour contract (include/mpccbf.h, swarm.knn_csr / swarm.fov_csr): the knn_k nearest others
by planar distance, distance <= knn_radius (inclusive), ties broken by agent index, the list
sorted by index, j != self. Nothing here touches a GPU."""
from __future__ import annotations

import math

import numpy as np

import oracle_lib as O
from mpccbf import swarm

# ---------------------------------------------------------------------------------------------
# replicas of the library's cell arithmetic (kernels/impc.hpp)
# ---------------------------------------------------------------------------------------------
GRID_CAP = 64   # slots per bucket (beyond: the full-table scan)
NB_CAP = 64     # candidates ranked at once (beyond: the streaming query)
CELL_MARGIN = 2.0 ** -20  # grid_inv_cell: the cell edge is knn_radius * (1 + 2^-20)


def cell_hash(cx: int, cy: int, mask: int) -> int:
    """cell_hash of kernels/impc.hpp (64-bit wrapping products of the signed cell indices)."""
    m64 = (1 << 64) - 1
    h = ((cx * 73856093) & m64) ^ ((cy * 19349663) & m64)
    return ((h ^ (h >> 29)) & 0xFFFFFFFF) & mask


def naive_cell(x: float, radius: float) -> int:
    """floor(x * inv) with inv = 1.0 / radius: a cell edge of exactly the radius. Two agents whose
    computed distance is <= radius can land two cells apart under it (the radius_edge pairs)."""
    return math.floor(x * (1.0 / radius))


def library_cell(x: float, radius: float) -> int:
    """floor(x * inv_cell) with the library's inv_cell (grid_inv_cell in kernels/impc.hpp)."""
    return math.floor(x * (1.0 / (radius * (1.0 + CELL_MARGIN))))


def block_hashes(cx: int, cy: int, mask: int = 1023):
    """The buckets of the 3 x 3 cells around (cx, cy), in the kernels' order."""
    return [cell_hash(cx + dx, cy + dy, mask) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def d2_matrix(states):
    p = np.asarray(states)[:, :2]
    return np.sum((p[:, None, :] - p[None, :, :]) ** 2, axis=-1)


def csr_rows(rp, col):
    return [list(col[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)]


def padded(rp, col, first=0, count=None, width=16):
    """The CSR lists of agents [first, first + count) as nb_out holds them: count x 16, -1 after
    the last entry."""
    count = len(rp) - 1 - first if count is None else count
    out = np.full((count, width), -1, dtype=np.int32)
    for a in range(count):
        row = col[rp[first + a]:rp[first + a + 1]]
        out[a, :len(row)] = row
    return out


def cuts_tie(states, k, radius, cone=None):
    """Agents whose k-th and (k+1)-th nearest candidates (within the radius; cone = (fov,) for
    the FoV filter) have equal squared distance: the cut falls inside a tie shell there."""
    d2 = d2_matrix(states)
    n = len(states)
    out = []
    for i in range(n):
        ok = d2[i] <= radius * radius
        ok[i] = False
        if cone is not None:
            d = states[:, :2] - states[i, :2]
            off = np.abs(np.angle(np.exp(1j * (np.arctan2(d[:, 1], d[:, 0]) - states[i, 2]))))
            ok &= off < 0.5 * cone
        d = np.sort(d2[i][ok])
        if len(d) > k and d[k - 1] == d[k]:
            out.append(i)
    return out


# ---------------------------------------------------------------------------------------------
# tie_lattice, subrange, fov_lattice
# ---------------------------------------------------------------------------------------------
TIE_SIDE, TIE_SPACING = 12, 2.0
# (k, radius); (8, 4.0) cuts no tie shell: the control
TIE_QUERIES = [(1, 2.0), (3, 2.0), (6, 4.0), (10, 4.0), (16, 4.0), (8, 4.0)]
TIE_CONTROL = (8, 4.0)
SUBRANGES = [(5, 50), (143, 1)]  # (agent_first, num_agents) on tie_lattice


def tie_lattice():
    """12 x 12 agents, spacing 2.0, x and y from -12 to +10 (negative coordinates, agents exactly
    on cell edges), velocities -0.25 * sign(position) per axis (towards the origin; none across an
    axis the agent sits on), targets -0.5 * position. Returns (states 144 x 6, targets 144 x 3)."""
    n = TIE_SIDE * TIE_SIDE
    g = np.arange(n)
    states = np.zeros((n, 6))
    states[:, 0] = -12.0 + TIE_SPACING * (g % TIE_SIDE)
    states[:, 1] = -12.0 + TIE_SPACING * (g // TIE_SIDE)
    states[:, 3] = -0.25 * np.sign(states[:, 0])
    states[:, 4] = -0.25 * np.sign(states[:, 1])
    targets = np.zeros((n, 3))
    targets[:, :2] = -0.5 * states[:, :2]
    return states, targets


FOV_YAW = 0.3
# (k, radius = fov_Rs); in the cone the candidates' squared distances in units of 4 are
# 1, 2, 4, 5, 5, 5, 8, 9 (the radius itself), 10, 10, 10: k = 4 and 5 cut the shell of three,
# k = 8 cuts none (the control)
FOV_QUERIES = [(4, 6.0), (5, 6.0), (8, 6.0)]


def fov_lattice():
    """tie_lattice positions, every yaw 0.3 (cone edges at 77.19 and -42.81 degrees, away from
    every lattice bearing), yaw targets 0.3. For swarm.fov_config(20)."""
    states, targets = tie_lattice()
    states[:, 2] = FOV_YAW
    targets[:, 2] = FOV_YAW
    return states, targets


def cone_margin(states, radius, fov):
    """Smallest | |bearing - yaw| - fov / 2 | over all ordered pairs within the radius."""
    best = np.inf
    d2 = d2_matrix(states)
    for i in range(len(states)):
        js = np.nonzero((d2[i] <= radius * radius) & (np.arange(len(states)) != i))[0]
        d = states[js, :2] - states[i, :2]
        off = np.abs(np.angle(np.exp(1j * (np.arctan2(d[:, 1], d[:, 0]) - states[i, 2]))))
        if len(off):
            best = min(best, float(np.min(np.abs(off - 0.5 * fov))))
    return best


# ---------------------------------------------------------------------------------------------
# radius_edge
# ---------------------------------------------------------------------------------------------
# (name, radius, axis, A, B, cells apart under naive_cell): a pair along one axis whose computed
# difference is exactly the radius. "miss" pairs sit two cells apart when the cell edge is exactly
# the radius (a 3 x 3 query never sees the partner); the mirrored reproducer is one cell apart
# (floor rounds the other way at negative coordinates) and stays as the at-the-radius case there.
# Found by scanning k * radius +- a few ulps for d * d <= r * r with floor cells 2 apart; no
# denormals. With radius 4.0 the reciprocal is exact: there the rounded subtraction alone
# (8.0 - 3.9999999999999996 == 4.0) puts the pair two cells apart.
RADIUS_EDGE_PAIRS = [
    ("r5_x", 5.0, 0, "0x1.3ffffffffffffp+3", "0x1.dffffffffffffp+3", 2),
    ("r5_y", 5.0, 1, "0x1.3ffffffffffffp+3", "0x1.dffffffffffffp+3", 2),
    ("r5_x_mirrored", 5.0, 0, "-0x1.3ffffffffffffp+3", "-0x1.dffffffffffffp+3", 1),
    ("r5_x_far", 5.0, 0, "0x1.3ffffffffffffp+4", "0x1.8ffffffffffffp+4", 2),
    ("r2.5_x", 2.5, 0, "0x1.3ffffffffffffp+2", "0x1.dffffffffffffp+2", 2),
    ("r2.5_y", 2.5, 1, "0x1.3ffffffffffffp+3", "0x1.8ffffffffffffp+3", 2),
    ("r10_x", 10.0, 0, "0x1.3ffffffffffffp+4", "0x1.dffffffffffffp+4", 2),
    ("r10_y", 10.0, 1, "0x1.3ffffffffffffp+5", "0x1.8ffffffffffffp+5", 2),
    ("r4_x", 4.0, 0, "0x1.fffffffffffffp+1", "0x1.0000000000000p+3", 2),
]
RADIUS_EDGE_K = 8
# six ordinary agents around the pair, offsets from A in units of the radius (dyadic, no ties
# with the pair, none at the radius)
_EDGE_OFFSETS = [(-0.3125, 0.375), (0.25, -0.5625), (0.5625, 0.3125), (0.4375, -0.34375),
                 (1.1875, 0.46875), (-0.625, -0.21875)]


def radius_edge(name):
    """States (8 x 6) and targets of one pair case: agents 0 (A) and 1 (B) on one axis, the other
    coordinate 0.75, and six ordinary agents. Returns (states, targets, radius)."""
    _, radius, axis, a, b, _ = next(p for p in RADIUS_EDGE_PAIRS if p[0] == name)
    a, b = float.fromhex(a), float.fromhex(b)
    states = np.zeros((8, 6))
    states[0, axis], states[1, axis] = a, b
    states[:2, 1 - axis] = 0.75
    for i, (ox, oy) in enumerate(_EDGE_OFFSETS):
        states[2 + i, axis] = a + ox * radius
        states[2 + i, 1 - axis] = 0.75 + oy * radius
    targets = states[:, :3].copy()
    targets[:, 1 - axis] += 1.0
    return states, targets, radius


# ---------------------------------------------------------------------------------------------
# coincident
# ---------------------------------------------------------------------------------------------
COINCIDENT_COUNTS = [2, 3, 70]
COINCIDENT_QUERY = (8, 4.0)


def coincident(m):
    """81 agents: a 9 x 9 lattice (spacing 1.0, centred on the origin), of which m agents, spread
    over the index range, sit at one position (0.5, -0.25) instead of their site. Their mutual
    distances are 0, so index alone orders them. m = 70 overflows the position's bucket (GRID_CAP
    64: the full-table scan) and puts more than 64 candidates within the radius (the streaming
    query). Returns (states, targets, indices of the coincident agents)."""
    n = 81
    g = np.arange(n)
    states = np.zeros((n, 6))
    states[:, 0] = (g % 9) - 4.0
    states[:, 1] = (g // 9) - 4.0
    who = np.sort(np.argsort((g * 37) % n, kind="stable")[:m])
    states[who, 0], states[who, 1] = 0.5, -0.25
    states[:, 3] = 0.125 * ((g % 3) - 1.0)
    targets = np.zeros((n, 3))
    targets[:, :2] = 1.5 * states[:, :2]
    return states, targets, who


# ---------------------------------------------------------------------------------------------
# shared_bucket
# ---------------------------------------------------------------------------------------------
SHARED_CELL = (-64, -31)  # its 3 x 3 block reaches buckets 74 and 308 twice at mask 1023
SHARED_QUERY = (8, 4.0)


def shared_bucket():
    """A dyadic 5 x 5 patch (spacing 2.0, radius 4.0) over the cell SHARED_CELL, whose 3 x 3 block
    maps two pairs of cells to one bucket each: a bucket read twice shows as a duplicated index.
    Returns (states 25 x 6, targets)."""
    r = SHARED_QUERY[1]
    g = np.arange(25)
    states = np.zeros((25, 6))
    states[:, 0] = SHARED_CELL[0] * r - 2.0 + 2.0 * (g % 5) + 0.5
    states[:, 1] = SHARED_CELL[1] * r - 2.0 + 2.0 * (g // 5) + 0.5
    states[:, 3] = 0.25 * np.where(g % 2 == 0, 1.0, -1.0)
    targets = states[:, :3].copy()
    targets[:, 0] += 1.0
    return states, targets


# ---------------------------------------------------------------------------------------------
# tiny
# ---------------------------------------------------------------------------------------------
def tiny_single():
    """One agent alone (an empty list). Returns (states, targets, k, radius)."""
    states = np.array([[-3.0, 2.5, 0.0, 0.25, 0.0, 0.0]])
    return states, np.array([[1.0, 2.0, 0.0]]), 8, 4.0


def tiny_pair():
    """Two agents exactly `radius` apart across the origin: each lists the other."""
    states = np.array([[-2.0, 1.0, 0.0, 0.25, 0.0, 0.0], [2.0, 1.0, 0.0, -0.25, 0.0, 0.0]])
    return states, np.array([[-4.0, 1.0, 0.0], [4.0, 1.0, 0.0]]), 8, 4.0


# ---------------------------------------------------------------------------------------------
# every neighbour-set case of the collision controller as one table
# ---------------------------------------------------------------------------------------------
def neighbour_cases():
    """{name: (states, targets, k, radius)}: every collision-controller neighbour-set case
    (tie_lattice with each query, radius_edge, coincident, shared_bucket, tiny)."""
    cases = {}
    st, tg = tie_lattice()
    for k, r in TIE_QUERIES:
        cases[f"tie_k{k}_r{r:g}"] = (st, tg, k, r)
    for name, *_ in RADIUS_EDGE_PAIRS:
        s, t, r = radius_edge(name)
        cases[f"edge_{name}"] = (s, t, RADIUS_EDGE_K, r)
    for m in COINCIDENT_COUNTS:
        s, t, _ = coincident(m)
        cases[f"coincident_{m}"] = (s, t) + COINCIDENT_QUERY
    cases["shared_bucket"] = shared_bucket() + SHARED_QUERY
    cases["tiny_single"] = tiny_single()
    cases["tiny_pair"] = tiny_pair()
    return cases


_REF = {}


def reference_lists(name):
    """swarm.knn_csr of a neighbour_cases() entry, computed once."""
    if name not in _REF:
        st, _, k, r = neighbour_cases()[name]
        _REF[name] = swarm.knn_csr(st, k, r)
    return _REF[name]


# ---------------------------------------------------------------------------------------------
# dependent_rows (CSR mode, collision controller, swarm.config(15))
# ---------------------------------------------------------------------------------------------
def dependent_point():
    """Ego 0 at rest at the origin, neighbours 1 and 2 both at (2, 0) at rest (the same state),
    neighbour 3 at (0, 2). Lists with duplicate entries, coincident neighbours and a corner of
    two active rows. Returns (states 4 x 6, [(name, target, list of agent 0)])."""
    states = np.zeros((4, 6))
    states[1, 0] = states[2, 0] = 2.0
    states[3, 1] = 2.0
    ahead, corner = [3.0, 0.0, 0.0], [3.0, 3.0, 0.0]
    lists = [("one", ahead, [1]), ("dup4", ahead, [1, 1, 1, 1]), ("twins", ahead, [1, 2]),
             ("mixed", ahead, [3, 1, 2, 1]), ("corner", corner, [1, 3]),
             ("corner_dup", corner, [1, 3, 2, 3, 1])]
    return states, lists


def point_batch(target, lst):
    """dependent_point as a one-agent batch: (states, targets 1 x 3, row_ptr, col) for agent 0."""
    states, _ = dependent_point()
    return (states, np.array([target], dtype=np.float64), np.array([0, len(lst)], np.int32),
            np.array(lst, np.int32))


def unique_sorted(lst):
    return sorted(set(int(v) for v in lst))


def collapsed(states, lst):
    """The list with neighbours in the same state collapsed to the smallest index among them,
    sorted and unique (coincident neighbours give the same CBF rows as one of them)."""
    states = np.asarray(states)
    first = {}
    for j in range(len(states)):
        first.setdefault(tuple(states[j]), j)
    return sorted(set(first[tuple(states[int(v)])] for v in lst))


def dependent_lattice(kind):
    """An 8 x 8 lattice at spacing exactly d_min = 2.0, x and y from -8 to +6 (every neighbour
    pair on its CBF boundary): kind "shear": rows alternating vx = +-0.5; kind "centre":
    velocities -0.25 * sign(position) per axis, as tie_lattice. Targets -0.5 * position, lists
    knn_csr(S, 8, 4.0): mirror-symmetric neighbours, linearly dependent CBF rows. Returns
    (states, targets, row_ptr, col)."""
    g = np.arange(64)
    states = np.zeros((64, 6))
    states[:, 0] = -8.0 + 2.0 * (g % 8)
    states[:, 1] = -8.0 + 2.0 * (g // 8)
    if kind == "shear":
        states[:, 3] = np.where((g // 8) % 2 == 0, 0.5, -0.5)
    elif kind == "centre":
        states[:, 3] = -0.25 * np.sign(states[:, 0])
        states[:, 4] = -0.25 * np.sign(states[:, 1])
    else:
        raise ValueError(kind)
    targets = np.zeros((64, 3))
    targets[:, :2] = -0.5 * states[:, :2]
    rp, col = swarm.knn_csr(states, 8, 4.0)
    return states, targets, rp, col


_ORACLE = {}


def oracle_agents(cfg, states, targets, rp, col, agents, key=None):
    """impc_optimize of the listed agents (list of dicts); cached under `key` when given."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    p = O.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    res = [O.impc_optimize(p, states, a, col[rp[a]:rp[a + 1]], refs[a]) for a in agents]
    if key is not None:
        _ORACLE[key] = res
    return res


def oracle_point(cfg, target, lst):
    """The oracle's result for agent 0 of dependent_point with the list `lst` (cached)."""
    key = ("point", tuple(target), tuple(lst))
    if key not in _ORACLE:
        states, tg, rp, col = point_batch(target, lst)
        _ORACLE[key] = oracle_agents(cfg, states, tg, rp, col, [0])[0]
    return _ORACLE[key]

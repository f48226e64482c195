"""Inputs of the FoV IMPC off the base field of view, shared by tests/test_fov_param_inputs.py (CPU:
every input pinned on the oracle) and tests/test_gpu_fov_params.py (GPU: impc_fov_kernel<SLACK> on
the same inputs against the same oracle values).

Every other FoV IMPC parity test stays at fov_beta 120 deg, Ds 0.2, Rs 6. Here: every fov_border
branch (< pi, == pi, > pi, 2 pi), Ds / Rs that make the safety and range rows bind, the Voronoi
shift of a non-square box, the row capacity of the kernel's image (WROWS = 192) from both sides,
the neighbour caps, and the plain-mode feasibility edge of neighbours outside the cone.

The reference's cone is not the field of view above pi: FovCBF imposes both border rows, so for
fov_beta > pi a neighbour must lie within pi - fov_beta / 2 of the heading (pi / 2 at exactly pi)
to be feasible at all (effective_half_angle). Lists for these configurations are built with that
cone (visible_csr); swarm.fov_csr filters by fov_beta / 2 and is left as it is.

Everything uses at most 33 agents per launch, k_hor 20 and impc_iter 2."""
import functools
import math

import numpy as np

import oracle_lib as O
from mpccbf import swarm

SHIFT = 1e-6  # the stability check: every inequality bound moved by +-SHIFT relative (cbf_control_cases.SHIFT)
LD = np.longdouble
DBL_MAX = np.finfo(np.float64).max
WROWS = 192      # rows of the kernel's image per IMPC iteration (impc.hpp)
WSL_CROWS = 80   # slack mode: the slack image kept behind the ordinary rows (impc.hpp)
NB_CAP = {"plain": 16, "slack": 8}

NO_SLACK = {}
SLACK = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.9)  # the example's setting
SLACK_ORDER = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.1)
SETTINGS = {"plain": NO_SLACK, "slack": SLACK, "slack01": SLACK_ORDER}
KERNEL = {"plain": "impc_fov_kernel<false>", "slack": "impc_fov_kernel<true>", "slack01": "impc_fov_kernel<true>"}
DEG = math.pi / 180.0
FREE = dict(fov_beta=2.0 * math.pi, fov_Ds=1e-3, fov_Rs=1e3)  # the FoV-free solve of the liveness counts


def config(setting, **over):
    return swarm.fov_config(20, **dict(SETTINGS[setting], **over))


def is_full_circle(beta):
    return abs(beta - 2.0 * math.pi) <= 1e-9 * 2.0 * math.pi  # (fov_cbf.hpp fov_border)


def effective_half_angle(beta):
    """Half-angle of the cone in which the reference's two border rows can both hold."""
    if is_full_circle(beta):
        return math.pi
    return 0.5 * beta if beta <= math.pi else math.pi - 0.5 * beta


def bearing_offsets(states, i):
    """(|bearing - yaw| of every agent as agent i sees it, squared planar distances, self = inf)."""
    d = states[:, :2] - states[i, :2]
    d2 = np.sum(d ** 2, axis=1)
    d2[i] = np.inf
    off = np.abs(np.angle(np.exp(1j * (np.arctan2(d[:, 1], d[:, 0]) - states[i, 2]))))
    return off, d2


def visible_csr(states, k, Rs, beta):
    """swarm.fov_csr with the reference's cone: the k nearest agents within Rs whose bearing lies
    strictly inside effective_half_angle(beta). Ties by index; rows sorted by index."""
    half = effective_half_angle(beta)
    rows = []
    for i in range(len(states)):
        off, d2 = bearing_offsets(states, i)
        cand = np.nonzero((d2 <= Rs * Rs) & (off < half))[0]
        order = np.lexsort((cand, d2[cand]))[:k]
        rows.append(np.sort(cand[order]))
    rp = np.zeros(len(states) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    return rp, col


def make_case(states, targets, rp, col, agent_first=0, num_agents=None):
    n = len(targets) if num_agents is None else num_agents
    return dict(states=np.asarray(states, dtype=np.float64), targets=np.asarray(targets, dtype=np.float64),
                refs=swarm.refs_from_targets(np.asarray(targets, dtype=np.float64), 20),
                rp=np.asarray(rp, dtype=np.int32), col=np.asarray(col, dtype=np.int32), agent_first=agent_first,
                num_agents=n)


def oracle_case(cfg, case):
    """Every observer of a case on the oracle: status, obj (agents x impc_iter) and x (agents x
    impc_iter x curve variables; the slack variables are dropped)."""
    p = O.make_params(cfg)
    nc = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    st, ob, xs = [], [], []
    for i in range(case["num_agents"]):
        lst = case["col"][case["rp"][i]:case["rp"][i + 1]]
        r = O.impc_optimize(p, case["states"], case["agent_first"] + i, lst, case["refs"][i])
        st.append(r["status"])
        ob.append(r["obj"])
        xs.append(r["x"][:, :nc])
    return np.array(st), np.array(ob), np.array(xs)


def liveness(cfg, case, ob=None):
    """Agents whose iteration-1 objective differs from the FoV-free solve of the same lists
    (fov_beta 2 pi, Ds 1e-3, Rs 1e3: no border rows, safety and range rows out of reach) by more than
    1e-3 relative: the FoV rows of cfg shape their optimum."""
    if ob is None:
        ob = oracle_case(cfg, case)[1]
    st0, ob0, _ = oracle_case(dict(cfg, **FREE), case)
    assert np.all(st0 == O.OPTIMAL)
    rel = np.abs(ob[:, 1] - ob0[:, 1]) / np.maximum(1.0, np.abs(ob0[:, 1]))
    return np.nonzero(rel > 1e-3)[0].tolist()


# ---- 2. swarm cases ------------------------------------------------------------------------------
SWARM_DMIN = 1.1          # lattice spacing 2.75 m: up to 8 neighbours in view
STEERED = tuple(range(0, 33, 4))
STEER_MARGIN = 0.3 * DEG  # the steered agents' nearest neighbour: this far inside the 181-degree cone


@functools.lru_cache(maxsize=None)
def swarm_states():
    """heading_swarm(33, d_min 1.1). No random heading puts a neighbour within a degree of the
    89.5-degree cone of fov_beta = 181 deg (kap = tan 89.5 deg = 115: the border rows are vacuous a
    degree inside it), so every fourth agent is steered: it stands still with its nearest neighbour
    STEER_MARGIN inside that cone, alternately to its left and right, and its target keeps its
    distance, 20 degrees off the heading on the other side."""
    states, targets = swarm.heading_swarm(33, d_min=SWARM_DMIN)
    half = effective_half_angle(181.0 * DEG)
    for n, a in enumerate(STEERED):
        d = states[:, :2] - states[a, :2]
        d2 = np.sum(d ** 2, axis=1)
        d2[a] = np.inf
        j = int(np.argmin(d2))
        side = 1.0 if n % 2 == 0 else -1.0
        yaw = math.atan2(d[j, 1], d[j, 0]) - side * (half - STEER_MARGIN)
        r = float(np.linalg.norm(targets[a, :2] - states[a, :2]))
        ang = yaw - side * 20.0 * DEG
        targets[a] = [states[a, 0] + r * math.cos(ang), states[a, 1] + r * math.sin(ang), yaw]
        states[a, 2:] = [yaw, 0.0, 0.0, 0.0]
    states.setflags(write=False)
    targets.setflags(write=False)
    return states, targets


# name -> overrides of the base FoV configuration
SWARM_CONFIGS = {
    "b40": dict(fov_beta=40.0 * DEG), "b60": dict(fov_beta=60.0 * DEG), "b90": dict(fov_beta=90.0 * DEG),
    "b180": dict(fov_beta=math.pi), "b181": dict(fov_beta=181.0 * DEG), "b240": dict(fov_beta=240.0 * DEG),
    "b300": dict(fov_beta=300.0 * DEG), "b360": dict(fov_beta=2.0 * math.pi),
    "ds1.0rs4.5": dict(fov_Ds=1.0, fov_Rs=4.5), "ds0.5rs3.0": dict(fov_Ds=0.5, fov_Rs=3.0),
    "ds1.5rs8.0": dict(fov_Ds=1.5, fov_Rs=8.0), "bbox": dict(bbox=[0.35, 0.1, 0.0]),
}


@functools.lru_cache(maxsize=None)
def swarm_case(name):
    cfg = config("plain", **SWARM_CONFIGS[name])
    states, targets = swarm_states()
    rp, col = visible_csr(states, 8, cfg["fov_Rs"], cfg["fov_beta"])
    return make_case(states, targets, rp, col)


def cone_margin(case, beta, Rs):
    """Smallest distance of any pair of the swarm from the query's decision boundaries: (angle to
    the fov_beta / 2 border, |distance - Rs|) — test_gpu_exact_geometry's margins."""
    st = case["states"]
    ang, rad = np.inf, np.inf
    for i in range(len(st)):
        off, d2 = bearing_offsets(st, i)
        near = np.isfinite(d2)
        ang = min(ang, float(np.min(np.abs(off[near] - 0.5 * beta))))
        rad = min(rad, float(np.min(np.abs(np.sqrt(d2[near]) - Rs))))
    return ang, rad


# ---- 3. fan cases --------------------------------------------------------------------------------
FAN_BETAS = {"b60": 60.0 * DEG, "b180": math.pi, "b240": 240.0 * DEG, "b360": 2.0 * math.pi}
FAN_KS = {"plain": (1, 8, 9, 13, 16), "slack": (1, 4, 8)}
FAN_OVER_CAP = {"plain": 17, "slack": 9}
FAN_YAW, FAN_YAW_RATE = 2.9, 0.2
TURNS = ("stay", "turn")


def fan(k, beta, turn, centre, spread=0.85):
    """One observer at `centre`, yaw 2.9, yaw rate 0.2, at rest, and k static neighbours at bearings
    spread over +-spread of the effective half-angle of beta and ranges 2.2 .. 5.6 m. Its target is
    2.5 m away, 1.2 rad off the heading: to the left ("stay": with the yaw rate) or to the right
    ("turn": against it). Which of the two makes a border row bind depends on the cone — at 60 deg
    both do, at pi and 240 deg mostly one of them (PINS["fan_live"])."""
    half = effective_half_angle(beta)
    obs = np.array([centre[0], centre[1], FAN_YAW, 0.0, 0.0, FAN_YAW_RATE])
    bear = FAN_YAW + (spread * half * np.linspace(-1.0, 1.0, k) if k > 1 else np.array([0.5 * half]))
    rng_ = np.linspace(2.2, 5.6, k) if k > 1 else np.array([2.2])
    nbs = np.zeros((k, 6))
    nbs[:, 0] = centre[0] + rng_ * np.cos(bear)
    nbs[:, 1] = centre[1] + rng_ * np.sin(bear)
    ang = FAN_YAW + (1.2 if turn == "stay" else -1.2)
    tg = np.array([centre[0] + 2.5 * math.cos(ang), centre[1] + 2.5 * math.sin(ang), FAN_YAW])
    return obs, tg, nbs


def ring_fan(kind, Ds, Rs, centre, k=4):
    """The 2 pi fans: no border rows, so the binding rows are the range row ("range": neighbour 0
    straight ahead at Rs - 0.1, the target 2.5 m behind the observer) or the safety row ("safety":
    neighbour 0 straight ahead at Ds + 0.3, the target 2.5 m ahead, beyond it). k - 1 further
    neighbours stand at +-70 .. +-150 degrees, 3.2 .. 5.2 m away."""
    obs = np.array([centre[0], centre[1], FAN_YAW, 0.0, 0.0, 0.0])
    r0 = Rs - 0.1 if kind == "range" else Ds + 0.3
    bear = [0.0] + [(1.0 if j % 2 == 0 else -1.0) * math.radians(70.0 + 80.0 * j / max(1, k - 2)) for j in range(k - 1)]
    rng_ = [r0] + list(np.linspace(3.2, 5.2, k - 1))
    nbs = np.zeros((k, 6))
    nbs[:, 0] = centre[0] + np.array(rng_) * np.cos(FAN_YAW + np.array(bear))
    nbs[:, 1] = centre[1] + np.array(rng_) * np.sin(FAN_YAW + np.array(bear))
    ang = FAN_YAW + (math.pi if kind == "range" else 0.0)
    tg = np.array([centre[0] + 2.5 * math.cos(ang), centre[1] + 2.5 * math.sin(ang), FAN_YAW])
    return obs, tg, nbs


def batch(fans, lead_rows=2):
    """Fans (observer, target, neighbours) in one batch: lead_rows unrelated rows, every fan's
    neighbours, then the observers (agent_first > 0), as fov_estimate_cases.fan_case."""
    lead = np.zeros((lead_rows, 6))
    lead[:, 0] = -100.0 - 10.0 * np.arange(lead_rows)
    row, lists = lead_rows, []
    for _, _, nb in fans:
        lists.append(np.arange(row, row + len(nb), dtype=np.int32))
        row += len(nb)
    states = np.concatenate([lead] + [nb for _, _, nb in fans] + [np.array([o for o, _, _ in fans])])
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return make_case(states, np.array([t for _, t, _ in fans]), rp, np.concatenate(lists), agent_first=row,
                     num_agents=len(fans))


@functools.lru_cache(maxsize=None)
def fan_batch(name, setting, over_cap=False):
    """Every fan of FAN_KS[setting] x TURNS at FAN_BETAS[name] in one batch, 40 m apart (observer
    2 j + t: count FAN_KS[j], turn TURNS[t]); over_cap: one fan of one neighbour more than the cap
    is appended."""
    ks = FAN_KS["plain" if setting == "plain" else "slack"]
    fans = [fan(k, FAN_BETAS[name], t, (40.0 * (2 * j + n), 0.0)) for j, k in enumerate(ks) for n, t in enumerate(TURNS)]
    if over_cap:
        fans.append(fan(FAN_OVER_CAP["plain" if setting == "plain" else "slack"], FAN_BETAS[name], "stay",
                        (40.0 * len(fans), 0.0)))
    return batch(fans)


# the 2 pi fans: (kind, Ds, Rs) per configuration (one context each: Ds is the context's)
RING_CONFIGS = {"range": ("range", 0.2, 6.0), "safety0.5": ("safety", 0.5, 6.0), "safety1.0": ("safety", 1.0, 6.0),
                "safety2.0": ("safety", 2.0, 6.0)}


@functools.lru_cache(maxsize=None)
def ring_batch(name):
    kind, Ds, Rs = RING_CONFIGS[name]
    return batch([ring_fan(kind, Ds, Rs, (40.0 * j, 0.0), k) for j, k in enumerate((1, 4, 8))])


def ring_config(name, setting):
    _, Ds, Rs = RING_CONFIGS[name]
    return config(setting, fov_beta=2.0 * math.pi, fov_Ds=Ds, fov_Rs=Rs)


# ---- 4. row-cap cases ----------------------------------------------------------------------------
def shared_rows(cfg, keep_redundant=False):
    from mpccbf import _lib
    return int(_lib.host_operators(cfg, keep_redundant=keep_redundant)["m"])


def fov_rows_kept(cfg, ego, nb_xy, cbf_filter):
    """numpy restatement of the kernel's row decision for one neighbour at one ego state: per kind
    (safety, left, right, range) whether the row enters the image — present, and not implied by the
    acceleration box (b >= bmax = sum_d max(-a_d a_min_d, -a_d a_max_d)) when the filter is on."""
    a, b, present = O.fov_cbf(ego, np.array([nb_xy[0], nb_xy[1], 0.0, 0.0, 0.0, 0.0]), cfg["fov_beta"], cfg["fov_Ds"],
                              cfg["fov_Rs"])
    lo, hi = np.array(cfg["a_min"]), np.array(cfg["a_max"])
    bmax = np.sum(np.maximum(-a * lo, -a * hi), axis=1)
    return [bool(present[r]) and not (cbf_filter and b[r] >= bmax[r]) for r in range(4)]


def image_rows(cfg, case, i, x0, cbf_filter=True, keep_redundant=False):
    """Rows of observer i's image in IMPC iterations 0 and 1 (plain mode): the shared box rows, 4
    Voronoi rows per neighbour and the kept FoV rows, at the state (iteration 0) and at the
    iteration-0 curve x0 sampled at k h, k < cbf_horizon (iteration 1; x0 None: iteration 0 only)."""
    p = O.make_params(cfg)
    me = case["states"][case["agent_first"] + i]
    lst = case["col"][case["rp"][i]:case["rp"][i + 1]]
    base = shared_rows(cfg, keep_redundant) + cfg["num_control_points"] * len(lst)
    egos = [[me]]
    if x0 is not None:
        egos.append([np.concatenate([O.eval_curve(p, x0, cfg["h"] * k, 0), O.eval_curve(p, x0, cfg["h"] * k, 1)])
                     for k in range(cfg["cbf_horizon"])])
    return [base + sum(sum(fov_rows_kept(cfg, e, case["states"][j, :2], cbf_filter)) for j in lst for e in es)
            for es in egos]


def slack_image_rows(cfg, nnb, keep_redundant=False):
    """Slack mode's capacity figure: the ordinary rows (box + Voronoi) rounded up to 16, plus the
    slack image."""
    m = shared_rows(cfg, keep_redundant) + cfg["num_control_points"] * nnb
    return (m + 15) // 16 * 16 + WSL_CROWS


def cap_fan(n, beta=120.0 * DEG):
    """The "stay" fan of n neighbours on its own (one observer)."""
    return batch([fan(n, beta, "stay", (0.0, 0.0))])


# name -> (configuration overrides, context options, neighbour counts on both sides of the edge)
ROW_CAP = {
    "h2": (dict(cbf_horizon=2), dict(no_cbf_filter=True), (10, 11)),
    "h3": (dict(cbf_horizon=3), dict(no_cbf_filter=True), (7, 8)),
    "h2b360": (dict(cbf_horizon=2, fov_beta=2.0 * math.pi), dict(no_cbf_filter=True), (15, 16)),
}


# the filter on: (configuration overrides, neighbours) whose kept rows come within 8 of the capacity,
# and the rows of its two iterations (image_rows; tests/test_fov_param_inputs.py recomputes them)
FILTERED_CAP = (dict(cbf_horizon=4, fov_beta=60.0 * DEG), 16)
FILTERED_ROWS = (149, 185)


# ---- 5. feasibility edge -------------------------------------------------------------------------
SWEEP_X = (4, 8, 12, 16, 20, 25, 30)
SWEEP_LAST_OPTIMAL = 16          # plain mode: OPTIMAL up to here, INFEASIBLE from the next x on
SWEEP_FAR = 45                   # both neighbours far outside: solved at both decay rates
# slack in use at objectives >= 1e4: (x, setting) -> whether the curve is compared, i.e. whether the
# oracle's own curve moves < 1e-6 under +-SHIFT. The margin is thin: the movement is 9.4e-7 .. 9.8e-7
# at decay 0.9 and 1.16e-6 at decay 0.1 whatever x — about SHIFT itself, a hard row with a bound of
# order 1 being active — so it says more about that row than about conditioning, and a changed
# oracle may flip an entry; tests/test_fov_param_inputs.py recomputes every one.
SWEEP_CURVES = {(20, "slack"): True, (25, "slack"): True, (30, "slack"): True, (SWEEP_FAR, "slack"): True,
                (SWEEP_FAR, "slack01"): False}


def sweep_case(x):
    """fov_beta 120 deg: one neighbour x degrees outside the left border at 3 m, one x / 2 degrees
    outside the right border at 2.5 m, one inside (10 degrees left, 4 m); observer at rest, yaw 0,
    target 2 m ahead."""
    obs = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    nbs = np.zeros((3, 6))
    for j, (b, r) in enumerate(((60.0 + x, 3.0), (-60.0 - 0.5 * x, 2.5), (10.0, 4.0))):
        nbs[j, :2] = [r * math.cos(b * DEG), r * math.sin(b * DEG)]
    return batch([(obs, np.array([2.0, 0.0, 0.0]), nbs)])


# ---- 6. slack order ------------------------------------------------------------------------------
def order_case():
    """A fan of 4 at 60 deg, decay 0.1, in the sweep's geometry (observer at rest, yaw 0, target
    2 m ahead): the two nearest neighbours stand outside the cone on either side (12.5 degrees at
    2.5 m to the right, 25 degrees at 3 m to the left: slacks in use), two more inside (10 degrees
    left at 4 m, 5 degrees right at 4.5 m). Covariance tables A (every neighbour 0.02 I) and B (the
    second-nearest ellipse of A grown to 0.6 I, which brings it in front of the nearest): the two
    nearest swap their places in the slack order. Returns (case, {"A": table, "B": table},
    (nearest, second) rows of the state table)."""
    obs = np.zeros(6)
    nbs = np.zeros((4, 6))
    for j, (b, r) in enumerate(((55.0, 3.0), (-42.5, 2.5), (10.0, 4.0), (-5.0, 4.5))):
        nbs[j, :2] = [r * math.cos(b * DEG), r * math.sin(b * DEG)]
    c = batch([(obs, np.array([2.0, 0.0, 0.0]), nbs)])
    me = c["states"][c["agent_first"]]
    A = np.tile([0.02, 0.0, 0.02], (len(c["states"]), 1))
    d = [O.distance_to_ellipse(me[:2], c["states"][j, :2], A[j]) for j in c["col"]]
    p, q = (int(c["col"][j]) for j in np.argsort(d)[:2])
    B = A.copy()
    B[q] = [0.6, 0.0, 0.6]
    return c, {"A": A, "B": B}, (p, q)


def oracle_cov(cfg, case, cov):
    """oracle_case with a covariance table (None: unknown, the list order)."""
    p = O.make_params(cfg)
    r = O.impc_optimize(p, case["states"], case["agent_first"], case["col"], case["refs"][0], covs=cov)
    return r["status"], r["obj"], r["x"][:, :cfg["num_pieces"] * 3 * cfg["num_control_points"]]


# ---- C. the all-others lists of the example ------------------------------------------------------
def all_others_case():
    """heading_swarm(8) with the example's all-others lists (seven neighbours each, most of them
    outside the field of view), the setting of FovImpcLoop's finding."""
    states, targets = swarm.heading_swarm(8)
    rp, col = swarm.all_csr(8)
    return make_case(states, targets, rp, col)


def recorded_cases():
    """The all-others cases recorded in tests/golden/regress_cases.json (reference "penalty"): (record,
    case) with row 0 the ego and rows 1.. its neighbours."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regress_cases.json")
    out = []
    with open(path) as f:
        records = json.load(f)["cases"]
    for rec in records:
        if rec.get("reference") != "penalty":
            continue
        states = np.array(rec["states"])
        n = len(states)
        out.append((rec, make_case(states, np.array([rec["target"]]), [0, n - 1], np.arange(1, n), num_agents=1)))
    return out


# ---- references beyond the oracle's own solve ----------------------------------------------------
def slack_weights(cfg, nnb):
    """Unknown covariances: the list order (oracle.cpp impc)."""
    return cfg["slack_cost"] * cfg["slack_decay_rate"] ** np.arange(nnb, dtype=np.float64)


def binding_fov_rows(cfg, case, i=0, nb=0, tol=1e-7):
    """(kind, sample) of neighbour nb's FoV rows that hold with equality (scaled, tol) at the oracle's
    iteration-1 solution of observer i, plain mode. The FoV rows are the one-sided rows behind the 4
    Voronoi rows per neighbour, per neighbour all samples of one kind, then the next kind."""
    r = python_impc(cfg, case, i)
    qp, x = r["qp"][1], r["x"][1]
    nnb = int(case["rp"][i + 1] - case["rp"][i])
    h = cfg["cbf_horizon"]
    fov = np.nonzero(qp["lo"] <= -DBL_MAX)[0][cfg["num_control_points"] * nnb:]
    assert len(fov) == 4 * h * nnb
    out = []
    for kind in range(4):
        for k in range(h):
            row = fov[nb * 4 * h + kind * h + k]
            hi = qp["hi"][row]
            if hi < DBL_MAX and abs(qp["A"][row] @ x - hi) <= tol * (1.0 + abs(hi)):
                out.append((kind, k))
    return out


def slack_weights_cov(cfg, case, cov, i=0):
    """Observer i's slack weights (oracle.cpp impc): the neighbours sorted by distanceToEllipse
    (ties keep the list order; cov None: every distance equal), weight of neighbour j =
    slack_cost * decay^(sorted list)[j] — the reference's indexing."""
    lst = case["col"][case["rp"][i]:case["rp"][i + 1]]
    me = case["states"][case["agent_first"] + i]
    d = [-5.0 if cov is None else O.distance_to_ellipse(me[:2], case["states"][j, :2], cov[j]) for j in lst]
    idx = np.argsort(np.array(d), kind="stable")
    return cfg["slack_cost"] * cfg["slack_decay_rate"] ** idx.astype(np.float64)


def shifted(qp, shift):
    """qp with every inequality bound moved outwards by shift relative (inwards: shift < 0)."""
    q = dict(qp)
    ineq = qp["lo"] < qp["hi"]
    lo, hi = qp["lo"].copy(), qp["hi"].copy()
    f = ineq & (hi < DBL_MAX)
    hi[f] += shift * np.maximum(1.0, np.abs(hi[f]))
    f = ineq & (lo > -DBL_MAX)
    lo[f] -= shift * np.maximum(1.0, np.abs(lo[f]))
    q["lo"], q["hi"] = lo, hi
    return q


def python_impc(cfg, case, i=0, shift=0.0):
    """Observer i's IMPC loop on O.assemble_qp / O.solve_dense_qp (the oracle's own assembly and
    solver, without its slack polish), every inequality bound moved by shift relative. Returns status,
    obj (impc_iter), the solutions and the unshifted QPs per iteration."""
    p = O.make_params(cfg)
    me = case["states"][case["agent_first"] + i]
    lst = case["col"][case["rp"][i]:case["rp"][i + 1]]
    nbs = case["states"][lst] if len(lst) else None
    sw = slack_weights(cfg, len(lst)) if cfg["slack_mode"] else None
    status = np.full(cfg["impc_iter"], O.UNKNOWN, dtype=np.int32)
    obj = np.full(cfg["impc_iter"], np.nan)
    xs, qps, pred = [], [], None
    for it in range(cfg["impc_iter"]):
        qp = O.assemble_qp(p, me, case["refs"][i], nbs, it, pred, slack_w=sw)
        qps.append(qp)
        r = O.solve_dense_qp(shifted(qp, shift) if shift else qp)
        status[it] = r["status"]
        if r["status"] != O.OPTIMAL:
            break
        obj[it] = r["obj"]
        xs.append(r["x"].copy())
        pred = np.array([np.concatenate([O.eval_curve(p, r["x"], cfg["h"] * k, 0), O.eval_curve(p, r["x"], cfg["h"] * k, 1)])
                         for k in range(cfg["cbf_horizon"])])
    return dict(status=status, obj=obj, x=xs, qp=qps)


def penalty_objective(qp, x, nslack):
    """The slack QP's objective at the curve x with every slack at its least feasible value
    v_j = max(0, largest excess of its rows), in np.longdouble: (objective, largest scaled violation
    of the hard rows and equalities at x). The objective convention is the oracle's (x^T H x + c x +
    c0 with its H)."""
    n = qp["n"]
    nc = n - nslack
    A, lo, hi = qp["A"].astype(LD), qp["lo"].astype(LD), qp["hi"].astype(LD)
    xc = np.asarray(x, dtype=LD)[:nc]
    ax = A[:, :nc] @ xc
    v = np.zeros(nslack, dtype=LD)
    soft = np.zeros(len(lo), dtype=bool)
    for j in range(nslack):
        rows = np.nonzero(qp["A"][:, nc + j] < 0.0)[0]
        soft[rows] = True
        for r in rows:
            if qp["hi"][r] < DBL_MAX:
                v[j] = max(v[j], (ax[r] - hi[r]) / -A[r, nc + j])
    full = np.concatenate([xc, v])
    obj = full @ (qp["H"].astype(LD) @ full) + qp["c"].astype(LD) @ full + LD(qp["c0"])
    viol = LD(0.0)
    for r in np.nonzero(~soft)[0]:
        if qp["hi"][r] < DBL_MAX:
            viol = max(viol, (ax[r] - hi[r]) / (1.0 + abs(hi[r])))
        if qp["lo"][r] > -DBL_MAX:
            viol = max(viol, (lo[r] - ax[r]) / (1.0 + abs(lo[r])))
    return float(obj), float(viol)


# ---- recorded oracle results (tests/test_fov_param_inputs.py holds the oracle to them) ----------
PINS = {'all_others_status': [[3, 5], [3, 5], [3, 5], [3, 5], [3, 5], [5, 5], [5, 5], [3, 5]],
 'cap_rows': {'h2': {'10': [152, 192], '11': [160, 204]},
              'h2b360': {'15': [162, 192], '16': [168, 200]},
              'h3': {'7': [128, 184], '8': [136, 200]}},
 'fan_live': {'b180/plain': [0, 2, 3, 4, 5, 6, 7, 8, 9],
              'b180/slack': [0, 2, 4, 5],
              'b240/plain': [2, 4, 5, 6, 7, 8, 9],
              'b240/slack': [2, 4],
              'b360/plain': [],
              'b360/slack': [],
              'b60/plain': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9],
              'b60/slack': [0, 1, 2, 3, 4, 5]},
 'order_obj': {'A': [-173.99076134776953, -145.13762829508664],
               'B': [-173.99076134773603, -148.60678191684462],
               'none': [-173.99076134773603, -148.60678191684462]},
 'ring_binding': {'range': [(3, 1)], 'safety0.5': [(0, 1)], 'safety1.0': [(0, 1)], 'safety2.0': [(0, 1)]},
 'ring_live': {'range': [0, 1, 2], 'safety0.5': [], 'safety1.0': [0, 1, 2], 'safety2.0': [0, 1, 2]},
 'shared_rows': {'kept': 117, 'reduced': 72},
 'swarm_live': {'b180': [0, 1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26,
                         27, 28, 30, 31, 32],
                'b181': [0, 4, 8, 12, 16, 20, 24, 28, 32],
                'b240': [0, 2, 3, 6, 7, 8, 11, 13, 14, 15, 19, 20, 23, 24, 25, 26, 30],
                'b300': [0, 1, 2, 5, 7, 8, 9, 10, 11, 14, 15, 16, 18, 19, 20, 21, 22, 24, 25, 26, 27, 31],
                'b360': [0, 4, 6, 29],
                'b40': [0, 1, 2, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 19, 20, 21, 24, 25, 26, 27],
                'b60': [0, 1, 2, 5, 7, 8, 9, 10, 11, 14, 15, 16, 18, 19, 20, 21, 22, 24, 25, 26, 27, 31],
                'b90': [1, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20, 21, 22, 24, 25, 27, 31],
                'bbox': [0, 2, 3, 6, 7, 8, 11, 13, 14, 15, 19, 20, 23, 24, 25, 26, 30],
                'ds0.5rs3.0': [3, 6, 7, 11, 13, 19, 23, 30],
                'ds1.0rs4.5': [0, 2, 3, 6, 7, 8, 11, 13, 14, 15, 19, 20, 23, 24, 25, 26, 30],
                'ds1.5rs8.0': [0, 1, 2, 3, 6, 7, 8, 11, 13, 14, 15, 19, 20, 23, 24, 25, 26, 28, 30]},
 'swarm_max_nb': {'b180': 8,
                  'b181': 8,
                  'b240': 6,
                  'b300': 4,
                  'b360': 8,
                  'b40': 2,
                  'b60': 4,
                  'b90': 5,
                  'bbox': 6,
                  'ds0.5rs3.0': 2,
                  'ds1.0rs4.5': 3,
                  'ds1.5rs8.0': 8}}

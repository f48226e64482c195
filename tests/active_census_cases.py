"""Inputs of test_gpu_active_census.py (GPU) and test_active_census_inputs.py (CPU): collision-IMPC
QPs whose active set at the optimum has a known size, 0 .. 6 sides, on both sides of the caps of the
two collision layouts (16 lanes per agent: DK = 5 sides in the dual active set's factor,
pdip_sep.hpp; one agent per wave: WK = 4, impc_wide.hpp). Numpy, the oracle and the host operators
only; nothing here touches a GPU.

A case is one ego robot at rest or moving slowly, a far target (the tracking cost pushes the curve
onto its velocity / acceleration bounds: the box sides) and 0 .. 2 static robots about 2.05 m away
(the pair's CBF row: a CBF side). census() names the active sides of the condensed QP as
mpccbf.decode_active_sides names them, so an exported record compares with it directly:
("box", channel, row, upper) and ("cbf", neighbour's state index, sample).

Admissibility (margins(), stable()): every side that is not active has scaled slack >= MIN_SLACK,
the active sides' multipliers are all positive and >= MIN_MULT of the largest (strict
complementarity), and no oracle status changes when every inequality bound moves by +-SHIFT
relative. The size of the active set is then a fact of the QP, not of a tolerance.

The literals below were found by tools/active_census_search.py (seeded; it prints them) and are
checked, case by case, by test_active_census_inputs.py. Found: box_0 .. box_6, cbf1_1 .. cbf1_6
(cbf1_3 grows to 4 sides in iteration 1), the 8 sign patterns of box_6 and of cbf1_6, and under
param_space_cases.ASYM box_4 .. box_6 and cbf1_4 .. cbf1_6. Of the optional cases the search found
cbf2_k for k = 2, 4, 6 (two CBF sides, two neighbours; k = 3 and 5 did not turn up in 300
candidates) and iter1_grows (5 sides in iteration 0, 6 in iteration 1: iteration 0's set, handed to
iteration 1 as its warm start, no longer fits the 16-lane factor once the sixth side joins).
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import oracle_lib as O
from fov_param_cases import shifted
from mpccbf import swarm
from param_space_cases import ASYM

ACTIVE_TOL = 1e-9  # scaled residual |g y - b| / (1 + |b|) of an active side
MIN_SLACK = 1e-4   # scaled slack of every other side
MIN_MULT = 1e-6    # smallest multiplier over the largest
SHIFT = 1e-6       # the stability check (conn_impc_cases.SHIFT, cbf_control_cases.SHIFT)
SPACING = 40.0     # metres between the cases of a batch: they share nothing
ROWS = 64          # rows of a batch's state table (one launch)

CONFIGS = {"base": swarm.config(15), "asym": swarm.config(15, **ASYM)}


@functools.lru_cache(maxsize=None)
def _operators(name):
    """Host operators of CONFIGS[name], the rows of G per channel in order (the box-key rule of
    active_store.hpp) and the acceleration maps of the samples k < cbf_horizon: acc(h k) =
    UZ[k] y + US[k] s."""
    import mpccbf
    cfg = CONFIGS[name]
    ops = mpccbf._lib.host_operators(cfg)
    G = ops["G"]
    chan_rows = [[i for i in range(ops["m"]) if np.any(G[i, 2 * d:2 * d + 2] != 0.0)] for d in range(3)]
    assert sorted(sum(chan_rows, [])) == list(range(ops["m"]))
    p = O.make_params(cfg)
    UZ, US = [], []
    for k in range(cfg["cbf_horizon"]):
        UZ.append(np.stack([O.eval_curve(p, ops["Z"][:, c], cfg["h"] * k, 2) for c in range(ops["nz"])], axis=1))
        US.append(np.stack([O.eval_curve(p, ops["Xs"][:, c], cfg["h"] * k, 2) for c in range(6)], axis=1))
    return ops, chan_rows, UZ, US


def _config_name(cfg):
    for name, c in CONFIGS.items():
        if c == cfg:
            return name
    raise ValueError("census knows CONFIGS only")


def reduced(cfg, state, x):
    """The condensed variables y of the curve x = Z y + Xs s."""
    ops = _operators(_config_name(cfg))[0]
    n = ops["n"]
    return np.linalg.lstsq(ops["Z"], np.asarray(x)[:n] - ops["Xs"] @ state, rcond=None)[0]


def sides(cfg, states, agent, neighbours, it, x_prev=None):
    """Every side of IMPC iteration `it`'s condensed QP as (key, g, b): g y <= b. Box sides of the
    kept rows, both sides each; CBF sides per listed neighbour and sample — sample 0 at the state in
    iteration 0, the samples k < cbf_horizon at the previous iteration's curve x_prev in later ones."""
    ops, chan_rows, UZ, US = _operators(_config_name(cfg))
    p = O.make_params(cfg)
    s = np.asarray(states[agent], dtype=np.float64)
    out = []
    for d in range(3):
        for r, i in enumerate(chan_rows[d]):
            shift = ops["Gs"][i] @ s
            out.append((("box", d, r, 0), -ops["G"][i], -(ops["lo"][i] - shift)))
            out.append((("box", d, r, 1), ops["G"][i], ops["hi"][i] - shift))
    n = ops["n"]
    egos = [s] if it == 0 else [np.concatenate([O.eval_curve(p, x_prev[:n], cfg["h"] * k, 0),
                                                O.eval_curve(p, x_prev[:n], cfg["h"] * k, 1)])
                                for k in range(cfg["cbf_horizon"])]
    for j in neighbours:
        for k, ego in enumerate(egos):
            a, b = O.safety_cbf(ego, states[int(j)], cfg["d_min"])
            out.append((("cbf", int(j), k), -(a @ UZ[k]), b + a @ (US[k] @ s)))
    return out


def census(cfg, states, agent, oracle_result, neighbours=()):
    """Per IMPC iteration, the set of active sides of the condensed QP at the oracle's optimum
    (None for an iteration that is not OPTIMAL): scaled residual |g y - b| / (1 + |b|) <=
    ACTIVE_TOL. Keys as mpccbf.decode_active_sides."""
    return [None if m is None else m["active"] for m in margins(cfg, states, None, agent, oracle_result, neighbours)]


def margins(cfg, states, targets, agent, oracle_result, neighbours=()):
    """Per IMPC iteration (None: not OPTIMAL) a dict: active (the census), slack (the smallest scaled
    slack of a side that is not active; negative: violated), and, when targets is given, mult (the
    smallest least-squares multiplier of stationarity P y + q + G_A^T lam = 0 over the largest; 1.0
    for an empty set) and stat (that system's residual over 1 + |q|)."""
    ops = _operators(_config_name(cfg))[0]
    r = oracle_result
    out, x_prev = [], None
    for it in range(cfg["impc_iter"]):
        if r["status"][it] != O.OPTIMAL:
            out.append(None)
            continue
        x = np.asarray(r["x"][it])
        y = reduced(cfg, states[agent], x)
        active, slack, rows = set(), np.inf, []
        for key, g, b in sides(cfg, states, agent, neighbours, it, x_prev):
            res = (b - g @ y) / (1.0 + abs(b))
            if abs(res) <= ACTIVE_TOL:
                active.add(key)
                rows.append(g)
            else:
                slack = min(slack, res)
        m = dict(active=frozenset(active), slack=float(slack))
        if targets is not None:
            q = ops["Qs"] @ states[agent] + ops["Qt"] @ targets[agent]
            grad = ops["Pr"] @ y + q
            if rows:
                N = np.array(rows)
                lam = np.linalg.lstsq(N.T, -grad, rcond=None)[0]
                m["mult"] = float(lam.min() / lam.max()) if lam.max() > 0.0 else -1.0
                m["stat"] = float(np.abs(N.T @ lam + grad).max() / (1.0 + np.abs(q).max()))
            else:
                m["mult"], m["stat"] = 1.0, float(np.abs(grad).max() / (1.0 + np.abs(q).max()))
        out.append(m)
        x_prev = x
    return out


def admissible(m):
    """The first two admissibility conditions on one iteration's margins."""
    return m is not None and m["slack"] >= MIN_SLACK and m["mult"] >= MIN_MULT


def python_impc(cfg, states, targets, agent, neighbours, shift=0.0):
    """The agent's IMPC loop on O.assemble_qp / O.solve_dense_qp (the oracle's own assembly and
    solver), every inequality bound moved by shift relative: the statuses per iteration."""
    p = O.make_params(cfg)
    nbs = states[list(neighbours)] if len(neighbours) else None
    ref = np.tile(targets[agent], cfg["k_hor"])
    status = np.full(cfg["impc_iter"], O.UNKNOWN, dtype=np.int32)
    pred = None
    for it in range(cfg["impc_iter"]):
        qp = O.assemble_qp(p, states[agent], ref, nbs, it, pred)
        r = O.solve_dense_qp(shifted(qp, shift) if shift else qp)
        status[it] = r["status"]
        if r["status"] != O.OPTIMAL:
            break
        pred = np.array([np.concatenate([O.eval_curve(p, r["x"], cfg["h"] * k, 0), O.eval_curve(p, r["x"], cfg["h"] * k, 1)])
                         for k in range(cfg["cbf_horizon"])])
    return status


def stable(cfg, states, targets, agent, neighbours, status):
    """The third condition: the statuses are `status` with every bound moved by +SHIFT and by -SHIFT."""
    return all(list(python_impc(cfg, states, targets, agent, neighbours, sh)) == list(status) for sh in (SHIFT, -SHIFT))


# ---- the named cases ------------------------------------------------------------------------------
# name -> (configuration, target offset (x, y, yaw), ego velocity (x, y, yaw rate), static robots'
# offsets (x, y), number of active sides (iteration 0, iteration 1), CBF sides among them (same)).
# Found by tools/active_census_search.py; every claim is checked by test_active_census_inputs.py.
FOUND = {
    "asym_box_4": ("asym", (3.0, -3.01, -3.95), (0.0, 0.0, 0.0), (), (4, 4), (0, 0)),  # slack 2.14e-04, multipliers 8.41e-02
    "asym_box_5": ("asym", (13.77, -2.63, -9.94), (0.3, 0.0, 0.0), (), (5, 5), (0, 0)),  # slack 1.79e-04, multipliers 7.37e-03
    "asym_box_6": ("asym", (-37.8, 5.88, 21.56), (0.0, 0.0, 0.0), (), (6, 6), (0, 0)),  # slack 1.04e-04, multipliers 3.99e-02
    "asym_cbf1_4": ("asym", (-3.34, 4.98, 1.44), (-0.13, 0.18, 0.0), ((-1.52, 1.5),), (4, 4), (1, 1)),  # slack 3.23e-04, multipliers 6.08e-02
    "asym_cbf1_5": ("asym", (16.99, 26.69, 28.99), (0.15, 0.31, 0.0), ((0.93, 1.99),), (5, 5), (1, 1)),  # slack 8.35e-04, multipliers 3.08e-01
    "asym_cbf1_6": ("asym", (55.06, -19.44, 29.13), (0.21, -0.05, 0.0), ((1.95, -0.93),), (6, 6), (1, 1)),  # slack 5.37e-04, multipliers 8.87e-02
    "box_0": ("base", (0.53, 0.7, -0.87), (0.37, 0.47, 0.0), (), (0, 0), (0, 0)),  # slack 3.54e-03, multipliers 1.00e+00
    "box_1": ("base", (2.03, -0.94, 2.08), (0.0, 0.0, 0.0), (), (1, 1), (0, 0)),  # slack 4.69e-04, multipliers 1.00e+00
    "box_2": ("base", (2.44, -2.19, 0.3), (0.26, -0.14, 0.0), (), (2, 2), (0, 0)),  # slack 3.21e-04, multipliers 3.94e-01
    "box_3": ("base", (-2.0, 4.02, -2.54), (0.0, 0.0, 0.0), (), (3, 3), (0, 0)),  # slack 2.56e-04, multipliers 1.17e-03
    "box_4": ("base", (3.92, 1.67, 4.04), (0.0, 0.0, 0.0), (), (4, 4), (0, 0)),  # slack 2.56e-04, multipliers 2.30e-01
    "box_5": ("base", (33.87, 46.94, -3.51), (0.0, 0.0, 0.0), (), (5, 5), (0, 0)),  # slack 2.29e-04, multipliers 9.36e-03
    "box_6": ("base", (39.87, 31.98, 3.94), (0.0, 0.0, 0.0), (), (6, 6), (0, 0)),  # slack 2.29e-04, multipliers 3.13e-03
    "cbf1_1": ("base", (-1.42, 1.02, 0.66), (-0.13, 0.12, 0.0), ((-1.45, 1.61),), (1, 1), (1, 1)),  # slack 2.90e-03, multipliers 1.00e+00
    "cbf1_2": ("base", (-1.26, 8.24, -1.04), (-0.01, 0.1, 0.0), ((-0.23, 2.14),), (2, 2), (1, 1)),  # slack 8.27e-04, multipliers 5.59e-01
    "cbf1_3": ("base", (-14.93, -29.56, -0.02), (-0.08, -0.21, 0.0), ((-1.19, -1.83),), (3, 4), (1, 1)),  # slack 6.03e-04, multipliers 9.76e-02
    "cbf1_4": ("base", (-2.66, -3.32, -3.91), (-0.3, -0.17, 0.0), ((-1.88, -1.14),), (4, 3), (1, 1)),  # slack 8.69e-04, multipliers 1.05e-01
    "cbf1_5": ("base", (27.41, -14.66, 9.44), (0.26, -0.06, 0.0), ((1.91, -1.03),), (5, 5), (1, 1)),  # slack 6.89e-04, multipliers 3.30e-01
    "cbf1_6": ("base", (28.9, 34.08, -7.77), (0.14, 0.22, 0.0), ((1.61, 1.47),), (6, 6), (1, 1)),  # slack 3.42e-04, multipliers 6.84e-02
    "cbf2_2": ("base", (0.88, -0.08, 0.77), (0.58, -0.07, 0.0), ((1.43, 1.65), (1.76, -1.33)), (2, 2), (2, 2)),  # slack 5.15e-04, multipliers 4.41e-01
    "cbf2_4": ("base", (-5.34, -0.67, 2.8), (-0.13, 0.02, 0.0), ((-1.49, -1.55), (-1.17, 1.82)), (4, 3), (2, 2)),  # slack 6.04e-04, multipliers 9.75e-02
    "cbf2_6": ("base", (-43.68, 37.47, 12.16), (-0.47, 0.18, 0.0), ((-2.08, -0.73), (-1.3, 1.76)), (6, 6), (2, 2)),  # slack 4.81e-04, multipliers 1.18e-02
    "iter1_grows": ("base", (-13.87, 21.71, -6.17), (-0.18, 0.31, 0.0), ((-1.15, 1.88),), (5, 6), (1, 1)),  # slack 4.05e-04, multipliers 1.03e-01
}
# optional cases the search found (cbf2_k: two CBF sides, two neighbours; iter1_grows: iteration 1's
# set larger than iteration 0's across a cap)
FOUND_OPTIONAL = [n for n in FOUND if n.startswith(("cbf2_", "iter1_grows"))]

SIGNS = list(itertools.product((1.0, -1.0), repeat=3))  # (x, y, yaw) mirrors


def mirrored(spec, sign):
    """The case mirrored through x, y and yaw where sign is -1 (base configuration: its limits are
    symmetric, so the census mirrors lower <-> upper on those channels)."""
    cfg, tg, vel, nbs, k, ncbf = spec
    s = np.asarray(sign)
    return (cfg, tuple(s * tg), tuple(s * vel), tuple((s[0] * x, s[1] * y) for x, y in nbs), k, ncbf)


def sign_name(base, sign):
    return base + "_" + "".join("p" if v > 0 else "m" for v in sign)


def named_cases():
    """name -> spec: FOUND plus the sign patterns of box_6 and cbf1_6 (the all-plus pattern is the
    case itself under its own name)."""
    cases = dict(FOUND)
    for base in ("box_6", "cbf1_6"):
        if base in FOUND:
            for sign in SIGNS[1:]:
                cases[sign_name(base, sign)] = mirrored(FOUND[base], sign)
    return cases


def sign_cases(base):
    """The names of the 8 sign patterns of a case."""
    return [base] + [sign_name(base, s) for s in SIGNS[1:]]


def case_rows(spec, origin=(0.0, 0.0)):
    """One case's robots: (states (1 + robots) x 6, targets, lists) — row 0 the ego, listing every
    robot of the case; the static robots keep their place (target = position) and list the case's
    other robots too. lists[i]: local row indices."""
    _, tg, vel, nbs, _, _ = spec
    n = 1 + len(nbs)
    states, targets = np.zeros((n, 6)), np.zeros((n, 3))
    states[:, :2] = origin
    states[0, 3:] = vel
    for i, off in enumerate(nbs):
        states[1 + i, :2] += off
    targets[:, :] = states[:, :3]
    targets[0] += tg
    lists = [[j for j in range(n) if j != i] for i in range(n)]
    return states, targets, lists


# an 8 x 8 grid of sites SPACING apart around the origin, nearest first: the condensed box bounds
# hi - Gs s grow with the distance from the origin, and with them the scale 1 + |b| of a side's slack
SITES = [(SPACING * i, SPACING * j) for _, i, j in sorted((i * i + j * j, i, j) for i in range(-4, 4) for j in range(-4, 4))]


def is_hard(spec):
    """A cap-crossing case: 4 or more active sides in one of its iterations."""
    return max(spec[4]) >= 4


@functools.lru_cache(maxsize=None)
def layout(config):
    """The unpermuted batch of one configuration: (names, states ROWS x 6, targets, lists, ego:
    name -> row). Rows: the egos — the cap-crossing cases of FOUND first (rows 0, 1, ...: at most
    three of them per residue of the row index mod 4, which permutations() needs), then the other
    cases by name — then the cases' static robots, then robots at rest on their targets with no
    neighbour (k = 0) up to ROWS rows. Case c stands on SITES[c], the fillers on the sites after the
    last case."""
    cases = {n: s for n, s in named_cases().items() if s[0] == config}
    names = sorted(cases, key=lambda n: (not (n in FOUND and is_hard(cases[n])), n))
    ego = {n: i for i, n in enumerate(names)}
    states, targets, lists = [None] * len(names), [None] * len(names), [None] * len(names)
    for site, name in enumerate(names):
        st, tg, ls = case_rows(cases[name], SITES[site])
        local = [ego[name]] + list(range(len(states), len(states) + len(st) - 1))  # local row -> batch row
        states[ego[name]], targets[ego[name]], lists[ego[name]] = st[0], tg[0], [local[j] for j in ls[0]]
        for i in range(1, len(st)):
            states.append(st[i])
            targets.append(tg[i])
            lists.append([local[j] for j in ls[i]])
    assert len(states) <= ROWS - 4, len(states)  # (the last four rows are fillers: permutations())
    site = len(names)
    while len(states) < ROWS:
        s = np.zeros(6)
        s[:2] = SITES[site]
        states.append(s)
        targets.append(s[:3].copy())
        lists.append([])
        site += 1
    return names, np.array(states), np.array(targets), lists, ego


def batch(order, config="base"):
    """The batch with its rows permuted: new row i is row order[i] of layout(config). Returns a dict:
    cfg, states, targets, rp, col (explicit CSR lists, each in its case's own order under every
    permutation: the order of the CBF rows is the order of a solver's sums), ego (name -> row), row_of
    (old row -> new row)."""
    names, st, tg, lists, ego = layout(config)
    order = np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(ROWS))
    row_of = np.empty(ROWS, dtype=np.int64)
    row_of[order] = np.arange(ROWS)
    new_lists = [[int(row_of[j]) for j in lists[o]] for o in order]
    rp = np.zeros(ROWS + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(ls) for ls in new_lists])
    col = np.array(sum(new_lists, []), dtype=np.int32)
    return dict(cfg=CONFIGS[config], states=st[order].copy(), targets=tg[order].copy(), rp=rp, col=col,
                ego={n: int(row_of[r]) for n, r in ego.items()}, row_of=row_of, names=names)


IDENTITY = tuple(range(ROWS))


@functools.lru_cache(maxsize=None)
def reference(config="base"):
    """The oracle's result of every row of batch(IDENTITY, config) (computed once, never modified)."""
    b = batch(IDENTITY, config)
    p = O.make_params(b["cfg"])
    refs = swarm.refs_from_targets(b["targets"], b["cfg"]["k_hor"])
    return [O.impc_optimize(p, b["states"], a, b["col"][b["rp"][a]:b["rp"][a + 1]], refs[a]) for a in range(ROWS)]


@functools.lru_cache(maxsize=None)
def batch_census(config="base"):
    """Per row of batch(IDENTITY, config): the margins (census included) of both iterations."""
    b, ref = batch(IDENTITY, config), reference(config)
    return [margins(b["cfg"], b["states"], b["targets"], a, ref[a], b["col"][b["rp"][a]:b["rp"][a + 1]])
            for a in range(ROWS)]


SOLVED = ROWS - 1  # agents per launch: rows 0 .. 62, so the last wave of every layout is partly filled


def permutations(config="base"):
    """Four permutations of the batch's rows (new row i = old row order[i]) for launches of SOLVED
    agents. In permutation p old row r sits in 16-lane group (r + p) % 4 of its wave, so every row
    passes through all four groups; and each cap-crossing case of FOUND sits once in the last wave
    (new rows 60 .. 62 of the 16-lane layout's four agents per wave; row 63, never solved, always
    holds a filler). The first permutation's solve is the one the others are compared with."""
    names, _, _, _, ego = layout(config)
    todo = [ego[n] for n in names if n in FOUND and is_hard(FOUND[n])]
    out = []
    for p in range(4):
        order = np.empty(ROWS, dtype=np.int64)
        for g in range(4):
            rows = [r for r in range(ROWS) if (r + p) % 4 == g]
            # (group g's rows start 5 g waves later: a wave holds rows from all over the table, so
            # the cases, which come first, share their waves with static robots and fillers)
            rows = rows[-5 * g:] + rows[:-5 * g] if g else rows
            pick = next((r for r in todo if r in rows), None) if g < 3 else max(rows)  # (max: a filler)
            if pick is not None:
                if g < 3:
                    todo.remove(pick)
                rows.remove(pick)
                rows.append(pick)
            order[g::4] = rows
        out.append(tuple(int(v) for v in order))
    assert not todo, todo
    return out

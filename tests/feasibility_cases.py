"""Inputs of test_gpu_feasibility.py (GPU) and test_feasibility_inputs.py (CPU): collision-IMPC QPs
whose distance from feasibility is chosen. t* is the optimum of the LP "min t" over the rows of
oracle_lib.assemble_qp: equalities kept, every finite inequality side (and variable bound) relaxed
by t, t free — so a feasible QP has a negative t* whose magnitude is the width of its interior, and
an infeasible one the minimal uniform row violation that the kernels' phase 1 and the oracle's
compare with feas_tol = 1e-6. Numpy, scipy (HiGHS), the oracle and mpccbf.swarm only; nothing here
touches a GPU or the product library.

A case is one ego robot at the origin of its site with target offset TARGET and 0 .. 3 robots about
2.1 m away that move towards it; one scalar of the geometry (a velocity excess, the ego's speed,
the robots' approach speed) was bisected until t* of IMPC iteration 0 stood on one of LEVELS. The
open band (-3e-6, 3e-6) holds no case: the oracle itself answers UNKNOWN on (0, 1e-6], the single-row
test of the kernels compares bmin - b, not t*, with feas_tol, and DESIGN.md leaves the band
undefined.

Admissibility is an LP proof (certificate()), not the census's +-SHIFT stability rule, which cannot
hold for cases that stand near the boundary on purpose: in np.longdouble the LP's point satisfies
every relaxed row and equality, and multipliers lambda >= 0 of sum 1 on the relaxed sides (plus the
equality multipliers) combine the rows to zero and give a dual value equal to the primal one — for a
positive level the Farkas certificate of infeasibility, for a negative one the primal point is
strictly interior.

The literals below were found by tools/feasibility_search.py (seeded; it prints them with repr
precision) and are checked, case by case, by test_feasibility_inputs.py.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.optimize import linprog

import oracle_lib as O
from active_census_cases import SPACING
from mpccbf import swarm
from param_space_cases import ASYM

FEAS_TOL = 1e-6  # launch_plan.hip feas_tol; the oracle's phase1(q) > 1e-6
LEVELS = (-1e-3, -1e-5, -3e-6, +3e-6, +8e-6, +1.2e-5, +1e-3, +1e-1)
TIGHT = (-3e-6, +3e-6, +8e-6, +1.2e-5)  # the levels of the asym and the optional families
LAST_WAVE = (+3e-6, +8e-6, +1.2e-5)     # pair egos at these sit once in the last wave
LEVEL_REL = 1e-3   # |t* - level| <= LEVEL_REL |level|: the levels stand >= 20 % from both thresholds
PRIMAL_TOL = 1e-12  # row violation of the LP's point over 1 + |bound|, in np.longdouble
GAP_REL = 1e-6     # |primal - dual| <= GAP_REL |t*|
ITER1_MIN = 1e-4   # |t1*| of a negative-level case's iteration 1
PAIR_ROW_MIN = 1.0  # b - bmin of each row of a pair / triple case alone
CBF_WEIGHT_MIN = 0.01  # the certificate's weight on the CBF rows of a case with robots (not a velocity case)
TARGET = (5.0, 0.0, 0.0)
ROWS = 128
SOLVED = ROWS - 1  # agents per launch: the last wave of every layout is partly filled

CONFIGS = {"base": swarm.config(15), "asym": swarm.config(15, **ASYM), "slack": swarm.config(15, slack_mode=1)}
TABLE_OF = {"base": "base", "asym": "asym", "slack": "base"}  # the slack configuration solves base's table
VEL_FAMILIES = {"vel_x_hi": (0, 1), "vel_y_lo": (1, 0), "vel_yaw_hi": (2, 1)}  # family -> (channel, upper)


# ---- t* -------------------------------------------------------------------------------------------

def relaxed_lp(qp):
    """The LP of t* in the form min t, G x - t <= h, E x = d: (G, h, E, d, cbf). Every finite side of
    an inequality row and every finite variable bound is one row of G; cbf marks the sides of the
    one-sided rows (the CBF rows: every box row has both sides)."""
    A, lo, hi = qp["A"], qp["lo"], qp["hi"]
    big = 1e300
    eq = lo == hi
    G, h, cbf = [], [], []
    for r in np.nonzero(~eq)[0]:
        one_sided = not (lo[r] > -big and hi[r] < big)
        if lo[r] > -big:
            G.append(-A[r]), h.append(-lo[r]), cbf.append(one_sided)
        if hi[r] < big:
            G.append(A[r]), h.append(hi[r]), cbf.append(one_sided)
    for i in range(qp["n"]):
        e = np.zeros(qp["n"])
        e[i] = 1.0
        if qp["vlo"][i] > -big:
            G.append(-e), h.append(-qp["vlo"][i])
        if qp["vhi"][i] < big:
            G.append(e), h.append(qp["vhi"][i])
    cbf += [False] * (len(G) - len(cbf))
    return np.array(G), np.array(h), A[eq].copy(), lo[eq].copy(), np.array(cbf)


def _highs(G, h, E, d):
    n = G.shape[1]
    c = np.zeros(n + 1)
    c[n] = 1.0
    res = linprog(c, A_ub=np.hstack([G, -np.ones((len(G), 1))]), b_ub=h,
                  A_eq=np.hstack([E, np.zeros((len(E), 1))]), b_eq=d, bounds=(None, None), method="highs-ds",
                  options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10, presolve=False))
    assert res.status == 0, res.message
    return res


ZOOM = 1e6  # the second solve's scale: HiGHS's absolute tolerances (1e-10) become 1e-16 of the QP's units


def tstar(qp):
    """t* of a QP by HiGHS: dict t, x, lam (multipliers of the relaxed sides, >= 0), nu (of the
    equalities) and the LP (G, h, E, d, cbf). Two solves — the LP, then the LP in the variables
    ZOOM (x - x0, t - t0) about the first solve's point, whose right-hand sides are computed in
    np.longdouble — and one refinement each of the point and of the multipliers; certificate() proves
    the result, whatever produced it."""
    L = np.longdouble
    G, h, E, d, cbf = relaxed_lp(qp)
    n = G.shape[1]
    r0 = _highs(G, h, E, d)
    x0, t0 = np.asarray(r0.x[:n], dtype=L), L(r0.x[n])
    res = _highs(G, (L(ZOOM) * (np.asarray(h, dtype=L) + t0 - np.asarray(G, dtype=L) @ x0)).astype(np.float64),
                 E, (L(ZOOM) * (np.asarray(d, dtype=L) - np.asarray(E, dtype=L) @ x0)).astype(np.float64))
    x, t = x0 + np.asarray(res.x[:n], dtype=L) / L(ZOOM), t0 + L(res.x[n]) / L(ZOOM)
    lam0 = np.maximum(-res.ineqlin.marginals, 0.0)
    near = (np.asarray(h, dtype=L) + t - np.asarray(G, dtype=L) @ x).astype(np.float64) / (1 + np.abs(h)) <= 1e-9
    lam, nu = _refined_dual(G, E, lam0, -res.eqlin.marginals, np.nonzero((lam0 > 0.0) | near)[0])
    x, t = _refined(G, h, E, d, x, t, np.nonzero(lam > 0)[0])
    return dict(t=t, x=x, lam=lam, nu=nu, G=G, h=h, E=E, d=d, cbf=cbf)


def _refined(G, h, E, d, x, t, act, rounds=3):
    """Iterative refinement of the simplex vertex (x, t), whose rows HiGHS satisfies to ~1e-12: the
    sides `act` (those with a positive multiplier: active by complementary slackness) and the
    equalities as one linear system, residuals in np.longdouble, minimum-norm corrections in double.
    certificate() judges the result."""
    L = np.longdouble
    Gl, hl, El, dl = (np.asarray(a, dtype=L) for a in (G, h, E, d))
    M = np.vstack([np.hstack([G[act], -np.ones((len(act), 1))]), np.hstack([E, np.zeros((len(E), 1))])])
    xl, tl = np.asarray(x, dtype=L), L(t)  # (x stays np.longdouble: at a site 200 m out, rounding it to
    for _ in range(rounds):                # double alone moves a CBF row by 1e-12)
        r = np.concatenate([hl[act] + tl - Gl[act] @ xl, dl - El @ xl]).astype(np.float64)
        delta = np.linalg.lstsq(M, r, rcond=None)[0]
        xl, tl = xl + delta[:-1], tl + delta[-1]
    return xl, float(tl)


def _refined_dual(G, E, lam, nu, sup, rounds=3):
    """The same for the multipliers: on the sides `sup`, the system G^T lam + E^T nu = 0, sum lam = 1;
    a side whose multiplier comes out negative leaves `sup` and the system is solved again. Returns
    np.longdouble arrays (lam is zero off the support)."""
    L = np.longdouble
    sup = list(sup)
    while True:
        M = np.vstack([np.hstack([G[sup].T, E.T]), np.concatenate([np.ones(len(sup)), np.zeros(len(E))])[None, :]])
        Ml = np.asarray(M, dtype=L)
        z = np.asarray(np.concatenate([lam[sup], nu]), dtype=L)
        rhs = np.zeros(M.shape[0], dtype=L)
        rhs[-1] = 1
        for _ in range(rounds):
            z = z + np.linalg.lstsq(M, (rhs - Ml @ z).astype(np.float64), rcond=None)[0]
        worst = int(np.argmin(z[:len(sup)]))
        if z[worst] >= 0 or len(sup) == 1:
            break
        del sup[worst]
    out = np.zeros(len(lam), dtype=L)
    out[sup] = z[:len(sup)]
    return out, z[len(sup):]


def certificate(lp):
    """The proof of lp["t"] in np.longdouble: dict primal (worst violation of a relaxed row or an
    equality by the LP's point over 1 + |bound|), lam_min, lam_sum, row (inf-norm of the combined row
    G^T lam + E^T nu), dual (the dual value -lam h - nu d), gap (|t - dual|) and cbf (the multipliers'
    weight on the CBF rows: 0 for a QP that its box rows decide alone). With lam >= 0 of sum
    1 and a zero combined row, every x has a relaxed side violated by >= dual: t* >= dual; the
    primal point shows t* <= t."""
    L = np.longdouble
    G, h, E, d = (np.asarray(lp[k], dtype=L) for k in ("G", "h", "E", "d"))
    x, lam, nu, t = np.asarray(lp["x"], dtype=L), np.asarray(lp["lam"], dtype=L), np.asarray(lp["nu"], dtype=L), L(lp["t"])
    viol = np.max((G @ x - t - h) / (1 + np.abs(h)))
    veq = np.max(np.abs(E @ x - d) / (1 + np.abs(d))) if len(d) else L(0)
    dual = -(lam @ h) - (nu @ d)
    row = np.max(np.abs(G.T @ lam + E.T @ nu))
    return dict(primal=float(max(viol, veq)), lam_min=float(lam.min()), lam_sum=float(lam.sum()), row=float(row),
                dual=float(dual), gap=float(abs(t - dual)), cbf=float(lam[lp["cbf"]].sum()))


def samples(cfg, x):
    """The curve x at the cbf_horizon samples: iteration 1's `pred` of O.assemble_qp."""
    p = O.make_params(cfg)
    return np.array([np.concatenate([O.eval_curve(p, x, cfg["h"] * k, 0), O.eval_curve(p, x, cfg["h"] * k, 1)])
                     for k in range(cfg["cbf_horizon"])])


def case_qp(cfg, states, targets, agent, neighbours, it=0, pred=None):
    """O.assemble_qp of `agent` against the listed rows of the table (iteration `it`, curve samples
    `pred`), without slack variables whatever cfg says: t* is a fact of the plain rows."""
    plain = dict(cfg, slack_mode=0)
    nbs = states[list(neighbours)] if len(neighbours) else None
    return O.assemble_qp(O.make_params(plain), states[agent], np.tile(targets[agent], cfg["k_hor"]), nbs, it, pred)


def row_margins(cfg, ego, nbs):
    """b - bmin of each neighbour's CBF row at the state alone: the row -a u <= b against the
    acceleration box (the single-row test of the row stagers, impc_common.hpp)."""
    out = []
    lo, hi = np.asarray(cfg["a_min"]), np.asarray(cfg["a_max"])
    for nb in nbs:
        a, b = O.safety_cbf(ego, nb, cfg["d_min"])
        out.append(b - float(np.sum(np.minimum(-a * lo, -a * hi))))
    return out


# ---- the families ---------------------------------------------------------------------------------
# spec: (table, family, level, ego velocity (x, y, yaw rate), robots ((x, y, vx, vy), ...), it):
# it = 0: iteration 0's t* stands on the level; it = 1 (the iter1_* cases): iteration 1's does.

def vel_spec(table, family, level, s):
    """The ego with one velocity component s beyond its limit (outward positive), no robot."""
    ch, up = VEL_FAMILIES[family]
    cfg = CONFIGS[table]
    v = [0.0, 0.0, 0.0]
    v[ch] = cfg["v_max"][ch] + s if up else cfg["v_min"][ch] - s
    return (table, family, level, tuple(v), (), 0)


def single_spec(table, level, s, gap=2.1, bearing=0.0, side=0.0, family="single", it=0):
    """One robot at rest `gap` away at `bearing`; the ego moves towards it at speed s and across at
    speed `side`."""
    c, sn = np.cos(bearing), np.sin(bearing)
    return (table, family, level, (float(s * c - side * sn), float(s * sn + side * c), 0.0),
            ((float(gap * c), float(gap * sn), 0.0, 0.0),), it)


def ring_spec(table, family, level, s, bearings, gap=2.1, ego=(0.0, 0.0), it=0):
    """Robots at `gap` on the given bearings, each approaching the ego's place at speed s; the ego
    moves at velocity `ego`."""
    robots = tuple((float(gap * np.cos(b)), float(gap * np.sin(b)), float(-s * np.cos(b)), float(-s * np.sin(b)))
                   for b in bearings)
    return (table, family, level, (float(ego[0]), float(ego[1]), 0.0), robots, it)


def case_rows(spec, origin=(0.0, 0.0)):
    """One case's robots: (states (1 + robots) x 6, targets, lists). Row 0 is the ego and lists every
    robot in the case's order; the robots list nobody and keep their place as target."""
    _, _, _, vel, robots, _ = spec
    n = 1 + len(robots)
    states, targets = np.zeros((n, 6)), np.zeros((n, 3))
    states[:, :2] = origin
    states[0, 3:] = vel
    for i, (x, y, vx, vy) in enumerate(robots):
        states[1 + i, :2] += (x, y)
        states[1 + i, 3:5] = (vx, vy)
    targets[:, :] = states[:, :3]
    targets[0] += TARGET
    return states, targets, [list(range(1, n))] + [[] for _ in robots]


def spec_tstar(spec, origin=(0.0, 0.0), with_iter1=False):
    """The LP of iteration 0 of a case on its own little table, and with with_iter1 the pair
    (iteration 0's, iteration 1's or None when the oracle's iteration 0 is not OPTIMAL)."""
    cfg = CONFIGS[spec[0]]
    st, tg, ls = case_rows(spec, origin)
    lp0 = tstar(case_qp(cfg, st, tg, 0, ls[0]))
    if not with_iter1:
        return lp0
    r = O.impc_optimize(O.make_params(cfg), st, 0, np.array(ls[0], dtype=np.int32), np.tile(tg[0], cfg["k_hor"]))
    if r["status"][0] != O.OPTIMAL:
        return lp0, None
    return lp0, tstar(case_qp(cfg, st, tg, 0, ls[0], 1, samples(cfg, r["x"][0])))


def level_tag(level):
    return ("m" if level < 0 else "p") + f"{abs(level):.1e}".replace(".0e", "e").replace("e-0", "e-")


def case_name(spec):
    return ("asym_" if spec[0] == "asym" else "") + f"{spec[1]}_{level_tag(spec[2])}"


# name -> spec. Found by tools/feasibility_search.py; every claim is checked by
# test_feasibility_inputs.py.
FOUND = {
    "asym_pair_skew_m3e-6": ('asym', 'pair_skew', -3e-06, (0.18, 0.11, 0.0), ((1.3093294155690383, -1.7927789828993537, -0.6041163420574834, 0.8271769261335948), (0.13135538804540914, 2.2161105031183443, -0.06060654835364439, -1.022499422085604)), 0),  # t* -3.0000000017199598e-06, t1* 3.224e-01, candidate 5
    "asym_pair_skew_p1.2e-5": ('asym', 'pair_skew', 1.2e-05, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110808171867452, -0.0), (-1.934228087406059, 0.8177785188481661, 0.2865244066932533, -0.12114057615288266)), 0),  # t* 1.2000000002324843e-05, candidate 0
    "asym_pair_skew_p3e-6": ('asym', 'pair_skew', 3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110805251226605, -0.0), (-1.934228087406059, 0.8177785188481661, 0.28652413768441715, -0.12114046241777096)), 0),  # t* 3.0000000016647578e-06, candidate 0
    "asym_pair_skew_p8e-6": ('asym', 'pair_skew', 8e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110806873805785, -0.0), (-1.934228087406059, 0.8177785188481661, 0.28652428713385636, -0.1211405256039804)), 0),  # t* 7.999999998433705e-06, candidate 0
    "iter1_pair_m3e-6": ('base', 'iter1_pair', -3e-06, (0.19, 0.14, 0.0), ((2.1002140026330194, -0.7193755230366079, -0.753518263602327, 0.258098743421852), (-1.9989925672229427, 0.9656234857269317, 0.7172018691044738, -0.3464479959405945)), 1),  # t* -3.0000000062792616e-06, t1* -3.000e-06, candidate 12
    "iter1_pair_p1.2e-5": ('base', 'iter1_pair', 1.2e-05, (0.12, 0.22, 0.0), ((-2.070699871796184, -0.7129530425934564, 0.6016215729841744, 0.2071415258150685), (2.178708148357216, 0.22210539003335775, -0.6330023202015836, -0.06453054638199379)), 1),  # t* 1.2000000020770581e-05, t1* 1.200e-05, candidate 1
    "iter1_pair_p3e-6": ('base', 'iter1_pair', 3e-06, (0.26, 0.06, 0.0), ((-2.256369216081554, 0.3910216882981228, 0.6812400386029696, -0.11805675601859635), (2.098750222568682, -0.9161591036866401, -0.6336519185116392, 0.27660555671195186)), 1),  # t* 2.9999999991734734e-06, t1* 3.000e-06, candidate 2
    "iter1_pair_p8e-6": ('base', 'iter1_pair', 8e-06, (-0.12, 0.23, 0.0), ((-1.0484111317075964, 1.922741297967981, 0.23541579375868887, -0.43174252463010576), (0.8713547335999166, -2.009189122067163, -0.19565861144731392, 0.4511539773641811)), 1),  # t* 8.000000000206513e-06, t1* 8.000e-06, candidate 3
    "iter1_single_m3e-6": ('base', 'iter1_single', -3e-06, (1.8957397250831796, -1.3129710305858817, 0.0), ((1.9338227837757958, -1.6621761161049182, 0.0, 0.0),), 1),  # t* -3.0000018511752754e-06, t1* -3.000e-06, candidate 2
    "iter1_single_p1.2e-5": ('base', 'iter1_single', 1.2e-05, (0.3147581756481796, -0.704787667239031, 0.0), ((0.5732852933169814, -2.237731881273193, 0.0, 0.0),), 1),  # t* 1.1999999823544249e-05, t1* 1.200e-05, candidate 1
    "iter1_single_p3e-6": ('base', 'iter1_single', 3e-06, (-0.8605356192665723, -1.3648807259723472, 0.0), ((-0.8733123699382365, -2.256928333933725, 0.0, 0.0),), 1),  # t* 2.9999997689671474e-06, t1* 3.000e-06, candidate 1
    "iter1_single_p8e-6": ('base', 'iter1_single', 8e-06, (0.9769684796585719, -1.3118473690228452, 0.0), ((1.8166326544747864, -1.6587482626052368, 0.0, 0.0),), 1),  # t* 8.000001612984744e-06, t1* 8.000e-06, candidate 1
    "pair_opposed_m1e-3": ('base', 'pair_opposed', -0.001, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12556942926717313, -0.0), (-2.1, 2.571758278209442e-16, 0.12556942926717313, -1.5377819962280355e-17)), 0),  # t* -0.0010000000000000117, t1* 3.949e-03, candidate 0
    "pair_opposed_m1e-5": ('base', 'pair_opposed', -1e-05, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.1261764585706553, -0.0), (-2.1, 2.571758278209442e-16, 0.1261764585706553, -1.5452159611630162e-17)), 0),  # t* -9.999999999986265e-06, t1* 5.000e-03, candidate 0
    "pair_opposed_m3e-6": ('base', 'pair_opposed', -3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12618067668372163, -0.0), (-2.1, 2.571758278209442e-16, 0.12618067668372163, -1.5452676181496674e-17)), 0),  # t* -2.9999999999445702e-06, t1* 5.007e-03, candidate 0
    "pair_opposed_p1.2e-5": ('base', 'pair_opposed', 1.2e-05, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12618971210253827, -0.0), (-2.1, 2.571758278209442e-16, 0.12618971210253827, -1.545378270116995e-17)), 0),  # t* 1.2000000000028796e-05, candidate 0
    "pair_opposed_p1e-1": ('base', 'pair_opposed', 0.1, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.15578988483280437, -0.0), (-2.1, 2.571758278209442e-16, 0.15578988483280437, -1.9078758380002867e-17)), 0),  # t* 0.10000000000000005, candidate 0
    "pair_opposed_p1e-3": ('base', 'pair_opposed', 0.001, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12677494278430956, -0.0), (-2.1, 2.571758278209442e-16, 0.12677494278430956, -1.5525452789289354e-17)), 0),  # t* 0.0009999999999999968, candidate 0
    "pair_opposed_p3e-6": ('base', 'pair_opposed', 3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.1261842914065645, -0.0), (-2.1, 2.571758278209442e-16, 0.1261842914065645, -1.545311885737261e-17)), 0),  # t* 3.000000000026735e-06, candidate 0
    "pair_opposed_p8e-6": ('base', 'pair_opposed', 8e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12618730310993387, -0.0), (-2.1, 2.571758278209442e-16, 0.12618730310993387, -1.5453487684661735e-17)), 0),  # t* 8.000000000024796e-06, candidate 0
    "pair_skew_m1e-3": ('base', 'pair_skew', -0.001, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.31104797147033203, -0.0), (-1.934228087406059, 0.8177785188481661, 0.28649415378504506, -0.12112778542844511)), 0),  # t* -0.001000000000001172, t1* -1.000e-03, candidate 0
    "pair_skew_m1e-5": ('base', 'pair_skew', -1e-05, (0.2, 0.17, 0.0), ((-0.9993093183314153, 1.9711623186069689, 0.46712637832101767, -0.9214183217176417), (0.3721583599674604, -2.1784393852265733, -0.17396514138761854, 1.0183098283441303)), 0),  # t* -1.0000000006251561e-05, t1* 2.127e+00, candidate 17
    "pair_skew_m3e-6": ('base', 'pair_skew', -3e-06, (0.01, -0.16, 0.0), ((1.1377496473836013, 1.8946307661068134, -0.5296057536581027, -0.8819228000600036), (-1.8606011551086137, -1.1925868277020724, 0.8660825158456, 0.5551316558439088)), 0),  # t* -3.000000004422068e-06, t1* 1.423e+00, candidate 10
    "pair_skew_p1.2e-5": ('base', 'pair_skew', 1.2e-05, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110808171867452, -0.0), (-1.934228087406059, 0.8177785188481661, 0.2865244066932533, -0.12114057615288266)), 0),  # t* 1.2000000002324828e-05, candidate 0
    "pair_skew_p1e-1": ('base', 'pair_skew', 0.1, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3142800627326221, -0.0), (-1.934228087406059, 0.8177785188481661, 0.289471106975798, -0.12238642104999639)), 0),  # t* 0.09999999999999826, candidate 0
    "pair_skew_p1e-3": ('base', 'pair_skew', 0.001, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3111128747423375, -0.0), (-1.934228087406059, 0.8177785188481661, 0.2865539336572725, -0.1211530599530399)), 0),  # t* 0.0010000000000009413, candidate 0
    "pair_skew_p3e-6": ('base', 'pair_skew', 3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110805251226605, -0.0), (-1.934228087406059, 0.8177785188481661, 0.28652413768441715, -0.12114046241777096)), 0),  # t* 3.0000000016646447e-06, candidate 0
    "pair_skew_p8e-6": ('base', 'pair_skew', 8e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.3110806873805785, -0.0), (-1.934228087406059, 0.8177785188481661, 0.28652428713385636, -0.1211405256039804)), 0),  # t* 7.999999998433673e-06, candidate 0
    "single_m1e-3": ('base', 'single', -0.001, (0.43822234706654306, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* -0.0010000000000001746, t1* -1.000e-03, candidate 0
    "single_m1e-5": ('base', 'single', -1e-05, (-0.49895284408736484, -1.586480375320269, 0.0), ((-0.9361763753163106, -2.100850731084818, 0.0, 0.0),), 0),  # t* -9.999999995111806e-06, t1* 1.548e+01, candidate 27
    "single_m3e-6": ('base', 'single', -3e-06, (-0.876582061678095, -1.8896184063169876, 0.0), ((-0.705976396858813, -2.2099767707101012, 0.0, 0.0),), 0),  # t* -3.000000107834564e-06, t1* 1.147e+02, candidate 15
    "single_p1.2e-5": ('base', 'single', 1.2e-05, (0.43825746887269024, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* 1.2000000001085544e-05, candidate 0
    "single_p1e-1": ('base', 'single', 0.1, (0.441696086936734, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* 0.09999999999999877, candidate 0
    "single_p1e-3": ('base', 'single', 0.001, (0.43829175149605404, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* 0.0009999999999999467, candidate 0
    "single_p3e-6": ('base', 'single', 3e-06, (0.438257156553189, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* 2.999999999759138e-06, candidate 0
    "single_p8e-6": ('base', 'single', 8e-06, (0.4382573300640863, 0.0, 0.0), ((2.1, 0.0, 0.0, 0.0),), 0),  # t* 8.000000000799568e-06, candidate 0
    "triple_m3e-6": ('base', 'triple', -3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12618067668372196, -0.0), (-0.8739083567489991, 1.9095245963339316, 0.05250968943530866, -0.11473576462363166), (-1.0295477248154687, -1.8303091220685352, 0.06186144218828677, 0.1099760207442842)), 0),  # t* -2.9999999999752447e-06, t1* 2.285e-03, candidate 0
    "triple_p1.2e-5": ('base', 'triple', 1.2e-05, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.1261897121025386, -0.0), (-0.8739083567489991, 1.9095245963339316, 0.05251344949626609, -0.11474398050671193), (-1.0295477248154687, -1.8303091220685352, 0.061865871900136975, 0.1099838957964184)), 0),  # t* 1.2000000000017617e-05, candidate 0
    "triple_p3e-6": ('base', 'triple', 3e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.12618429140656484, -0.0), (-0.8739083567489991, 1.9095245963339316, 0.052511193690784726, -0.11473905148181139), (-1.0295477248154687, -1.8303091220685352, 0.06186321434527664, 0.10997917124913804)), 0),  # t* 2.9999999999937257e-06, candidate 0
    "triple_p8e-6": ('base', 'triple', 8e-06, (0.0, 0.0, 0.0), ((2.1, 0.0, -0.1261873031099342, -0.0), (-0.8739083567489991, 1.9095245963339316, 0.052512447001614504, -0.11474179001593551), (-1.0295477248154687, -1.8303091220685352, 0.06186469086544414, 0.10998179617682848)), 0),  # t* 8.000000000012808e-06, candidate 0
    "vel_x_hi_m1e-3": ('base', 'vel_x_hi', -0.001, (1.999, 0.0, 0.0), (), 0),  # t* -0.0009999999999998899, t1* -1.000e-03, candidate 0
    "vel_x_hi_m1e-5": ('base', 'vel_x_hi', -1e-05, (1.99999, 0.0, 0.0), (), 0),  # t* -1.0000000000065529e-05, t1* -1.000e-05, candidate 0
    "vel_x_hi_m3e-6": ('base', 'vel_x_hi', -3e-06, (1.999997, 0.0, 0.0), (), 0),  # t* -2.999999999975195e-06, t1* -3.000e-06, candidate 0
    "vel_x_hi_p1.2e-5": ('base', 'vel_x_hi', 1.2e-05, (2.000012, 0.0, 0.0), (), 0),  # t* 1.199999999990105e-05, candidate 0
    "vel_x_hi_p1e-1": ('base', 'vel_x_hi', 0.1, (2.0999999999999996, 0.0, 0.0), (), 0),  # t* 0.09999999999999964, candidate 0
    "vel_x_hi_p1e-3": ('base', 'vel_x_hi', 0.001, (2.0010000000000003, 0.0, 0.0), (), 0),  # t* 0.001000000000000334, candidate 0
    "vel_x_hi_p3e-6": ('base', 'vel_x_hi', 3e-06, (2.0000030000000004, 0.0, 0.0), (), 0),  # t* 3.0000000004192767e-06, candidate 0
    "vel_x_hi_p8e-6": ('base', 'vel_x_hi', 8e-06, (2.0000080000000002, 0.0, 0.0), (), 0),  # t* 8.000000000230144e-06, candidate 0
    "vel_y_lo_m1e-3": ('base', 'vel_y_lo', -0.001, (0.0, -1.999, 0.0), (), 0),  # t* -0.0009999999999998899, t1* -1.000e-03, candidate 0
    "vel_y_lo_m1e-5": ('base', 'vel_y_lo', -1e-05, (0.0, -1.99999, 0.0), (), 0),  # t* -1.000000000006552e-05, t1* -1.000e-05, candidate 0
    "vel_y_lo_m3e-6": ('base', 'vel_y_lo', -3e-06, (0.0, -1.999997, 0.0), (), 0),  # t* -2.9999999999752913e-06, t1* -3.000e-06, candidate 0
    "vel_y_lo_p1.2e-5": ('base', 'vel_y_lo', 1.2e-05, (0.0, -2.000012, 0.0), (), 0),  # t* 1.1999999999900969e-05, candidate 0
    "vel_y_lo_p1e-1": ('base', 'vel_y_lo', 0.1, (0.0, -2.0999999999999996, 0.0), (), 0),  # t* 0.09999999999999964, candidate 0
    "vel_y_lo_p1e-3": ('base', 'vel_y_lo', 0.001, (0.0, -2.0010000000000003, 0.0), (), 0),  # t* 0.001000000000000334, candidate 0
    "vel_y_lo_p3e-6": ('base', 'vel_y_lo', 3e-06, (0.0, -2.0000030000000004, 0.0), (), 0),  # t* 3.0000000004194334e-06, candidate 0
    "vel_y_lo_p8e-6": ('base', 'vel_y_lo', 8e-06, (0.0, -2.0000080000000002, 0.0), (), 0),  # t* 8.000000000229966e-06, candidate 0
    "vel_yaw_hi_m1e-3": ('base', 'vel_yaw_hi', -0.001, (0.0, 0.0, 2.6169938779914945), (), 0),  # t* -0.0009999999999998899, t1* -1.000e-03, candidate 0
    "vel_yaw_hi_m1e-5": ('base', 'vel_yaw_hi', -1e-05, (0.0, 0.0, 2.6179838779914943), (), 0),  # t* -1.000000000006559e-05, t1* -1.000e-05, candidate 0
    "vel_yaw_hi_m3e-6": ('base', 'vel_yaw_hi', -3e-06, (0.0, 0.0, 2.6179908779914944), (), 0),  # t* -2.9999999999752443e-06, t1* -3.000e-06, candidate 0
    "vel_yaw_hi_p1.2e-5": ('base', 'vel_yaw_hi', 1.2e-05, (0.0, 0.0, 2.6180058779914948), (), 0),  # t* 1.2000000000345126e-05, candidate 0
    "vel_yaw_hi_p1e-1": ('base', 'vel_yaw_hi', 0.1, (0.0, 0.0, 2.7179938779914945), (), 0),  # t* 0.10000000000000009, candidate 0
    "vel_yaw_hi_p1e-3": ('base', 'vel_yaw_hi', 0.001, (0.0, 0.0, 2.6189938779914943), (), 0),  # t* 0.0009999999999998899, candidate 0
    "vel_yaw_hi_p3e-6": ('base', 'vel_yaw_hi', 3e-06, (0.0, 0.0, 2.6179968779914944), (), 0),  # t* 2.999999999975205e-06, candidate 0
    "vel_yaw_hi_p8e-6": ('base', 'vel_yaw_hi', 8e-06, (0.0, 0.0, 2.618001877991494), (), 0),  # t* 7.999999999785995e-06, candidate 0
}
# what the search looked for as an option: three robots (triple) and iteration 1 on a level (iter1_*)
FOUND_OPTIONAL = [n for n in FOUND if FOUND[n][1].startswith(("triple", "iter1_"))]


def named_cases(table=None):
    return {n: s for n, s in FOUND.items() if table is None or s[0] == table}


# ---- the batch ------------------------------------------------------------------------------------

# a 12 x 12 grid of sites SPACING apart around the origin, nearest first (active_census_cases.SITES'
# rule on a table twice as long)
SITES = [(SPACING * i, SPACING * j) for _, i, j in sorted((i * i + j * j, i, j) for i in range(-6, 6) for j in range(-6, 6))]


def in_last_wave(spec):
    """The egos that permutations() puts once into the last, partly filled wave."""
    return spec[1].startswith("pair_") and spec[2] in LAST_WAVE


@functools.lru_cache(maxsize=None)
def layout(table):
    """The unpermuted batch of one table: (names, states ROWS x 6, targets, lists, ego: name -> row).
    Rows: the egos — those of in_last_wave() first, then the others by name — then the cases' robots,
    then robots at rest on their targets with no neighbour up to ROWS rows. Case c stands on SITES[c],
    the fillers on the sites after the last case."""
    cases = named_cases(table)
    names = sorted(cases, key=lambda n: (not in_last_wave(cases[n]), n))
    ego = {n: i for i, n in enumerate(names)}
    states, targets, lists = [None] * len(names), [None] * len(names), [None] * len(names)
    for site, name in enumerate(names):
        st, tg, ls = case_rows(cases[name], SITES[site])
        local = [ego[name]] + list(range(len(states), len(states) + len(st) - 1))  # local row -> batch row
        states[ego[name]], targets[ego[name]], lists[ego[name]] = st[0], tg[0], [local[j] for j in ls[0]]
        for i in range(1, len(st)):
            states.append(st[i])
            targets.append(tg[i])
            lists.append([])
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
    """The batch of CONFIGS[config] with its rows permuted: new row i is row order[i] of
    layout(TABLE_OF[config]). Returns a dict: cfg, states, targets, rp, col (explicit CSR lists, each
    in its case's own order under every permutation), ego (name -> row), row_of (old row -> new
    row), names."""
    names, st, tg, lists, ego = layout(TABLE_OF[config])
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
def batch_tstar(table="base"):
    """name -> (iteration 0's LP, iteration 1's LP or None) of every ego on batch(IDENTITY, table)'s
    own state table; iteration 1's from the oracle's iteration-0 curve, None unless that is OPTIMAL."""
    b, ref = batch(IDENTITY, table), reference(table)
    out = {}
    for name, a in b["ego"].items():
        nbs = b["col"][b["rp"][a]:b["rp"][a + 1]]
        lp0 = tstar(case_qp(b["cfg"], b["states"], b["targets"], a, nbs))
        lp1 = None
        if ref[a]["status"][0] == O.OPTIMAL:
            lp1 = tstar(case_qp(b["cfg"], b["states"], b["targets"], a, nbs, 1, samples(b["cfg"], ref[a]["x"][0])))
        out[name] = (lp0, lp1)
    return out


def permutations(table="base"):
    """Four permutations of the batch's rows (new row i = old row order[i]) for launches of SOLVED
    agents (active_census_cases.permutations' construction on ROWS rows). In permutation p old row r
    sits in 16-lane group (r + p) % 4 of its wave, so every row passes through all four groups; and
    each ego of in_last_wave() sits once in the last wave (new rows ROWS - 4 .. ROWS - 2 of the
    16-lane layout's four agents per wave; row ROWS - 1, never solved, always holds a filler)."""
    names, _, _, _, ego = layout(table)
    cases = named_cases(table)
    todo = [ego[n] for n in names if in_last_wave(cases[n])]
    per = ROWS // 4
    out = []
    for p in range(4):
        order = np.empty(ROWS, dtype=np.int64)
        for g in range(4):
            rows = [r for r in range(ROWS) if (r + p) % 4 == g]
            # (group g's rows start 5 g waves later: a wave holds rows from all over the table)
            rows = rows[-5 * g:] + rows[:-5 * g] if g else rows
            pick = next((r for r in todo if r in rows), None) if g < 3 else max(rows)  # (max: a filler)
            if pick is not None:
                if g < 3:
                    todo.remove(pick)
                rows.remove(pick)
                rows.append(pick)
            assert len(rows) == per
            order[g::4] = rows
        out.append(tuple(int(v) for v in order))
    assert not todo, todo
    return out

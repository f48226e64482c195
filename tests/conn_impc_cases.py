"""Inputs of test_gpu_conn_impc.py (GPU) and test_conn_impc_inputs.py (CPU): seeded teams on which
the connectivity rows of the batched IMPC matter — the lambda2 row binding at an OPTIMAL point, CLF
rows binding, added rows turning an OPTIMAL QP INFEASIBLE — and their CPU reference results
(conn_impc_ref.py). Nothing here touches a GPU."""
from __future__ import annotations

import functools

import numpy as np

import conn_impc_ref as R
import oracle_lib as O
from mpccbf import swarm

K_HOR = 15
D_MAX = 3.2
SHIFT = 1e-6  # the stability check: every added bound moved by +-SHIFT relative
GAP = 30.0    # between team centres: teams do not interact

# (sizes, spacing, shape, speed range, seed): rings and lines of 2-6, 0.05 position noise, outward
# velocity plus 0.3 noise, targets at 3 x the offset from the centre
GROUPS = [
    ((3, 4, 5, 6), 2.6, "ring", (0.5, 2.0), 3),   # connectivity row binding / INFEASIBLE
    ((3, 3, 3, 4), 2.7, "ring", (0.5, 2.0), 11),  # connectivity row binding
    ((2, 3, 4, 5, 6), 2.9, "ring", (0.0, 0.3), 3),  # CLF rows binding
    ((3, 4), 2.8, "line", (0.2, 0.5), 3),         # CLF rows: INFEASIBLE
]


def config(**over):
    return swarm.config(K_HOR, **over)


def build(groups=GROUPS):
    """The groups side by side: (states, targets, team_ptr)."""
    st, tg, tp = [], [], [0]
    for g, (sizes, spacing, shape, speed, seed) in enumerate(groups):
        s, t, p = swarm.team_swarm(sizes, spacing, seed=seed, shape=shape, speed=speed, gap=GAP)
        s[:, 1] += 4.0 * GAP * g
        t[:, 1] += 4.0 * GAP * g
        st.append(s)
        tg.append(t)
        base = tp[-1]
        tp += [base + int(v) for v in p[1:]]
    return np.vstack(st), np.vstack(tg), np.asarray(tp, dtype=np.int32)


def team_of(team_ptr, row):
    t = int(np.searchsorted(team_ptr, row, side="right")) - 1
    return int(team_ptr[t]), int(team_ptr[t + 1] - team_ptr[t])


def reference(cfg, states, targets, team_ptr, rp, col, d_max=D_MAX, l2_min=0.1, l2_switch=0.1, rows=None,
              shift=0.0, attach=True):
    """conn_impc_ref.impc_agent of every row in `rows` (default: all)."""
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    out = {}
    for i in (range(len(states)) if rows is None else rows):
        team = team_of(team_ptr, i) if attach and i < team_ptr[-1] and i >= team_ptr[0] else None
        out[i] = R.impc_agent(cfg, states, i, col[rp[i]:rp[i + 1]], refs[i], team, d_max, l2_min, l2_switch, shift)
    return out


def classify(a, free):
    """'conn' / 'clf': an added row binds at OPTIMAL and the objective differs from the row-free
    QP's; 'infeasible': INFEASIBLE although the row-free QP is OPTIMAL; else 'other'."""
    if all(s == O.OPTIMAL for s in a["status"]):
        last = len(a["status"]) - 1
        bind = any(R.binding(a["rows"][it], a["x"][it]) for it in range(last + 1))
        differs = abs(a["obj"][last] - free["obj"][last]) > 1e-6 * max(1.0, abs(free["obj"][last]))
        if bind and differs:
            return "conn" if a["conn_mode"] else "clf"
        return "other"
    if O.INFEASIBLE in list(a["status"]) and all(s == O.OPTIMAL for s in free["status"]):
        return "infeasible"
    return "other"


@functools.lru_cache(maxsize=None)
def cases():
    """The batch and its reference, computed once per process: dict with cfg, states, targets,
    team_ptr, row_ptr, col, ref (per row, the attached result), free (without added rows), kind (per
    row), keep (rows whose statuses do not change when every added bound moves by +-SHIFT relative:
    the others sit on a decision boundary and are left out of the comparisons), spectra (per team:
    lambda2, Fiedler vector, eigenvalues)."""
    cfg = config()
    states, targets, team_ptr = build()
    rp, col = swarm.team_csr(team_ptr)
    ref = reference(cfg, states, targets, team_ptr, rp, col)
    free = reference(cfg, states, targets, team_ptr, rp, col, attach=False)
    up = reference(cfg, states, targets, team_ptr, rp, col, shift=SHIFT)
    dn = reference(cfg, states, targets, team_ptr, rp, col, shift=-SHIFT)
    n = len(states)
    keep = np.array([list(ref[i]["status"]) == list(up[i]["status"]) == list(dn[i]["status"]) for i in range(n)])
    kind = [classify(ref[i], free[i]) for i in range(n)]
    spectra = [R.team_spectrum(states, int(team_ptr[t]), int(team_ptr[t + 1] - team_ptr[t]), D_MAX)
               for t in range(len(team_ptr) - 1)]
    return dict(cfg=cfg, states=states, targets=targets, team_ptr=team_ptr, row_ptr=rp, col=col, ref=ref, free=free,
                kind=kind, keep=keep, spectra=spectra)


def closed_loop(cfg, states, targets, team_ptr, rp, col, steps, d_max=D_MAX):
    """The Jacobi closed loop on the reference: every step all rows re-plan from the previous
    step's table; a row's next state is its last OPTIMAL curve at t = h, or its state when no
    iteration was OPTIMAL. Returns (trace steps + 1 x n x 6, statuses steps x n x impc_iter,
    stable: whether no status changes when the added bounds move by +-SHIFT relative)."""
    cur = np.array(states, dtype=np.float64)
    trace, stats, stable = [cur.copy()], [], True
    for _ in range(steps):
        ref = reference(cfg, cur, targets, team_ptr, rp, col, d_max)
        for sh in (SHIFT, -SHIFT):
            alt = reference(cfg, cur, targets, team_ptr, rp, col, d_max, shift=sh)
            stable = stable and all(list(alt[i]["status"]) == list(ref[i]["status"]) for i in ref)
        nxt = cur.copy()
        for i, r in ref.items():
            ok = [it for it in range(len(r["status"])) if r["status"][it] == O.OPTIMAL]
            if ok:
                nxt[i] = R.next_state(cfg, r["x"][ok[-1]])
        stats.append(np.array([ref[i]["status"] for i in range(len(cur))]))
        cur = nxt
        trace.append(cur.copy())
    return np.array(trace), np.array(stats), stable


def loop_teams():
    """Two teams for the closed-loop comparison: a ring of 3 in connectivity mode and a ring of 4
    in CLF mode."""
    return build([((3,), 2.6, "ring", (0.5, 1.0), 5), ((4,), 2.9, "ring", (0.0, 0.3), 5)])

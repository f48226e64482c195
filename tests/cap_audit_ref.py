"""The neighbour-cap audit (mpccbf_cap_audit_run, include/mpccbf.h) restated in numpy on the CPU
oracle's row and curve functions — TEST INFRASTRUCTURE ONLY (tests/test_cap_audit.py,
tests/test_gpu_cap_audit.py)."""
import numpy as np

OPTIMAL, INFEASIBLE = 0, 3


def scenario(n, scale=0.45, k_hor=15):
    """The audit tests' swarm: the n-agent lattice with positions x scale (a crowd: neighbours
    inside d_min), config k_hor."""
    from mpccbf import swarm
    cfg = swarm.config(k_hor)
    states, targets = swarm.lattice_swarm(n)
    states[:, :2] *= scale
    return cfg, states, targets


def audit(O, cfg, states, lists, status, x0, x, first=0, tol=1e-6):
    """The audit of agents first .. first + len(lists) - 1 of `states` with neighbour lists
    `lists` (index arrays), the solve's statuses (agents x impc_iter), iteration-0 solutions x0 and
    returned solutions x (iteration 1's where status[1] is OPTIMAL). Returns a dict: counts
    (agents x 8), excess (agents x 2), live_nb (agents x 8), and for the margin checks
    bmargin = the smallest |b - bmax| / max(1, |bmax|) over every dropped row, live_sc = the scaled
    excesses of every live dropped row of a solved iteration, gap (agents x 2) = the distance
    between the two largest scaled excesses of the iteration (inf with fewer than two)."""
    p = O.make_params(cfg)
    ns, na = len(states), len(lists)
    iters = cfg["impc_iter"]
    a_lo, a_hi = np.array(cfg["a_min"]), np.array(cfg["a_max"])
    counts = np.zeros((na, 8), dtype=np.int32)
    excess = np.full((na, 2), np.nan)
    live_nb = np.full((na, 8), -1, dtype=np.int32)
    gap = np.full((na, 2), np.inf)
    bmargin, live_sc = np.inf, []
    for ai in range(na):
        self = first + ai
        st0 = int(status[ai, 0])
        st1 = int(status[ai, 1]) if iters > 1 else -1
        has1 = iters > 1 and st0 == OPTIMAL
        solved = [st0 == OPTIMAL, has1 and st1 == OPTIMAL]
        member = np.zeros(ns, dtype=bool)
        member[self] = True
        member[np.asarray(lists[ai], dtype=np.int64)] = True
        dropped = np.nonzero(~member)[0]
        # (iteration, sample, ego, acceleration of the iteration's solution there)
        slots = [(0, 0, states[self], O.eval_curve(p, x0[ai], 0.0, 2) if solved[0] else None)]
        if has1:
            for k in range(cfg["cbf_horizon"]):
                t = cfg["h"] * k
                e = np.concatenate([O.eval_curve(p, x0[ai], t, 0), O.eval_curve(p, x0[ai], t, 1)])
                slots.append((1, k, e, O.eval_curve(p, x[ai], t, 2) if solved[1] else None))
        nlive, nviol = [0, 0], [0, 0]
        rows = [[], []]  # (scaled excess, neighbour, sample) of the live rows of a solved iteration
        livej = []
        for j in dropped:
            anylive = False
            for it, k, e, acc in slots:
                a, b = O.safety_cbf(e, states[j], cfg["d_min"])
                bmax = float(np.sum(np.maximum(-a * a_lo, -a * a_hi)))
                bmargin = min(bmargin, abs(b - bmax) / max(1.0, abs(bmax)))
                if b >= bmax:
                    continue
                anylive = True
                nlive[it] += 1
                if acc is None:
                    continue
                sc = (-float(a @ acc) - b) / (1.0 + abs(b))
                live_sc.append(sc)
                nviol[it] += sc > tol
                rows[it].append((sc, int(j), k))
            if anylive:
                livej.append(j)
        best = [-1, -1]
        for it in range(2):
            if rows[it]:
                r = sorted(rows[it], key=lambda v: (-v[0], v[1], v[2]))
                best[it], excess[ai, it] = r[0][1], r[0][0]
                if len(r) > 1:
                    gap[ai, it] = r[0][0] - r[1][0]
        c0 = (solved[0] and nviol[0] == 0) or st0 == INFEASIBLE
        c1 = c0 and ((not has1) or (st1 == OPTIMAL and nviol[1] == 0) or st1 == INFEASIBLE)
        counts[ai] = [nlive[0], nviol[0], nlive[1] if has1 else -1, nviol[1] if has1 else -1,
                      best[0], best[1] if has1 else -1, len(dropped), int(c0) | (int(c1) << 1)]
        live_nb[ai, :min(8, len(livej))] = livej[:8]
    return dict(counts=counts, excess=excess, live_nb=live_nb, bmargin=bmargin,
                live_sc=np.array(live_sc), gap=gap)

"""Seeded CPU search for the literals of tests/feasibility_cases.py: per family and level, candidates
of the secondary geometry (gap, bearings, the ego's own velocity; the first candidate of a family is
its plain form), one scalar bisected until t* of the LP stands on the level, and the first candidate
that passes every admissibility check of test_feasibility_inputs.py on its own little table is kept.
Prints the FOUND entries with repr precision and what it did not find; no GPU.

    python tools/feasibility_search.py [candidates per family and level, default 12]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mpc-cbf_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import feasibility_cases as F  # noqa: E402
import oracle_lib as O  # noqa: E402

BISECTIONS = 80
BISECT_REL = 1e-5  # what the bisection must reach (the test asks LEVEL_REL = 1e-3)


def oracle_statuses(spec, config=None):
    """The oracle's statuses of every robot of the case on its own table (row 0: the ego)."""
    cfg = F.CONFIGS[config or spec[0]]
    st, tg, ls = F.case_rows(spec)
    p = O.make_params(cfg)
    return [list(O.impc_optimize(p, st, a, np.array(ls[a], dtype=np.int32), np.tile(tg[a], cfg["k_hor"]))["status"])
            for a in range(len(st))]


def level_of(spec):
    """t* of the iteration that the spec puts on its level (None: iteration 1 has no QP)."""
    if spec[5] == 0:
        return F.spec_tstar(spec)["t"]
    lp0, lp1 = F.spec_tstar(spec, with_iter1=True)
    return None if lp1 is None or lp0["t"] > -F.ITER1_MIN else lp1["t"]


def bisect(make, level, lo, hi):
    """The scalar s in [lo, hi] with t*(make(s)) = level, or None when the ends do not bracket it."""
    flo, fhi = level_of(make(lo)), level_of(make(hi))
    if flo is None or fhi is None or not (flo < level < fhi):
        return None
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        f = level_of(make(mid))
        if f is None:
            return None
        if f < level:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def admissible(spec):
    """Every check of test_feasibility_inputs.py on the case's own table; (ok, note)."""
    table, family, level, _, robots, it = spec
    lp0, lp1 = F.spec_tstar(spec, with_iter1=True)
    lp = lp0 if it == 0 else lp1
    if lp is None or abs(lp["t"] - level) > (BISECT_REL if it == 0 else 10.0 * BISECT_REL) * abs(level):
        return False, "level"
    for q in (lp0, lp1):
        if q is not None:
            c = F.certificate(q)
            if not (c["primal"] <= F.PRIMAL_TOL and c["lam_min"] >= 0.0 and abs(c["lam_sum"] - 1.0) <= 1e-12
                    and c["row"] <= 1e-12 and c["gap"] <= F.GAP_REL * abs(q["t"])):
                return False, f"certificate {c}"
    if robots and F.certificate(lp)["cbf"] < F.CBF_WEIGHT_MIN:
        return False, "box rows decide"
    sts = oracle_statuses(spec)
    if any(s != [O.OPTIMAL, O.OPTIMAL] for s in sts[1:]):
        return False, "robots"
    if it == 0 and level > 0:
        want = [O.INFEASIBLE, O.UNKNOWN]
    else:
        if lp1 is None or abs(lp1["t"]) < (F.ITER1_MIN if it == 0 and robots else 0.0):
            return False, "iteration 1 margin"
        want = [O.OPTIMAL, O.OPTIMAL if lp1["t"] < 0 else O.INFEASIBLE]
        if it == 1 and lp0["t"] > -F.ITER1_MIN:
            return False, "iteration 0 margin"
    if sts[0] != want:
        return False, f"oracle {sts[0]} != {want}"
    if len(robots) >= 2:
        st = F.case_rows(spec)[0]
        if min(F.row_margins(F.CONFIGS[table], st[0], st[1:])) < F.PAIR_ROW_MIN:
            return False, "row margin"
    if table == "base":
        slack = oracle_statuses(spec, "slack")[0]
        if robots and slack != [O.OPTIMAL, O.OPTIMAL]:
            return False, f"slack {slack}"
        if not robots and level > 0 and slack != [O.INFEASIBLE, O.UNKNOWN]:
            return False, f"slack {slack}"
    return True, f"t* {lp['t']!r}" + (f", t1* {lp1['t']:.3e}" if lp1 is not None else "")


def candidates(rng, table, family, level, i):
    """The i-th candidate of a family: (make(s) -> spec, lo, hi); i = 0 is the plain form."""
    plain = i == 0
    gap = 2.1 if plain else round(float(rng.uniform(2.04, 2.6)), 2)
    if family in F.VEL_FAMILIES:
        return (lambda s: F.vel_spec(table, family, level, s)), -0.1, 0.5
    if family in ("single", "iter1_single"):
        bearing = 0.0 if plain else round(float(rng.uniform(-np.pi, np.pi)), 2)
        side = 0.0 if plain else round(float(rng.uniform(-1.0, 1.0)), 2)
        return (lambda s: F.single_spec(table, level, s, gap, bearing, side, family, int(family != "single"))), 0.0, 2.5
    turn = 0.0 if plain else round(float(rng.uniform(-np.pi, np.pi)), 2)
    ego = (0.0, 0.0) if plain else tuple(round(float(v), 2) for v in rng.uniform(-0.3, 0.3, 2))
    if family == "pair_opposed":
        bearings = (turn, turn + np.pi)
    elif family == "iter1_pair":
        # (not 0: with two exactly opposed robots iteration 1's LP is degenerate, and multipliers of
        # 1e-14 on box rows keep the dual value 1e-11 from the primal one)
        a = 0.1 if plain else round(float(rng.uniform(0.05, 0.8)), 2)
        bearings = (turn, turn + np.pi - a)
    elif family == "pair_skew":
        a = 0.4 if plain else round(float(rng.uniform(0.2, 1.2)), 2)
        bearings = (turn, turn + np.pi - a)
    else:  # triple
        a = (2.0, 4.2) if plain else tuple(round(float(v), 2) for v in (rng.uniform(1.5, 2.5), rng.uniform(3.8, 4.8)))
        bearings = (turn, turn + a[0], turn + a[1])
    it = 1 if family.startswith("iter1_") else 0
    return (lambda s: F.ring_spec(table, family, level, s, bearings, gap, ego, it)), 0.0, 1.5


def iter1_bracket(make, lo, hi):
    """The upper end for an iter1_* bisection: where iteration 0's own t* is -2 ITER1_MIN (beyond it
    iteration 0 is no longer feasible by ITER1_MIN and level_of() has no value)."""
    s = bisect(lambda v: make(v)[:5] + (0,), -2.0 * F.ITER1_MIN, lo, hi)
    return hi if s is None else s


def main():
    budget = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    required = [("base", f, F.LEVELS) for f in list(F.VEL_FAMILIES) + ["single", "pair_opposed", "pair_skew"]]
    required.append(("asym", "pair_skew", F.TIGHT))
    optional = [("base", f, F.TIGHT) for f in ("triple", "iter1_single", "iter1_pair")]
    found, missing = {}, []
    for fam_index, (table, family, levels) in enumerate(required + optional):
        for level in levels:
            rng = np.random.default_rng([20251015, fam_index, F.LEVELS.index(level)])
            why = []
            for i in range(budget):
                make, lo, hi = candidates(rng, table, family, level, i)
                if family.startswith("iter1_"):
                    hi = iter1_bracket(make, lo, hi)
                s = bisect(make, level, lo, hi)
                if s is None:
                    why.append("no bracket")
                    continue
                spec = make(s)
                ok, note = admissible(spec)
                if ok:
                    found[F.case_name(spec)] = (spec, note, i)
                    break
                why.append(note.split(" ")[0])
            else:
                missing.append((table, family, level, why))
    for name in sorted(found):
        spec, note, i = found[name]
        print(f'    "{name}": {spec!r},  # {note}, candidate {i}')
    for table, family, level, why in missing:
        print(f"# not found: {table}/{family} at {level:+.1e} in {budget} candidates ({', '.join(sorted(set(why)))})")


if __name__ == "__main__":
    main()

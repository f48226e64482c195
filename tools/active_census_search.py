"""Seeded CPU search for the literals of tests/active_census_cases.py: one ego, 0 .. 2 static robots,
random far targets, slow initial velocities and gaps just above d_min, each candidate rounded to two
decimals, solved by the oracle and kept when it is admissible (active_census_cases: slack, strict
complementarity, status stability) for every robot of the case and both IMPC iterations. Prints the
FOUND entries; no GPU.

    python tools/active_census_search.py [candidates per family, default 300]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mpc-cbf_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import active_census_cases as A  # noqa: E402
import oracle_lib as O  # noqa: E402
from mpccbf import swarm  # noqa: E402


def evaluate(spec):
    """evaluate_at on the batch's farthest site and at the origin (the scale 1 + |b| of a side's slack
    grows with the distance from the origin): None unless admissible with the same census sizes on
    both; else the far site's result."""
    far = evaluate_at(spec, A.SITES[-1])
    if far is None:
        return None
    near = evaluate_at(spec, (0.0, 0.0))
    return far if near is not None and near[:2] == far[:2] else None


def evaluate_at(spec, origin):
    """None unless every robot of the case is OPTIMAL and admissible in both iterations and the
    static robots have no active side; else the ego's (sizes, CBF counts, worst slack, worst
    multiplier ratio) per iteration."""
    cfg = A.CONFIGS[spec[0]]
    states, targets, lists = A.case_rows(spec, origin)
    p = O.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    ego, worst = None, np.inf
    for a in range(len(states)):
        r = O.impc_optimize(p, states, a, np.array(lists[a], dtype=np.int32), refs[a])
        if any(s != O.OPTIMAL for s in r["status"]):
            return None
        ms = A.margins(cfg, states, targets, a, r, lists[a])
        if not all(A.admissible(m) for m in ms):
            return None
        if a > 0 and any(m["active"] for m in ms):
            return None
        if not A.stable(cfg, states, targets, a, lists[a], r["status"]):
            return None
        worst = min(worst, min(m["slack"] for m in ms))
        if a == 0:
            ego = ms
    k = tuple(len(m["active"]) for m in ego)
    ncbf = tuple(sum(1 for s in m["active"] if s[0] == "cbf") for m in ego)
    return k, ncbf, worst, min(m["mult"] for m in ego)


def candidate(rng, config, robots):
    d = float(np.exp(rng.uniform(np.log(0.3), np.log(80.0))))
    ang = rng.uniform(0.0, 2.0 * np.pi)
    tg = (d * np.cos(ang), d * np.sin(ang), rng.choice([-1.0, 1.0]) * min(d, 30.0) * rng.uniform(0.0, 1.0))
    speed = rng.choice([0.0, 0.3, 0.6]) if robots == 0 else rng.uniform(0.1, 0.6)
    va = ang + rng.uniform(-0.4, 0.4)
    vel = (speed * np.cos(va), speed * np.sin(va), 0.0)
    nbs = []
    for i in range(robots):
        na = va + (rng.uniform(-0.3, 0.3) if robots == 1 else (-1.0) ** i * rng.uniform(0.5, 1.0))
        gap = rng.uniform(2.03, 2.25)
        nbs.append((gap * np.cos(na), gap * np.sin(na)))
    r2 = lambda v: tuple(round(float(x), 2) + 0.0 for x in v)  # noqa: E731
    return (config, r2(tg), r2(vel), tuple(r2(n) for n in nbs), None, None)


def main():
    budget = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    found = {}

    def offer(name, spec, res):
        # the first admissible candidate, except that a later one with a wider margin replaces it
        score = min(res[2] / A.MIN_SLACK, res[3] / A.MIN_MULT)
        if name not in found or score > found[name][2]:
            found[name] = (spec[:4] + (res[0], res[1]), res, score)

    for config in ("base", "asym"):
        for robots, family in ((0, "box"), (1, "cbf1"), (2, "cbf2")):
            if config == "asym" and robots == 2:
                continue
            rng = np.random.default_rng([20251015, robots, config == "asym"])
            for _ in range(budget):
                spec = candidate(rng, config, robots)
                res = evaluate(spec)
                if res is None:
                    continue
                (k0, k1), (c0, c1) = res[0], res[1]
                if c0 != robots:
                    continue
                name = f"{family}_{k0}" if config == "base" else f"asym_{family}_{k0}"
                if config == "asym" and k0 < 4:
                    continue
                if config == "base" and family in ("box", "cbf1") and k0 == 6:
                    # all 8 sign patterns must be admissible with the mirrored census sizes
                    ok = True
                    for sign in A.SIGNS[1:]:
                        m = evaluate(A.mirrored(spec, sign))
                        ok = ok and m is not None and m[0] == res[0] and m[1] == res[1]
                    if not ok:
                        continue
                offer(name, spec, res)
                if config == "base" and k1 > k0 and (k0, k1) in ((4, 5), (5, 6)):
                    offer("iter1_grows", spec, res)
    for name in sorted(found):
        spec, res, _ = found[name]
        print(f'    "{name}": {spec!r},  # slack {res[2]:.2e}, multipliers {res[3]:.2e}')


if __name__ == "__main__":
    main()

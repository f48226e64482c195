"""CPU: the inputs of test_gpu_feasibility.py are what they claim (feasibility_cases.py). Every named
case, on the batch's own state table: t* of the LP stands on its level; both LP certificates hold in
np.longdouble; the oracle's statuses are those of the level; iteration 1 of a negative-level case is
decided by a margin the device's curve cannot move; the rows of a pair or triple case are each
feasible alone; the slack configuration turns every case with robots OPTIMAL and leaves the velocity
cases INFEASIBLE; and the four permutations place the egos where the GPU test wants them."""
import numpy as np
import pytest

import feasibility_cases as F
import oracle_lib as O

TABLES = ["asym", "base"]
OPT, INF, UNK = O.OPTIMAL, O.INFEASIBLE, O.UNKNOWN


def _certified(lp, what):
    c = F.certificate(lp)
    assert c["primal"] <= F.PRIMAL_TOL, (what, c)
    assert c["lam_min"] >= 0.0 and abs(c["lam_sum"] - 1.0) <= 1e-12 and c["row"] <= 1e-12, (what, c)
    assert c["gap"] <= F.GAP_REL * abs(lp["t"]), (what, c)
    return c


def test_required_cases_exist():
    cases = F.named_cases()
    for family in list(F.VEL_FAMILIES) + ["single", "pair_opposed", "pair_skew"]:
        for level in F.LEVELS:
            spec = cases[f"{family}_{F.level_tag(level)}"]
            assert spec[:3] == ("base", family, level) and spec[5] == 0
            assert len(spec[4]) == {"single": 1, "pair_opposed": 2, "pair_skew": 2}.get(family, 0)
    for level in F.TIGHT:
        spec = cases[f"asym_pair_skew_{F.level_tag(level)}"]
        assert spec[:3] == ("asym", "pair_skew", level) and len(spec[4]) == 2
    assert len({F.level_tag(v) for v in F.LEVELS}) == len(F.LEVELS)
    assert all(F.case_name(s) == n for n, s in cases.items())
    # the levels stand at least 20 % from both thresholds (feas_tol and the certificate's 10 feas_tol)
    for level in F.LEVELS:
        for thr in (F.FEAS_TOL, 10.0 * F.FEAS_TOL):
            assert abs(level - thr) >= 0.2 * thr * (1.0 - 1e-9), (level, thr)
    print(f"optional cases found: {F.FOUND_OPTIONAL}")


@pytest.mark.parametrize("table", TABLES)
def test_every_level_is_proved(oracle, table):
    """t* near its level and proved from both sides; iteration 1's own LP too."""
    b, ref, lps = F.batch(F.IDENTITY, table), F.reference(table), F.batch_tstar(table)
    cases = F.named_cases(table)
    for name in b["names"]:
        _, family, level, _, robots, it = cases[name]
        lp0, lp1 = lps[name]
        lp = lp0 if it == 0 else lp1
        assert abs(lp["t"] - level) <= F.LEVEL_REL * abs(level), (name, lp["t"])
        c0 = _certified(lp0, name)
        c1 = _certified(lp1, name + " iteration 1") if lp1 is not None else None
        if robots:  # not a velocity case in disguise: the CBF rows carry the certificate
            assert F.certificate(lp)["cbf"] >= F.CBF_WEIGHT_MIN, (name, F.certificate(lp))
        else:
            assert c0["cbf"] == 0.0
        status = [int(s) for s in ref[b["ego"][name]]["status"]]
        if it == 0 and level > 0:
            assert lp1 is None and status == [INF, UNK], (name, status)
        else:
            assert lp1 is not None and status == [OPT, OPT if lp1["t"] < 0 else INF], (name, status, lp1["t"])
            if it == 1:    # iter1_*: iteration 0 is feasible by a margin, iteration 1 stands on the level
                assert lp0["t"] <= -F.ITER1_MIN, (name, lp0["t"])
            elif robots:   # iteration 1 by a margin that a 1e-9 difference of the curve cannot move
                assert abs(lp1["t"]) >= F.ITER1_MIN, (name, lp1["t"])
            else:          # no robot, no CBF row: iteration 1's rows do not depend on the curve at all
                assert np.array_equal(lp1["G"], lp0["G"]) and np.array_equal(lp1["h"], lp0["h"]), name
                assert np.array_equal(lp1["E"], lp0["E"]) and np.array_equal(lp1["d"], lp0["d"]), name
        print(f"{table}/{name}: t* {lp0['t']:+.9e} (gap {c0['gap']:.1e}, primal {c0['primal']:.1e}, CBF weight "
              f"{c0['cbf']:.2f})" + (f", t1* {lp1['t']:+.6e} (gap {c1['gap']:.1e})" if lp1 is not None else "")
              + f", oracle {status}")


@pytest.mark.parametrize("table", TABLES)
def test_every_other_row_is_an_ordinary_optimal_row(oracle, table):
    """The cases' robots and the fillers list nobody and are OPTIMAL twice: they stay in every check."""
    b, ref = F.batch(F.IDENTITY, table), F.reference(table)
    egos = set(b["ego"].values())
    listed = set()
    for name, a in b["ego"].items():
        nbs = b["col"][b["rp"][a]:b["rp"][a + 1]].tolist()
        assert len(nbs) == len(F.FOUND[name][4]) and not (set(nbs) & egos)
        listed |= set(nbs)
    for a in range(F.ROWS):
        if a not in egos:
            assert b["rp"][a + 1] == b["rp"][a] and [int(s) for s in ref[a]["status"]] == [OPT, OPT], (table, a)
    assert len(listed) == sum(len(F.FOUND[n][4]) for n in b["names"])
    assert len(egos) + len(listed) <= F.ROWS - 4


@pytest.mark.parametrize("table", TABLES)
def test_pair_rows_are_each_feasible_alone(oracle, table):
    """A joint conflict, not the single-row test: every row of a pair or triple case has b - bmin >=
    PAIR_ROW_MIN at the state, and the single cases stand on the single-row test's own side."""
    b = F.batch(F.IDENTITY, table)
    for name, a in b["ego"].items():
        _, family, level, _, robots, it = F.FOUND[name]
        nbs = b["col"][b["rp"][a]:b["rp"][a + 1]]
        m = F.row_margins(b["cfg"], b["states"][a], b["states"][nbs])
        if len(robots) >= 2:
            assert min(m) >= F.PAIR_ROW_MIN, (name, m)
        elif family == "single":
            assert (m[0] < -F.FEAS_TOL) == (level > 0), (name, m)
        if robots:
            print(f"{table}/{name}: b - bmin {[f'{v:+.3e}' for v in m]}")


def test_slack_configuration(oracle):
    """Slack rows relax the CBF rows, not the box: every case with robots is OPTIMAL twice, every
    velocity case keeps its plain statuses."""
    b, ref, plain = F.batch(F.IDENTITY, "slack"), F.reference("slack"), F.reference("base")
    for name, a in b["ego"].items():
        status = [int(s) for s in ref[a]["status"]]
        if F.FOUND[name][4]:
            assert status == [OPT, OPT], (name, status)
        else:
            assert status == [int(s) for s in plain[a]["status"]], (name, status)
            if F.FOUND[name][2] > 0:
                assert status == [INF, UNK], (name, status)
    for a in set(range(F.ROWS)) - set(b["ego"].values()):
        assert [int(s) for s in ref[a]["status"]] == [OPT, OPT], a


@pytest.mark.parametrize("table", TABLES)
def test_permutations_place_the_egos(oracle, table):
    names, _, _, lists, ego = F.layout(table)
    perms = F.permutations(table)
    assert len(perms) == 4 and len(set(perms)) == 4
    fillers = [r for r in range(F.ROWS) if r >= len(names) and not lists[r] and r >= F.ROWS - 4]
    for order in perms:
        assert sorted(order) == list(range(F.ROWS)) and order[F.SOLVED] in fillers
    last = 0
    for name in names:
        where = [order.index(ego[name]) for order in perms]
        assert {w % 4 for w in where} == {0, 1, 2, 3}, (name, where)  # every 16-lane group of a wave
        if F.in_last_wave(F.FOUND[name]):  # the last, partly filled wave (rows 124 .. 126 of 127 solved)
            assert sum(F.ROWS - 4 <= w < F.SOLVED for w in where) == 1, (name, where)
            last += 1
    assert last == (6 if table == "base" else 3)

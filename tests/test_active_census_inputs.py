"""CPU: the inputs of test_gpu_active_census.py are what they claim (active_census_cases.py). Every
named case has the active-set size it is named for, in both IMPC iterations, on the batch's own
state table; every row of the batch — the cases' static robots and the fillers too — is OPTIMAL in
the oracle and passes the three admissibility checks (slack of the other sides, strict
complementarity, statuses stable under +-SHIFT); the sign patterns cover both sides of every
channel; and the four permutations place the cap-crossing cases where the GPU test wants them."""
import numpy as np
import pytest

import active_census_cases as A
import oracle_lib as O

CONFIGS = sorted(A.CONFIGS)


def test_required_cases_exist():
    cases = A.named_cases()
    for k in range(7):
        assert cases[f"box_{k}"][4][0] == k and cases[f"box_{k}"][5] == (0, 0)
    for k in range(2, 7):
        assert cases[f"cbf1_{k}"][4][0] == k and cases[f"cbf1_{k}"][5][0] == 1 and len(cases[f"cbf1_{k}"][3]) == 1
    cbf2 = [n for n in cases if n.startswith("cbf2_") and cases[n][4][0] in (4, 5, 6)]
    assert cbf2 and all(cases[n][5][0] == 2 and len(cases[n][3]) == 2 for n in cbf2)
    for fam in ("box", "cbf1"):
        for k in (4, 5, 6):
            assert cases[f"asym_{fam}_{k}"][0] == "asym" and cases[f"asym_{fam}_{k}"][4][0] == k
        assert all(n in cases for n in A.sign_cases(f"{fam}_6"))
    k0, k1 = cases["iter1_grows"][4]
    assert k1 > k0 and (k0, k1) in ((4, 5), (5, 6))
    print(f"optional cases found: {A.FOUND_OPTIONAL}")


@pytest.mark.parametrize("config", CONFIGS)
def test_every_case_has_its_census_and_margins(oracle, config):
    b, ref, cens = A.batch(A.IDENTITY, config), A.reference(config), A.batch_census(config)
    cases = A.named_cases()
    assert all(list(r["status"]) == [O.OPTIMAL] * 2 for r in ref), [list(r["status"]) for r in ref]
    worst = dict(slack=np.inf, mult=np.inf, stat=0.0)
    for a, ms in enumerate(cens):  # every row: cases, static robots, fillers
        for m in ms:
            assert A.admissible(m), (config, a, m)
            assert m["stat"] <= 1e-9, (config, a, m)  # (the multipliers do solve stationarity)
            worst = dict(slack=min(worst["slack"], m["slack"]), mult=min(worst["mult"], m["mult"]),
                         stat=max(worst["stat"], m["stat"]))
    egos = set(b["ego"].values())
    for a in range(A.ROWS):
        if a not in egos:
            assert [len(m["active"]) for m in cens[a]] == [0, 0], (config, a)
    for name in b["names"]:
        ms = cens[b["ego"][name]]
        k = tuple(len(m["active"]) for m in ms)
        ncbf = tuple(sum(1 for s in m["active"] if s[0] == "cbf") for m in ms)
        print(f"{config}/{name}: k {k}, CBF sides {ncbf}, slack {min(m['slack'] for m in ms):.2e}, "
              f"multipliers {min(m['mult'] for m in ms):.2e}")
        assert (k, ncbf) == cases[name][4:6], (name, k, ncbf, cases[name][4:6])
    print(f"{config}: worst slack {worst['slack']:.2e} (>= {A.MIN_SLACK}), worst multiplier ratio "
          f"{worst['mult']:.2e} (>= {A.MIN_MULT}), worst stationarity residual {worst['stat']:.2e}")


@pytest.mark.parametrize("config", CONFIGS)
def test_statuses_are_stable(oracle, config):
    b, ref = A.batch(A.IDENTITY, config), A.reference(config)
    for a in range(A.ROWS):
        nbs = b["col"][b["rp"][a]:b["rp"][a + 1]]
        assert list(A.python_impc(b["cfg"], b["states"], b["targets"], a, nbs)) == list(ref[a]["status"]), a
        assert A.stable(b["cfg"], b["states"], b["targets"], a, nbs, ref[a]["status"]), (config, a)


def test_census_helper_agrees_with_margins(oracle):
    b, ref, cens = A.batch(A.IDENTITY), A.reference(), A.batch_census()
    a = b["ego"]["cbf1_6"]
    got = A.census(b["cfg"], b["states"], a, ref[a], b["col"][b["rp"][a]:b["rp"][a + 1]])
    assert got == [m["active"] for m in cens[a]] and all(len(s) == 6 for s in got)


@pytest.mark.parametrize("base", ["box_6", "cbf1_6"])
def test_sign_patterns_cover_both_sides_of_every_channel(oracle, base):
    """The 8 mirrors have the mirrored census — lower <-> upper on the mirrored channels, the CBF
    side on the case's own robot — and together an active lower and upper side on every channel."""
    b, cens = A.batch(A.IDENTITY), A.batch_census()
    own = [cens[b["ego"][base]][it]["active"] for it in range(2)]
    seen = set()
    for name, sign in zip(A.sign_cases(base), A.SIGNS):
        a = b["ego"][name]
        nbs = b["col"][b["rp"][a]:b["rp"][a + 1]]
        for it in range(2):
            want = set()
            for s in own[it]:
                if s[0] == "box":
                    want.add(("box", s[1], s[2], s[3] if sign[s[1]] > 0 else 1 - s[3]))
                else:
                    want.add(("cbf", int(nbs[0]), s[2]))
            assert cens[a][it]["active"] == want, (name, it)
            seen |= {(s[1], s[3]) for s in want if s[0] == "box"}
    assert seen == {(d, up) for d in range(3) for up in (0, 1)}, seen


@pytest.mark.parametrize("config", CONFIGS)
def test_permutations_place_the_cap_crossing_cases(oracle, config):
    names, _, _, lists, ego = A.layout(config)
    cases = A.named_cases()
    perms = A.permutations(config)
    assert len(perms) == 4 and len(set(perms)) == 4
    fillers = [r for r in range(A.ROWS) if r >= len(names) and not lists[r]]
    for order in perms:
        assert sorted(order) == list(range(A.ROWS)) and order[A.SOLVED] in fillers
    for name in names:
        if not A.is_hard(cases[name]):
            continue
        where = [order.index(ego[name]) for order in perms]
        assert {w % 4 for w in where} == {0, 1, 2, 3}, (name, where)  # every 16-lane group of a wave
        if name in A.FOUND:  # the last, partly filled wave (rows 60 .. 62 of 63 solved)
            assert any(60 <= w < A.SOLVED for w in where), (name, where)
    # wave-mates that are k = 0 robots: every cap-crossing case shares a wave with one at least once
    cens = A.batch_census(config)
    easy = {r for r in range(A.ROWS) if all(not m["active"] for m in cens[r])}
    for name in names:
        if A.is_hard(cases[name]):
            mates = set()
            for order in perms:
                w = order.index(ego[name]) // 4
                mates |= set(order[4 * w:4 * w + 4]) - {ego[name]}
            assert mates & easy, name

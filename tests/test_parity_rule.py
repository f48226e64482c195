"""The comparison rules of parity_rule.py, on 2 agents x 2 iterations x 3 control-point entries:
what each rule must reject and what it must accept. CPU only."""
import copy

import numpy as np
import pytest

import oracle_lib as O
import parity_rule as PR
from parity_rule import check_parity, check_routes_agree, same_bits, same_values

INFEASIBLE = O.INFEASIBLE


def _ref():
    """Agent 0: OPTIMAL, OPTIMAL. Agent 1: OPTIMAL, INFEASIBLE (its curve is iteration 0's). The
    oracle's vectors carry two more entries behind the curve (slacks), as impc_optimize's do."""
    return [dict(status=[O.OPTIMAL, O.OPTIMAL], obj=[-50.0, 0.25],
                 x=[np.array([9.0, 9.0, 9.0, 7.0, 7.0]), np.array([1.0, -2.0, 3.0, 7.0, 7.0])]),
            dict(status=[O.OPTIMAL, INFEASIBLE], obj=[2000.0, np.nan],
                 x=[np.array([0.5, 0.0, -0.5, 7.0, 7.0]), None])]


def _got():
    return dict(status=np.array([[0, 0], [0, INFEASIBLE]], np.int32), obj=np.array([[-50.0, 0.25], [2000.0, np.nan]]),
                x=np.array([[1.0, -2.0, 3.0], [0.5, 0.0, -0.5]]))


def _arrays(ref):
    """The same reference as the FoV case modules' array tuple (status, obj, x by iteration)."""
    x = np.array([[np.full(3, np.nan) if v is None else v[:3] for v in r["x"]] for r in ref])
    return np.array([r["status"] for r in ref]), np.array([r["obj"] for r in ref], dtype=np.float64), x


def test_status_constant_is_the_oracles():
    assert PR.OPTIMAL == O.OPTIMAL
    assert (PR.OBJ_TOL, PR.X_TOL, PR.ROUTE_REL) == (1e-4, 1e-5, 1e-7)


@pytest.mark.parametrize("shape", ["dicts", "arrays", "mapping"])
def test_check_parity_accepts(shape, capsys):
    conv = {"dicts": lambda r: r, "arrays": _arrays, "mapping": lambda r: dict(enumerate(r))}[shape]
    g = _got()
    assert check_parity(g, conv(_ref())) == (0.0, 0.0)
    # within the bounds: 5e-5 relative (of max(1, |ref|)) and 5e-6
    g["obj"][0] += [-50.0 * 5e-5, 5e-5]
    g["obj"][1, 0] += 2000.0 * 5e-5
    g["x"] += 5e-6
    # an arbitrary objective where the oracle is not OPTIMAL
    g["obj"][1, 1] = 123.0
    eo, ex = check_parity(g, conv(_ref()), label="close")
    assert 4.9e-5 <= eo <= 5.1e-5 and 4.9e-6 <= ex <= 5.1e-6
    assert "close: 2 agents, worst objective error 5.0" in capsys.readouterr().out


def test_control_points_are_held_to_the_last_optimal_iteration_only():
    """Agent 0's curve is iteration 1's (iteration 0's, 9 9 9, is far away); agent 1's is
    iteration 0's, its iteration 1 being INFEASIBLE."""
    ref = _ref()
    check_parity(_got(), ref)
    ref[0]["x"][0] = np.full(5, np.nan)  # never looked at
    check_parity(_got(), ref)
    g = _got()
    g["x"][1] = [9.0, 9.0, 9.0]
    with pytest.raises(AssertionError):
        check_parity(g, ref)


def _broken(what):
    g = _got()
    if what == "status":
        g["status"][1, 1] = O.OPTIMAL
    elif what == "objective 2e-4 off":
        g["obj"][1, 0] += 2000.0 * 2e-4
    elif what == "objective 2e-4 off below 1":
        g["obj"][0, 1] += 2e-4
    elif what == "NaN objective":
        g["obj"][0, 1] = np.nan
    elif what == "x 2e-5 off":
        g["x"][1, 2] -= 2e-5
    elif what == "NaN x":
        g["x"][0, 1] = np.nan
    return g


@pytest.mark.parametrize("shape", ["dicts", "arrays"])
@pytest.mark.parametrize("what", ["status", "objective 2e-4 off", "objective 2e-4 off below 1", "NaN objective",
                                  "x 2e-5 off", "NaN x"])
def test_check_parity_rejects(what, shape):
    ref = _ref() if shape == "dicts" else _arrays(_ref())
    with pytest.raises(AssertionError):
        check_parity(_broken(what), ref)


def test_nan_under_optimal_passed_the_old_accumulation():
    """What test_gpu_conn_impc._compare did before: worst = max(worst, e), asserted at the end.
    max(0.0, nan) is 0.0, so NaN control points (or a NaN objective) under a matching OPTIMAL status
    passed; check_parity asserts per agent and its maxima keep the NaN."""
    for what in ("NaN x", "NaN objective"):
        g, ref = _broken(what), _ref()
        worst = dict(obj=0.0, x=0.0)
        for i, r in enumerate(ref):
            assert list(g["status"][i]) == list(r["status"])
            ok = [it for it in range(2) if r["status"][it] == O.OPTIMAL]
            for it in ok:
                worst["obj"] = max(worst["obj"], abs(g["obj"][i, it] - r["obj"][it]) / max(1.0, abs(r["obj"][it])))
            worst["x"] = max(worst["x"], float(np.max(np.abs(g["x"][i] - r["x"][ok[-1]][:3]))))
        assert worst["obj"] <= PR.OBJ_TOL and worst["x"] <= PR.X_TOL  # the old rule lets it through
        with pytest.raises(AssertionError):
            check_parity(g, ref)
    assert np.isnan(PR.worse(0.0, np.nan)) and np.isnan(PR.worse(np.nan, 1.0)) and np.isnan(PR.worse(-np.inf, np.nan))
    assert PR.worse(0.5, 0.25) == 0.5 and PR.worse(0.25, 0.5) == 0.5


def test_check_parity_agents_first_and_no_curves():
    ref = _ref()
    g = _got()
    g["obj"][0, 0] = 1.0  # agent 0 is wrong ...
    check_parity(g, ref[1:], agents=[1])  # ... and not listed: the reference list follows `agents`
    with pytest.raises(AssertionError):
        check_parity(g, ref, agents=[0, 1])
    # rows first .. of a batch: agent a is row a - first
    tail = {k: v[1:] for k, v in _got().items()}
    check_parity(tail, {1: ref[1]}, agents=[1], first=1)
    # x=False, or a reference without curves: statuses and objectives only
    g = _got()
    g["x"][:] = np.nan
    check_parity(g, ref, x=False)
    check_parity(dict(status=g["status"], obj=g["obj"]), _arrays(ref)[:2])
    with pytest.raises(AssertionError):
        check_parity(g, ref)


def test_same_bits():
    a = np.array([0.0, 1.5, np.nan, -np.inf])
    same_bits(a, a.copy())  # identical NaNs
    neg = a.copy()
    neg[0] = -0.0
    payload = a.copy()
    payload.view(np.uint64)[2] ^= 1  # another NaN
    assert np.isnan(payload[2])
    ints = np.array([1, 2, 3], np.int32)
    other = ints.copy()
    other[1] = 7
    for x, y in ((a, neg), (a, payload), (a, a.astype(np.float32)), (a, a.reshape(2, 2)), (ints, other),
                 (ints, ints.astype(np.int64))):
        with pytest.raises(AssertionError):
            same_bits(x, y)
    same_bits(ints, ints.copy())
    same_bits(a[::2], a.copy()[::2])  # (views need not be contiguous)


def test_same_values():
    a = np.array([0.0, 1.5, np.nan])
    same_values(a, np.array([-0.0, 1.5, np.nan]))
    with pytest.raises(AssertionError):
        same_values(a, np.array([0.0, 1.5, 2.0]))  # NaN against a number
    with pytest.raises(AssertionError):
        same_values(a, np.array([0.0, 1.0, np.nan]))
    with pytest.raises(AssertionError):
        same_values(a, a[:2])
    same_values(np.array([1, 2]), np.array([1, 2]))


def test_identity_rules_on_dicts_name_the_first_differing_key():
    a = dict(status=np.array([0, 3], np.int32), obj=np.array([1.0, np.nan]), x=np.array([0.0, 2.0]))
    b = copy.deepcopy(a)
    same_bits(a, b)
    same_values(a, b, keys=("status", "obj"))
    b["x"][0] = -0.0
    same_values(a, b)
    same_bits(a, b, keys=("status", "obj"))
    with pytest.raises(AssertionError, match="'x'.*first at \\(0,\\)"):
        same_bits(a, b, what="run 2")
    b["obj"][0] = 2.0
    with pytest.raises(AssertionError, match="'obj'"):
        same_values(a, b)


def test_check_routes_agree(capsys):
    ref = np.array([[1.0, np.nan, -2000.0], [0.0, 5.0, np.nan]])
    assert check_routes_agree(ref.copy(), ref, "same") == 0.0
    close = ref.copy()
    close[0, 2] -= 2000.0 * 5e-8
    close[1, 0] += 5e-8
    assert 4.9e-8 <= check_routes_agree(close, ref, "close") <= 5.1e-8
    assert "close: largest relative difference 5.0" in capsys.readouterr().out
    moved = ref.copy()
    moved[0, 1], moved[0, 0] = 1.0, np.nan
    far = ref.copy()
    far[1, 1] += 5.0 * 2e-7
    lost = ref.copy()
    lost[1, 2] = 0.0
    for bad in (moved, far, lost, ref[:1]):
        with pytest.raises(AssertionError):
            check_routes_agree(bad, ref, "bad")
    check_routes_agree(far, ref, "wider", rel=1e-6)

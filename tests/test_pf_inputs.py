"""CPU: the particle-filter cases (tests/pf_cases.py) pinned on the reference alone (tests/pf_ref.py).

The device and the numpy reference differ only through libm's last bits and the order of sums of
<= 1024 terms, about 1e-13; a decision margin of >= 1e-10 (three orders above) means both take the
same discrete decisions (inside / outside the FoV, the ancestor of every resampling draw), which is
what lets tests/test_gpu_pf.py compare ancestors and flags exactly."""
import math

import numpy as np
import pytest

import pf_cases
import pf_ref

MARGIN = 1e-10


@pytest.fixture(scope="module")
def runs():
    return {c["name"]: (c, *pf_cases.run_reference(c)) for c in pf_cases.all_cases()}


def test_case_shapes_cover_the_issue_list(runs):
    cases = [v[0] for v in runs.values()]
    assert sorted({c["par"]["num_particles"] for c in cases}) == sorted(pf_cases.PARTICLE_COUNTS)
    assert {len(c["rp"]) - 1 for c in cases} == {1, 5}
    shape = runs["shape_P100"][0]
    assert sorted(set(np.diff(shape["rp"]))) == [0, 1, 2, 3, 9]
    assert shape["agent_first"] > 0 and shape["num_states"] > len(shape["rp"]) - 1
    yaw = shape["states"](0)[:, 2]
    assert yaw.max() == math.pi and yaw.min() < -1.0 and np.all((yaw > -math.pi) & (yaw <= math.pi))
    for c in cases:
        assert c["col"].min() >= 0 and c["col"].max() < c["num_states"]
        assert c["agent_first"] + len(c["rp"]) - 1 <= c["num_states"]


def test_every_margin_is_above_the_bound(runs):
    for name, (c, _, steps) in runs.items():
        worst = min(float(r["margin"].min()) for r in steps)
        print(f"{name}: smallest decision margin over {len(steps)} steps = {worst:.3e}")
        assert worst >= MARGIN, (name, worst)


def test_scenarios_are_what_they_say(runs):
    c, _, steps = runs["scenarios"]
    m = np.array([r["flags"] & pf_ref.FLAG_MEASURED for r in steps])  # steps x pairs (0, 1, 2, 4, 5)
    assert m[:, 0].all()          # visible
    assert not m[:, 1].any()      # behind the observer
    assert not m[:, 2].any()      # beyond Rs
    assert m[0, 3] and not m[-1, 3] and not m[0, 4] and m[-1, 4]  # crossing the edge, both ways
    assert not any((r["flags"] & pf_ref.FLAG_DEGENERATE).any() for r in steps)
    # a hidden neighbour just outside the edge (pair 4 at step 0): its particles inside the FoV are
    # the ones with reduced weights, and there are some on either side
    w = steps[0]["pre_weights"][4]
    assert set(np.round(w * 1000).astype(int)) == {1, 10}


def test_degenerate_case_reaches_a_zero_sum(runs):
    c, st, steps = runs["degenerate"]
    par = c["par"]
    # the measurement weights of pair 0 at step 0, before the rule replaces them
    r0 = steps[0]
    x, y = r0["predicted"][0]
    tgt = c["states"](0)[1]
    with np.errstate(under="ignore"):
        w = np.exp(-0.5 * ((x - tgt[0]) ** 2 + (y - tgt[1]) ** 2) / par["meas_cov"][0])
    assert w.sum() == 0.0
    assert r0["flags"][0] == pf_ref.FLAG_MEASURED | pf_ref.FLAG_DEGENERATE
    np.testing.assert_array_equal(r0["pre_weights"][0], np.full(100, 0.01))
    assert r0["flags"][1] == pf_ref.FLAG_MEASURED
    assert np.isfinite(r0["est_xy"]).all() and np.isfinite(r0["est_cov"]).all()


def test_stream_is_keyed_on_global_rows_not_on_the_csr_position(runs):
    """A pair's results do not depend on the batch it is part of."""
    c, _, _ = runs["shape_P65"]
    par, s0 = c["par"], c["states"](0)
    full = pf_ref.init(par, s0, c["agent_first"], c["rp"], c["col"])
    # observer row 5 (list row 3) alone, its pairs at CSR entries 0 .. 2
    lo, hi = c["rp"][3], c["rp"][4]
    alone = pf_ref.init(par, s0, 5, np.array([0, hi - lo]), c["col"][lo:hi])
    np.testing.assert_array_equal(alone["particles"], full["particles"][lo:hi])
    a = pf_ref.step(par, s0, 5, np.array([0, hi - lo]), c["col"][lo:hi], alone["particles"], alone["weights"], 0)
    f = pf_ref.step(par, s0, c["agent_first"], c["rp"], c["col"], full["particles"], full["weights"], 0)
    np.testing.assert_array_equal(a["ancestors"], f["ancestors"][lo:hi])
    np.testing.assert_array_equal(a["est_xy"], f["est_xy"][lo:hi])


def test_normals_have_unit_moments():
    z = pf_ref.normal(pf_ref.keys(3, 0, 1, 2, 200000, pf_ref.COMP_X))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    u = pf_ref.uniform(pf_ref.keys(3, 0, 1, 2, 200000, pf_ref.COMP_RESAMPLE))
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.005

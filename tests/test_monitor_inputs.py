"""CPU: the inputs of test_gpu_monitor.py exercise what they claim (monitor_cases.py), and
mpccbf.monitor.result_from_outputs turns the monitor's raw outputs into the return values of
metrics.instance_success. The raw outputs here come from monitor_cases.model_outputs, a numpy
restatement of the device's; no GPU, no library call."""
import numpy as np
import pytest

import exact_geometry_cases as G
import monitor_cases as M
from mpccbf import metrics
from mpccbf.monitor import decode_key, result_from_outputs


def _cells(xy, watch):
    return [(M.cell_of(x, watch), M.cell_of(y, watch)) for x, y in xy]


def test_row_counts():
    assert [M.case(n)[0]["samples"].shape[1] for n in ("rows_1", "rows_2", "rows_65", "rows_300")] == [1, 2, 65, 300]
    _, o = M.case("rows_1")
    assert o["summary"].tolist() == [1, -1, 0, 0, M.INF_BITS] and o["reached_at"].tolist() == [0]
    assert np.isinf(o["min_d2"][0])
    _, o = M.case("rows_2")
    assert decode_key(o["summary"][1]) == (0, 0, 1) and o["summary"][2] == 1 and o["summary"][3] == 1
    _, o = M.case("rows_65")
    assert o["summary"][2] >= 1 and o["summary"][3] > 60
    _, o = M.case("rows_300")
    assert o["summary"][2] >= 2 and decode_key(o["summary"][1])[1] == 0  # (the hit pair (0, 299) comes first)


def test_crowded_cell_holds_more_than_a_fixed_bucket():
    c, o = M.case("crowded_cell")
    xy = c["samples"][0, :, :2]
    cells = _cells(xy, M.watch_of(c["monitor"]))
    assert cells.count(cells[0]) == M.CROWD > G.GRID_CAP
    pairs = M.CROWD * (M.CROWD - 1) // 2
    assert o["summary"][2] == pairs and o["summary"][3] == pairs and o["summary"][4] == 0
    assert (o["hit_samples"][:M.CROWD] == 1).all() and (o["hit_samples"][M.CROWD:] == 0).all()


def test_shared_bucket_case_shares_buckets():
    c, o = M.case("shared_bucket")
    xy = c["samples"][0, :, :2]
    n = len(xy)
    mask = M.table_size(n) - 1
    assert mask == 1023
    # the centre cell's 3 x 3 block reaches a bucket twice
    hs = G.block_hashes(*G.SHARED_CELL, mask=mask)
    assert len(set(hs)) < 9
    cells = _cells(xy, M.SHARED_WATCH)
    assert G.SHARED_CELL in cells[:25]
    # a row of the second cluster sits in a distant cell with the first cluster's centre bucket
    h0 = G.cell_hash(*G.SHARED_CELL, mask)
    far = [cl for cl in cells[25:] if G.cell_hash(cl[0], cl[1], mask) == h0]
    assert far and all(abs(cl[0] - G.SHARED_CELL[0]) >= 8 and abs(cl[1] - G.SHARED_CELL[1]) >= 8 for cl in far)
    # both clusters have the same pair structure: every count is twice one cluster's
    one = M.model_outputs(dict(c, samples=c["samples"][:, :25], num_agents=25))
    assert one["summary"][3] > 0 and o["summary"][3] == 2 * one["summary"][3]
    assert (o["unsafe_samples"][:25] == o["unsafe_samples"][25:]).all()
    assert np.array_equal(o["min_d2"][:25], o["min_d2"][25:])


def test_awkward_coordinates():
    c, o = M.case("cell_edges")
    xy = c["samples"][0, :, :2]
    edge = M.EDGE_WATCH * (1.0 + M.CELL_MARGIN)
    assert any(x < 0 for x, _ in xy) and all((x / edge) == round(x / edge) for x, _ in xy[:25])
    # a row on the edge and its partner to the left are in different cells and collide
    cells = _cells(xy, M.EDGE_WATCH)
    assert sum(cells[i] != cells[25 + i] for i in range(25)) >= 20
    assert o["summary"][2] == 25 and (o["hit_samples"] == 1).all()
    c, o = M.case("negative_lattice")
    assert c["samples"][..., :2].min() == -12.0
    assert o["summary"][2] == 0 and o["summary"][3] == 2 * 12 * 11 and o["summary"][4] == M.bits(4.0)


def test_box_threshold():
    c, o = M.case("box_threshold")
    xy = c["samples"][0, :, :2]
    hit = [bool(metrics.collision_check(*xy[2 * k], *xy[2 * k + 1], [0.25, 0.25], "box")) for k in range(5)]
    assert hit == [False, False, True, True, False]
    assert xy[5, 0] == np.nextafter(0.5, 0.0) and xy[7, 1] == np.nextafter(0.5, 0.0)
    assert o["summary"][2] == 2 and decode_key(o["summary"][1]) == (0, 4, 5)
    assert o["hit_samples"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0]


def test_circle_threshold_is_inclusive():
    c, o = M.case("circle_pairs")
    assert o["summary"][2] == 1 and decode_key(o["summary"][1]) == (0, 0, 1)
    assert bool(metrics.collision_check(0.0, 0.0, 0.0, 0.5, 0.25, "circle"))


def test_watch_radius_edge():
    c, o = M.case("watch_edge")
    assert o["min_d2"].tolist() == [25.0, 25.0, np.inf] and o["summary"][4] == M.bits(25.0)
    p = c["samples"][0, :, :2]
    d = p[2] - p[0]
    assert d[0] * d[0] + d[1] * d[1] > 25.0


def test_exact_goal_arrival():
    c, o = M.case("goal_exact")
    p, g = c["samples"][0, :, :2], c["goals"][:, :2]
    assert (p[0] - g[0]).tolist() == [0.75, 1.0] and np.hypot(0.75, 1.0) == 1.25
    assert o["reached_at"].tolist() == [0, -1]
    assert metrics.reach_goal_area(p, g, 1.25).tolist() == [True, False]


def test_first_collision_order():
    c, o = M.case("first_order")
    assert o["summary"][2] == 3 and decode_key(o["summary"][1]) == (0, 1, 4)
    assert M.script_result(dict(c, goals=np.zeros((7, 3)) + 99.0))[2] == (0, 1, 4)


@pytest.mark.parametrize("name,ok,makespan,collision", [
    ("collision_before_arrival", False, float("inf"), (2, 0, 1)),
    ("collision_at_arrival", False, float("inf"), (3, 0, 1)),
    ("collision_after_arrival", True, 3, None),
])
def test_collision_timing_relative_to_arrival(name, ok, makespan, collision):
    c, o = M.case(name)
    assert o["reached_at"].tolist() == [1, 3]
    r = M.model_result(c)
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == (ok, makespan, collision)
    assert M.script_result(c) == (ok, makespan, collision)
    assert r["first_collision_any"] is not None  # (the later collision is still counted)


def test_fixed_rows_case():
    c, o = M.case("fixed_rows")
    assert (c["agent_first"], c["num_agents"]) == (3, 3)
    assert (c["samples"][:, [0, 1, 2, 6, 7]] == c["samples"][0, [0, 1, 2, 6, 7]]).all()
    assert decode_key(o["summary"][1]) == (0, 0, 1)  # two fixed rows, in every sample
    assert o["hit_samples"].tolist() == [4, 4, 0, 0, 1, 0, 1, 0]
    assert o["reached_at"].tolist() == [-1, -1, -1, 2, -1, 0, -1, -1]
    assert o["unsafe_samples"][4] == 2 and o["unsafe_samples"][6] == 2
    r = M.model_result(c)
    assert r["goal_reached_frac"] == pytest.approx(2 / 3) and not r["instance_success"]


def test_ten_sample_trace():
    c, o = M.case("trace10")
    assert c["samples"].shape[:2] == (10, 33) and c["layout"] == "trace"
    assert o["summary"][0] == 10 and o["sample_log"][:10, 1].min() > 0
    assert o["sample_log"][0, 0] == 0 and o["sample_log"][9, 0] > 0
    assert (o["sample_log"][10:] == [0, 0, M.INF_BITS]).all()


ALL_AGENT_CASES = [n for n in M.CASES if M.CASES[n]()["goals"] is not None and M.CASES[n]()["agent_first"] == 0]


@pytest.mark.parametrize("name", ALL_AGENT_CASES)
def test_result_is_the_scripts_on_the_cases(name):
    c, _ = M.case(name)
    r = M.model_result(c)
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == M.script_result(c)
    assert r["min_pair_distance_m"] == metrics.min_pair_distance(np.transpose(c["samples"], (1, 0, 2))) or (
        np.isinf(r["min_pair_distance_m"]))


def test_result_from_outputs_is_the_scripts_on_200_random_traces():
    seen = set()
    for seed in range(200):
        c = M.random_trace(seed)
        r = M.model_result(c)
        want = M.script_result(c)
        assert (r["instance_success"], r["makespan"], r["first_collision"]) == want, seed
        n, S = c["num_agents"], c["samples"].shape[0]
        if n > 1:
            d = metrics.min_pair_distance(np.transpose(c["samples"], (1, 0, 2)))
            assert r["min_pair_distance_m"] == (d if d <= M.watch_of(c["monitor"]) else np.inf), seed
        o = M.model_outputs(c)
        late = r["first_collision_any"] is not None and r["first_collision"] is None
        seen.add(("fail" if not want[0] else "all_arrived_early" if want[1] < S else "ran_out", late))
    # the traces cover every branch of the walk, a collision after the last arrival included
    assert {("fail", False), ("all_arrived_early", False), ("ran_out", False), ("all_arrived_early", True)} <= seen


def test_result_from_outputs_edges():
    inf = M.INF_BITS
    # no samples at all: the script's loop body never runs
    r = result_from_outputs([0, -1, 0, 0, inf], [-1, -1])
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == (True, 0, None)
    assert np.isinf(r["min_pair_distance_m"]) and r["goal_reached_frac"] == 0.0
    # everybody arrives in the last sample: the walk runs out (True, ts)
    r = result_from_outputs([4, -1, 0, 0, inf], [3, 0])
    assert (r["instance_success"], r["makespan"]) == (True, 4)
    # arrival in sample 0, a sample follows: max(0, t - 1) = 0
    r = result_from_outputs([4, (2 << 40) | (0 << 20) | 1, 1, 0, M.bits(0.25)], [0, 0])
    assert (r["instance_success"], r["makespan"], r["first_collision"]) == (True, 0, None)
    assert r["first_collision_any"] == (2, 0, 1) and r["min_pair_distance_m"] == 0.5
    # the agents are a sub-range of the rows
    r = result_from_outputs([3, -1, 0, 0, inf], [-1, 1, 2, -1], agent_first=1, num_agents=2)
    assert (r["instance_success"], r["makespan"], r["goal_reached_frac"]) == (True, 3, 1.0)

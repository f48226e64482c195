"""CPU: what makes each input of exact_geometry_cases.py a case (test_gpu_exact_geometry.py runs
them on the device): the k-nearest cut falls inside a tie shell, a pair sits at exactly the radius
and two cells apart under a cell edge of exactly the radius, coincident agents overflow a bucket
and the candidate capacity, a 3 x 3 block reaches one bucket twice, no bearing is near the cone
edge, and the oracle gives sure verdicts on lists with duplicate and coincident neighbours."""
import collections

import numpy as np
import pytest

import exact_geometry_cases as X
import oracle_lib as O
from mpccbf import swarm
from parity_rule import check_parity


def _hist(rp):
    return dict(collections.Counter(np.diff(rp).tolist()))


def test_coordinates_are_dyadic():
    """Every coordinate of the exact cases is an integer multiple of 2^-5 below 2^9: squared
    distances need at most 30 bits, exact in double with any association or contraction."""
    tables = [X.tie_lattice()[0], X.shared_bucket()[0], X.tiny_single()[0], X.tiny_pair()[0],
              X.dependent_point()[0], X.dependent_lattice("shear")[0]]
    tables += [X.coincident(m)[0] for m in X.COINCIDENT_COUNTS]
    for st in tables:
        p = st[:, :2] * 32.0
        assert np.all(p == np.round(p)) and np.all(np.abs(st[:, :2]) < 512.0)


def test_tie_lattice_lists_and_cuts():
    st, _ = X.tie_lattice()
    assert st[:, :2].min() == -12.0 and st[:, :2].max() == 10.0
    # negative coordinates and agents exactly on cell edges (multiples of the radius)
    assert np.any(st[:, 0] < 0) and np.any(st[:, 0] % 4.0 == 0.0)
    hist = {q: _hist(X.reference_lists(f"tie_k{q[0]}_r{q[1]:g}")[0]) for q in X.TIE_QUERIES}
    assert hist[(1, 2.0)] == {1: 144}
    assert hist[(3, 2.0)] == {3: 140, 2: 4}
    assert hist[(6, 4.0)] == {6: 140, 5: 4}
    assert hist[(10, 4.0)] == {10: 100, 8: 32, 7: 8, 5: 4}
    assert hist[(16, 4.0)] == {12: 64, 11: 32, 10: 4, 8: 32, 7: 8, 5: 4}
    assert hist[(8, 4.0)] == {8: 132, 7: 8, 5: 4}
    # each tie query cuts a shell (k-th and (k+1)-th candidates at equal d2) at many agents; the
    # control and k = 16 (every candidate kept) cut none
    cut = {q: len(X.cuts_tie(st, *q)) for q in X.TIE_QUERIES}
    assert cut == {(1, 2.0): 144, (3, 2.0): 100, (6, 4.0): 140, (10, 4.0): 96, (16, 4.0): 0, (8, 4.0): 0}
    # (10, 4.0) cuts the shell at exactly the radius: an interior agent keeps 2 of its 4 at d2 = 16
    d2 = X.d2_matrix(st)
    rp, col = X.reference_lists("tie_k10_r4")
    i = 6 * 12 + 6
    row = col[rp[i]:rp[i + 1]]
    assert sorted(d2[i, row]) == [4.0] * 4 + [8.0] * 4 + [16.0] * 2
    at_r = np.nonzero(d2[i] == 16.0)[0]
    assert list(row[d2[i, row] == 16.0]) == list(at_r[:2])  # the two smallest indices
    # the subranges are inside the table
    for first, count in X.SUBRANGES:
        assert 0 <= first and first + count <= len(st)


@pytest.mark.parametrize("name", [p[0] for p in X.RADIUS_EDGE_PAIRS])
def test_radius_edge_pairs(name):
    """Each pair is listed by knn_csr (computed distance exactly the radius); the "miss" pairs
    have floor cells 2 apart under inv = 1.0 / radius, and at most 1 apart under the library's
    inv_cell; no coordinate is denormal; the six other agents are nowhere near the radius."""
    _, radius, axis, _, _, apart = next(p for p in X.RADIUS_EDGE_PAIRS if p[0] == name)
    st, _, r = X.radius_edge(name)
    assert r == radius
    a, b = st[0, axis], st[1, axis]
    assert min(abs(a), abs(b)) > 1.0  # ordinary magnitudes
    d = b - a
    assert abs(d) == radius and d * d <= radius * radius
    rp, col = X.reference_lists(f"edge_{name}")
    rows = X.csr_rows(rp, col)
    assert 1 in rows[0] and 0 in rows[1]
    assert abs(X.naive_cell(a, radius) - X.naive_cell(b, radius)) == apart
    assert abs(X.library_cell(a, radius) - X.library_cell(b, radius)) <= 1
    d2 = X.d2_matrix(st)
    off = d2[~np.eye(len(st), dtype=bool)]
    rest = np.sort(np.abs(off - radius * radius))
    assert rest[0] == 0.0 and rest[1] == 0.0 and rest[2] > 0.05 * radius * radius
    assert len(st) - 1 <= X.RADIUS_EDGE_K  # the cut never decides here: the radius alone does


def test_radius_edge_covers_the_radii():
    miss = collections.Counter(p[1] for p in X.RADIUS_EDGE_PAIRS if p[5] == 2)
    assert miss[5.0] >= 2 and miss[2.5] >= 1 and miss[10.0] >= 1
    assert {p[2] for p in X.RADIUS_EDGE_PAIRS if p[1] == 5.0 and p[5] == 2} == {0, 1}  # both axes
    assert any(float.fromhex(p[3]) < 0 for p in X.RADIUS_EDGE_PAIRS)  # mirrored to negative x


def test_cell_margin_bound():
    """The margin of the library's cell edge against its stated bound: with inv_cell =
    1 / (r (1 + 2^-20)), u = 2^-53 and |x| <= 2^30 r, the computed cell coordinates of two agents
    whose computed d2 is <= r^2 differ by at most (1 + 4u) / (1 + 2^-20) + 6u 2^30 <= 1."""
    from fractions import Fraction as F
    u, m = F(1, 2 ** 53), F(1, 2 ** 20)
    assert (1 + 4 * u) / (1 + m) + 6 * u * 2 ** 30 <= 1
    # and at the far end of the guarantee the reproducer's pattern is still at most a cell apart
    for radius in (2.5, 5.0, 10.0):
        for kk in (3, 2 ** 20 + 1, 2 ** 29 + 3):
            a = np.nextafter(kk * radius, 0.0)
            b = a + radius
            if (b - a) * (b - a) <= radius * radius:
                assert abs(X.library_cell(a, radius) - X.library_cell(b, radius)) <= 1


@pytest.mark.parametrize("m", X.COINCIDENT_COUNTS)
def test_coincident(m):
    st, _, who = X.coincident(m)
    k, r = X.COINCIDENT_QUERY
    assert len(st) == 81 and len(who) == m
    assert np.all(st[who, 0] == 0.5) and np.all(st[who, 1] == -0.25)
    assert who[-1] - who[0] > 40  # spread over the index range
    d2 = X.d2_matrix(st)
    assert np.all(d2[np.ix_(who, who)] == 0.0)
    rp, col = X.reference_lists(f"coincident_{m}")
    rows = X.csr_rows(rp, col)
    if m == 70:
        # one position holds more agents than a bucket has slots and than the query ranks at once
        assert m > X.GRID_CAP and m - 1 > X.NB_CAP
        cells = {(X.library_cell(x, r), X.library_cell(y, r)) for x, y in st[:, :2]}
        cx, cy = X.library_cell(0.5, r), X.library_cell(-0.25, r)
        assert all(abs(c[0] - cx) <= 1 and abs(c[1] - cy) <= 1 for c in cells)  # everyone reads it
        for i in who:  # index alone orders them: the 8 smallest other indices
            assert rows[i] == [j for j in who if j != i][:k]
    else:
        for i in who:
            assert all(j in rows[i] for j in who if j != i)
    assert len(X.cuts_tie(st, k, r)) >= 27


def test_shared_bucket():
    st, _ = X.shared_bucket()
    k, r = X.SHARED_QUERY
    hs = X.block_hashes(*X.SHARED_CELL)
    twice = {h for h in hs if hs.count(h) == 2}
    assert len(set(hs)) == 7 and len(twice) == 2
    # 756 of the 128 x 128 cells around the origin reach some bucket twice at mask 1023
    n = sum(len(set(X.block_hashes(cx, cy))) < 9 for cx in range(-64, 64) for cy in range(-64, 64))
    assert n == 756
    # agents whose query block is that cell's, and agents they list in a bucket read twice
    cells = [(X.library_cell(x, r), X.library_cell(y, r)) for x, y in st[:, :2]]
    assert cells == [(X.naive_cell(x, r), X.naive_cell(y, r)) for x, y in st[:, :2]]
    centre = [i for i, c in enumerate(cells) if c == X.SHARED_CELL]
    assert len(centre) == 4
    rp, col = X.reference_lists("shared_bucket")
    rows = X.csr_rows(rp, col)
    hit = sum(X.cell_hash(*cells[j], 1023) in twice for i in centre for j in rows[i])
    assert hit >= 4


def test_tiny():
    st, _, k, r = X.tiny_single()
    assert _hist(swarm.knn_csr(st, k, r)[0]) == {0: 1}
    st, _, k, r = X.tiny_pair()
    assert X.d2_matrix(st)[0, 1] == r * r and st[0, 0] < 0 < st[1, 0]
    assert X.csr_rows(*swarm.knn_csr(st, k, r)) == [[1], [0]]


def test_fov_lattice_cone_margin_and_cuts():
    st, _ = X.fov_lattice()
    cfg = swarm.fov_config(20)
    assert np.all(st[:, 2] == X.FOV_YAW)
    lo, hi = np.degrees(X.FOV_YAW - 0.5 * cfg["fov_beta"]), np.degrees(X.FOV_YAW + 0.5 * cfg["fov_beta"])
    assert abs(hi - 77.19) < 0.005 and abs(lo + 42.81) < 0.005
    for k, r in X.FOV_QUERIES:
        assert r == cfg["fov_Rs"]
        assert X.cone_margin(st, r, cfg["fov_beta"]) > 1e-6  # (measured: 0.0382 rad, the 45 degree bearings)
    cut = {q: len(X.cuts_tie(st, *q, cone=cfg["fov_beta"])) for q in X.FOV_QUERIES}
    assert cut[(4, 6.0)] >= 90 and cut[(5, 6.0)] >= 90 and cut[(8, 6.0)] == 0
    # a neighbour at exactly the radius, straight ahead in x, inside the cone
    rp, col = swarm.fov_csr(st, 8, 6.0, cfg["fov_beta"])
    i = 6 * 12 + 2
    assert i + 3 in col[rp[i]:rp[i + 1]] and st[i + 3, 0] - st[i, 0] == 6.0


def test_dependent_point_oracle_verdicts():
    """The oracle attempts both IMPC iterations of every list and returns OPTIMAL, OPTIMAL; a list
    with duplicates gives the result of its sorted unique list (measured: objective within 6e-9
    absolute, control points within 4.3e-6), and coincident neighbours that of one of them."""
    cfg = swarm.config(15)
    states, lists = X.dependent_point()
    assert np.all(states[1] == states[2])
    n = 36
    want = {"one": (-98.229119, -62.123255), "corner": (-196.458238, -124.263361)}
    for name, target, lst in lists:
        r = X.oracle_point(cfg, target, lst)
        assert r["attempted"] == 2 and list(r["status"]) == [O.OPTIMAL, O.OPTIMAL], (name, r["status"])
        for other in (X.unique_sorted(lst), X.collapsed(states, lst)):
            u = X.oracle_point(cfg, target, other)
            assert list(u["status"]) == [O.OPTIMAL, O.OPTIMAL]
            for k in (1, 2):  # the rule holds the last curve: over iteration 0 alone, then over both
                got = dict(status=np.array([r["status"][:k]]), obj=np.array([r["obj"][:k]]), x=np.array([r["x"][k - 1][:n]]))
                check_parity(got, [dict(status=u["status"][:k], obj=u["obj"][:k], x=u["x"][:k])], label=name)
        if name in want:
            np.testing.assert_allclose(r["obj"], want[name], atol=2e-6)
    # an active CBF row in iteration 0: without the neighbour the optimum is lower
    free = X.oracle_point(cfg, [3.0, 0.0, 0.0], [])
    assert free["obj"][0] < X.oracle_point(cfg, [3.0, 0.0, 0.0], [1])["obj"][0] - 1.0
    # the corner holds two active rows: dropping either neighbour lowers the optimum
    both = X.oracle_point(cfg, [3.0, 3.0, 0.0], [1, 3])["obj"][0]
    assert X.oracle_point(cfg, [3.0, 3.0, 0.0], [1])["obj"][0] < both - 1.0
    assert X.oracle_point(cfg, [3.0, 3.0, 0.0], [3])["obj"][0] < both - 1.0


@pytest.mark.parametrize("kind", ["shear", "centre"])
def test_dependent_lattice_oracle_verdicts(kind):
    """Sure verdicts only: no UNKNOWN for an attempted QP (UNKNOWN marks the iteration the loop
    never attempted after an INFEASIBLE one)."""
    cfg = swarm.config(15)
    st, tg, rp, col = X.dependent_lattice(kind)
    assert np.all(np.diff(st[:8, 0]) == cfg["d_min"])
    res = X.oracle_agents(cfg, st, tg, rp, col, range(64), key=("lattice", kind))
    for r in res:
        for it in range(2):
            assert (r["status"][it] == O.UNKNOWN) == (it >= r["attempted"]), r["status"]
            if it < r["attempted"]:
                assert r["status"][it] in (O.OPTIMAL, O.INFEASIBLE)
    verdicts = collections.Counter(tuple(int(v) for v in r["status"]) for r in res)
    if kind == "shear":
        assert verdicts == {(O.OPTIMAL, O.OPTIMAL): 16, (O.OPTIMAL, O.INFEASIBLE): 48}
        # every agent has an active CBF row in iteration 0: without neighbours its optimum is lower
        none = X.oracle_agents(cfg, st, tg, np.zeros(65, np.int32), np.zeros(0, np.int32), range(64))
        assert all(f["obj"][0] < r["obj"][0] - 1e-3 for f, r in zip(none, res))
    else:
        assert verdicts == {(O.OPTIMAL, O.OPTIMAL): 25, (O.INFEASIBLE, O.UNKNOWN): 39}

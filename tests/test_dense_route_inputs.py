"""The inputs of test_gpu_dense_routes.py, checked on the CPU alone: with the oracle's dense solver,
that every QP has the status and the property its GPU test relies on (reduced dimension, active
rows at the optimum, constant rows in the equalities' row space), and, for predicted_route (the
restatement of the host's launch rules in dense_route_cases.py), that the calls between them take
every route and that the rules are the host's own: predicted_route against the route that
tools/dense_route_check.cpp prints from csrc/host/dense_route.hpp, field by field."""
import os
import re
import subprocess

import numpy as np
import pytest

import dense_route_cases as C
import oracle_lib as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "mpc-cbf_amd", "build", "dense_route_check")
KKT = 1e-9


def _optimal(q):
    r = C.oracle_result(q)
    assert r["status"] == O.OPTIMAL, r["status"]
    assert np.max(r["kkt"]) <= KKT, r["kkt"]
    return r


def _infeasible(q):
    assert C.oracle_result(q)["status"] == O.INFEASIBLE


def test_group1_reduced_dimensions(oracle):
    g = C.group1()
    assert [nz for nz, _ in g] == [1, 2, 3, 4, 5, 6, 7, 8, 8, 1]
    for nz, q in g:
        assert C.reduced_dimension(q) == nz
        assert C.plan(q)["mi"] == 10
        _optimal(q)
    assert g[8][1]["c"].shape[0] == 64 and C.plan(g[8][1])["me"] == 56  # no padding at 64 variables
    nz, q = g[9]
    assert nz == 1 and len(C.active_rows(q, _optimal(q)["x"])) == 1  # the interval's end point
    r = C.predicted_route([q for _, q in g])
    assert r["R"] == 1 and r["active_set"] and r["early_exit"] and len(r["slices"]) == 1


def test_group2_row_edges_take_their_routes(oracle):
    got = []
    for mi in C.ROW_EDGES:
        q = C.row_edge_qp(mi)
        assert "vlo" not in q and C.plan(q)["mi"] == mi and C.reduced_dimension(q) == 7
        _optimal(q)
        r = C.predicted_route([q])
        assert r["rows_max"] == mi
        got.append((r["R"], r["active_set"]))
    assert tuple(got) == C.ROW_EDGE_ROUTES == ((1, True), (2, True), (2, True), (4, True), (4, True), (4, False),
                                                (4, False))
    assert C.plan(C.row_edge_qp(257))["mi"] == 257


def test_group2_constant_rows(oracle):
    cr = C.constant_rows()
    base, wc, bad = cr["base"], cr["with_const"], cr["violated"]
    assert C.plan(base)["mi"] == 240 and C.plan(wc)["mi"] == 300 and wc["A"].shape[0] == 305
    assert cr["const_idx"] == list(range(0, 300, 5))
    # a constant row in each of the five 64-row chunks, kept rows before and after each boundary
    assert sorted({k // 64 for k in cr["const_idx"]}) == [0, 1, 2, 3, 4]
    E, b, _, _, _ = C.split_rows(base)
    rows = wc["A"][5:][cr["const_idx"]]
    fit = np.linalg.lstsq(E.T, rows.T, rcond=None)[0]
    assert np.max(np.abs(E.T @ fit - rows.T)) <= 1e-12  # in the equalities' row space
    val = cr["combos"] @ b
    lo, hi = wc["lo"][5:][cr["const_idx"]], wc["hi"][5:][cr["const_idx"]]
    assert np.all(lo < val - 0.4) and np.all(hi > val + 0.4)  # satisfied, far from the tolerance
    rb, rc = _optimal(base), _optimal(wc)
    assert np.max(np.abs(rb["x"] - rc["x"])) <= 1e-9 and abs(rb["obj"] - rc["obj"]) <= 1e-9
    _infeasible(bad)
    changed = np.nonzero((bad["lo"] != wc["lo"]) | (bad["hi"] != wc["hi"]))[0]
    assert len(changed) == 1 and (changed[0] - 5) in cr["const_idx"]
    assert abs(bad["lo"][changed[0]] - val[(changed[0] - 5) // 5] - 1e-3) <= 1e-12
    r = C.predicted_route([wc])
    assert r["rows_max"] == 256 and r["R"] == 4 and not r["active_set"]


def test_group2_zero_rows(oracle):
    z = C.zero_rows()
    assert C.plan(z["dropped"])["mi"] == 65 and C.plan(z["infeasible"])["mi"] == 65
    assert not z["dropped"]["A"][35].any() and z["dropped"]["lo"][35] < 0 < z["dropped"]["hi"][35]
    assert z["infeasible"]["lo"][35] == 1.0
    rb, rd = _optimal(z["base"]), _optimal(z["dropped"])
    assert np.max(np.abs(rb["x"] - rd["x"])) <= 1e-9
    _infeasible(z["infeasible"])


def test_group3_base_set(oracle):
    base = C.base16()
    assert len(base) == 16
    vertex = 0
    dims = set()
    for k, q in enumerate(base[:14]):
        n, me, mi, _ = C.BASE_SHAPES[k]
        p = C.plan(q)
        assert (p["n"], p["me"], p["mi"]) == (n, me, mi) and 6 <= n <= 40 and mi <= 60
        nz = C.reduced_dimension(q)
        assert nz == n - me and 2 <= nz <= 8
        dims.add(nz)
        assert np.min(np.linalg.eigvalsh(q["H"])) > 0.05  # strictly convex
        r = _optimal(q)
        vertex += len(C.active_rows(q, r["x"])) == nz
    assert dims == {2, 3, 4, 5, 6, 7, 8}
    assert vertex >= 4
    assert any(C.plan(q)["mi"] == 0 for q in base[:14])
    _infeasible(base[C.BASE_INFEASIBLE])
    sd = base[C.BASE_SEMIDEFINITE]
    assert np.min(np.linalg.eigvalsh(sd["H"])) == 0.0
    r = _optimal(sd)
    assert np.max(np.abs(r["x"] - C.semidefinite_box_optimum(sd))) <= 1e-9
    for q in C.route_extras().values():
        _optimal(q)


def test_group3_calls_take_their_routes():
    calls = C.route_calls()
    route = {k: C.predicted_route(v[0]) for k, v in calls.items()}
    assert [len(calls[k][0]) for k in "abcde"] == [16, 17, 17, 65, 1027]
    assert [(route[k]["R"], route[k]["active_set"], route[k]["early_exit"]) for k in "abcde"] == [
        (1, True, True), (2, True, True), (4, False, False), (1, True, False), (1, True, False)]
    e = route["e"]
    assert [(s[0], s[1]) for s in e["slices"]] == [(0, 257), (257, 514), (514, 771), (771, 1027)]
    # per-slice LDS geometry and staging: only the third slice holds the 64-variable QP
    assert [s[2:] for s in e["slices"]] == [(40, 41, True), (40, 41, True), (64, 65, False), (40, 41, True)]
    assert e["host_reduced"] == [C.E_N80_AT] and calls["e"][1][C.E_N64_AT] == "n64"
    tags = calls["e"][1]
    for q0, q1, *_ in e["slices"]:  # every base QP in every slice
        assert set(range(16)) <= set(tags[q0:q1])
    for k in "abcd":
        assert len(route[k]["slices"]) == 1 and not route[k]["host_reduced"]
    # within a call the copies of a base QP are one object (one oracle solve each)
    qps = calls["e"][0]
    assert len({id(q) for q in qps}) == 18


def test_group4_degenerate_optima(oracle):
    d = C.degenerate()
    rs, rt = _optimal(d["single"]), _optimal(d["tripled"])
    assert np.max(np.abs(rs["x"] - rt["x"])) <= 1e-9
    act = C.active_rows(d["tripled"], rt["x"])
    assert len(act) == 3 * len(C.active_rows(d["single"], rs["x"])) > C.reduced_dimension(d["tripled"])
    assert all(a // 3 * 3 + j in act for a in act for j in range(3))  # repeated active rows
    rc = _optimal(d["corner"])
    assert np.max(np.abs(rc["x"] - 1.0)) <= 1e-9 and abs(rc["obj"] - 6.0) <= 1e-9
    assert len(C.active_rows(d["corner"], np.ones(6))) == 26 > 6  # 6 bounds + 20 rows through the corner
    # UNBOUNDED by construction (the oracle does not decide it): a recession direction
    u = d["unbounded"]
    dd = C.recession_direction(u)
    assert not (u["H"] @ dd).any() and u["c"] @ dd < -0.1 and np.all(u["A"] @ dd <= 1e-15)
    assert np.all(u["A"] @ np.zeros(6) <= u["hi"])  # feasible
    assert C.reduced_dimension(u) == 6
    _infeasible(d["infeasible200"])
    # the PDIP's own cases at R = 2: a semidefinite H (never the active set's) with a unique optimum
    # (the oracle's KKT point; as many active rows as dimensions), and an INFEASIBLE QP
    s = d["semidefinite100"]
    assert np.min(np.linalg.eigvalsh(s["H"])) == 0.0 and C.plan(s)["mi"] == 100
    assert len(C.active_rows(s, _optimal(s)["x"])) >= 3  # the three flat directions are held by rows
    _infeasible(d["infeasible100"])
    route = {k: C.predicted_route([q]) for k, q in d.items()}
    for k in ("semidefinite100", "infeasible100"):
        assert (route[k]["rows_max"], route[k]["R"], route[k]["active_set"]) == (100, 2, True)
    assert (route["tripled"]["R"], route["tripled"]["active_set"]) == (2, True)
    assert (route["infeasible200"]["R"], route["infeasible200"]["active_set"]) == (4, False)
    assert route["corner"]["early_exit"] and route["unbounded"]["R"] == 1


def test_group5_failing_calls():
    f = C.failing_calls()
    assert len(f["invalid"]) == 1027 and len(f["capacity"]) == 16
    bad = [k for k, q in enumerate(f["invalid"]) if np.isnan(q["c"]).any()]
    assert bad == list(C.BAD_AT) == [300, 900]
    s = C.predicted_route(f["invalid"])["slices"]
    assert s[1][0] <= 300 < s[1][1] and s[3][0] <= 900 < s[3][1]  # the second and the fourth slice
    assert [k for k, q in enumerate(f["capacity"]) if C.plan(q)["mi"] > 256] == [C.CAP_AT]


def _gpu_test_calls():
    calls = [[q for _, q in C.group1()]] + [[C.row_edge_qp(mi)] for mi in C.ROW_EDGES]
    calls += [[C.constant_rows()["with_const"]], [C.zero_rows()["dropped"]]]
    calls += [v[0] for v in C.route_calls().values()] + [[q] for q in C.degenerate().values()]
    return calls


def test_every_route_is_taken():
    """Every route the host can choose is taken by at least one call of the GPU tests."""
    calls = _gpu_test_calls()
    routes = [C.predicted_route(c) for c in calls]
    assert {(r["R"], r["active_set"]) for r in routes} == {(1, True), (2, True), (4, True), (4, False)}
    assert {len(r["slices"]) for r in routes} == {1, 4}
    assert {s[4] for r in routes for s in r["slices"]} == {True, False}
    assert any(r["early_exit"] for r in routes)
    # launches after the active-set launch: count > 64, and a host-reduced QP in the batch
    assert any(r["active_set"] and not r["early_exit"] and not r["host_reduced"] for r in routes)
    assert any(r["active_set"] and r["host_reduced"] for r in routes)


def _program(text=""):
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} not built (make -C mpc-cbf_amd)")
    r = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def _program_routes(calls):
    """dense_route_check on lists of shapes: (its limits, one route per call in predicted_route's form)."""
    text = "".join(f"{len(c)}\n" + "".join(f"{p['n']} {p['me']} {p['mi']} {p['nd']} {p['ni']} {int(p['cap'])}\n"
                                           for p in c) for c in calls)
    lines = _program(text)
    assert lines[0].startswith("limits ") and len(lines) == 1 + len(calls), lines[:2]
    limits = {k: int(v) for k, v in (f.split("=") for f in lines[0].split()[1:])}
    routes = []
    for ln in lines[1:]:
        f = dict(t.split("=") for t in ln.split()[1:])
        sl = [tuple(int(v) for v in s.split(":")) for s in f["slices"].split(";")]
        routes.append(dict(slices=[s[:4] for s in sl], slice_lds=[s[4:] for s in sl], rows_max=int(f["rows_max"]),
                           active_set=bool(int(f["active_set"])), R=int(f["R"]), early_exit=bool(int(f["early_exit"])),
                           host_reduced=[int(v) for v in f["host_reduced"].split(",") if v]))
    return limits, routes


def _shape(n=12, me=5, mi=10, nd=300, ni=60, cap=False):
    return dict(n=n, me=me, mi=mi, nd=nd, ni=ni, cap=cap)


def _edge_calls():
    """name -> shapes: a call at every edge of the route's rules (no QP behind them)."""
    calls = {f"count {c}": [_shape()] * c for c in (1, 64, 65, 1023, 1024, 1027)}
    calls.update({f"rows {m}": [_shape(mi=m)] for m in (64, 65, 128, 129, 192, 193, 256, 300)})
    # image (40 + 8) x 41 doubles = 15744 bytes; 4126 doubles + 100 ints staged: 49152 bytes in all
    calls["48 KB"] = [_shape(n=40, me=10, nd=4125, ni=99)]
    calls["48 KB + an int"] = [_shape(n=40, me=10, nd=4125, ni=100)]
    calls["48 KB + a double"] = [_shape(n=40, me=10, nd=4126, ni=99)]
    calls["n 64, me 1"] = [_shape(n=64, me=1)]
    calls["n 1, me 64"] = [_shape(n=1, me=64)]
    cap = _shape(n=80, me=70, mi=40, nd=0, ni=0, cap=True)
    calls["cap alone"] = [cap]
    calls["cap first in a slice"] = [_shape()] * 257 + [cap] + [_shape()] * 769
    calls["cap last in a call"] = [_shape()] * 1026 + [cap]
    calls["cap in a small call"] = [_shape()] * 15 + [cap]
    calls["only the host-reduced QP beyond 192 rows"] = [_shape(mi=192), dict(cap, mi=193)]
    calls["only the host-reduced QP beyond 128 rows"] = [_shape(mi=64), dict(cap, mi=129)]
    return calls


def test_predicted_route_is_the_programs_route():
    """predicted_route restates csrc/host/dense_route.hpp, which mpccbf_qp_solve_dense_batch follows:
    field by field against tools/dense_route_check.cpp (the header's own functions), for every call of
    the GPU tests and at every edge of the rules; the constants kept on the Python side against the
    limits the program prints."""
    calls = {f"gpu call {k}": [C.plan(q) for q in c] for k, c in enumerate(_gpu_test_calls())}
    calls.update(_edge_calls())
    limits, got = _program_routes(list(calls.values()))
    assert limits == dict(DENSE_NZ=C.DENSE_NZ, DENSE_ROWS=C.DENSE_ROWS, DENSE_NMAX=C.DENSE_NMAX,
                          DENSE_EMAX=C.DENSE_EMAX, ET_PAD=C.ET_PAD, DAS_ROWS=64 * C.WR, SLICE_COUNT=C.SLICE_COUNT,
                          MAX_SLICES=4, EARLY_COUNT=C.EARLY_COUNT, STAGE_BYTES=C.STAGE_BYTES, PACK_SPARE=1)
    assert C.WROWS == 64 * C.WR
    want = {}
    for (name, shapes), g in zip(calls.items(), got):
        w = want[name] = C.route_of_shapes(shapes)
        assert [s[:4] for s in w["slices"]] == g["slices"], name
        assert w["slice_lds"] == g["slice_lds"], name
        for key in ("rows_max", "active_set", "R", "early_exit", "host_reduced"):
            assert w[key] == g[key], (name, key, w[key], g[key])
    # the edges are edges: both sides of every comparison are among the calls
    assert [len(want[f"count {c}"]["slices"]) for c in (1023, 1024, 1027)] == [1, 4, 4]
    assert [want[f"count {c}"]["early_exit"] for c in (1, 64, 65)] == [True, True, False]
    assert [(want[f"rows {m}"]["R"], want[f"rows {m}"]["active_set"]) for m in (64, 65, 128, 129, 192, 193, 256, 300)] \
        == [(1, True), (2, True), (2, True), (4, True), (4, True), (4, False), (4, False), (4, False)]
    assert want["rows 300"]["rows_max"] == 256
    assert want["48 KB"]["slice_lds"] == [(C.STAGE_BYTES, 4126, 100)]
    assert want["48 KB + an int"]["slice_lds"] == want["48 KB + a double"]["slice_lds"] == [(15744, 0, 0)]
    assert want["n 64, me 1"]["slices"] == [(0, 1, 64, 65, True)] and want["n 1, me 64"]["slices"] == [(0, 1, 1, 65, True)]
    assert want["cap alone"]["slices"] == [(0, 1, 1, 1, True)] and want["cap alone"]["slice_lds"] == [(72, 0, 0)]
    assert want["cap alone"]["host_reduced"] == [0] and not want["cap alone"]["early_exit"]
    assert want["cap first in a slice"]["host_reduced"] == [257] and want["cap first in a slice"]["slices"][1][:2] == (257, 514)
    assert want["cap last in a call"]["host_reduced"] == [1026]
    assert want["cap in a small call"]["active_set"] and not want["cap in a small call"]["early_exit"]
    w = want["only the host-reduced QP beyond 192 rows"]
    assert (w["rows_max"], w["active_set"], w["R"]) == (193, False, 4)
    w = want["only the host-reduced QP beyond 128 rows"]
    assert (w["rows_max"], w["active_set"], w["R"]) == (129, True, 4)


def test_dense_route_check_checks_itself():
    """Without input the program checks the three buffers' layout (alignment, disjoint sections inside
    the reserved totals), the slices, the slot bounds against plan_qp's exact sizes and the
    host-reduced block by position."""
    last = _program()[-1]
    m = re.fullmatch(r"dense_route_check: (\d+) checks, 0 failures", last)
    assert m and int(m.group(1)) > 50000, last


@pytest.mark.parametrize("shape", [(6, 2, 5, 0, 0), (12, 5, 20, 0, 1), (20, 14, 0, 0, 3), (40, 33, 40, 2, 2)])
def test_plan_matches_the_packer_counts(shape):
    """plan() against the counts read off the QP directly: fixed variables are equality rows,
    redundant equalities count, dense rows have n nonzeros each."""
    n, me, mi, red, fx = shape
    q = C._random_qp(np.random.default_rng(5), *shape)
    p = C.plan(q)
    assert (p["n"], p["me"], p["mi"]) == (n, me + red + fx, mi) and not p["cap"]
    nh = n * (n + 1) // 2
    assert p["nh"] == nh and p["nd"] == n + 1 + nh + p["me"] + (me + red) * n + fx + 2 * mi + mi * n

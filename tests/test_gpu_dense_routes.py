"""The generic dense-QP path (mpccbf_qp_solve_dense_batch) on every launch route the host can
choose for a call — 1 or 4 pack / reduce slices with their own LDS geometry and staging, with and
without the dual active-set launch, dense_qp_kernel<8, 1 / 2 / 4>, the early exit after the active
set and the PDIP / expansion launches after it, host-reduced QPs in a large batch — and on the
row and dimension edges of the reduction: reduced dimension 1 .. 8, 64 .. 257 inequality rows,
constant rows dropped across the 64-row chunks of the compaction, degenerate optima. The route is
not observable from outside: it follows from the inputs by the host's rules, restated by
dense_route_cases.predicted_route and pinned with the inputs' properties on the CPU
(test_dense_route_inputs.py).

Against the oracle's dense solve of the same QP, at test_dense_qp.py's tolerances: statuses equal,
objective within 1e-6 max(1, |ref|), x within 1e-5; closed forms where they exist; copies of one QP
within a call and repeated calls bit for bit. Every QP of every call is compared.
"""
import numpy as np
import pytest

import dense_route_cases as C
from parity_rule import same_bits

pytestmark = pytest.mark.gpu


def _compare(mpclib, got, k, q, ref=None, where=""):
    """QP k of a call's result (st, xs, obj) against the oracle's solve of q (or of ref)."""
    st, xs, obj = got
    r = C.oracle_result(q if ref is None else ref)
    assert st[k] == r["status"], (where, k, st[k], r["status"])
    if r["status"] != mpclib.OPTIMAL:
        assert xs[k] is None and np.isnan(obj[k]), (where, k)
        return
    assert abs(obj[k] - r["obj"]) <= 1e-6 * max(1.0, abs(r["obj"])), (where, k, obj[k], r["obj"])
    assert xs[k].shape == r["x"].shape
    assert np.max(np.abs(xs[k] - r["x"])) <= 1e-5, (where, k, np.max(np.abs(xs[k] - r["x"])))


def _same_bits(a, b, what=""):
    """Two results of one QP (status, x or None, objective): bit-identical (NaN by bit pattern)."""
    assert a[0] == b[0] and (a[1] is None) == (b[1] is None), (what, a[0], b[0])
    same_bits(np.float64(a[2]), np.float64(b[2]), what=what)
    if a[1] is not None:
        same_bits(a[1], b[1], what=what)


def _qp(got, k):
    return got[0][k], got[1][k], got[2][k]


def _identical_calls(a, b):
    assert len(a[0]) == len(b[0])
    for k in range(len(a[0])):
        _same_bits(_qp(a, k), _qp(b, k), what=k)


def test_reduced_dimension_1_to_8(mpclib, oracle):
    """nz = 1 .. 8 at 12 variables, nz = 8 at 64 variables (no padding anywhere), nz = 1 with an
    active row, in one batch (R = 1, the active set, early exit possible)."""
    qps = [q for _, q in C.group1()]
    got = mpclib.dense_qp_solve_batch(qps)
    assert list(got[0]) == [mpclib.OPTIMAL] * len(qps)
    for k, q in enumerate(qps):
        _compare(mpclib, got, k, q, where="group1")


@pytest.mark.parametrize("mi", C.ROW_EDGES)
def test_row_count_edges(mpclib, oracle, mi):
    """64 .. 256 two-sided rows at nz = 7, a call each: dense_qp_kernel<8, 1 / 2 / 4> with the
    active-set launch up to 192 rows, without it beyond."""
    q = C.row_edge_qp(mi)
    got = mpclib.dense_qp_solve_batch([q])
    assert got[0][0] == mpclib.OPTIMAL
    _compare(mpclib, got, 0, q, where=f"mi={mi}")


def test_row_capacity_error(mpclib):
    with pytest.raises(mpclib.MpccbfError, match="QP 0: reduced rows exceed 256"):
        mpclib.dense_qp_solve_batch([C.row_edge_qp(257)])


def test_constant_rows_dropped_across_chunks(mpclib, oracle):
    """300 input rows, every 5th a satisfied constant row (a combination of the equality rows): the
    240 kept rows are compacted across every 64-row chunk boundary and the QP has the optimum of
    its 240-row form; with one constant row violated by 1e-3 it is INFEASIBLE."""
    cr = C.constant_rows()
    got = mpclib.dense_qp_solve_batch([cr["with_const"]])
    assert got[0][0] == mpclib.OPTIMAL
    _compare(mpclib, got, 0, cr["with_const"], ref=cr["base"], where="300 rows")
    plain = mpclib.dense_qp_solve_batch([cr["base"]])
    _compare(mpclib, plain, 0, cr["base"], where="240 rows")
    got = mpclib.dense_qp_solve_batch([cr["violated"]])
    assert got[0][0] == mpclib.INFEASIBLE and got[1][0] is None
    _compare(mpclib, got, 0, cr["violated"], where="violated")


def test_zero_rows(mpclib, oracle):
    """An all-zero row is a constant row: dropped when its bounds contain 0, INFEASIBLE otherwise."""
    z = C.zero_rows()
    got = mpclib.dense_qp_solve_batch([z["dropped"]])
    assert got[0][0] == mpclib.OPTIMAL
    _compare(mpclib, got, 0, z["dropped"], ref=z["base"], where="zero row")
    got = mpclib.dense_qp_solve_batch([z["infeasible"]])
    assert got[0][0] == mpclib.INFEASIBLE and got[1][0] is None
    _compare(mpclib, got, 0, z["infeasible"], where="zero row, lo = 1")


@pytest.fixture(scope="module")
def route_results(mpclib):
    """The five calls of the 16 base QPs, solved once each in the order a .. e."""
    return {name: mpclib.dense_qp_solve_batch(qps) for name, (qps, _) in C.route_calls().items()}


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_base_set_on_every_route(mpclib, oracle, route_results, name):
    """The 16 base QPs (14 strictly convex, one INFEASIBLE, one with a semidefinite H) as a call of
    16 (R = 1), with a 100-row QP (R = 2), with a 200-row QP (R = 4, no active set), tiled to 65
    (launches after the active set) and tiled to 1027 in shuffled order with a 64-variable QP in
    the third slice and a host-reduced 80-variable QP in the second (4 slices of different LDS
    geometry and staging): every QP of the call against the oracle, and all copies of one QP within
    the call bit-identical in status, x and objective, across slices too (same kernel, same packed
    words; the reduction's sums do not depend on the slice's LDS stride, dense_qp.hip col_dot_pad)."""
    qps, tags = C.route_calls()[name]
    got = route_results[name]
    assert len(got[0]) == len(qps)
    first = {}
    for k, (q, tag) in enumerate(zip(qps, tags)):
        _compare(mpclib, got, k, q, where=f"call {name}, base {tag}")
        if tag in first:
            _same_bits(_qp(got, first[tag]), _qp(got, k), what=(name, tag, first[tag], k))
        else:
            first[tag] = k
    assert got[0][tags.index(C.BASE_INFEASIBLE)] == mpclib.INFEASIBLE
    k = tags.index(C.BASE_SEMIDEFINITE)
    assert got[0][k] == mpclib.OPTIMAL
    np.testing.assert_allclose(got[1][k], C.semidefinite_box_optimum(qps[k]), atol=1e-7)


def test_base_set_statuses_identical_across_routes(mpclib, route_results):
    calls = C.route_calls()
    want = [int(s) for s in route_results["a"][0][:16]]
    assert sorted(set(want)) == [mpclib.OPTIMAL, mpclib.INFEASIBLE]
    for name, got in route_results.items():
        for k, tag in enumerate(calls[name][1]):
            if isinstance(tag, int):
                assert got[0][k] == want[tag], (name, k, tag)


def test_degenerate_optima(mpclib, oracle):
    """Rows repeated three times (R = 2, the active set on repeated active rows), a corner with 26
    active rows in 6 dimensions, an UNBOUNDED QP with rows at nz = 6, an INFEASIBLE one among 200
    rows and one among 100 (phase 1 in dense_qp_kernel<8, 4> and <8, 2>), a semidefinite H under
    100 rows (the PDIP itself at R = 2): a call each."""
    d = C.degenerate()
    for name in ("single", "tripled"):
        got = mpclib.dense_qp_solve_batch([d[name]])
        assert got[0][0] == mpclib.OPTIMAL
        _compare(mpclib, got, 0, d[name], where=name)
        _compare(mpclib, got, 0, d[name], ref=d["single"], where=name + " vs single")
    got = mpclib.dense_qp_solve_batch([d["corner"]])
    assert got[0][0] == mpclib.OPTIMAL
    np.testing.assert_allclose(got[1][0], np.ones(6), atol=1e-8)
    _compare(mpclib, got, 0, d["corner"], where="corner")
    got = mpclib.dense_qp_solve_batch([d["unbounded"]])
    assert got[0][0] == mpclib.UNBOUNDED and got[1][0] is None
    for name in ("infeasible200", "infeasible100"):
        got = mpclib.dense_qp_solve_batch([d[name]])
        assert got[0][0] == mpclib.INFEASIBLE and got[1][0] is None
        _compare(mpclib, got, 0, d[name], where=name)
    # the PDIP with the ridge on 100 rows (dense_qp_kernel<8, 2>: a semidefinite H is never the active set's)
    got = mpclib.dense_qp_solve_batch([d["semidefinite100"]])
    assert got[0][0] == mpclib.OPTIMAL
    _compare(mpclib, got, 0, d["semidefinite100"], where="semidefinite100")


def test_call_sequence_on_one_thread(mpclib, oracle):
    """The buffers kept across calls (pinned input and output, device blocks) and the error returns
    in mid-pipeline: a large call, a single QP, a small call, a call that fails in its second slice
    (invalid QPs 300 and 900 of 1027: the error names the first), a capacity error, then the small
    and the large call again, each bit for bit what it returned the first time."""
    calls = C.route_calls()
    big, small = calls["e"][0], calls["a"][0]
    fail = C.failing_calls()
    big1 = mpclib.dense_qp_solve_batch(big)
    st, x, obj = mpclib.dense_qp_solve(**C.toy())
    assert st == mpclib.OPTIMAL and abs(obj - 0.5) < 1e-8
    np.testing.assert_allclose(x, [0.5, 0.5], atol=1e-6)
    small1 = mpclib.dense_qp_solve_batch(small)
    with pytest.raises(mpclib.MpccbfError, match=r"QP 300: .*non-finite"):
        mpclib.dense_qp_solve_batch(fail["invalid"])
    with pytest.raises(mpclib.MpccbfError, match=f"QP {C.CAP_AT}: reduced rows exceed 256"):
        mpclib.dense_qp_solve_batch(fail["capacity"])
    small2 = mpclib.dense_qp_solve_batch(small)
    big2 = mpclib.dense_qp_solve_batch(big)
    for k, q in enumerate(small):
        _compare(mpclib, small1, k, q, where="small, first")
    for k, q in enumerate(big):
        _compare(mpclib, big1, k, q, where="large, first")
    _identical_calls(small1, small2)
    _identical_calls(big1, big2)


def test_fresh_thread_grows_every_buffer_from_nothing(mpclib, route_results):
    """The pinned input, the pinned output and the device block are kept per thread: on a fresh
    thread all three are empty, so the sequence one QP (n = 1, no rows: every section at its
    smallest), call d (65 QPs), call e (1027 QPs, 4 slices, one host-reduced), one QP again lays
    every section out at its smallest, grows each buffer twice and reuses it. The one-QP call
    against its closed form x = -c / (2 h), obj = -c^2 / (4 h) (this file's tolerances: x 1e-5,
    objective 1e-6); every call bit for bit what the main thread's call returned."""
    import threading
    calls = C.route_calls()
    h, c = 2.5, -3.0
    one = [dict(H=np.array([[h]]), c=np.array([c]))]
    order = (one, calls["d"][0], calls["e"][0], one)
    main_one = mpclib.dense_qp_solve_batch(one)
    got, err = [], []

    def worker():
        try:
            for qps in order:
                got.append(mpclib.dense_qp_solve_batch(qps))
        except BaseException as ex:  # (reported on the main thread)
            err.append(ex)

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert not err, err
    assert len(got) == 4
    for r in (main_one, got[0], got[3]):
        assert r[0][0] == mpclib.OPTIMAL
        assert abs(r[1][0][0] + c / (2.0 * h)) <= 1e-5 and abs(r[2][0] + c * c / (4.0 * h)) <= 1e-6
    _identical_calls(got[0], main_one)
    _identical_calls(got[3], main_one)
    _identical_calls(got[1], route_results["d"])
    _identical_calls(got[2], route_results["e"])

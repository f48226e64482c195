"""Inputs of test_gpu_dense_routes.py (pinned on the CPU by test_dense_route_inputs.py): seeded
dense QPs built so that the calls between them take every launch route of
mpccbf_qp_solve_dense_batch, and predicted_route(), a restatement in Python of the rules by which
the host chooses that route (csrc/host/dense_route.hpp, which dense_qp.hip follows):

  slices      4 pack / reduce slices when count >= 1024, else 1; each slice's reduce launch is sized
              by its own largest QP (LDS image rows and stride) and stages the packed QPs in LDS when
              image + the largest packed QP fit 48 KB;
  active set  the dual active-set launch runs when the batch's rows_max <= 192 (WROWS = 64 * WR);
  PDIP        dense_qp_kernel<8, R>, R = 1 / 2 / 4 for rows_max <= 64 / 128 / 256;
  early exit  possible (no PDIP and no expansion launch when the active set settles every QP) for
              count <= 64 without a host-reduced QP (more than 64 variables or equality rows).

rows_max is the largest *packed* inequality-row count of the call (rows of A with a finite side
and lo != hi, plus bounded variables), before the device drops constant rows: the row-count cases
use no variable bounds, so their mi is the number of such rows of A.

No GPU and no oracle at import; oracle_result() caches one oracle solve per distinct QP.
"""
from __future__ import annotations

import functools

import numpy as np

INF = np.finfo(np.float64).max  # numeric_limits<double>::max() as qpcpp::Problem uses it

# the host's constants (test_dense_route_inputs.py checks them against the limits dense_route_check prints)
WR = 3
WROWS = 64 * WR
DENSE_ROWS = 256
DENSE_NZ = 8
DENSE_NMAX = 64
DENSE_EMAX = 64
ET_PAD = 8
SLICE_COUNT = 1024   # count >= SLICE_COUNT: 4 slices
EARLY_COUNT = 64     # count <= EARLY_COUNT: the early exit's host check
STAGE_BYTES = 48 * 1024
K_INF = 1e300


def toy():
    # min x^2 + y^2  s.t.  x + y >= 1   (CPLEXTest.cpp:34-47)
    return dict(H=np.eye(2), c=np.zeros(2), A=np.array([[1.0, 1.0]]), lo=np.array([1.0]),
                hi=np.array([INF]))


def _random_qp(rng, n, me, mi, redundant=0, fixed=0):
    """A strictly convex QP with me equalities (redundant copies appended), mi two-sided rows
    and `fixed` fixed variables, feasible by construction around x0."""
    M = rng.standard_normal((n, n))
    H = M @ M.T / n + 0.1 * np.eye(n)
    c = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    E = rng.standard_normal((me, n))
    if redundant:
        E = np.vstack([E, rng.standard_normal((redundant, me)) @ E])
    G = rng.standard_normal((mi, n))
    gx = G @ x0
    A = np.vstack([E, G])
    lo = np.concatenate([E @ x0, gx - rng.uniform(0.05, 1.0, mi)])
    hi = np.concatenate([E @ x0, gx + rng.uniform(0.05, 1.0, mi)])
    vlo = np.full(n, -INF)
    vhi = np.full(n, INF)
    for i in range(fixed):
        vlo[i] = vhi[i] = x0[i]
    return dict(H=H, c=c, A=A, lo=lo, hi=hi, vlo=vlo, vhi=vhi, c0=0.25)


# ------------------------------------------------------------------------------------------------
# the host's rules
# ------------------------------------------------------------------------------------------------
def _fin(v):
    return np.isfinite(v) & (np.abs(v) < K_INF)


def plan(q):
    """dense_pack.hpp plan_qp: n, me, mi (packed rows), the packed sizes nd / ni, cap."""
    c = np.asarray(q["c"], dtype=np.float64)
    n = c.shape[0]
    H = np.asarray(q["H"], dtype=np.float64).reshape(n, n)
    A = np.asarray(q.get("A", np.zeros((0, n))), dtype=np.float64).reshape(-1, n)
    lo = np.asarray(q.get("lo", np.zeros(0)), dtype=np.float64)
    hi = np.asarray(q.get("hi", np.zeros(0)), dtype=np.float64)
    vlo = np.asarray(q["vlo"], dtype=np.float64) if q.get("vlo") is not None else np.full(n, -K_INF)
    vhi = np.asarray(q["vhi"], dtype=np.float64) if q.get("vhi") is not None else np.full(n, K_INF)
    hs = 0.5 * (H + H.T)
    nh = int(np.count_nonzero(np.triu(hs)))
    eq = _fin(lo) & (lo == hi)
    ine = ~eq & (_fin(lo) | _fin(hi))
    nnz = np.count_nonzero(A, axis=1) if A.shape[0] else np.zeros(0, dtype=int)
    veq = _fin(vlo) & (vlo == vhi)
    vin = ~veq & (_fin(vlo) | _fin(vhi))
    me = int(eq.sum() + veq.sum())
    mi = int(ine.sum() + vin.sum())
    enz = int(nnz[eq].sum() + veq.sum())
    inz = int(nnz[ine].sum() + vin.sum())
    cap = n > DENSE_NMAX or me > DENSE_EMAX
    ni = 4 + (mi + 1) + (2 * (me + 1) + 2 * nh + enz + inz + 3) // 4
    nd = n + 1 + nh + me + enz + 2 * mi + inz
    return dict(n=n, me=me, mi=mi, nh=nh, nd=nd, ni=ni, cap=cap)


def route_of_shapes(shapes):
    """The route of a call from its QPs' shapes alone (dicts with n, me, mi, nd, ni, cap, as plan()
    gives them; mi: the rows the route counts): predicted_route's dict, and under slice_lds, per
    slice, (dynamic LDS bytes, staged doubles, staged ints) of its reduce launch."""
    count = len(shapes)
    nslice = 4 if count >= SLICE_COUNT else 1
    step = (count + nslice - 1) // nslice
    rows_max = 1
    slices, slice_lds = [], []
    for q0 in range(0, count, step):
        q1 = min(count, q0 + step)
        nmax = emax = 1
        sd = si = 0
        for p in shapes[q0:q1]:
            if p["cap"]:
                continue
            nmax, emax = max(nmax, p["n"]), max(emax, p["me"])
            sd, si = max(sd, p["nd"] + 1), max(si, p["ni"] + 1)
        stride = max(nmax, emax) | 1
        lds = (nmax + ET_PAD) * stride * 8
        staged = lds + sd * 8 + si * 4 <= STAGE_BYTES
        slices.append((q0, q1, nmax, stride, staged))
        slice_lds.append((lds + sd * 8 + si * 4, sd, si) if staged else (lds, 0, 0))
    for p in shapes:
        rows_max = max(rows_max, min(p["mi"], DENSE_ROWS))
    big = [k for k, p in enumerate(shapes) if p["cap"]]
    das = rows_max <= WROWS
    return dict(slices=slices, slice_lds=slice_lds, rows_max=rows_max, active_set=das,
                R=1 if rows_max <= 64 else (2 if rows_max <= 128 else DENSE_ROWS // 64),
                early_exit=das and count <= EARLY_COUNT and not big, host_reduced=big)


def predicted_route(qps):
    """The route one mpccbf_qp_solve_dense_batch call on qps takes: dict with
    slices      [(q0, q1, lds_rows, lds_stride, staged)] per pack / reduce slice,
    rows_max    the call's largest packed inequality-row count (capped at 256; a host-reduced
                QP's packed count stands for its reduced one, an upper bound),
    active_set  whether the dual active-set launch runs,
    R           the PDIP instantiation's row slots per lane,
    early_exit  whether the early exit after the active-set launch is possible,
    host_reduced  indices of the QPs reduced on the host."""
    return route_of_shapes([plan(q) for q in qps])


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def oracle_form(q):
    """The dict oracle_lib.solve_dense_qp takes."""
    c = np.asarray(q["c"], dtype=np.float64)
    n = c.shape[0]
    return dict(n=n, H=0.5 * (np.asarray(q["H"]) + np.asarray(q["H"]).T), c=c, c0=q.get("c0", 0.0),
                A=q.get("A", np.zeros((0, n))), lo=q.get("lo", np.zeros(0)), hi=q.get("hi", np.zeros(0)),
                vlo=q["vlo"] if q.get("vlo") is not None else np.full(n, -INF),
                vhi=q["vhi"] if q.get("vhi") is not None else np.full(n, INF))


_ORACLE = {}


def oracle_result(q):
    """oracle_lib.solve_dense_qp(q), once per distinct QP object (the tiled calls repeat objects)."""
    import oracle_lib
    key = id(q)
    if key not in _ORACLE:
        _ORACLE[key] = (q, oracle_lib.solve_dense_qp(oracle_form(q)))  # (q kept alive: the id stays its own)
    return _ORACLE[key][1]


def split_rows(q):
    """(E, b, G, glo, ghi): the equality rows of A and the rest."""
    eq = q["lo"] == q["hi"]
    return q["A"][eq], q["lo"][eq], q["A"][~eq], q["lo"][~eq], q["hi"][~eq]


def active_rows(q, x, tol=1e-7):
    """Indices (into the inequality rows of A, then the bounded variables) of the rows active at x."""
    _, _, G, glo, ghi = split_rows(q)
    v = G @ x if G.shape[0] else np.zeros(0)
    act = list(np.nonzero((np.abs(v - glo) <= tol) | (np.abs(v - ghi) <= tol))[0])
    if q.get("vlo") is not None:
        vb = (np.abs(x - q["vlo"]) <= tol) | (np.abs(x - q["vhi"]) <= tol)
        act += [G.shape[0] + int(i) for i in np.nonzero(vb)[0]]
    return act


def reduced_dimension(q):
    E = split_rows(q)[0]
    n = q["c"].shape[0]
    return n - (np.linalg.matrix_rank(E) if E.shape[0] else 0)


def pushed(q, rng, scale):
    """q with a strong linear term along a random direction: its optimum moves to the boundary of
    the rows' polytope (a vertex, for a strong enough term)."""
    q = dict(q)
    q["c"] = q["c"] + scale * rng.standard_normal(q["c"].shape[0])
    return q


def semidefinite_box():
    """min x^T H x + c^T x, H = diag(1, 1, 1, 0, 0, 0), on [-1, 1]^6: positive semidefinite H (the
    positive-definiteness flag is 0: the PDIP with the ridge) with the unique optimum
    x = clip(-c / 2) on the first three coordinates and -sign(c) on the rest."""
    rng = np.random.default_rng(303)
    c = rng.standard_normal(6)
    c[3:] = np.sign(c[3:]) * (0.3 + np.abs(c[3:]))  # (away from 0: a unique optimum)
    return dict(H=np.diag([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]), c=c, A=np.zeros((0, 6)), lo=np.zeros(0),
                hi=np.zeros(0), vlo=np.full(6, -1.0), vhi=np.full(6, 1.0), c0=0.0)


def semidefinite_box_optimum(q):
    c = q["c"]
    return np.concatenate([np.clip(-c[:3] / 2.0, -1.0, 1.0), -np.sign(c[3:])])


# ------------------------------------------------------------------------------------------------
# group 1: reduced dimension 1 .. 8
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group1():
    """One batch: [(nz, qp)] — n = 12 with 11 .. 4 independent equalities (nz = 1 .. 8) and 10
    two-sided rows; nz = 8 at n = 64 with 56 equalities; nz = 1 with an active row."""
    rng = np.random.default_rng(101)
    out = [(12 - me, _random_qp(rng, 12, me, 10)) for me in range(11, 3, -1)]
    out.append((8, _random_qp(rng, 64, 56, 10)))
    out.append((1, pushed(_random_qp(rng, 12, 11, 10), rng, 100.0)))
    return out


# ------------------------------------------------------------------------------------------------
# group 2: row-count edges, constant rows
# ------------------------------------------------------------------------------------------------
ROW_EDGES = (64, 65, 128, 129, 192, 193, 256)
ROW_EDGE_ROUTES = ((1, True), (2, True), (2, True), (4, True), (4, True), (4, False), (4, False))  # (R, active set)


@functools.lru_cache(maxsize=None)
def row_edge_qp(mi):
    """nz = 7 (12 variables, 5 equalities), mi two-sided rows, no variable bounds. A call of its own."""
    q = _random_qp(np.random.default_rng(2000 + mi), 12, 5, mi)
    del q["vlo"], q["vhi"]
    return q


@functools.lru_cache(maxsize=None)
def constant_rows():
    """dict: base (240 rows), with_const (300 input rows, every 5th a constant row: a random
    combination of the equality rows, bounds value +- 0.5, so the device's compaction crosses every
    64-row chunk boundary), violated (one constant row's bounds moved to exclude its value by 1e-3),
    const_idx (the 60 positions), combos (60 x 5: the combinations)."""
    rng = np.random.default_rng(2300)
    base = _random_qp(rng, 12, 5, 240)
    del base["vlo"], base["vhi"]
    E, b, G, glo, ghi = split_rows(base)
    W = rng.standard_normal((60, E.shape[0]))
    rows, lo, hi, const_idx = [], [], [], []
    g = 0
    for k in range(300):
        if k % 5 == 0:
            j = k // 5
            const_idx.append(k)
            rows.append(W[j] @ E)
            lo.append(W[j] @ b - 0.5)
            hi.append(W[j] @ b + 0.5)
        else:
            rows.append(G[g])
            lo.append(glo[g])
            hi.append(ghi[g])
            g += 1
    assert g == 240
    with_const = dict(base, A=np.vstack([E, np.array(rows)]), lo=np.concatenate([b, lo]),
                      hi=np.concatenate([b, hi]))
    violated = dict(with_const, lo=with_const["lo"].copy(), hi=with_const["hi"].copy())
    j = 5 + const_idx[37]  # (a constant row in the third 64-row chunk)
    violated["lo"][j] = W[37] @ b + 1e-3
    violated["hi"][j] = W[37] @ b + 0.5
    return dict(base=base, with_const=with_const, violated=violated, const_idx=const_idx, combos=W)


@functools.lru_cache(maxsize=None)
def zero_rows():
    """dict: base (the 64-row QP), dropped (+ an all-zero row with bounds [-1, 2] after row 30),
    infeasible (the same row with lo = 1)."""
    base = row_edge_qp(64)
    A = np.insert(base["A"], 5 + 30, 0.0, axis=0)
    dropped = dict(base, A=A, lo=np.insert(base["lo"], 5 + 30, -1.0), hi=np.insert(base["hi"], 5 + 30, 2.0))
    infeasible = dict(dropped, lo=np.insert(base["lo"], 5 + 30, 1.0))
    return dict(base=base, dropped=dropped, infeasible=infeasible)


# ------------------------------------------------------------------------------------------------
# group 3: one set of 16 base QPs on every route
# ------------------------------------------------------------------------------------------------
# (n, equalities, two-sided rows, scale of the pushed linear term or 0)
BASE_SHAPES = ((6, 4, 8, 0.0), (8, 5, 12, 60.0), (10, 6, 20, 0.0), (12, 7, 30, 60.0), (16, 10, 40, 0.0),
               (20, 13, 60, 60.0), (24, 16, 50, 0.0), (20, 14, 0, 0.0), (30, 26, 16, 60.0), (36, 30, 24, 0.0),
               (40, 34, 20, 0.0), (32, 24, 30, 60.0), (14, 12, 10, 60.0), (28, 25, 18, 60.0))
BASE_INFEASIBLE = 14   # index in base16()
BASE_SEMIDEFINITE = 15


@functools.lru_cache(maxsize=None)
def base16():
    """14 strictly convex QPs (n 6 .. 40, nz 2 .. 8, at most 60 rows, one without inequality rows,
    the pushed ones with an optimum at a vertex of their rows), one INFEASIBLE by contradictory
    two-sided rows, one with a semidefinite H."""
    rng = np.random.default_rng(3000)
    qps = []
    for n, me, mi, push in BASE_SHAPES:
        q = _random_qp(rng, n, me, mi)
        qps.append(pushed(q, rng, push) if push else q)
    q = _random_qp(rng, 18, 12, 25)
    E, b, G, glo, ghi = split_rows(q)
    # (row 3 again, from its upper bound + 1 upwards: no point satisfies both)
    qps.append(dict(q, A=np.vstack([q["A"], G[3]]), lo=np.concatenate([q["lo"], [ghi[3] + 1.0]]),
                    hi=np.concatenate([q["hi"], [ghi[3] + 2.0]])))
    qps.append(semidefinite_box())
    return tuple(qps)


@functools.lru_cache(maxsize=None)
def route_extras():
    """dict: rows100 / rows200 (nz = 7: their presence moves the whole call to R = 2 / R = 4
    without the active set), n64 (64 variables, 58 equalities: the largest LDS image, not staged),
    n80 (80 variables, 74 equalities, 2 fixed variables: reduced on the host)."""
    rng = np.random.default_rng(3100)
    return dict(rows100=_random_qp(rng, 12, 5, 100), rows200=_random_qp(rng, 12, 5, 200),
                n64=_random_qp(rng, 64, 58, 30), n80=_random_qp(rng, 80, 74, 40, 0, 2))


E_COUNT = 1027
E_N80_AT = 300   # second slice [257, 514)
E_N64_AT = 600   # third slice [514, 771)


@functools.lru_cache(maxsize=None)
def route_calls():
    """The five calls: name -> (list of QPs, list of base index or extra's name per QP). The QPs of
    one base index within a call are the same object (oracle_result solves each once)."""
    base = base16()
    ex = route_extras()
    ids = list(range(16))
    calls = {"a": (list(base), ids), "b": (list(base) + [ex["rows100"]], ids + ["rows100"]),
             "c": (list(base) + [ex["rows200"]], ids + ["rows200"]),
             "d": ([base[k % 16] for k in range(65)], [k % 16 for k in range(65)])}
    order = np.random.default_rng(3200).permutation(E_COUNT - 2) % 16
    qps, tags = [], []
    it = iter(order)
    for k in range(E_COUNT):
        if k == E_N80_AT:
            qps.append(ex["n80"])
            tags.append("n80")
        elif k == E_N64_AT:
            qps.append(ex["n64"])
            tags.append("n64")
        else:
            j = int(next(it))
            qps.append(base[j])
            tags.append(j)
    calls["e"] = (qps, tags)
    return calls


# ------------------------------------------------------------------------------------------------
# group 4: degenerate optima for the active set
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate():
    """dict of QPs, each a call of its own: single / tripled (40 rows, each repeated three times: the
    same optimum), corner (min |x - 2|^2 on [-1, 1]^6 with 20 redundant rows through the optimal
    corner x = 1), unbounded (the semidefinite H with the one row sum(x) <= 3), infeasible200
    (200 rows, one of them a repeat of row 0 from its upper bound + 0.5 upwards), semidefinite100
    (the semidefinite H under 100 two-sided rows) and infeasible100 (as infeasible200, 100 rows)."""
    rng = np.random.default_rng(4000)
    single = pushed(_random_qp(rng, 12, 5, 40), rng, 30.0)
    del single["vlo"], single["vhi"]
    E, b, G, glo, ghi = split_rows(single)
    tripled = dict(single, A=np.vstack([E, np.repeat(G, 3, axis=0)]), lo=np.concatenate([b, np.repeat(glo, 3)]),
                   hi=np.concatenate([b, np.repeat(ghi, 3)]))
    W = rng.uniform(0.2, 1.0, (20, 6))
    # |x - 2|^2 = x^T x - 4 sum(x) + 24
    corner = dict(H=np.eye(6), c=np.full(6, -4.0), c0=24.0, A=W, lo=np.full(20, -INF), hi=W.sum(axis=1),
                  vlo=np.full(6, -1.0), vhi=np.full(6, 1.0))
    sd = semidefinite_box()
    unbounded = dict(H=sd["H"], c=sd["c"], c0=0.0, A=np.ones((1, 6)), lo=np.array([-INF]), hi=np.array([3.0]))
    q = _random_qp(rng, 12, 5, 199)
    del q["vlo"], q["vhi"]
    E, b, G, glo, ghi = split_rows(q)
    infeasible200 = dict(q, A=np.vstack([q["A"], G[0]]), lo=np.concatenate([q["lo"], [ghi[0] + 0.5]]),
                         hi=np.concatenate([q["hi"], [INF]]))
    # the PDIP itself on 65 .. 128 rows (the active set does not take a semidefinite H, and leaves
    # an INFEASIBLE QP to phase 1): dense_qp_kernel<8, 2> by value, not only after a settled batch
    G = rng.standard_normal((100, 6))
    x0 = rng.standard_normal(6)
    semidefinite100 = dict(H=sd["H"], c=sd["c"], c0=0.5, A=G, lo=G @ x0 - rng.uniform(0.05, 1.0, 100),
                           hi=G @ x0 + rng.uniform(0.05, 1.0, 100))
    q = _random_qp(rng, 12, 5, 99)
    del q["vlo"], q["vhi"]
    E, b, G, glo, ghi = split_rows(q)
    infeasible100 = dict(q, A=np.vstack([q["A"], G[0]]), lo=np.concatenate([q["lo"], [ghi[0] + 0.5]]),
                         hi=np.concatenate([q["hi"], [INF]]))
    return dict(single=single, tripled=tripled, corner=corner, unbounded=unbounded, infeasible200=infeasible200,
                semidefinite100=semidefinite100, infeasible100=infeasible100)


def recession_direction(q):
    """d with H d = 0, c.d < 0 and A d <= 0 for the unbounded QP: the tail of -c, made sum-free."""
    c = q["c"]
    d = np.zeros(6)
    d[3:] = -(c[3:] - c[3:].mean())
    return d


# ------------------------------------------------------------------------------------------------
# group 5: call sequences
# ------------------------------------------------------------------------------------------------
BAD_AT = (300, 900)  # NaN in c: the error names the first
CAP_AT = 5           # the 257-row QP's index in the batch of 16


@functools.lru_cache(maxsize=None)
def failing_calls():
    """dict: invalid (the 1027 call with a NaN in c at QPs 300 and 900), capacity (the 16 call with
    a 257-row QP at index 5)."""
    qps = list(route_calls()["e"][0])
    for k in BAD_AT:
        bad = dict(base16()[0])
        bad["c"] = bad["c"].copy()
        bad["c"][2] = np.nan
        qps[k] = bad
    cap = list(base16())
    cap[CAP_AT] = row_edge_qp(257)
    return dict(invalid=qps, capacity=cap)

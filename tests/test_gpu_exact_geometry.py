"""GPU: the neighbour queries against the CPU lists on exact geometry, and the solvers on
duplicate, coincident and mirror-symmetric neighbours (inputs: exact_geometry_cases.py, pinned on
the CPU by test_exact_geometry_inputs.py).

Four device queries share one contract (include/mpccbf.h, swarm.knn_csr / swarm.fov_csr): the knn_k
nearest others by planar distance, distance <= knn_radius inclusive, ties by agent index, sorted by
index, j != self — knn_query_kernel (mpccbf_build_neighbors), grid_neighbors_finish (16-lane,
dense and FoV kernels), grid_neighbors_stream (more than 64 candidates) and the one-agent-per-wave
kernel's query. Here mpccbf_batch.nb_out, the list a kernel actually used, is compared entry for
entry with the CPU list, where queries go wrong: the k-nearest cut inside a tie shell, a neighbour
at exactly the radius, agents on cell edges and at negative coordinates, coincident agents, a
bucket reached from two cells of the 3 x 3 block.

What it caught: the radius_edge pairs (test_nb_out_equals_cpu_lists[edge_*],
test_build_neighbors_equals_cpu_lists[edge_*]) failed with a cell edge of exactly knn_radius
(inv = 1.0 / radius): the rounded subtraction, reciprocal and products put two agents with computed
d2 <= r^2 two cells apart, and every query dropped the neighbour. The cell edge now carries a
margin (grid_inv_cell in kernels/impc.hpp).
"""
import functools

import numpy as np
import pytest

import exact_geometry_cases as X
import oracle_lib as O
from mpccbf import swarm
from gpu_harness import require_gpu, run_gpu, run_oracle, to_host
from parity_rule import ROUTE_REL, check_parity

pytestmark = pytest.mark.gpu

WIDE, DENSE64, DENSE16, SEP16 = "impc_wide_kernel<256>", "impc_kernel<6,64,1>", "impc_kernel<6,16,4>", \
    "impc_sep_kernel<1,1,false,256>"
# variant -> kernel at these sizes (variant 0, share-adaptive, is the one-agent-per-wave kernel)
KERNELS = {0: WIDE, 1: DENSE64, 3: DENSE16, 4: SEP16, 5: WIDE}
FOV_KERNELS = {0: "impc_fov_kernel<false>", 1: "impc_fov_kernel<true>"}
SENTINEL = -5

CASES = sorted(X.neighbour_cases())
SUB_QUERY = (10, 4.0)  # the subranges' query on tie_lattice: cuts the shell at exactly the radius


@functools.lru_cache(maxsize=None)
def _ctx(mpclib, variant, fov=False, slack=0):
    """One context per (controller, variant), shared by the tests (no store attached)."""
    if fov:
        cfg = swarm.fov_config(20, slack_mode=slack, slack_cost=1000.0, slack_decay_rate=0.5) if slack \
            else swarm.fov_config(20)
    else:
        cfg = swarm.config(15)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    return ctx


def _host(out):
    return to_host(out)


def _solve(ctx, states, targets, k=0, radius=0.0, rp=None, col=None, first=0, count=None):
    """One impc_solve of agents [first, first + count): grid mode (k, radius) or CSR lists (the
    agents' own rows). Returns host outputs with nb_out (initialised to SENTINEL) and the kernel."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    count = len(states) - first if count is None else count
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    tg = torch.tensor(np.ascontiguousarray(targets[first:first + count]), dtype=torch.float64, device=dev)
    out = ctx.alloc_outputs(count)
    nbo = torch.full((count, 16), SENTINEL, dtype=torch.int32, device=dev)
    if rp is None:
        ctx.impc_solve(st, targets=tg, agent_first=first, num_agents=count, knn_k=k, knn_radius=radius,
                       nb_out=nbo, **out)
    else:
        sub = np.asarray(rp[first:first + count + 1], dtype=np.int32)
        cl = np.asarray(col if len(col) else np.zeros(1), dtype=np.int32)
        ctx.impc_solve(st, torch.tensor(sub, device=dev), torch.tensor(cl, device=dev), targets=tg,
                       agent_first=first, num_agents=count, nb_out=nbo, **out)
    torch.cuda.synchronize()
    g = _host(out)
    g["nb_out"] = nbo.cpu().numpy()
    g["kernel"] = ctx.kernel_name
    return g


@functools.lru_cache(maxsize=None)
def _grid(mpclib, case, variant):
    """The grid-mode solve of a neighbour case (computed once, never modified)."""
    st, tg, k, r = X.neighbour_cases()[case]
    return _solve(_ctx(mpclib, variant), st, tg, k, r)


@functools.lru_cache(maxsize=None)
def _csr(mpclib, case, variant):
    """The CSR-mode solve of a neighbour case on the CPU lists, same context as _grid."""
    st, tg, _, _ = X.neighbour_cases()[case]
    rp, col = X.reference_lists(case)
    return _solve(_ctx(mpclib, variant), st, tg, rp=rp, col=col)


def _check_lists(nb_out, want, what):
    """nb_out equals the padded CPU lists entry for entry; no sentinel, no duplicate index."""
    assert not np.any(nb_out == SENTINEL), (what, "sentinel left")
    for a, row in enumerate(nb_out):
        kept = row[row >= 0]
        assert len(set(kept.tolist())) == len(kept), (what, a, row)
    bad = np.nonzero(np.any(nb_out != want, axis=1))[0]
    assert len(bad) == 0, (what, f"{len(bad)} agents differ, first {bad[0]}: device {nb_out[bad[0]]} "
                                 f"cpu {want[bad[0]]}")


def _check_same_solution(g, ref, what):
    """test_grid_neighbours_match_csr's criteria: statuses equal, objectives rtol 1e-10 / atol 1e-9."""
    np.testing.assert_array_equal(g["status"], ref["status"], err_msg=what)
    ok = ref["status"] == O.OPTIMAL
    np.testing.assert_allclose(g["obj"][ok], ref["obj"][ok], rtol=1e-10, atol=1e-9, err_msg=what)


@pytest.mark.parametrize("case", CASES)
def test_nb_out_equals_cpu_lists(mpclib, case):
    """nb_out of every collision kernel == swarm.knn_csr, entry for entry, rows padded with -1.
    Caught: the edge_* cases (all but the mirrored pair) lost the neighbour at exactly the radius
    in every variant while the cell edge was exactly the radius."""
    want = X.padded(*X.reference_lists(case))
    fails = []
    for variant, kernel in KERNELS.items():
        g = _grid(mpclib, case, variant)
        assert g["kernel"] == kernel, (variant, g["kernel"])
        try:
            _check_lists(g["nb_out"], want, (case, variant))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("first,count", X.SUBRANGES)
def test_nb_out_equals_cpu_lists_on_subranges(mpclib, first, count):
    """agent_first > 0: the batch's rows are the agents' own lists, indices into the whole table."""
    st, tg = X.tie_lattice()
    k, r = SUB_QUERY
    want = X.padded(*X.reference_lists(f"tie_k{k}_r{r:g}"), first=first, count=count)
    for variant, kernel in KERNELS.items():
        g = _solve(_ctx(mpclib, variant), st, tg, k, r, first=first, count=count)
        assert g["kernel"] == kernel, (variant, g["kernel"])
        _check_lists(g["nb_out"], want, (first, count, variant))


@pytest.mark.parametrize("slack", [0, 1])
@pytest.mark.parametrize("k,radius", X.FOV_QUERIES)
def test_fov_nb_out_equals_cpu_lists(mpclib, k, radius, slack):
    """The FoV kernels' query (grid_neighbors_finish with the cone filter) == swarm.fov_csr, and
    the grid path == the CSR path on those lists, with and without slack mode."""
    st, tg = X.fov_lattice()
    ctx = _ctx(mpclib, 0, fov=True, slack=slack)
    rp, col = swarm.fov_csr(st, k, radius, ctx.cfg["fov_beta"])
    g = _solve(ctx, st, tg, k, radius)
    assert g["kernel"] == FOV_KERNELS[slack]
    _check_lists(g["nb_out"], X.padded(rp, col), ("fov", k, slack))
    ref = _solve(ctx, st, tg, rp=rp, col=col)
    _check_lists(ref["nb_out"], X.padded(rp, col), ("fov csr", k, slack))
    _check_same_solution(g, ref, f"fov k={k} slack={slack}")


def _build(ctx, states, first, count, k, radius):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    n = len(states)
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    rp = torch.full((count + 1,), SENTINEL, dtype=torch.int32, device=dev)
    col = torch.full((max(1, count * (k if k > 0 else n - 1)),), SENTINEL, dtype=torch.int32, device=dev)
    ctx.build_neighbors(st, first, count, k, radius, rp, col)
    torch.cuda.synchronize()
    return rp.cpu().numpy(), col.cpu().numpy()


def _check_csr(got, want_rows, what):
    rp, col = got
    lens = [len(r) for r in want_rows]
    np.testing.assert_array_equal(rp, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), err_msg=str(what))
    flat = np.concatenate([np.asarray(r, np.int32) for r in want_rows]) if sum(lens) else np.zeros(0, np.int32)
    np.testing.assert_array_equal(col[:rp[-1]], flat, err_msg=str(what))


@pytest.mark.parametrize("case", CASES)
def test_build_neighbors_equals_cpu_lists(mpclib, case):
    """mpccbf_build_neighbors (knn_query_kernel): row_ptr and col == swarm.knn_csr. Caught: the
    edge_* cases, as test_nb_out_equals_cpu_lists."""
    st, _, k, r = X.neighbour_cases()[case]
    rows = X.csr_rows(*X.reference_lists(case))
    _check_csr(_build(_ctx(mpclib, 0), st, 0, len(st), k, r), rows, case)


@pytest.mark.parametrize("first,count", X.SUBRANGES + [(0, 144)])
def test_build_neighbors_subranges_and_all_others(mpclib, first, count):
    """The subranges of tie_lattice, and k <= 0: every other agent, in index order."""
    st, _ = X.tie_lattice()
    k, r = SUB_QUERY
    rows = X.csr_rows(*X.reference_lists(f"tie_k{k}_r{r:g}"))[first:first + count]
    ctx = _ctx(mpclib, 0)
    _check_csr(_build(ctx, st, first, count, k, r), rows, (first, count))
    others = [[j for j in range(len(st)) if j != i] for i in range(first, first + count)]
    for kk in (0, -1):
        _check_csr(_build(ctx, st, first, count, kk, r), others, (first, count, kk))


def test_build_neighbors_all_others_tiny(mpclib):
    ctx = _ctx(mpclib, 0)
    _check_csr(_build(ctx, X.tiny_single()[0], 0, 1, 0, 4.0), [[]], "single")
    _check_csr(_build(ctx, X.tiny_pair()[0], 0, 2, 0, 4.0), [[1], [0]], "pair")


@pytest.mark.parametrize("case", CASES)
def test_grid_path_equals_csr_path(mpclib, case):
    """The grid query's solve == the solve on the CPU lists given as CSR, same context, in every
    collision kernel (coincident agents may yield ERROR or INFEASIBLE: equal on both paths)."""
    for variant in KERNELS:
        g, ref = _grid(mpclib, case, variant), _csr(mpclib, case, variant)
        np.testing.assert_array_equal(ref["nb_out"], X.padded(*X.reference_lists(case)))
        _check_same_solution(g, ref, f"{case} variant {variant}")


def test_tie_control_matches_oracle(mpclib):
    """tie_lattice (8, 4.0), every 7th agent, against the oracle on the CPU lists."""
    cfg = swarm.config(15)
    st, tg = X.tie_lattice()
    case = f"tie_k{X.TIE_CONTROL[0]}_r{X.TIE_CONTROL[1]:g}"
    rp, col = X.reference_lists(case)
    agents = list(range(0, len(st), 7))
    ref = run_oracle(cfg, st, tg, rp, col, agents)
    assert not any(r["status"][it] == O.UNKNOWN for r in ref for it in range(r["attempted"]))
    for variant in KERNELS:
        check_parity(_grid(mpclib, case, variant), ref, agents)


@pytest.mark.parametrize("variant", [0, 3, 4])
def test_run_steps_nb_out_equals_lists_of_the_table_read(mpclib, variant):
    """Two closed-loop steps: the second reads the neighbour table the first step's kernel filled
    itself (grid_insert); its nb_out == knn_csr of the state table it read. Jittered on purpose:
    after one step the coordinates are no longer exact."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    states, targets = swarm.lattice_swarm(144)
    states[:, :2] *= 0.55
    ctx = _ctx(mpclib, variant)
    a = torch.tensor(states, device=dev)
    b = torch.full_like(a, float("nan"))
    nbo = torch.full((144, 16), SENTINEL, dtype=torch.int32, device=dev)
    out = ctx.alloc_outputs(144)
    r = ctx.run_steps(a, b, 2, targets=torch.tensor(targets, device=dev), knn_k=8, knn_radius=6.0,
                      x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"], nb_out=nbo)
    torch.cuda.synchronize()
    assert ctx.kernel_name == KERNELS[variant]
    assert r["final"] is a  # step 1 read b (step 0's next states) and wrote a
    table = b.cpu().numpy()
    assert np.all(np.isfinite(table)) and np.max(np.abs(table[:, :2] - states[:, :2])) > 1e-3
    _check_lists(nbo.cpu().numpy(), X.padded(*swarm.knn_csr(table, 8, 6.0)), ("run_steps", variant))


# ---------------------------------------------------------------------------------------------
# dependent_rows: duplicate, coincident and mirror-symmetric neighbours (CSR mode)
# ---------------------------------------------------------------------------------------------
DEP_VARIANTS = [0, 3, 4, 5]


def _point(ctx, target, lst):
    st, tg, rp, col = X.point_batch(target, lst)
    return _solve(ctx, st, tg, rp=rp, col=col, first=0, count=1)


def _sure(g):
    """No ERROR, and no UNKNOWN for an attempted QP (UNKNOWN only after an INFEASIBLE one)."""
    s = g["status"]
    assert not np.any(s == O.ERROR), s
    unk = s == O.UNKNOWN
    assert not np.any(unk[:, 0]) and np.all(s[unk[:, 1], 0] == O.INFEASIBLE), s


@pytest.mark.parametrize("variant", DEP_VARIANTS)
def test_duplicate_and_coincident_neighbours(mpclib, variant):
    """A list with duplicate or coincident entries returns what its sorted unique list (and the
    list with coincident neighbours collapsed to one) returns on the same device: equal statuses,
    objective within 1e-7 relative, control points within 1e-6 (test_wide_and_16lane_layouts_agree's
    bounds); both match the oracle on the unique list. Measured on an MI355X: identical (0.0 in
    objective and control points) in all four variants."""
    cfg = swarm.config(15)
    ctx = _ctx(mpclib, variant)
    states, lists = X.dependent_point()
    for name, target, lst in lists:
        g = _point(ctx, target, lst)
        np.testing.assert_array_equal(g["nb_out"][0, :len(lst)], lst)  # the list as given
        _sure(g)
        uniq = X.unique_sorted(lst)
        ref = [X.oracle_point(cfg, target, uniq)]
        for other in (uniq, X.collapsed(states, lst)):
            u = _point(ctx, target, other)
            _sure(u)
            what = (name, variant, other)
            np.testing.assert_array_equal(g["status"], u["status"], err_msg=str(what))
            ok = u["status"] == O.OPTIMAL
            assert ok.all(), what
            err = np.abs(g["obj"][ok] - u["obj"][ok]) / np.maximum(1.0, np.abs(u["obj"][ok]))
            dx = np.max(np.abs(g["x"] - u["x"]))
            print(f"{name} variant {variant} vs {other}: obj rel {err.max():.3e}, x {dx:.3e}")
            assert err.max() <= ROUTE_REL, (what, err.max())
            assert dx <= 1e-6, (what, dx)
            check_parity(u, ref, [0])
        check_parity(g, ref, [0])


@pytest.mark.parametrize("kind", ["shear", "centre"])
@pytest.mark.parametrize("variant", DEP_VARIANTS)
def test_symmetric_lattice_matches_oracle(mpclib, variant, kind):
    """An 8 x 8 lattice at spacing exactly d_min (mirror-symmetric neighbours, every pair on its
    CBF boundary): all 64 agents against the oracle, INFEASIBLE verdicts included."""
    cfg = swarm.config(15)
    st, tg, rp, col = X.dependent_lattice(kind)
    ref = X.oracle_agents(cfg, st, tg, rp, col, range(64), key=("lattice", kind))
    g = run_gpu(_ctx(mpclib, variant), st, tg, rp, col, require_gpu())
    _sure(g)
    check_parity(g, ref, list(range(64)))


@pytest.mark.parametrize("variant,kernel", [(4, "impc_sep_store_kernel<1,256,false>"),
                                            (5, "impc_wide_store_kernel<256>")])
def test_active_store_record_has_no_repeated_side(mpclib, variant, kernel):
    """With an active-set store attached, the exported record of a solve on [1, 1, 1, 1] and on
    the twins [1, 2] holds at most 5 sides and no key twice, and the solve is the oracle's."""
    torch = require_gpu()
    cfg = swarm.config(15)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    store = ctx.alloc_active_store(4)
    ctx.set_active_store(store)
    states, lists = X.dependent_point()
    for name, target, lst in lists:
        if name not in ("dup4", "twins"):
            continue
        store.zero_()
        g = _point(ctx, target, lst)
        assert g["kernel"] == kernel
        _sure(g)
        check_parity(g, [X.oracle_point(cfg, target, X.unique_sorted(lst))], [0])
        rec = store.cpu().numpy()[0]
        k = int(rec[0])
        keys = [int(v) for v in rec[1:1 + max(k, 0)]]
        print(f"{name} variant {variant}: record {rec.tolist()}")
        assert 0 <= k <= 5, rec
        assert len(set(keys)) == len(keys), rec
        mpclib.decode_active_sides(rec)  # every key decodes
    ctx.set_active_store(None)

"""The inputs of test_gpu_curve_shape.py, checked without a device: per case the oracle's status
mix (no attempted QP without a verdict, never all of one kind on the collision lattice), the live
iteration-1 CBF rows the capacity cases rely on, the host operators' sizes, and the kernel name the
launch plan gives for every variant the GPU test runs — so a GPU pass means what the case says
wherever it runs."""
import numpy as np
import pytest

import curve_shape_cases as S
import oracle_lib as O
import param_space_cases as P
from mpccbf import _lib, swarm
from mpccbf._lib import MpccbfError

OK, INF, UNK = O.OPTIMAL, O.INFEASIBLE, O.UNKNOWN

# the collision lattice: 14 agents stand so close to a neighbour that a CBF row of iteration 0
# excludes every acceleration of the box (in slack mode all 64 are OPTIMAL); from k_hor = 8 on one
# more agent's iteration 1 is infeasible
MIX_SHORT = {(OK, OK): 50, (INF, UNK): 14}
MIX = {(OK, OK): 49, (OK, INF): 1, (INF, UNK): 14}
MIX_C3 = {(OK, OK): 47, (OK, INF): 1, (INF, UNK): 16}
LATTICE_MIX = {"K1": MIX_SHORT, "K2": MIX_SHORT, "K3": MIX_SHORT, "c3K8": MIX_C3, "c3K16": MIX_C3}
# (largest live iteration-1 row count of an agent, agents with more than one live row)
LATTICE_LIVE = {"K1": (2, 4), "K2": (4, 31), "K3": (4, 31), "K8": (4, 29), "K11": (5, 29), "K14": (5, 29),
                "K16": (5, 29), "K17p4": (5, 29), "K20p4": (4, 29), "K21p4": (4, 29), "p1": (5, 29),
                "c3K8": (5, 26), "c3K16": (5, 27), "T037": (5, 29), "p5": (5, 29), "p6": (5, 29), "p10": (5, 29)}
# FoV swarm (scale 0.7, at most 3 observed neighbours): every QP OPTIMAL; agents whose curve a
# neighbour's rows move
FOV_MOVED = {"fovK2": 18, "fovK6": 23, "fovK12": 21, "fovK21": 22, "fovK12slack": 21, "fovK12c5": 21}

_res = {}


def oracle_res(c):
    if c.name not in _res:
        _res[c.name] = S.oracle_batch(c.cfg, *S.inputs(c))
    return _res[c.name]


def check_plan_and_sizes(c, csr=True):
    o = _lib.host_operators(c.cfg, keep_redundant=bool(c.opts.get("keep_redundant")))
    assert (o["m"], o["nz"], o["n"]) == c.sizes
    opts = {k: int(v) for k, v in c.opts.items()}
    for variant, name in (c.names or {}).items():
        p = _lib.host_launch_plan(c.cfg, variant=variant, num_agents=len(S.inputs(c)[0]), csr=csr, wide_max=1024,
                                  **opts)
        assert p["kernel_name"] == name, (c.name, variant, p["kernel_name"])
    return o


LATTICE_CASES = S.HORIZON + S.BEYOND16 + S.SHAPES


@pytest.mark.parametrize("c", LATTICE_CASES, ids=[c.name for c in LATTICE_CASES])
def test_collision_lattice_cases(oracle, mpclib, c):
    res = oracle_res(c)
    assert P.attempted_unknown(res) == []
    mix = P.status_mix(res)
    assert mix == LATTICE_MIX.get(c.name, MIX)
    assert mix[(OK, OK)] >= 40 and mix[(INF, UNK)] >= 10
    live = P.live_rows_it1(c.cfg, *S.inputs(c), res)
    assert (live.max(), int((live > 1).sum())) == LATTICE_LIVE[c.name]
    o = check_plan_and_sizes(c)
    # a forced 16-lane layout in these cases has the slots its agents need
    if c.names.get(3) == S.DENSE16:
        assert live.max() <= 64 - o["m"]
    if c.name in S.HOT:
        hot = _lib.host_launch_plan(c.cfg, variant=5, num_agents=64, csr=True)
        assert hot["hot"] == S.HOT[c.name] and hot["wide_capacity"] == 2048


def test_horizon_16_is_the_base_config():
    assert swarm.BASE_CONFIG["k_hor"] == 16 and S.config(16) == swarm.config(16)


def test_c3_rows_per_channel_are_uneven_at_k8(mpclib):
    """num_control_points = 3 at k_hor = 8: the x and y channels keep 3 box rows each and yaw 10."""
    o = _lib.host_operators(S.SHAPES[1].cfg)
    per = [int(np.count_nonzero(np.any(o["G"][:, 2 * d:2 * d + 2] != 0.0, axis=1))) for d in range(3)]
    assert S.SHAPES[1].name == "c3K8" and per == [3, 3, 10]


@pytest.mark.parametrize("c", S.SLACK_CASES, ids=[c.name for c in S.SLACK_CASES])
def test_slack_cases(oracle, mpclib, c):
    """Slack mode: every QP OPTIMAL where the plain controller's mix has 14 infeasible agents
    (the lattice cases above); 22 box rows per channel at k_hor = 21."""
    res = oracle_res(c)
    assert P.attempted_unknown(res) == [] and P.status_mix(res) == {(OK, OK): 64}
    check_plan_and_sizes(c)
    p = _lib.host_launch_plan(c.cfg, num_agents=64, csr=True)
    assert p["sep_rows_per_dim"] == {"slackK2": 3, "slackK16": 17, "slackK21p4": 22}[c.name]


FOV_ALL = S.FOV_CASES + [S.FOV_C5]


@pytest.mark.parametrize("c", FOV_ALL, ids=[c.name for c in FOV_ALL])
def test_fov_cases(oracle, mpclib, c):
    """The FoV swarm of test_refs_fov_and_slack_match_oracle: all 64 agents OPTIMAL in both
    iterations, and about a third of them with a neighbour's row active at the optimum (their curve
    differs from the one they plan alone) — not a set of unconstrained QPs."""
    res = oracle_res(c)
    assert P.attempted_unknown(res) == [] and P.status_mix(res) == {(OK, OK): 64}
    moved = S.moved_by_neighbours(c.cfg, *S.inputs(c), res)
    assert len(moved) == FOV_MOVED[c.name] and len(moved) >= 10
    assert np.diff(S.inputs(c)[2]).max() == 3
    check_plan_and_sizes(c)


@pytest.mark.parametrize("c", S.REFUSED, ids=[c.name for c in S.REFUSED])
def test_refused_shapes_have_no_kernel(mpclib, c):
    check_plan_and_sizes(c)
    assert c.sizes[1] not in (6, 15)


def test_continuity_degree_4_gives_the_operators_of_degree_3(mpclib):
    """The fourth derivative of a cubic piece is zero: continuity_upto_degree = 4 adds only zero
    rows to the equalities, and the condensed operators are those of degree 3, bit for bit."""
    a = _lib.host_operators(swarm.config(15))
    b = _lib.host_operators(swarm.config(15, continuity_upto_degree=4))
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("c", S.CAPACITY, ids=[c.name for c in S.CAPACITY])
def test_capacity_cases_exceed_the_16_lane_slots(oracle, mpclib, c):
    """Each capacity case has agents that stage more CBF rows than the 16-lane dense layout's
    64 - m slots, and the plan gives the default variant the 64-lane instantiation with caller
    lists (and variant 3 the 16-lane one it asks for)."""
    o = check_plan_and_sizes(c)
    slots16 = 64 - o["m"]
    opts = {k: int(v) for k, v in c.opts.items()}
    n = len(S.inputs(c)[0])
    assert _lib.host_launch_plan(c.cfg, variant=3, num_agents=n, csr=True, **opts)["kernel_name"] == S.DENSE16
    st, tg, rp, col = S.inputs(c)
    res = oracle_res(c)
    assert P.attempted_unknown(res) == []
    live = P.live_rows_it1(c.cfg, st, tg, rp, col, res)
    if c.swarm == "lattice":
        assert P.status_mix(res) == MIX
        if c.opts.get("no_cbf_filter"):
            # every CBF row is staged: neighbours x cbf_horizon in iteration 1 (7 or 8 neighbours)
            staged = np.diff(rp) * c.cfg["cbf_horizon"]
            assert slots16 == 13 and np.all(staged[[r["status"][0] == OK for r in res]] > slots16)
            assert sum(r["status"][0] == OK for r in res) == 50
        else:
            assert slots16 == 1 and (live.max(), int((live > slots16).sum())) == {"capK20p4": (4, 29),
                                                                                   "capK11keep": (5, 29)}[c.name]
    else:
        assert P.status_mix(res) == {(OK, OK): 1, (INF, UNK): 12} and list(res[0]["status"]) == [OK, OK]
        assert slots16 == 13 and live[0] == {2: 24, 8: 55}[c.cfg["cbf_horizon"]] and np.all(live[1:] == 0)
        assert live[0] <= 256 - o["m"]


def test_default_variant_keeps_the_16_lane_layout_where_its_slots_suffice(mpclib):
    """Grid lists bound an agent's rows by knn_k x cbf_horizon: at k_hor = 16 (m = 51, 13 slots) the
    default variant keeps impc_kernel<6,16,4> up to 6 nearest neighbours and takes the 64-lane one
    from 7 on and with caller lists; explicit variants keep what they ask for."""
    cfg = S.config(16)
    plan = lambda **kw: _lib.host_launch_plan(cfg, num_agents=64, **kw)["kernel_name"]  # noqa: E731
    assert [plan(knn_k=k) for k in (1, 6, 7, 8, 16)] == [S.DENSE16] * 2 + [S.DENSE64] * 3
    assert plan(csr=True) == S.DENSE64
    assert plan(variant=3, csr=True) == S.DENSE16 and plan(variant=3, knn_k=16) == S.DENSE16
    assert plan(variant=1, csr=True) == "impc_kernel<6,64,1>"
    # the separable kernels' choice (k_hor = 15) does not depend on the lists
    base = swarm.config(15)
    for kw in (dict(csr=True), dict(knn_k=8), dict(knn_k=16)):
        assert _lib.host_launch_plan(base, num_agents=64, **kw)["kernel_name"] == S.WIDE
        assert _lib.host_launch_plan(base, num_agents=2048, **kw)["kernel_name"] == S.SEP


def test_forced_16_lane_case(oracle, mpclib):
    c = S.FORCED16
    check_plan_and_sizes(c)
    assert c.cfg == S.CAPACITY[3].cfg and c.swarm == S.CAPACITY[3].swarm  # (the ring case's oracle results)


def test_range_edge_is_refused_by_operators_and_oracle(oracle, mpclib):
    """k_hor = 16 on ten pieces of 0.15: (K - 1) h = 1.5 passes swarm.validate's comparison with
    num_pieces x piece_max_parameter, but the curve's parameter range is the accumulated sum of the
    pieces, which ends just below 1.5 — the operators' build and the oracle both refuse the last
    sample, and the library's message says why."""
    cfg = swarm.config(**{**S.RANGE_EDGE, "spd_f": 8})
    with pytest.raises(MpccbfError) as e:
        _lib.host_operators(cfg)
    assert "out of range" in str(e.value), str(e.value)
    with pytest.raises(MpccbfError) as e:
        _lib.host_launch_plan(cfg, num_agents=64)
    assert "out of range" in str(e.value), str(e.value)
    st, tg, rp, col = S.lattice()
    with pytest.raises(RuntimeError):
        O.impc_optimize(O.make_params(cfg), st, 0, col[rp[0]:rp[1]], swarm.refs_from_targets(tg, 16)[0])
    # one sample fewer is inside the range for both
    assert _lib.host_operators(swarm.config(**{**S.RANGE_EDGE, "k_hor": 15}))["n"] == 120

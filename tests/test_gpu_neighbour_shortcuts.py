"""GPU: the 16-lane neighbour query's short cuts (grid_neighbors_finish, kernels/impc_common.hpp:
no ranking when no group of the wave has more than knn_k candidates, one candidate slot per lane
when none has more than 16) return the lists of the full ranking. nb_out, the list a kernel built
its rows from, is compared entry for entry with swarm.knn_csr on neighbour_shortcut_cases.py's swarm
(pinned on the CPU by test_neighbour_shortcut_inputs.py: candidate counts 0, 1, k - 1, k, k + 1, 16,
17 and 32, k = 1 and 16, waves that mix the branches, a tie shell cut at k + 1 candidates) in every
kernel that instantiates the 16-lane query — the separable kernel, the same with an active-set
store, the 16-lane dense kernel — and in the 64-lane dense kernel, which keeps the loop. One solve
is compared with the oracle under test_gpu_parity.py's rule."""
import functools

import numpy as np
import pytest

import exact_geometry_cases as X
import neighbour_shortcut_cases as S
import oracle_lib as O
from mpccbf import swarm
from gpu_harness import require_gpu, run_oracle, to_host
from parity_rule import check_parity

pytestmark = pytest.mark.gpu

SENTINEL = -5
# name -> (variant, active-set store attached, what the launched kernel's name starts with)
KERNELS = {"sep16": (4, False, "impc_sep_kernel<"), "sep16_store": (4, True, "impc_sep_store_kernel<"),
           "dense16": (3, False, "impc_kernel<6,16,"), "dense64": (1, False, "impc_kernel<6,64,")}


@functools.lru_cache(maxsize=None)
def _ctx(mpclib, name):
    variant, store, _ = KERNELS[name]
    ctx = mpclib.Context(swarm.config(15))
    ctx.set_variant(variant)
    if store:
        ctx.set_active_store(ctx.alloc_active_store(64))
    return ctx


def _solve(mpclib, name, states, targets, k, radius):
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    ctx = _ctx(mpclib, name)
    n = len(states)
    out = ctx.alloc_outputs(n)
    nbo = torch.full((n, 16), SENTINEL, dtype=torch.int32, device=dev)
    ctx.impc_solve(torch.tensor(states, dtype=torch.float64, device=dev),
                   targets=torch.tensor(targets, dtype=torch.float64, device=dev), knn_k=k, knn_radius=radius,
                   nb_out=nbo, **out)
    torch.cuda.synchronize()
    g = to_host(out)
    g["nb_out"] = nbo.cpu().numpy()
    g["kernel"] = ctx.kernel_name
    return g


@pytest.mark.parametrize("query", sorted(S.QUERIES))
def test_nb_out_equals_cpu_lists(mpclib, query):
    """nb_out == swarm.knn_csr entry for entry (rows padded with -1), no sentinel left, no index
    twice, in every kernel that shares the query."""
    k, r = query
    st, tg = S.shortcut_swarm()
    want = X.padded(*S.reference_lists(query))
    fails = []
    for name, (_, _, prefix) in KERNELS.items():
        g = _solve(mpclib, name, st, tg, k, r)
        assert g["kernel"].startswith(prefix), (name, g["kernel"])
        nb = g["nb_out"]
        if np.any(nb == SENTINEL):
            fails.append(f"{name}: sentinel left")
        for a, row in enumerate(nb):
            kept = row[row >= 0]
            if len(set(kept.tolist())) != len(kept):
                fails.append(f"{name}: agent {a} lists an index twice: {row}")
        bad = np.nonzero(np.any(nb != want, axis=1))[0]
        if len(bad):
            fails.append(f"{name}: {len(bad)} agents differ, first {bad[0]} (count "
                         f"{S.counts(st, r)[bad[0]]}): device {nb[bad[0]]} cpu {want[bad[0]]}")
    assert not fails, "\n".join(fails)


def test_solve_matches_oracle(mpclib):
    """The solve lattice (waves without a ranked group and waves that mix both), every agent,
    against the oracle on the CPU lists: parity_rule.check_parity's statuses and tolerances."""
    cfg = swarm.config(15)
    st, tg = S.solve_lattice()
    k, r = S.SOLVE_QUERY
    rp, col = swarm.knn_csr(st, k, r)
    agents = list(range(len(st)))
    ref = run_oracle(cfg, st, tg, rp, col, agents)
    assert not any(res["status"][it] == O.UNKNOWN for res in ref for it in range(res["attempted"]))
    for name in ("sep16", "dense16"):
        g = _solve(mpclib, name, st, tg, k, r)
        np.testing.assert_array_equal(g["nb_out"], X.padded(rp, col), err_msg=name)
        check_parity(g, ref, agents)

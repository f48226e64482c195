"""GPU: the launch clock (mpccbf_run::kernel_clock) where waves and agents do not line up, and the
device's answers against the host-only launch plan (mpccbf_host_launch_plan).

A kernel indexes the clock by block * (block size / 64) + wave with no bound of its own: the buffer
here is sized exactly launch_waves(n), so a launch whose grid disagrees with that count would write
outside it. Lane 0 of a wave writes its pair if and only if the wave's first group holds an agent,
so ceil(n / agents per wave) pairs are written."""
import numpy as np
import pytest

from conn_impc_cases import D_MAX
from gpu_harness import require_gpu
from mpccbf import swarm

pytestmark = pytest.mark.gpu

SEP, WIDE = "impc_sep_kernel<1,1,false,256>", "impc_wide_kernel<256>"
SLACK, SLACK32 = "impc_sep_kernel<1,2,true,256>", "impc_sep_kernel<2,2,true,128>"
CONN = "impc_sep_conn_kernel<4,64>"

# label: (configuration, variant, agents, agents per wave, waves, kernel, team of connectivity)
CASES = {
    "16-lane n=1": (swarm.config(15), 4, 1, 4, 4, SEP, None),
    "16-lane n=5": (swarm.config(15), 4, 5, 4, 4, SEP, None),
    "16-lane n=17": (swarm.config(15), 4, 17, 4, 8, SEP, None),
    "wide n=5": (swarm.config(15), 0, 5, 1, 8, WIDE, None),
    "slack K=15 n=5": (swarm.config(15, slack_mode=1), 0, 5, 4, 4, SLACK, None),
    "slack K=16 n=9": (swarm.config(16, slack_mode=1), 0, 9, 4, 4, SLACK32, None),  # two 128-thread blocks
    "connectivity n=5": (swarm.config(15), 0, 5, 4, 2, CONN, [0, 5]),
}


@pytest.mark.parametrize("label", list(CASES))
def test_clock_pairs_where_waves_and_agents_do_not_line_up(mpclib, label):
    torch = require_gpu()
    cfg, variant, n, per_wave, waves, kernel, team = CASES[label]
    dev = torch.device("cuda", 0)
    states, targets = swarm.lattice_swarm(n, seed=4)
    ctx = mpclib.Context(cfg)
    ctx.set_variant(variant)
    if team:
        ctx.set_connectivity(team, D_MAX)
    assert ctx.launch_waves(n) == waves
    tg = torch.tensor(targets, device=dev)
    a = torch.tensor(states, device=dev)
    kc = torch.zeros((1, waves, 2), dtype=torch.int64, device=dev)
    guard = torch.zeros((1, waves + 8, 2), dtype=torch.int64, device=dev)  # (a second run: what lies past the waves)
    for clock in (kc, guard):
        ctx.run_steps(a.clone(), torch.empty_like(a), 1, targets=tg, knn_k=8, knn_radius=6.0, kernel_clock=clock)
    torch.cuda.synchronize()
    assert ctx.kernel_name == kernel
    pairs = kc.cpu().numpy()[0]
    written = pairs[:, 1] != 0
    print(f"{label}: {int(written.sum())} of {waves} pairs written")
    assert written.sum() == -(-n // per_wave), pairs
    assert np.all(pairs[written, 1] > pairs[written, 0]) and np.all(pairs[~written] == 0)
    g = guard.cpu().numpy()[0]
    assert np.all(g[waves:] == 0) and np.array_equal(g[:waves, 1] != 0, written)
    with pytest.raises(mpclib.MpccbfError, match="kernel_clock_waves"):
        ctx.run_steps(a.clone(), torch.empty_like(a), 1, targets=tg, knn_k=8, knn_radius=6.0,
                      kernel_clock=torch.zeros((1, waves - 1, 2), dtype=torch.int64, device=dev))


@pytest.mark.parametrize("attach", ["plain", "store", "connectivity"])
def test_device_answers_equal_the_host_plan(mpclib, attach):
    """After one solve of 64 agents with the default variant: kernel_name and launch_waves are the
    host export's for this device's share-adaptive threshold (4 x its compute units)."""
    torch = require_gpu()
    dev = torch.device("cuda", 0)
    n, cfg = 64, swarm.config(15)
    states, targets = swarm.lattice_swarm(n, seed=4)
    ctx = mpclib.Context(cfg)
    if attach == "store":
        ctx.set_active_store(ctx.alloc_active_store(n))
    if attach == "connectivity":
        ctx.set_connectivity([0, 16, 32, 48, 64], D_MAX)
    out = ctx.alloc_outputs(n)
    ctx.impc_solve(torch.tensor(states, device=dev), targets=torch.tensor(targets, device=dev), knn_k=8,
                   knn_radius=6.0, **out)
    torch.cuda.synchronize()
    wide_max = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    plan = mpclib._lib.host_launch_plan(cfg, variant=0, num_agents=n, knn_k=8, store=attach == "store",
                                        connectivity=attach == "connectivity", wide_max=wide_max)
    assert ctx.kernel_name == plan["kernel_name"]
    assert ctx.launch_waves(n) == plan["clock_waves"] > 0
    if wide_max >= n:  # (an MI355X: 1,024)
        assert plan["kernel_name"] == {"plain": WIDE, "store": "impc_wide_store_kernel<256>", "connectivity": CONN}[attach]

"""CPU: what mpccbf_run_steps decides without a device, no GPU.

tools/run_owners_check.cpp drives the two owners behind the run loop (csrc/capi_run.hip):

GroupSync (csrc/host/group_sync.hpp), the in-process communicator group's barrier, abort rule and
num_steps agreement, from real threads in groups of 2, 3 and 8 ranks next to a per-generation
arrival count: thousands of consecutive barriers and back-to-back agreements with changing counts,
the zero-step call, an abort before the peers arrive, while they wait and between two barriers
(through a guard that leaves scope armed), and the parity slots of the group's device half with
integers in place of tables and events.

StepEvents (csrc/host/step_events.hpp), the layout of the timing events, for every num_steps 0..6,
reserve_steps 0..8, solve_stride 0..4 and step_ms / solve_ms given or not: the events the call
reads were recorded before the one it waits for, inside the pool, once each, in distinct roles,
with contiguous step intervals and the solve interval on the stride's steps only.

A rank that blocks is this test's timeout. tests/test_gpu_multirank.py and
tests/test_gpu_context_reuse.py hold the library to the same behaviour on the device."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "mpc-cbf_amd", "build", "run_owners_check")

GROUPS = (2, 3, 8)  # the group sizes of the program


def test_group_synchronisation_and_event_layout_hold_their_models():
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} not built (make -C mpc-cbf_amd)")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    m = re.fullmatch(r"run_owners_check: (\d+) barriers, (\d+) agreements, (\d+) aborted ranks, (\d+) slot reads, "
                     r"(\d+) event plans, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m, r.stdout[-500:]
    barriers, agreements, aborted, slot_reads, plans = map(int, m.groups())
    ranks = sum(GROUPS)
    assert agreements == 2000 * ranks
    assert barriers >= agreements + 2000 * ranks + 500 * ranks  # agreements, plain barriers, slot steps
    # three abort cases, each by the first and by the last rank: every other rank saw the failure
    assert aborted == 6 * (ranks - len(GROUPS))
    assert slot_reads == 500 * sum(n * (n - 1) for n in GROUPS)
    assert plans == 7 * 9 * 5 * 4

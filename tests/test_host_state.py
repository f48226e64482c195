"""CPU: the host state an IMPC step carries from call to call, no GPU.

tools/host_state_check.cpp drives the owners of that state — GridRotation (the neighbour-table
rotation and its continuation record, csrc/host/grid_rotation.hpp) and DeferQueues (the two
alternating deferral queues, csrc/host/defer_queues.hpp) — through every sequence of up to four
calls on one context (grid runs of 1 .. 3 steps with and without continue_tables, CSR runs, solves,
zero-step runs with and without a caller refill, a larger num_states, another knn_k or radius, a
main launch that fails, a table allocation that fails) next to a model of what the device buffers
hold, and asserts on the model: every step reads a table holding its states, inserts into a zeroed
one, no call continues across an invalidating event, every call that may continue does, and the
queue a launch appends to was zeroed. tests/test_gpu_context_reuse.py holds the library to the same
behaviour on the device."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "mpc-cbf_amd", "build", "host_state_check")

LETTERS = 16  # the call alphabet of the program


def test_every_short_call_sequence_keeps_the_tables_and_queues_sound():
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} not built (make -C mpc-cbf_amd)")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    m = re.fullmatch(r"host_state_check: (\d+) sequences, (\d+) steps, (\d+) continued, (\d+) rebuilt, "
                     r"(\d+) queue growths, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m, r.stdout[-500:]
    sequences, steps, continued, rebuilt, growths = map(int, m.groups())
    assert sequences == sum(LETTERS ** n for n in range(1, 5))
    # the sequences exercise both outcomes, and the queues grow (first use, then 1,025 agents)
    assert steps > sequences and continued > 0 and rebuilt > continued and growths > sequences

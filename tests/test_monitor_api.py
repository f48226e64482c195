"""CPU: the argument checks of mpccbf_monitor_reset / mpccbf_monitor_score / mpccbf_set_monitor (made
on the host before any device call, so they need no GPU), the header's declarations and the binding."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mpccbf import _lib

INVALID = -1  # MPCCBF_ERR_INVALID_ARGUMENT
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")
ROWS, SAMPLES = 8, 4


def _monitor(mpclib, **over):
    """A well-formed monitor over host memory: only ever handed to calls that must refuse it or that
    enqueue nothing."""
    L = mpclib.load()
    nbytes = int(L.mpccbf_monitor_scratch_bytes(ROWS, SAMPLES))
    keep = dict(summary=np.zeros(5, np.int64), reached_at=np.zeros(ROWS, np.int64), min_d2=np.zeros(ROWS),
                hit_samples=np.zeros(ROWS, np.int32), unsafe_samples=np.zeros(ROWS, np.int32),
                scratch=np.zeros(nbytes, np.uint8), sample_log=np.zeros((3, 3), np.int64))
    m = _lib.Monitor(shape_type=1, shape=(C.c_double * 2)(0.2, 0.2), d_min=1.0, goal_radius=1.0, watch_radius=0.0,
                     rows=ROWS, summary=keep["summary"].ctypes.data, reached_at=keep["reached_at"].ctypes.data,
                     min_d2=keep["min_d2"].ctypes.data, hit_samples=keep["hit_samples"].ctypes.data,
                     unsafe_samples=keep["unsafe_samples"].ctypes.data, sample_log=None, sample_log_rows=0,
                     scratch=keep["scratch"].ctypes.data, scratch_bytes=nbytes)
    for k, v in over.items():
        if k == "shape":
            v = (C.c_double * 2)(*v)
        setattr(m, k, v)
    m._keep = keep
    return m


STATES = np.zeros((ROWS, 6))


def _score(mpclib, m, **over):
    a = dict(samples=STATES.ctypes.data, num_samples=1, sample_stride=6, row_stride=6, agent_first=0,
             num_agents=ROWS, fixed_states=None, num_states=ROWS, goals=None, sample_first=0)
    a.update(over)
    return mpclib.load().mpccbf_monitor_score(
        None if m is None else C.byref(m), a["samples"], a["num_samples"], a["sample_stride"], a["row_stride"],
        a["agent_first"], a["num_agents"], a["fixed_states"], a["num_states"], a["goals"], a["sample_first"], 0, None)


BAD_MONITORS = [
    ("shape_type_2", dict(shape_type=2)),
    ("shape_type_negative", dict(shape_type=-1)),
    ("box_zero_extent", dict(shape=(0.2, 0.0))),
    ("box_negative_extent", dict(shape=(-0.2, 0.2))),
    ("box_nan_extent", dict(shape=(0.2, math.nan))),
    ("circle_zero_radius", dict(shape_type=0, shape=(0.0, 0.0))),
    ("circle_inf_radius", dict(shape_type=0, shape=(math.inf, 0.0))),
    ("d_min_zero", dict(d_min=0.0)),
    ("d_min_nan", dict(d_min=math.nan)),
    ("goal_radius_negative", dict(goal_radius=-1.0)),
    ("watch_below_d_min", dict(watch_radius=0.9)),
    ("watch_below_box_reach", dict(shape=(1.5, 1.5), watch_radius=4.0)),
    ("default_watch_below_circle_reach", dict(shape_type=0, shape=(2.0, 0.0))),
    ("watch_inf", dict(watch_radius=math.inf)),
    ("rows_zero", dict(rows=0)),
    ("null_summary", dict(summary=None)),
    ("null_reached_at", dict(reached_at=None)),
    ("null_min_d2", dict(min_d2=None)),
    ("null_hit_samples", dict(hit_samples=None)),
    ("null_unsafe_samples", dict(unsafe_samples=None)),
    ("null_scratch", dict(scratch=None)),
    ("sample_log_rows_negative", dict(sample_log_rows=-1)),
]


@pytest.mark.parametrize("name,over", BAD_MONITORS, ids=[b[0] for b in BAD_MONITORS])
def test_bad_monitors_are_refused_everywhere(mpclib, name, over):
    L = mpclib.load()
    m = _monitor(mpclib, **over)
    assert L.mpccbf_monitor_reset(C.byref(m), 0, None) == INVALID
    assert L.mpccbf_last_error().decode().startswith("monitor:")
    assert _score(mpclib, m) == INVALID
    # (checked before the context: a NULL context is only reported for a good monitor)
    assert L.mpccbf_set_monitor(None, C.byref(m)) == INVALID
    assert L.mpccbf_last_error().decode().startswith("monitor:")


def test_a_sample_log_needs_rows(mpclib):
    m = _monitor(mpclib)
    m.sample_log = m._keep["sample_log"].ctypes.data
    assert _score(mpclib, m) == INVALID
    assert _score(mpclib, m, num_samples=0) == INVALID


BAD_SCORES = [
    ("num_states_beyond_2_20", dict(num_states=(1 << 20) + 1, num_agents=0)),
    ("num_states_beyond_rows", dict(num_states=ROWS + 1, num_agents=0)),
    ("samples_beyond_2_23", dict(sample_first=(1 << 23) - 1, num_samples=2)),
    ("sample_first_below_minus_1", dict(sample_first=-2)),
    ("num_samples_negative", dict(num_samples=-1)),
    ("num_states_negative", dict(num_states=-1, num_agents=0)),
    ("num_agents_negative", dict(num_agents=-1)),
    ("agent_first_negative", dict(agent_first=-1)),
    ("agents_beyond_states", dict(agent_first=1)),
    ("scratch_too_small_for_the_samples", dict(num_samples=SAMPLES + 1)),
    ("null_samples", dict(samples=None)),
]


@pytest.mark.parametrize("name,over", BAD_SCORES, ids=[b[0] for b in BAD_SCORES])
def test_bad_scores_are_refused(mpclib, name, over):
    assert _score(mpclib, _monitor(mpclib), **over) == INVALID
    assert mpclib.load().mpccbf_last_error().decode().startswith("monitor:")


def test_scratch_is_checked_against_the_call(mpclib):
    m = _monitor(mpclib)
    m.scratch_bytes = int(mpclib.load().mpccbf_monitor_scratch_bytes(ROWS, 1)) - 1
    assert _score(mpclib, m) == INVALID
    assert _score(mpclib, None) == INVALID


def test_nothing_to_score_is_a_successful_no_op(mpclib):
    m = _monitor(mpclib)
    assert _score(mpclib, m, num_samples=0) == 0
    assert _score(mpclib, m, num_states=0, num_agents=0, samples=None) == 0
    assert _score(mpclib, m, sample_first=(1 << 23), num_samples=0) == 0
    # a good monitor and no context
    assert mpclib.load().mpccbf_set_monitor(None, C.byref(m)) == INVALID
    assert "context" in mpclib.load().mpccbf_last_error().decode()


def test_sizes(mpclib):
    import monitor_cases as M
    L = mpclib.load()
    for n in (0, 1, 70, 512, 513, 4096, 100000, 1 << 20):
        assert L.mpccbf_monitor_table_size(n) == M.table_size(n)
    sizes = [L.mpccbf_monitor_scratch_bytes(r, s) for r, s in ((8, 1), (8, 10), (4096, 1), (4096, 10))]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # per sample: the bucket counts, their starts, and three words per row
    T = M.table_size(4096)
    assert sizes[2] >= 4 * (2 * T + 1 + 3 * 4096)
    assert L.mpccbf_monitor_scratch_bytes((1 << 20) + 1, 1) == 0 and L.mpccbf_monitor_scratch_bytes(-1, 1) == 0


def test_header_declares_and_library_exports_the_monitor(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_MONITOR\s+1\b", text)
    assert re.search(r"#define\s+MPCCBF_MONITOR_WORDS\s+5\b", text)
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", text)
    m = re.search(r"typedef\s+struct\s+mpccbf_monitor\s*\{(.*?)\}\s*mpccbf_monitor\s*;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t shape_type", "double shape[2]", "double d_min", "double goal_radius",
                      "double watch_radius", "int32_t rows", "int64_t* summary", "int64_t* reached_at",
                      "double* min_d2", "int32_t* hit_samples", "int32_t* unsafe_samples", "int64_t* sample_log",
                      "int32_t sample_log_rows", "void* scratch", "size_t scratch_bytes"]
    names = [f.split()[-1].split("[")[0].lstrip("*") for f in fields]
    assert names == [f[0] for f in _lib.Monitor._fields_]
    assert C.sizeof(_lib.Monitor) == 128
    L = mpclib.load()
    assert L.mpccbf_abi_version() == 12
    for name in ("mpccbf_monitor_scratch_bytes", "mpccbf_monitor_table_size", "mpccbf_monitor_reset",
                 "mpccbf_monitor_score", "mpccbf_set_monitor"):
        assert hasattr(L, name) and name in _lib.EXPORTED
    for name in ("SafetyMonitor", "monitor"):
        assert hasattr(mpclib, name), name
    assert _lib.MONITOR_WORDS == 5
    import inspect
    assert "substeps" in inspect.signature(mpclib.Context.prepare_run_steps).parameters
    assert hasattr(mpclib.Context, "set_monitor")
    from mpccbf import sim
    assert "monitor" in inspect.signature(sim.Simulator.__init__).parameters

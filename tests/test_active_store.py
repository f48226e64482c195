"""CPU: the active-set store's interface (mpccbf_set_active_store, include/mpccbf.h) — the header
declares it and the library exports it, its argument errors that need no device, the record
decoding of mpccbf.decode_active_sides, and the ABI version, which the feature leaves at 12 (no
struct changed layout; the feature macro announces it instead)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")


def test_header_declares_and_library_exports_the_entry_point(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_ACTIVE_STORE\s+1\b", text)
    assert re.search(r"int\s+mpccbf_set_active_store\s*\(\s*mpccbf_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*store\s*,"
                     r"\s*int32_t\s+rows\s*,\s*int32_t\s+min_steps\s*\)\s*;", text)
    L = mpclib.load()
    assert hasattr(L, "mpccbf_set_active_store")
    assert "mpccbf_set_active_store" in mpclib._lib.EXPORTED
    for name in mpclib._lib.EXPORTED:  # every listed symbol resolves
        assert hasattr(L, name), name


def test_abi_version_is_still_12(mpclib):
    assert mpclib.load().mpccbf_abi_version() == 12
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", open(HEADER).read())


def test_argument_errors_without_a_device(mpclib):
    """The checks that come before the context is touched: a negative row count, a buffer with no
    rows, a null context. (The rows < num_states error is raised by the solve call, which needs a
    context and so a device: tests/test_gpu_active_store.py.)"""
    L = mpclib.load()
    buf = (ctypes.c_int32 * 8)()
    assert L.mpccbf_set_active_store(None, ctypes.cast(buf, ctypes.c_void_p), -1, 0) == -1
    assert L.mpccbf_last_error().decode() == "active store: rows must be >= 0"
    assert L.mpccbf_set_active_store(None, None, -5, 0) == -1
    assert L.mpccbf_last_error().decode() == "active store: rows must be >= 0"
    assert L.mpccbf_set_active_store(None, ctypes.cast(buf, ctypes.c_void_p), 0, 0) == -1
    assert L.mpccbf_last_error().decode() == "active store: a buffer needs rows >= 1"
    assert L.mpccbf_set_active_store(None, ctypes.cast(buf, ctypes.c_void_p), 1, 0) == -1
    assert L.mpccbf_last_error().decode() == "null context"


def test_decode_round_trips_hand_built_records(mpclib):
    dec, enc = mpclib.decode_active_sides, mpclib.encode_active_side
    # the header's encoding, spelled out: box (channel * 16 + row) * 2 + upper; CBF -(1 + nb * 8 + k)
    assert enc(("box", 0, 0, 0)) == 0 and enc(("box", 0, 0, 1)) == 1
    assert enc(("box", 1, 3, 1)) == (16 + 3) * 2 + 1 == 39
    assert enc(("box", 2, 15, "upper")) == 95
    assert enc(("cbf", 0, 0)) == -1 and enc(("cbf", 0, 1)) == -2 and enc(("cbf", 5, 1)) == -42
    assert enc(("cbf", 4095, 7)) == -(1 + 4095 * 8 + 7)
    sides = [("box", 1, 3, 1), ("cbf", 5, 1), ("box", 2, 15, 0), ("cbf", 0, 0), ("cbf", 4095, 7)]
    for k in range(len(sides) + 1):
        keys = [enc(s) for s in sides[:k]]
        rec = [k] + keys + [0] * (5 - k) + [3, 1]
        assert dec(rec) == sides[:k]
    # keys past k are ignored; a zero record is the empty set
    assert dec([1, 39, -42, 7, 7, 7, 2, 0]) == [("box", 1, 3, 1)]
    assert dec([0] * 8) == []
    assert dec(np.array([2, -1, 95, 0, 0, 0, 4, 1], dtype=np.int32)) == [("cbf", 0, 0), ("box", 2, 15, 1)]
    for bad in ([6, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0], [1, 96, 0, 0, 0, 0, 0, 0], [0] * 7):
        with pytest.raises(ValueError):
            dec(bad)
    for bad in (("box", 3, 0, 0), ("box", 0, 16, 0), ("box", 0, 0, 2), ("cbf", -1, 0), ("cbf", 0, 8), ("fov", 0, 0)):
        with pytest.raises(ValueError):
            enc(bad)


def test_scenario_has_long_iteration0_solves(oracle):
    """The GPU tests' scenario (tests/test_gpu_active_store.py: 64 agents, 0.6 x lattice, 8 nearest
    within 6 m) on the CPU oracle: at the first step some agents' iteration-0 optimum has >= 3
    independent active inequality rows, so a cold dual active-set solve of it takes >= 3 steps —
    there is something to warm-start."""
    from mpccbf import swarm
    cfg = swarm.config(15)
    states, targets = swarm.lattice_swarm(64)
    states[:, :2] *= 0.6
    rp, col = swarm.knn_csr(states, 8, 6.0)
    p = oracle.make_params(cfg)
    counts = []
    for a in range(64):
        nb = states[col[rp[a]:rp[a + 1]]]
        qp = oracle.assemble_qp(p, states[a], np.tile(targets[a], cfg["k_hor"]), nb)
        sol = oracle.solve_dense_qp(qp)
        if sol["status"] != oracle.OPTIMAL:
            continue
        A, lo, hi, x = qp["A"], qp["lo"], qp["hi"], sol["x"][:qp["n"]]
        eq = lo == hi
        ax = A @ x
        tight = ~eq & ((np.abs(ax - hi) <= 1e-7 * (1 + np.abs(hi))) | (np.abs(ax - lo) <= 1e-7 * (1 + np.abs(lo))))
        r_eq = np.linalg.matrix_rank(A[eq])
        counts.append(np.linalg.matrix_rank(np.vstack([A[eq], A[tight]])) - r_eq if tight.any() else 0)
    counts = np.array(counts)
    print("independent active inequality rows per agent:", np.bincount(counts))
    assert np.count_nonzero(counts >= 3) >= 1

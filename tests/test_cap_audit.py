"""CPU: the neighbour-cap audit's interface (mpccbf_cap_audit_run, include/mpccbf.h) — the header
declares it and the library exports it with the ABI still at 12, its argument errors that need no
device, mpccbf.audit_summary on hand-built counts, and the GPU tests' scenario on the CPU oracle:
it is not vacuous (rows are dropped live and violated) and stays inside the decision margins."""
import ctypes
import os
import re

import numpy as np
import pytest

import cap_audit_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")


def test_header_declares_and_library_exports_the_entry_point(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_CAP_AUDIT\s+1\b", text)
    m = re.search(r"typedef\s+struct\s+mpccbf_cap_audit\s*\{(.*?)\}\s*mpccbf_cap_audit\s*;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t* counts", "double* excess", "int32_t* live_nb", "double* x0_out", "double tol"]
    assert re.search(r"int\s+mpccbf_cap_audit_run\s*\(\s*mpccbf_ctx\s*\*\s*\w*\s*,\s*const\s+mpccbf_batch\s*\*\s*\w*\s*,"
                     r"\s*const\s+mpccbf_cap_audit\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", text)
    L = mpclib.load()
    assert hasattr(L, "mpccbf_cap_audit_run")
    assert "mpccbf_cap_audit_run" in mpclib._lib.EXPORTED
    for name in mpclib._lib.EXPORTED:
        assert hasattr(L, name), name
    assert L.mpccbf_abi_version() == 12
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", text)
    # the Python mirror of the struct has the header's layout: 4 pointers and a double
    assert ctypes.sizeof(mpclib._lib.CapAudit) == 4 * ctypes.sizeof(ctypes.c_void_p) + 8


def test_argument_errors_without_a_device(mpclib):
    """The checks that come before the context is touched, then the null context (-1, as for the
    store). The pointers are never dereferenced. (Slack mode, the FoV controller, the dense layouts
    and the capacity need a context and so a device: tests/test_gpu_cap_audit.py.)"""
    L = mpclib.load()
    lib = mpclib._lib
    fake = ctypes.addressof((ctypes.c_double * 8)())

    def batch(**over):
        kw = dict(num_states=4, states=fake, agent_first=0, num_agents=4, targets=fake, x=fake, status=fake,
                  nb_out=fake, knn_k=1, knn_radius=6.0)
        kw.update(over)
        return lib.Batch(**kw)

    def call(b, a, ctx=None):
        rc = L.mpccbf_cap_audit_run(ctx, None if b is None else ctypes.byref(b),
                                    None if a is None else ctypes.byref(a), None)
        return rc, L.mpccbf_last_error().decode()

    ok = lib.CapAudit(counts=fake)
    assert call(None, ok) == (-1, "cap audit: null batch")
    assert call(batch(), None) == (-1, "cap audit: null audit")
    assert call(batch(), lib.CapAudit(excess=fake)) == (-1, "cap audit: counts is required")
    assert call(batch(x=None), ok) == (-1, "cap audit: the solve's x and status are required")
    assert call(batch(status=None), ok) == (-1, "cap audit: the solve's x and status are required")
    assert call(batch(nb_out=None), ok) == (-1, "cap audit: grid mode needs the solve's nb_out")
    for bad in (dict(agent_first=1), dict(num_agents=5), dict(agent_first=-1), dict(num_agents=-1)):
        assert call(batch(**bad), ok) == (-1, "cap audit: agent range outside states"), bad
    assert call(batch(), lib.CapAudit(counts=fake, tol=-1.0)) == (-1, "cap audit: tol must be >= 0")
    # every device-free check passed: the null context is reported (grid and CSR batches)
    assert call(batch(), ok) == (-1, "null context")
    assert call(batch(nb_out=None, nb_row_ptr=fake, nb_col=fake), ok) == (-1, "null context")


def test_audit_summary_on_hand_built_counts(mpclib):
    S = mpclib.audit_summary
    rows = [
        [2, 0, 4, 0, 7, 9, 60, 3],      # certified in both iterations
        [3, 2, 5, 1, 1, 2, 61, 0],      # violated rows in both: no bit
        [1, 0, 6, 3, 4, 5, 62, 1],      # iteration 0 certified, iteration 1 not
        [4, 0, -1, -1, 8, -1, 63, 3],   # no iteration 1 (INFEASIBLE or one IMPC iteration)
        [5, 0, -1, -1, -1, -1, 59, 0],  # ERROR / UNKNOWN: live rows, no solution, no bit
        [0, 0, 0, 0, -1, -1, 0, 2],     # (bit 1 alone cannot come from the kernel; counted as set)
    ]
    s = S(np.array(rows, dtype=np.int32))
    assert s == dict(agents=6, live0=15, violated0=2, live1=15, violated1=4, certified0=3, certified1=3,
                     uncertified=3)
    assert S(np.zeros((0, 8), dtype=np.int32)) == dict(agents=0, live0=0, violated0=0, live1=0, violated1=0,
                                                       certified0=0, certified1=0, uncertified=0)
    for bits in range(4):
        s = S([[0, 0, 0, 0, -1, -1, 5, bits]])
        assert (s["certified0"], s["certified1"], s["uncertified"]) == (bits & 1, bits >> 1, 1 - (bits >> 1))
    assert S(rows[3])["live1"] == 0  # a single row; -1 words add nothing
    with pytest.raises(ValueError):
        S(np.zeros((2, 7), dtype=np.int32))


# live / violated totals of iteration 0 and 1 (from the CPU oracle; the issue's table)
EXPECTED = {1: (23, 14, 41, 28), 2: (3, 2, 6, 4)}


@pytest.mark.parametrize("k", [1, 2])
def test_scenario_is_not_vacuous_and_inside_the_margins(oracle, k):
    """64 agents on the 0.45 x lattice with the k nearest within 6 m, solved by the oracle: rows are
    dropped live and violated (the totals below), no dropped row sits within 1e-3 of the live
    threshold, and no live row's scaled excess within 1e-3 of zero — so the GPU tests' equalities
    do not hang on rounding."""
    from mpccbf import swarm
    cfg, states, targets = R.scenario(64)
    rp, col = swarm.knn_csr(states, k, 6.0)
    lists = [col[rp[a]:rp[a + 1]] for a in range(64)]
    p = oracle.make_params(cfg)
    refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    status = np.zeros((64, 2), dtype=np.int32)
    x0, x1 = np.full((64, n), np.nan), np.full((64, n), np.nan)
    for a in range(64):
        r = oracle.impc_optimize(p, states, a, lists[a], refs[a])
        status[a] = r["status"]
        x0[a], x1[a] = r["x"][0][:n], r["x"][1][:n]
    ref = R.audit(oracle, cfg, states, lists, status, x0, x1)
    c = ref["counts"]
    totals = tuple(int(np.clip(c[:, w], 0, None).sum()) for w in range(4))
    print(f"k = {k}: live / violated totals {totals}, agents with a violated iteration-0 row "
          f"{np.count_nonzero(c[:, 1] > 0)}, certified {np.count_nonzero(c[:, 7] == 3)}, "
          f"min |b - bmax| margin {ref['bmargin']:.3e}, "
          f"scaled excess nearest zero {np.min(np.abs(ref['live_sc'])):.3e}")
    assert totals == EXPECTED[k]
    assert ref["bmargin"] >= 1e-3
    assert not np.any(np.abs(ref["live_sc"]) <= 1e-3)

"""CPU: the connectivity interface (mpccbf_set_connectivity, include/mpccbf.h) — the header declares
it and the library exports it with the ABI still at 12, and its argument errors that need no
device. (Slack mode, the FoV controller, d_max <= d_min and the cap audit while attached need a
context and so a device: tests/test_gpu_conn_impc.py.)"""
import ctypes
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mpccbf.h")


def test_header_declares_and_library_exports_the_entry_point(mpclib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MPCCBF_HAS_CONNECTIVITY\s+1\b", text)
    m = re.search(r"typedef\s+struct\s+mpccbf_connectivity\s*\{(.*?)\}\s*mpccbf_connectivity\s*;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["double d_max", "double lambda2_min", "double lambda2_switch", "int32_t num_teams",
                      "const int32_t* team_ptr", "double* lambda2", "double* fiedler"]
    assert re.search(r"int\s+mpccbf_set_connectivity\s*\(\s*mpccbf_ctx\s*\*\s*\w*\s*,\s*const\s+mpccbf_connectivity\s*\*",
                     text)
    L = mpclib.load()
    assert hasattr(L, "mpccbf_set_connectivity")
    assert "mpccbf_set_connectivity" in mpclib._lib.EXPORTED
    assert L.mpccbf_abi_version() == 12
    assert re.search(r"#define\s+MPCCBF_ABI_VERSION\s+12\b", text)
    # the Python mirror has the header's layout: 3 doubles, an int32 (padded), 3 pointers
    assert ctypes.sizeof(mpclib._lib.Connectivity) == 3 * 8 + 8 + 3 * ctypes.sizeof(ctypes.c_void_p)


def test_argument_errors_without_a_device(mpclib):
    L = mpclib.load()
    lib = mpclib._lib

    def call(ctx=None, **over):
        tp = np.ascontiguousarray(over.pop("team_ptr", [0, 3, 7]), dtype=np.int32)
        kw = dict(d_max=3.2, lambda2_min=0.0, lambda2_switch=0.0, num_teams=len(tp) - 1, team_ptr=tp.ctypes.data)
        kw.update(over)
        k = lib.Connectivity(**kw)
        rc = L.mpccbf_set_connectivity(ctx, ctypes.byref(k))
        return rc, L.mpccbf_last_error().decode()

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(d_max=bad) == (-1, "connectivity: d_max must be positive and finite"), bad
    for bad in (dict(lambda2_min=-0.1), dict(lambda2_switch=float("nan"))):
        assert call(**bad) == (-1, "connectivity: lambda2_min and lambda2_switch must be >= 0 and finite"), bad
    assert call(num_teams=-1) == (-1, "connectivity: num_teams < 0")
    k = lib.Connectivity(d_max=3.2, num_teams=2, team_ptr=None)
    assert L.mpccbf_set_connectivity(None, ctypes.byref(k)) == -1
    assert L.mpccbf_last_error().decode() == "connectivity: team_ptr is required"
    assert call(team_ptr=[-1, 3]) == (-1, "connectivity: team_ptr[0] < 0")
    assert call(team_ptr=[0, 5, 3, 8]) == (-1, "connectivity: team_ptr decreases at team 1")
    # every device-free check passed: the null context is reported (attach and detach)
    assert call() == (-1, "null context")
    assert call(team_ptr=[0, 3, 3, 20]) == (-1, "null context")  # (an empty team is allowed)
    assert L.mpccbf_set_connectivity(None, None) == -1
    assert L.mpccbf_last_error().decode() == "null context"

"""The suite's comparison rules, each defined once (numpy only: usable from CPU tests).

Parity with the oracle: statuses equal; objectives within OBJ_TOL * max(1, |ref|)
on the oracle's OPTIMAL iterations; control points within X_TOL (inf-norm) of the curve of the
oracle's last OPTIMAL iteration. Route equivalence: two device routes to the same QP have NaN in
the same places and agree within ROUTE_REL relative elsewhere. Identity: same_bits (dtype, shape
and bit patterns) and same_values (==, NaN matching NaN). The rules are themselves tested in
test_parity_rule.py."""
from collections.abc import Mapping

import numpy as np

OPTIMAL = 0  # oracle_lib.OPTIMAL (asserted in test_parity_rule.py)
OBJ_TOL = 1e-4
X_TOL = 1e-5
ROUTE_REL = 1e-7


def worse(worst, e):
    """max(worst, e) that keeps a NaN (Python's max(0.0, nan) is 0.0)."""
    e = float(e)
    return e if (e != e or e > worst) and worst == worst else worst


def _reference(ref, i, a):
    """(status, obj, curves or None) of agent a, the i-th listed one. ref: the array tuple
    (status, obj[, x]) of the FoV case modules, rows by agent; a mapping agent -> result dict; or a
    sequence of oracle_lib.impc_optimize result dicts in the order of the listed agents."""
    if isinstance(ref, tuple):
        return ref[0][a], ref[1][a], (ref[2][a] if len(ref) > 2 else None)
    r = ref[a] if isinstance(ref, Mapping) else ref[i]
    return r["status"], r["obj"], r.get("x")


def check_parity(got, ref, agents=None, first=0, label="", x=True):
    """The parity rule on every listed agent (default: every agent of ref), asserted per agent and
    per iteration; a NaN on the device side where the oracle is OPTIMAL fails. got: host arrays
    "status", "obj" and, unless x is False or ref has no curves, "x"; agent a is row a - first.
    Prints and returns (worst relative objective error, worst |dx|); NaN propagates into both."""
    if agents is None:
        agents = range(len(ref[0])) if isinstance(ref, tuple) else (sorted(ref) if isinstance(ref, Mapping) else range(len(ref)))
    agents = [int(a) for a in agents]
    worst_obj = worst_x = 0.0
    for i, a in enumerate(agents):
        g = a - first
        rst, rob, rx = _reference(ref, i, a)
        gst = [int(s) for s in got["status"][g]]
        assert gst == [int(s) for s in rst], (label, a, gst, list(rst))
        last = None
        for it in range(len(rst)):
            if rst[it] != OPTIMAL:
                continue
            err = abs(got["obj"][g, it] - rob[it]) / max(1.0, abs(rob[it]))
            worst_obj = worse(worst_obj, err)
            assert err <= OBJ_TOL, (label, a, it, got["obj"][g, it], rob[it])
            last = it
        if x and rx is not None and last is not None:
            xr = np.asarray(rx[last])
            if not isinstance(ref, tuple):  # the oracle's vector carries its slacks behind the curve
                xr = xr[:got["x"].shape[1]]
            dx = float(np.max(np.abs(got["x"][g] - xr)))  # (np.max keeps a NaN)
            worst_x = worse(worst_x, dx)
            assert dx <= X_TOL, (label, a, dx)
    print(f"{label}: {len(agents)} agents, worst objective error {worst_obj:.3e} (relative), worst |dx| {worst_x:.3e}")
    return worst_obj, worst_x


def check_routes_agree(got, ref, what, rel=ROUTE_REL):
    """Route equivalence of two arrays: NaN in the same places, elsewhere |got - ref| <=
    rel * max(1, |ref|). Prints and returns the largest relative difference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:4].tolist())
    err = np.abs(got[~nan] - ref[~nan]) / np.maximum(1.0, np.abs(ref[~nan]))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: largest relative difference {worst:.3e}, "
          f"{int(np.count_nonzero(got[~nan] != ref[~nan]))} of {err.size} entries differ")
    assert worst <= rel, (what, worst)  # (fails on a NaN difference, inf - inf)
    return worst


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind in "fc" and a.dtype.itemsize <= 8 else a


def _bits_differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype:
        return f"dtype {a.dtype} != {b.dtype}"
    if a.shape != b.shape:
        return f"shape {a.shape} != {b.shape}"
    ne = _bits(a) != _bits(b)
    return _first(a, b, ne) if np.any(ne) else None


def _values_differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shape {a.shape} != {b.shape}"
    ne = a != b
    if a.dtype.kind in "fc" and b.dtype.kind in "fc":
        ne &= ~(np.isnan(a) & np.isnan(b))
    return _first(a, b, ne) if np.any(ne) else None


def _first(a, b, ne):
    i = tuple(int(v) for v in np.argwhere(ne)[0])
    return f"{int(np.count_nonzero(ne))} entries differ, first at {i}: {a[i]!r} != {b[i]!r}"


def _identity(differ, rule, a, b, keys, what):
    if keys is None and not isinstance(a, Mapping):
        why = differ(a, b)
        assert why is None, (what, rule, why)
        return
    for k in (keys if keys is not None else a):
        why = differ(a[k], b[k])
        assert why is None, (what, rule, k, why)


def same_bits(a, b, keys=None, what=""):
    """Assert dtype, shape and bit patterns equal: -0.0 differs from 0.0 and NaNs differ by
    payload. Arrays, or dicts of arrays over `keys` (default: a's); names the first differing key."""
    _identity(_bits_differ, "same_bits", a, b, keys, what)


def same_values(a, b, keys=None, what=""):
    """Assert shape and values equal by ==, NaN matching NaN (-0.0 equals 0.0):
    np.testing.assert_array_equal's rule. Arrays or dicts, as same_bits."""
    _identity(_values_differ, "same_values", a, b, keys, what)

"""Checks of the reference's own known-answer tests (tests/golden/reference_kats.json), shared by the
oracle's and the device's tests."""
import numpy as np


def voronoi_kat_checks(vor_fn, case, tol):
    """The expectations of separating_hyperplanes/tests/VoronoiTest.cpp:10-73 for one case;
    vor_fn(p1, p2) -> (normal (2+), offset) with bbox 0."""
    p1, p2 = np.array(case["p1"]), np.array(case["p2"])
    n, off = vor_fn(p1, p2)
    n = np.asarray(n, dtype=np.float64)[:2]
    ev = lambda p: float(n @ p + off)  # noqa: E731
    if case["name"] == "ComputeVoronoiHyperplane2D":
        np.testing.assert_allclose(n, case["expected_normal"], atol=tol)
        assert abs(ev(np.array(case["midpoint"]))) <= tol
        assert ev(p1) < 0.0 and ev(p2) > 0.0
        nn = np.linalg.norm(n)
        assert abs(abs(ev(p1)) / nn - abs(ev(p2)) / nn) <= tol
    else:
        perp = np.array([-n[1], n[0]])
        for t in case["t"]:
            pt = perp * t - n * off / (n @ n)
            assert abs(ev(pt)) <= tol
            assert abs(np.linalg.norm(pt - p1) - np.linalg.norm(pt - p2)) <= tol

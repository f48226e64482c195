"""CPU: the inputs of test_gpu_conn_impc.py (conn_impc_cases.py) exercise what they are meant to,
by the reference alone: agents where the connectivity row binds at OPTIMAL with another objective
than the row-free QP's, agents where CLF rows bind, agents the added rows make INFEASIBLE; unique
Fiedler vectors; no team on the mode switch; statuses that do not hang on rounding."""
import numpy as np

import conn_impc_cases as Cs
import conn_impc_ref as R
import oracle_lib as O
from mpccbf import swarm


def test_cases_cover_binding_rows_and_infeasibility(oracle):
    c = Cs.cases()
    keep = c["keep"]
    kinds = [k for k, kp in zip(c["kind"], keep) if kp]
    print({k: kinds.count(k) for k in sorted(set(kinds))}, "dropped", int((~keep).sum()), "of", len(keep))
    assert kinds.count("conn") >= 6
    assert kinds.count("clf") >= 6
    assert kinds.count("infeasible") >= 6
    # the generator may drop at most 5 % of the agents (statuses that change with the bounds)
    assert (~keep).sum() <= 0.05 * len(keep)
    for i in np.nonzero(keep)[0]:
        a, f = c["ref"][i], c["free"][i]
        if c["kind"][i] in ("conn", "clf"):
            assert all(s == O.OPTIMAL for s in a["status"]) and a["conn_mode"] == (c["kind"][i] == "conn")
            assert abs(a["obj"][-1] - f["obj"][-1]) > 1e-6 * max(1.0, abs(f["obj"][-1]))
            assert R.row_excess(a["rows"][-1], a["x"][-1]) <= 1e-8
        if c["kind"][i] == "infeasible":
            assert O.INFEASIBLE in list(a["status"]) and all(s == O.OPTIMAL for s in f["status"])


def test_spectra_are_well_separated(oracle):
    c = Cs.cases()
    tp = c["team_ptr"]
    for t, (l2, ev, lam) in enumerate(c["spectra"]):
        n = int(tp[t + 1] - tp[t])
        assert 2 <= n <= 16
        assert abs(l2 - lam[1]) <= 1e-10 * max(1.0, lam[-1])  # the oracle's Jacobi sweep against LAPACK
        if n > 2:
            assert lam[2] - lam[1] >= 1e-3 * lam[-1], (t, lam)  # a unique Fiedler vector
        assert abs(l2 - 0.1) >= 1e-6, (t, l2)
        assert abs(float(ev @ ev) - 1.0) <= 1e-12
    modes = [l2 > 0.1 for l2, _, _ in c["spectra"]]
    assert any(modes) and not all(modes)


def test_team_swarm_is_seeded_and_laid_out_as_documented():
    a = swarm.team_swarm((3, 1, 5), 2.5, seed=4)
    b = swarm.team_swarm((3, 1, 5), 2.5, seed=4)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    st, tg, tp = a
    assert list(tp) == [0, 3, 4, 9] and st.shape == (9, 6) and tg.shape == (9, 3)
    d = np.linalg.norm(st[0, :2] - st[1, :2])
    assert abs(d - 2.5) < 0.3  # ring neighbours are `spacing` apart up to the position noise
    assert not np.array_equal(swarm.team_swarm((3, 1, 5), 2.5, seed=5)[0], st)
    rp, col = swarm.team_csr(tp)
    assert list(rp) == [0, 2, 4, 6, 6, 10, 14, 18, 22, 26] and list(col[:6]) == [1, 2, 0, 2, 0, 1]
    line = swarm.team_swarm((4,), 2.0, seed=1, shape="line", pos_noise=0.0)[0]
    np.testing.assert_allclose(np.diff(line[:, 0]), 2.0)


def test_reference_without_a_team_is_the_oracle(oracle):
    """conn_impc_ref.impc_agent with no team is oracle_lib.impc_optimize (the loop it restates)."""
    c = Cs.cases()
    p = O.make_params(c["cfg"])
    refs = swarm.refs_from_targets(c["targets"], c["cfg"]["k_hor"])
    for i in (0, 5, 20, 40):
        nb = c["col"][c["row_ptr"][i]:c["row_ptr"][i + 1]]
        r = O.impc_optimize(p, c["states"], i, nb, refs[i])
        f = c["free"][i]
        assert list(r["status"]) == list(f["status"])
        ok = r["status"] == O.OPTIMAL
        np.testing.assert_allclose(r["obj"][ok], f["obj"][ok], rtol=1e-9)

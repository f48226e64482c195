"""CPU: what makes neighbour_shortcut_cases.py's swarm a case of each branch of the 16-lane query's
ranking (test_gpu_neighbour_shortcuts.py runs it on the device): with swarm.knn_csr, every
candidate count a query claims is some agent's, lists are cut only where the count exceeds knn_k,
waves mix the branches, and the cut at knn_k + 1 candidates falls inside a tie shell."""
import numpy as np
import pytest

import exact_geometry_cases as X
import neighbour_shortcut_cases as S
from mpccbf import swarm


def test_swarm_is_small_and_dyadic():
    st, tg = S.shortcut_swarm()
    assert len(st) == 63 <= 64 and tg.shape == (63, 3)
    p = st[:, :2] * 32.0
    assert np.all(p == np.round(p)) and np.all(np.abs(st[:, :2]) < 512.0)
    assert len({tuple(r) for r in st[:, :2]}) == len(st)  # no two agents coincide


@pytest.mark.parametrize("query", sorted(S.QUERIES))
def test_counts_are_what_the_query_claims(query):
    k, r = query
    st, _ = S.shortcut_swarm()
    cnt = S.counts(st, r)
    # knn_csr with room for everyone lists exactly the candidates
    rp_all, _ = swarm.knn_csr(st, len(st), r)
    np.testing.assert_array_equal(np.diff(rp_all), cnt)
    assert S.QUERIES[query] <= set(cnt.tolist()), sorted(set(cnt.tolist()))
    assert cnt.max() <= 32  # the two-candidates-per-lane path, never the loop or the stream
    rp, _ = S.reference_lists(query)
    np.testing.assert_array_equal(np.diff(rp), np.minimum(cnt, k))


def test_main_query_covers_every_branch_and_mixes_them_in_a_wave():
    k, r = 8, 4.0
    st, _ = S.shortcut_swarm()
    cnt = S.counts(st, r)
    assert {0, 1, k - 1, k, k + 1, 16, 17, 32} <= set(cnt.tolist())
    kinds = np.where(cnt <= k, 0, np.where(cnt <= 16, 1, 2))  # kept unranked / ranked / two per lane
    waves = [set(kinds[w:w + 4].tolist()) for w in range(0, len(st) - 3, 4)]
    assert {0, 1, 2} in waves, waves                       # one wave holds all three
    assert any(w == {2} for w in waves)                    # and one only the line
    # a wave in which no group ranks: under the largest k (its first four agents see 16, 0, 1, 7)
    assert np.all(cnt[:4] <= S.K_MAX) and cnt[0] == 16


def test_largest_k_keeps_sixteen_and_cuts_seventeen():
    st, _ = S.shortcut_swarm()
    assert S.K_MAX == 16
    cnt = S.counts(st, 4.0)
    rp, col = S.reference_lists((16, 4.0))
    rows = X.csr_rows(rp, col)
    for i in np.nonzero(cnt == 16)[0]:  # the line's ends: every candidate kept
        assert len(rows[i]) == 16
    for i in np.nonzero(cnt == 17)[0]:  # one dropped: the farthest, alone at its distance
        assert len(rows[i]) == 16
    assert {15, 16, 17} <= set(S.counts(st, 3.75).tolist())


def test_cut_at_k_plus_one_falls_in_a_tie_shell():
    k, r = 8, 4.0
    st, _ = S.shortcut_swarm()
    cnt = S.counts(st, r)
    tied = [i for i in X.cuts_tie(st, k, r) if cnt[i] == k + 1]
    assert len(tied) == 2  # the middle column of the 2 x 5 patch
    d2 = X.d2_matrix(st)
    rp, col = S.reference_lists((k, r))
    for i in tied:
        row = col[rp[i]:rp[i + 1]]
        shell = np.nonzero((d2[i] == np.sort(d2[i][row])[-1]) & (np.arange(len(st)) != i))[0]
        assert len(shell) == 2 and shell[0] in row and shell[1] not in row  # the smaller index stays
    # k = 1 cuts a tie everywhere two nearest candidates are equally far (the line's interior)
    assert len(X.cuts_tie(st, 1, r)) >= 31


def test_solve_lattice_counts():
    st, _ = S.solve_lattice()
    k, r = S.SOLVE_QUERY
    cnt = S.counts(st, r)
    assert set(cnt.tolist()) == {5, 7, 8, 10, 11, 12}
    kinds = cnt <= k
    waves = [set(kinds[w:w + 4].tolist()) for w in range(0, 36, 4)]
    assert {True, False} in waves  # a wave mixes kept-unranked and ranked groups
    assert waves[0] == {True}      # and in the first one no group ranks
    assert cnt.max() <= 16         # no second candidate slot anywhere

"""The inputs of tests/test_gpu_svd.py, checked on the CPU: on every case the numpy restatement (tests/svd_reference.py) alone
stays within the bars the device is held to, and the preconditions that make those bars meaningful hold -- a positive relative
gap down to sigma_k, an NNDSVD tie margin >= 1e-6, and no entry within a factor 2^20 of the zero threshold (rows and columns
of A that are entirely zero are exempt: their entries are zero in exact arithmetic, the device computes them as exact zeros
and LAPACK leaves rounding noise far below the threshold).  A case that violates a precondition gets another seed, never
another bar."""
import numpy as np
import pytest

import svd_reference as R


def _entries_clear_of_threshold(A, U, S, V):
    live_r, live_c = np.any(A != 0, axis=1), np.any(A != 0, axis=0)
    info = {}
    R.nndsvd_from_svd(U[live_r], S, V[live_c], info=info)
    return info


def _check_case(A, k, oversample=8, power_iters=0, omega=None, rng=None):
    Un, Sn, Vn = R.numpy_svd(A, k)
    g = R.relative_gap(Sn, k)
    assert g > 0
    bar_s, bar_v = R.bars(Sn, k)
    U, S, V = R.svd_restated(A, k, oversample=oversample, power_iters=power_iters, omega=omega, rng=rng)
    es = np.max(np.abs(S - Sn[:k]) / Sn[:k])
    ev = max(np.max(np.abs(R.align(U, Un) - Un)), np.max(np.abs(R.align(V, Vn) - Vn)))
    l = min(k + oversample, *A.shape)
    eo = max(np.max(np.abs(U.T @ U - np.eye(k))), np.max(np.abs(V.T @ V - np.eye(k))))
    print(f"{A.shape} k={k}: cond={Sn[0] / Sn[k - 1]:.1f} gap={g:.2e} S {es:.1e} (bar {bar_s:.1e}) vectors {ev:.1e} (bar {bar_v:.1e}) orth {eo:.1e}")
    assert es <= bar_s and ev <= bar_v and eo <= 64 * l * R.U53
    info = _entries_clear_of_threshold(A, Un, Sn[:k], Vn)
    print(f"    tie margin {info['tie_margin']:.2e}, entries 2^{info['threshold_distance_log2']:.1f} from the zero threshold")
    assert info["tie_margin"] >= 1e-6
    assert info["threshold_distance_log2"] >= 20
    Wn, Hn = R.nndsvd_from_svd(Un, Sn[:k], Vn)
    W, H = R.nndsvd_from_svd(U, S, V)
    assert np.max(np.abs(W - Wn)) <= bar_v * Wn.max() and np.max(np.abs(H - Hn)) <= bar_v * Hn.max()
    assert np.array_equal(W == 0, Wn == 0) and np.array_equal(H == 0, Hn == 0)


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_exact_rank_cases_meet_the_bars_and_preconditions(case):
    m, n, r, k = case
    A = R.exact_rank(m, n, r, R.EXACT_SEEDS[case])
    assert A.max() <= 256 and np.linalg.matrix_rank(A) == min(r, m, n)
    _check_case(A, k, rng=np.random.default_rng(5))


@pytest.mark.parametrize("case", R.SPARSE_CASES, ids=str)
def test_sparse_cases_meet_the_bars_and_preconditions(case):
    m, n, r, k = case
    (vals, rows, indptr, shape), D = R.sparse_exact_rank(m, n, r, R.SPARSE_SEEDS[case])
    assert len(vals) == np.count_nonzero(D) + 1                       # the duplicated entry
    assert np.any(~D.any(axis=0)) and np.any(~D.any(axis=1))          # an empty column, an empty row
    import scipy.sparse as sp
    assert np.array_equal(sp.csc_matrix((vals, rows, indptr), shape=shape).toarray(), D)
    _check_case(D, k, rng=np.random.default_rng(6))


@pytest.mark.parametrize("case", R.REPLAY_CASES, ids=str)
def test_replay_cases_two_summation_orders_agree(case):
    """full-rank data with the caller's Omega: the restatement against itself with A' (another summation order)"""
    m, n, k = case
    A = R.replay_values(m, n, 3)
    omega = np.random.default_rng(9).random((n, k + 8)) - 0.5
    Sn = np.linalg.svd(A, compute_uv=False)
    opt = np.sum(Sn[k:] ** 2)
    prev = None
    for q in (0, 2):
        U, S, V = R.svd_restated(A, k, power_iters=q, omega=omega)
        U2, S2, V2 = R.svd_restated(np.ascontiguousarray(A.T).T, k, power_iters=q, omega=np.asfortranarray(omega))
        res = np.linalg.norm(A - (U * S) @ V.T) ** 2
        print(f"{case} q={q}: S {np.max(np.abs(S - S2)) / S[0]:.1e} vectors {np.max(np.abs(R.align(U2, U) - U)):.1e} residual / optimal {res / opt:.3f}")
        assert np.max(np.abs(S - S2)) <= 1e-12 * S[0]
        assert np.max(np.abs(R.align(U2, U) - U)) <= 1e-10 and np.max(np.abs(R.align(V2, V) - V)) <= 1e-10
        assert prev is None or res <= prev
        prev = res


def test_rank_below_k_gives_exact_zeros():
    m, n, r, k = R.LOW_RANK_CASE
    for A in (R.exact_rank(m, n, r, 1), np.zeros((65, 63))):
        kk = k if A.any() else 3
        U, S, V = R.svd_restated(A, kk, power_iters=0, rng=np.random.default_rng(1))
        rank = r if A.any() else 0
        assert np.all(S[rank:] == 0) and np.all(S[:rank] > 0)
        assert not U[:, rank:].any() and not V[:, rank:].any()
        W, H = R.nndsvd_from_svd(U, S, V)
        assert not W[:, rank:].any() and not H[rank:].any()

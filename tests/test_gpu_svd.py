"""Truncated SVD and the NNDSVD start on the device (DenseMatrix.svd / .nndsvd, SparseMatrix likewise,
NmfSolver.set_factors_nndsvd; smallk_amd/csrc/svd.cpp, svd.hip) against numpy.linalg.svd of the stored matrix
and against the numpy restatement of the algorithm (tests/svd_reference.py).  The cases and their preconditions are checked on
the CPU by tests/test_svd_cpu.py.  Shapes: the smallest at which 64-wide tiles, padded ranks and two groups of 64 factor rows
can go wrong.  Bars (u = 2^-53): S relative 64 u (sigma_1 / sigma_k)^2 (the Gram route squares the condition number), vectors
that over the relative gap g, orthonormality 64 l u."""
import functools

import numpy as np
import pytest

import svd_reference as R

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _exact(case):
    m, n, r, k = case
    A = R.exact_rank(m, n, r, R.EXACT_SEEDS[case])
    Un, Sn, Vn = R.numpy_svd(A, k)
    return A, Un, Sn, Vn


@functools.lru_cache(maxsize=None)
def _sparse(case):
    m, n, r, k = case
    csc, D = R.sparse_exact_rank(m, n, r, R.SPARSE_SEEDS[case])
    Un, Sn, Vn = R.numpy_svd(D, k)
    return csc, D, Un, Sn, Vn


def _dense_matrix(gpu, A, storage):
    D = gpu.DenseMatrix.from_host(A, storage=storage)
    if not np.array_equal(D.download(), A):
        assert storage == "bf16"             # only bf16 may fail to hold a case; fp32 holds integers <= 2^24
        D.close()
        return None
    return D


def _check_svd(mat, A, k, Un, Sn, Vn, tag):
    l = min(k + 8, *A.shape)
    bar_s, bar_v = R.bars(Sn, k)
    U, S, V = mat.svd(k, power_iters=0)
    U2, S2, V2 = mat.svd(k, power_iters=0)
    assert np.array_equal(S, S2) and bool((U == U2).all()) and bool((V == V2).all())
    U, V = _np(U), _np(V)
    es = np.max(np.abs(S - Sn[:k]) / Sn[:k])
    ev = max(np.max(np.abs(R.align(U, Un) - Un)), np.max(np.abs(R.align(V, Vn) - Vn)))
    eo = max(np.max(np.abs(U.T @ U - np.eye(k))), np.max(np.abs(V.T @ V - np.eye(k))))
    print(f"svd {tag} k={k}: S {es:.2e} (bar {bar_s:.2e})  vectors {ev:.2e} (bar {bar_v:.2e})  orthonormality {eo:.2e} (bar {64 * l * R.U53:.2e})")
    assert es <= bar_s
    assert ev <= bar_v
    assert eo <= 64 * l * R.U53


def _check_nndsvd(mat, A, k, Un, Sn, Vn, tag):
    _, bar_v = R.bars(Sn, k)
    mean = A.sum() / (A.shape[0] * A.shape[1])
    for variant in ("nndsvd", "nndsvda"):
        Wr, Hr = R.nndsvd_from_svd(Un, Sn[:k], Vn, variant=variant, mean=mean)
        Wz, Hz = R.nndsvd_from_svd(Un, Sn[:k], Vn)
        W, H = mat.nndsvd(k, variant=variant, power_iters=0)
        W, H = _np(W), _np(H)
        ew, eh = np.max(np.abs(W - Wr)) / Wr.max(), np.max(np.abs(H - Hr)) / Hr.max()
        print(f"{variant} {tag} k={k}: W {ew:.2e} H {eh:.2e} (bar {bar_v:.2e})")
        assert ew <= bar_v and eh <= bar_v
        if variant == "nndsvd":
            assert np.array_equal(W == 0, Wr == 0) and np.array_equal(H == 0, Hr == 0)
            assert W.min() >= 0 and H.min() >= 0
        else:
            assert np.all(np.abs(W[Wz == 0] - mean) <= 2 * R.U53 * mean) and np.all(np.abs(H[Hz == 0] - mean) <= 2 * R.U53 * mean)


# ---- 1, 2: exact-rank cases, dense -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_svd_matches_numpy_on_exact_rank_data(gpu, case, storage):
    A, Un, Sn, Vn = _exact(case)
    D = _dense_matrix(gpu, A, storage)
    if D is None:
        assert case == (200, 300, 70, 66)
        return
    _check_svd(D, A, case[3], Un, Sn, Vn, f"{case} {storage}")
    assert np.array_equal(D.download(), A)
    D.close()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_nndsvd_matches_the_start_built_from_numpys_svd(gpu, case, storage):
    A, Un, Sn, Vn = _exact(case)
    D = _dense_matrix(gpu, A, storage)
    if D is None:
        assert case == (200, 300, 70, 66)
        return
    _check_nndsvd(D, A, case[3], Un, Sn, Vn, f"{case} {storage}")
    D.close()


# ---- 3: rank below k --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rank4_k6", "zero_k3"])
def test_rank_below_k_returns_exact_zeros(gpu, which):
    m, n, r, k = R.LOW_RANK_CASE
    A, rank = (R.exact_rank(m, n, r, 1), r) if which == "rank4_k6" else (np.zeros((65, 63)), 0)
    k = k if rank else 3
    D = gpu.DenseMatrix.from_host(A)
    U, S, V = D.svd(k, power_iters=0)           # returns: SMK_OK
    assert np.all(S[rank:] == 0.0) and np.all(S[:rank] > 0)
    assert not _np(U)[:, rank:].any() and not _np(V)[:, rank:].any()
    W, H = D.nndsvd(k, power_iters=0)
    assert not _np(W)[:, rank:].any() and not _np(H)[rank:].any()
    if rank:
        Sn = np.linalg.svd(A, compute_uv=False)
        assert np.max(np.abs(S[:rank] - Sn[:rank]) / Sn[:rank]) <= 64 * R.U53 * (Sn[0] / Sn[rank - 1]) ** 2
    D.close()


# ---- 4: replay with the caller's Omega: full-rank data, power iterations -----------------------------------------------------
@pytest.mark.parametrize("case", R.REPLAY_CASES, ids=str)
def test_replay_with_the_callers_omega(gpu, case):
    import torch
    m, n, k = case
    A = R.replay_values(m, n, 3)
    omega = np.random.default_rng(9).random((n, k + 8)) - 0.5
    D = gpu.DenseMatrix.from_host(A)
    assert np.array_equal(D.download(), A)
    om = torch.from_numpy(omega).cuda()
    res = {}
    for q in (0, 2):
        Ur, Sr, Vr = R.svd_restated(A, k, power_iters=q, omega=omega)
        U, S, V = D.svd(k, power_iters=q, omega=om)
        U, V = _np(U), _np(V)
        es = np.max(np.abs(S - Sr)) / Sr[0]
        ev = max(np.max(np.abs(R.align(U, Ur) - Ur)), np.max(np.abs(R.align(V, Vr) - Vr)))
        res[q] = np.linalg.norm(A - (U * S) @ V.T) ** 2
        rr = np.linalg.norm(A - (Ur * Sr) @ Vr.T) ** 2
        print(f"replay {case} q={q}: S {es:.2e} (bar 1e-12)  vectors {ev:.2e} (bar 1e-10)  residual {abs(res[q] - rr) / rr:.2e} (bar 1e-9)")
        assert es <= 1e-12
        assert ev <= 1e-10
        assert abs(res[q] - rr) <= 1e-9 * rr
    assert res[2] <= res[0]
    D.close()


# ---- 5: sparse ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SPARSE_CASES, ids=str)
def test_sparse_svd_and_nndsvd(gpu, case):
    (vals, rows, indptr, shape), Dn, Un, Sn, Vn = _sparse(case)
    S = gpu.SparseMatrix(vals, rows, indptr, shape)
    _check_svd(S, Dn, case[3], Un, Sn, Vn, f"sparse {case}")
    _check_nndsvd(S, Dn, case[3], Un, Sn, Vn, f"sparse {case}")
    S.close()


# ---- 6: solver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,variant", [("BPP", "nndsvd"), ("MU", "nndsvda")])
def test_solver_start_is_the_matrix_entrys_start_and_the_updates_descend(gpu, alg, variant):
    m, n, k = 129, 257, 8
    A = R.replay_values(m, n, 3)
    D = gpu.DenseMatrix.from_host(A)
    W0, H0 = D.nndsvd(k, variant=variant)
    o = gpu.make_options(m, n, k, alg)
    s1, s2 = gpu.NmfSolver(D, o), gpu.NmfSolver(D, o)
    s1.set_factors_nndsvd(variant)
    s2.set_factors_device(W0, H0)
    Wa, Ha = s1.factors_device()
    Wb, Hb = s2.factors_device()
    assert bool((Wa == Wb).all()) and bool((Ha == Hb).all())
    assert bool((Wa == W0).all()) and bool((Ha == H0).all())
    assert s1.iteration_count == 0
    start = D.residual(W0, H0).resid_sq
    s1.iterate(5)
    after = s1.residual().resid_sq
    print(f"{alg} from {variant}: resid_sq {start:.6e} -> {after:.6e} after 5 iterations")
    assert after <= start
    s1.close()
    s2.close()
    D.close()


# ---- 7: refusals --------------------------------------------------------------------------------------------------------------
def _code(fn):
    from smallk_amd import _lib as L
    with pytest.raises(L.SmallkError) as e:
        fn()
    return e.value.code


def test_refusals(gpu):
    import torch
    from smallk_amd import _lib as L
    A = R.replay_values(65, 63, 1)
    D1 = gpu.DenseMatrix.from_host(A, storage="bf16", single_copy=True)
    assert D1.single_copy
    assert _code(lambda: D1.svd(4)) == L.UNSUPPORTED
    assert _code(lambda: D1.nndsvd(4)) == L.UNSUPPORTED
    assert D1.single_copy                              # the transpose was not built behind the caller's back
    D1.close()
    big = gpu.DenseMatrix.from_host(R.replay_values(140, 130, 2))
    assert _code(lambda: big.svd(121)) == L.UNSUPPORTED                 # k + p = 129
    assert _code(lambda: big.svd(1, oversample=128)) == L.UNSUPPORTED
    big.close()
    D = gpu.DenseMatrix.from_host(A)
    assert _code(lambda: D.svd(64)) == L.BAD_PARAM                      # k > min(m, n)
    assert _code(lambda: D.svd(0)) == L.BAD_PARAM
    bad = torch.zeros((63, 11), dtype=torch.float64, device="cuda")
    assert _code(lambda: D.svd(4, omega=bad)) == L.BAD_PARAM            # Omega is (n, l) = (63, 12)
    assert _code(lambda: D.nndsvd(4, omega=bad.t())) == L.BAD_PARAM
    with pytest.raises(ValueError):
        D.nndsvd(4, variant="random")
    s = gpu.NmfSolver(D, gpu.make_options(65, 63, 4, "BPP"))
    assert _code(lambda: s.set_factors_nndsvd(oversample=125)) == L.UNSUPPORTED
    s.close()
    D.close()
    shard = gpu.DenseMatrix(65, 63, col0=16, ncols=32)
    shard.upload(A[:, 16:48])
    assert _code(lambda: shard.svd(4)) == L.UNSUPPORTED
    shard.close()

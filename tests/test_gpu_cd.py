"""Coordinate-descent NMF on the device (smallk_amd.cd_sweep, nmf_cd, NMF; smallk_amd/csrc/cd.hip, cd.cpp) against
the numpy restatement tests/cd_reference.py and against scikit-learn's recorded result (tests/golden/cd_sklearn.npz).  That the
cases hold these bars by themselves -- no zero pattern, no iteration count hangs on a rounding -- is checked on the CPU by
tests/test_cd_cpu.py.

Bars (u = 2^-53).  One sweep: x within 64 k u of the restatement's largest |x|, the violation within 64 k u relative, equal zero
patterns.  A fit: the same n_iter, factors within 1e-12 of the largest factor entry, equal zero patterns, the final
violation / violation_init within 1e-9 relative.  Everything has the same bits on a second run."""
import functools
import os

import numpy as np
import pytest

import cd_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cd_sklearn.npz")


# ---- the sweep by itself ---------------------------------------------------------------------------------------------------
def _check_sweep(gpu, G, Rm, X, l1, l2, k, tag):
    ref = X.copy()
    vref = R.sweep(ref, G, Rm, l1, l2)
    got, v = gpu.cd_sweep(G, Rm, X, l1, l2)
    got2, v2 = gpu.cd_sweep(G, Rm, X, l1, l2)
    top = np.abs(ref).max()
    ex = np.abs(got - ref).max() / top if top > 0 else np.abs(got).max()
    ev = abs(v - vref) / vref
    print(f"sweep {tag}: x {ex:.2e}, violation {ev:.2e} (bar {R.sweep_bar(k):.2e})")
    assert ex <= R.sweep_bar(k)
    assert np.array_equal(got == 0, ref == 0)
    assert ev <= R.sweep_bar(k)
    assert np.array_equal(got, got2) and v == v2
    return got, ref


@pytest.mark.parametrize("reg", R.SWEEP_REGS)
@pytest.mark.parametrize("k", R.SWEEP_KS)
def test_sweep(gpu, k, reg):
    for N in R.SWEEP_NS:
        G, Rm, X, l1, l2 = R.sweep_case(k, N, reg)
        got, _ = _check_sweep(gpu, G, Rm, X, l1, l2, k, f"k={k} N={N} {reg}")
        if reg == "l1":
            assert (got[:, 1::4] == 0).all()


@pytest.mark.parametrize("k, t0", [(3, 1), (17, 16), (65, 0)])
def test_sweep_zero_diagonal(gpu, k, t0):
    """G'[t0, t0] == 0 with l2 = 0: x[t0] is unchanged (its zeros too), and its projected gradient is counted -- the violation
    matches the restatement, which counts it"""
    G, Rm, X, l1, l2 = R.sweep_case(k, 63, "none", zero_diag=t0)
    X[t0, ::2] = 0.0
    got, _ = _check_sweep(gpu, G, Rm, X, l1, l2, k, f"k={k} zero diagonal at {t0}")
    assert np.array_equal(got[t0], X[t0])


def test_sweep_argument_errors(gpu):
    G, Rm, X, l1, l2 = R.sweep_case(3, 5, "none")
    with pytest.raises(ValueError):
        gpu.cd_sweep(G, Rm, X[:, :4])
    from smallk_amd import _lib as L
    big = np.zeros((129, 2))
    with pytest.raises(L.SmallkError) as e:
        gpu.cd_sweep(np.eye(129), big, big)
    assert e.value.code == L.UNSUPPORTED


# ---- fits ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name):
    A, csc, W0, H0, kw = R.fit_case(name)
    return A, csc, W0, H0, kw, R.fit(A, W0, H0, **kw)


def _matrix(gpu, name):
    A, csc = _reference(name)[:2]
    if csc is not None:
        vals, rows, indptr, shape = csc
        return gpu.SparseMatrix(vals, rows, indptr, shape)
    mat = gpu.DenseMatrix.from_host(A)
    assert np.array_equal(mat.download(), A)
    return mat


def _compare(got_W, got_H, n_iter, ratio, ref, tag, ref_ratio=None):
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(got_W - ref["W"]).max() / top, np.abs(got_H - ref["H"]).max() / top
    rr = ref["violation"] / ref["violation_init"] if ref_ratio is None else ref_ratio
    er = abs(ratio - rr) / rr
    print(f"fit {tag}: n_iter {n_iter} (restatement {ref['n_iter']}), W {ew:.2e} H {eh:.2e} (bar {R.FIT_BAR:.0e}), ratio {er:.2e} (bar {R.RATIO_BAR:.0e})")
    assert n_iter == ref["n_iter"]
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert np.array_equal(got_W == 0, ref["W"] == 0) and np.array_equal(got_H == 0, ref["H"] == 0)
    assert er <= R.RATIO_BAR


@pytest.mark.parametrize("name", list(R.FIT_CASES))
def test_fit(gpu, name):
    A, csc, W0, H0, kw, ref = _reference(name)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_cd(mat, W0, H0, **kw)
        r2 = gpu.nmf_cd(mat, W0, H0, **kw)
    finally:
        mat.close()
    _compare(r.W, r.H, r.n_iter, r.violation / r.violation_init, ref, name)
    assert r.converged == ref["converged"]
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.n_iter, r.violation, r.violation_init) == (r2.n_iter, r2.violation, r2.violation_init)
    if name == R.RUNS_TO_MAX_ITER:
        assert r.n_iter == R.FIT_MAX_ITER and not r.converged
    if name in R.GOLDEN_CASES:            # scikit-learn's own numbers, at the same bar
        g = np.load(GOLDEN)
        sk = {"W": g[f"{name}/W"], "H": g[f"{name}/H"], "n_iter": int(g[f"{name}/n_iter"])}
        _compare(r.W, r.H, r.n_iter, 1.0, sk, name + " against sklearn", ref_ratio=1.0)


def test_fit_fp32_views_and_a_strided_w(gpu):
    """fp32 factor views, W a view of every second column of a wider tensor, updated in place.  The start is exact in fp32, the
    iteration runs in fp64 as ever and the result is rounded to fp32 once on the way out: it is the restatement rounded to fp32
    except where a 1e-15 difference straddles a rounding boundary of fp32, which these fixed inputs do not meet."""
    import torch
    name = R.FP32_VIEW_CASE
    A, _, W0, H0, kw, ref = _reference(name)
    dev = torch.device("cuda", 0)
    mat = _matrix(gpu, name)
    try:
        out = []
        for _ in range(2):
            wide = torch.full((A.shape[0], 2 * W0.shape[1]), -7.0, dtype=torch.float32, device=dev)
            W = wide[:, ::2]
            W.copy_(torch.from_numpy(W0))
            H = torch.from_numpy(H0).to(dev, torch.float32)
            r = gpu.nmf_cd(mat, W, H, inplace=True, **kw)
            assert r.W is W and r.H is H and bool((wide[:, 1::2] == -7.0).all())
            out.append((W.cpu().numpy().copy(), H.cpu().numpy().copy(), r))
    finally:
        mat.close()
    (Wg, Hg, r), (Wg2, Hg2, _) = out
    ref32 = dict(ref, W=ref["W"].astype(np.float32).astype(np.float64), H=ref["H"].astype(np.float32).astype(np.float64))
    _compare(Wg.astype(np.float64), Hg.astype(np.float64), r.n_iter, r.violation / r.violation_init, ref32, name + " fp32 views")
    assert np.array_equal(Wg, Wg2) and np.array_equal(Hg, Hg2)


def test_update_w_false(gpu):
    """W is untouched bit for bit, H is the restatement's, and W'A is formed once: one pass over A however many sweeps"""
    import torch
    name = "d96_plain"
    A, _, _, _, kw, fitted = _reference(name)
    W = fitted["W"]
    k = W.shape[1]
    H0 = np.full((k, A.shape[1]), np.sqrt(A.mean() / k))
    ref = R.fit(A, W, H0, update_W=False, **kw)
    dev = torch.device("cuda", 0)
    Wt, Ht = torch.from_numpy(W).to(dev), torch.from_numpy(H0).to(dev)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_cd(mat, Wt, Ht, update_W=False, inplace=True, **kw)
        from smallk_amd.solver import cd_last_profile
        products, sweeps = cd_last_profile()
    finally:
        mat.close()
    assert np.array_equal(Wt.cpu().numpy(), W)
    _compare(W, Ht.cpu().numpy(), r.n_iter, r.violation / r.violation_init, dict(ref, W=W), name + " update_W=False")
    assert r.n_iter > 1 and products == 1 and sweeps == r.n_iter


# ---- the estimator -----------------------------------------------------------------------------------------------------------
def test_estimator_is_nmf_cd_of_the_transpose(gpu):
    import scipy.sparse as sp
    for name in ("d96_elastic", "s300_sparse"):
        A, csc, W0, H0, kw, _ = _reference(name)
        k = W0.shape[1]
        mat = _matrix(gpu, name)
        try:
            r = gpu.nmf_cd(mat, W0, H0, **kw)
            resid = mat.residual(r.W, r.H)
        finally:
            mat.close()
        X = np.ascontiguousarray(A.T)                    # samples x features
        if csc is not None:
            vals, rows, indptr, shape = csc              # the CSC of A is the CSR of X = A', the duplicate entry included
            X = sp.csr_matrix((vals, rows.astype(np.int32), indptr.astype(np.int32)), shape=(shape[1], shape[0]))
        # sklearn's alpha_W weighs its W = H', its alpha_H the components W'
        est = gpu.NMF(k, init="custom", alpha_W=kw["alpha_H"], alpha_H=kw["alpha_W"], l1_ratio=kw["l1_ratio"], tol=kw["tol"], max_iter=kw["max_iter"])
        Wsk = est.fit_transform(X, W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
        assert np.array_equal(Wsk, r.H.T) and np.array_equal(est.components_, r.W.T)
        assert est.n_iter_ == r.n_iter and est.n_components_ == k
        assert est.reconstruction_err_ == np.sqrt(resid.resid_sq)
        assert abs(est.reconstruction_err_ - np.linalg.norm(A - r.W @ r.H)) <= 1e-9 * est.reconstruction_err_
        assert np.allclose(est.inverse_transform(Wsk), (r.W @ r.H).T, rtol=0, atol=1e-12 * A.max())


def test_estimator_transform_of_the_training_data(gpu):
    """transform(X) of the training data of a converged fit: the restatement's update_W = False run from the constant start"""
    name = "d96_plain"
    A, _, W0, H0, kw, ref = _reference(name)
    k = W0.shape[1]
    X = np.ascontiguousarray(A.T)
    est = gpu.NMF(k, init="custom", tol=kw["tol"], max_iter=kw["max_iter"])
    est.fit(X, W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
    assert est.n_iter_ == ref["n_iter"] and ref["converged"]
    W = est.components_.T
    tref = R.fit(A, W, np.full((k, A.shape[1]), np.sqrt(A.mean() / k)), update_W=False, **kw)
    got = est.transform(X)
    top = tref["H"].max()
    e = np.abs(got.T - tref["H"]).max() / top
    print(f"transform: {e:.2e} (bar {R.FIT_BAR:.0e}), {tref['n_iter']} iterations")
    assert e <= R.FIT_BAR and np.array_equal(got.T == 0, tref["H"] == 0)


def test_estimator_default_and_random_starts(gpu):
    """init=None (NNDSVDA on the device) and init="random" run, descend and are repeatable; a tensor in gives tensors out"""
    import torch
    A = R.fit_case("d96_plain")[0]
    X = np.ascontiguousarray(A.T)
    for init in (None, "random"):
        a = gpu.NMF(5, init=init, random_state=3, max_iter=30).fit(X)
        b = gpu.NMF(5, init=init, random_state=3, max_iter=30).fit(X)
        assert np.array_equal(a.components_, b.components_) and a.components_.shape == (5, A.shape[0])
        assert (a.components_ >= 0).all() and a.reconstruction_err_ < 0.5 * np.linalg.norm(A)
    Xt = torch.from_numpy(X).to(torch.device("cuda", 0))
    t = gpu.NMF(5, init="nndsvda", max_iter=30)
    Wt = t.fit_transform(Xt)
    assert isinstance(Wt, torch.Tensor) and isinstance(t.components_, torch.Tensor) and tuple(Wt.shape) == (A.shape[1], 5)
    assert np.array_equal(t.components_.cpu().numpy(), gpu.NMF(5, init="nndsvda", max_iter=30).fit(X).components_)


# ---- error returns -----------------------------------------------------------------------------------------------------------
def test_error_returns_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    A = rng.integers(0, 8, (140, 130)).astype(np.float64)

    def attempt(mat, k, code, **kw):
        W = torch.from_numpy(rng.random((mat.height, k))).to(dev)
        H = torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            gpu.nmf_cd(mat, W, H, inplace=True, **kw)
        assert e.value.code == code, (kw, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())

    mat = gpu.DenseMatrix.from_host(A)
    single = gpu.DenseMatrix.from_host(A, single_copy=True)
    try:
        attempt(mat, 129, L.UNSUPPORTED)
        attempt(single, 4, L.UNSUPPORTED)
        attempt(mat, 4, L.BAD_PARAM, l1_ratio=1.5)
        attempt(mat, 4, L.BAD_PARAM, alpha_W=-1e-3)
        attempt(mat, 4, L.BAD_PARAM, alpha_W=0.0, alpha_H=-1e-3)
        attempt(mat, 4, L.BAD_PARAM, max_iter=0)
        attempt(mat, 4, L.BAD_PARAM, tol=-1.0)
    finally:
        mat.close()
        single.close()

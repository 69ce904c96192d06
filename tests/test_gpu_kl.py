"""KL-divergence NMF on the device (smallk_amd.nmf_kl, SparseMatrix.kl_divergence, NMF(solver="mu", beta_loss="kullback-leibler");
smallk_amd/csrc/kl.hip, kl.cpp) against the numpy restatement tests/kl_reference.py and against scikit-learn's
recorded result (tests/golden/kl_sklearn.npz).  That the cases hold these bars by themselves -- no zero pattern, no iteration count
hangs on a rounding -- is checked on the CPU by tests/test_kl_cpu.py.  Meant to pass under SMK_POISON=1 as well.

Bars (u = 2^-53).  One H step / one W step by itself against the numpy.longdouble restatement, entry by entry and relative (every
summand is non-negative): 4 (k + L) u with L the longest column of the side swept, exact zeros equal.  A fit: the restatement's
n_iter, factors within 1e-12 of the largest factor entry, W's zero pattern, error_init and error within 1e-12 relative, the same
bits on a second run.  The divergence: within 1e-12 (sum |a log(a / d)| + sum a + sum WH) of the longdouble value."""
import functools
import os

import numpy as np
import pytest

import kl_cases as C
import kl_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kl_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the restatement's fit, formed once per session (its quick summation order; test_kl_cpu.py holds the orders together)"""
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], order="gemm", **c["kw"])


def _matrix(gpu, name):
    vals, rows, indptr, shape = C.case(name)["csc"]
    return gpu.SparseMatrix(vals, rows, indptr, shape)


def _penalties(c):
    m, n = c["A"].shape
    kw = c["kw"]
    return (m * kw["alpha_H"] * kw["l1_ratio"], m * kw["alpha_H"] * (1 - kw["l1_ratio"]),
            n * kw["alpha_W"] * kw["l1_ratio"], n * kw["alpha_W"] * (1 - kw["l1_ratio"]))


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    err = np.asarray(np.abs(got.astype(np.longdouble) - ref) / np.where(live, ref, 1), dtype=np.float64)
    worst = err[live].max() if live.any() else 0.0
    print(f"{tag}: {worst / R.U53:.1f} u (bar {bar / R.U53:.0f} u), {int((~live).sum())} exact zeros")
    assert np.array_equal(got == 0, ref64 == 0)
    assert worst <= bar


# ---- one H step and one W step by themselves -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_one_step_of_each_side(gpu, name):
    c = C.case(name)
    E = R.Entries(c["A"])
    l1h, l2h, l1w, l2w = _penalties(c)
    Lc, Lr = C.longest(c["A"])
    ld = np.longdouble
    kw = dict(c["kw"], tol=0.0, max_iter=1)
    mat = _matrix(gpu, name)
    try:
        h = gpu.nmf_kl(mat, c["W0"], c["H0"], update_W=False, **kw)
        both = gpu.nmf_kl(mat, c["W0"], c["H0"], **kw)
    finally:
        mat.close()
    Href = R.step_h(E, c["W0"].astype(ld), c["H0"].astype(ld), l1h, l2h)
    assert np.array_equal(h.W, c["W0"]) and h.n_iter == 1 and not h.converged
    _check_step(h.H, Href, R.step_bar(c["k"], Lc), f"{name} H step (k {c['k']}, L {Lc})")
    # the W step from the device's own new H: what is compared is the W step alone
    assert np.array_equal(both.H, h.H)
    Wref = R.step_w(E, c["W0"].astype(ld), both.H.astype(ld), l1w, l2w)
    _check_step(both.W, Wref, R.step_bar(c["k"], Lr), f"{name} W step (k {c['k']}, L {Lr})")
    if name == "degenerate_k4":
        t, j = C.DEGENERATE_COMPONENT, C.DEGENERATE_COLUMN
        assert (h.H[t] == 0).all() and (h.H[:, j] == 0).all() and (both.W[:, t] == 0).all() and np.isfinite(both.W).all()


# ---- whole fits --------------------------------------------------------------------------------------------------------------
def _compare_fit(r, ref, tag):
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    e0, e1 = abs(r.error_init - ref["error_init"]) / ref["error_init"], abs(r.error - ref["error"]) / ref["error"]
    print(f"fit {tag}: n_iter {r.n_iter} (restatement {ref['n_iter']}), W {ew:.2e} H {eh:.2e} (bar {R.FIT_BAR:.0e}), error_init {e0:.2e} error {e1:.2e}")
    assert r.n_iter == ref["n_iter"]
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert np.array_equal(r.W == 0, ref["W"] == 0)
    assert e0 <= 1e-12 and e1 <= 1e-12


@pytest.mark.parametrize("name", list(C.CASES))
def test_fit(gpu, name):
    c, ref = C.case(name), _reference(name)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_kl(mat, c["W0"], c["H0"], **c["kw"])
        r2 = gpu.nmf_kl(mat, c["W0"], c["H0"], **c["kw"])
        d = mat.kl_divergence(r.W, r.H)
    finally:
        mat.close()
    _compare_fit(r, ref, name)
    assert r.converged == ref["converged"]
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.n_iter, r.error_init, r.error) == (r2.n_iter, r2.error_init, r2.error)
    assert d.error == r.error
    if name in C.GOLDEN_CASES:            # scikit-learn's own numbers, at the same bar
        g = np.load(GOLDEN)
        sk = {"W": g[f"{name}/W"], "H": g[f"{name}/H"], "n_iter": int(g[f"{name}/n_iter"]), "error_init": ref["error_init"],
              "error": float(g[f"{name}/reconstruction_err"])}
        _compare_fit(r, sk, name + " against sklearn")


# ---- the divergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5", "k17_elastic", "k128", "degenerate_k4", "kmin_k30"])
def test_divergence(gpu, name):
    c = C.case(name)
    E = R.Entries(c["A"])
    ld = np.longdouble
    mat = _matrix(gpu, name)
    try:
        starts = [(c["W0"], c["H0"])]
        if name == "k5":
            starts.append((_reference(name)["W"], _reference(name)["H"]))      # near the optimum: D is small beside its terms
        for W, H in starts:
            got = mat.kl_divergence(W, H)
            D, alog, swh, mag, sa = R.divergence(E, W.astype(ld), H.astype(ld))
            bar = 1e-12 * float(mag + sa + swh)
            print(f"divergence {name}: D {got.divergence:.6e}, off by {abs(got.divergence - float(D)):.2e} (bar {bar:.2e})")
            assert abs(got.divergence - D) <= bar and abs(got.a_log_ratio - alog) <= bar and abs(got.sum_wh - swh) <= bar
            assert got == mat.kl_divergence(W, H)
    finally:
        mat.close()


# ---- fold-in -----------------------------------------------------------------------------------------------------------------
def test_fold_in(gpu):
    """update_W=False leaves W bit for bit, sweeps the entries once per iteration, and NMF.transform is sklearn's transform"""
    import scipy.sparse as sp
    import torch
    from smallk_amd.solver import kl_last_profile
    name = C.TRANSFORM_CASE
    c = C.case(name)
    g = np.load(GOLDEN)
    W, want = g[f"{name}/W"], g[f"{name}/transform_H"]
    k = c["k"]
    H0 = np.full((k, c["A"].shape[1]), np.sqrt(c["X"].mean() / k))
    dev = torch.device("cuda", 0)
    Wt, Ht = torch.from_numpy(W).to(dev), torch.from_numpy(H0).to(dev)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_kl(mat, Wt, Ht, update_W=False, inplace=True, **c["kw"])
        entry, div = kl_last_profile()
        gpu.nmf_kl(mat, c["W0"], c["H0"], **dict(c["kw"], max_iter=20))
        entry2, div2 = kl_last_profile()
    finally:
        mat.close()
    assert np.array_equal(Wt.cpu().numpy(), W)
    assert r.n_iter > 1 and entry == r.n_iter and div == 1 + r.n_iter // 10 + (1 if r.n_iter % 10 else 0)
    assert (entry2, div2) == (40, 3)
    e = np.abs(Ht.cpu().numpy() - want).max() / want.max()
    print(f"fold-in: {r.n_iter} iterations, {e:.2e} from sklearn's transform")
    assert e <= 1e-12
    est = gpu.NMF(k, solver="mu", beta_loss="kullback-leibler", init="custom", **c["sk"])
    X = sp.csr_matrix(c["X"])
    est.fit(X, W=c["Wsk0"], H=c["Hsk0"])
    got = est.transform(X)
    e = np.abs(got.T - want).max() / want.max()
    print(f"NMF.transform: {e:.2e} from sklearn's transform")
    assert e <= 1e-12


# ---- the estimator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k17_elastic", "k3_l1"])
def test_estimator_end_to_end(gpu, name):
    import scipy.sparse as sp
    c = C.case(name)
    g = np.load(GOLDEN)
    est = gpu.NMF(c["k"], solver="mu", beta_loss="kullback-leibler", init="custom", **c["sk"])
    Wsk = est.fit_transform(sp.csr_matrix(c["X"]), W=c["Wsk0"], H=c["Hsk0"])
    top = max(g[f"{name}/W"].max(), g[f"{name}/H"].max())
    ew, eh = np.abs(est.components_.T - g[f"{name}/W"]).max() / top, np.abs(Wsk.T - g[f"{name}/H"]).max() / top
    err = float(g[f"{name}/reconstruction_err"])
    print(f"estimator {name}: n_iter {est.n_iter_}, components {ew:.2e}, fit_transform {eh:.2e}, reconstruction_err {abs(est.reconstruction_err_ - err) / err:.2e}")
    assert est.n_iter_ == int(g[f"{name}/n_iter"]) and est.n_components_ == c["k"]
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert abs(est.reconstruction_err_ - err) <= 1e-12 * err
    assert np.allclose(est.inverse_transform(Wsk), Wsk @ est.components_, rtol=0, atol=1e-12 * c["X"].max())


def test_estimator_default_start_descends(gpu):
    """init=None (NNDSVDA on the device, no zeros) and init="random" run, descend and are repeatable"""
    import scipy.sparse as sp
    c = C.case("k5")
    X = sp.csr_matrix(c["X"])
    start = _reference("k5")["error_init"]
    for init in (None, "random"):
        a = gpu.NMF(5, solver="mu", beta_loss=1, init=init, random_state=3, max_iter=30, tol=1e-3).fit(X)
        b = gpu.NMF(5, solver="mu", beta_loss=1, init=init, random_state=3, max_iter=30, tol=1e-3).fit(X)
        assert np.array_equal(a.components_, b.components_) and a.components_.shape == (5, c["A"].shape[0])
        assert (a.components_ >= 0).all() and np.isfinite(a.components_).all() and 0 < a.reconstruction_err_ < start


# ---- error returns -----------------------------------------------------------------------------------------------------------
def test_error_returns_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    c = C.case("k64")                      # 140 x 260: k = 129 is within min(m, n)
    vals, rows, indptr, shape = c["csc"]

    def attempt(mat, k, code, divergence=True, **kw):
        W = torch.from_numpy(rng.random((mat.height, k))).to(dev)
        H = torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            gpu.nmf_kl(mat, W, H, inplace=True, **kw)
        assert e.value.code == code, (kw, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())
        if divergence and not kw:          # refused for what the matrix or k is: the divergence by itself refuses alike
            with pytest.raises(L.SmallkError) as e:
                mat.kl_divergence(W, H)
            assert e.value.code == code, e.value

    mat = gpu.SparseMatrix(vals, rows, indptr, shape)
    dense = gpu.DenseMatrix.from_host(c["A"])
    # column 0 stores its first entry twice
    dup = gpu.SparseMatrix(np.concatenate([vals[:1], vals]), np.concatenate([rows[:1], rows]), np.concatenate([[0], indptr[1:] + 1]), shape)
    neg_vals = vals.copy()
    neg_vals[7] = -1.0
    neg = gpu.SparseMatrix(neg_vals, rows, indptr, shape)
    try:
        attempt(dense, 4, L.UNSUPPORTED, divergence=False)       # (kl_divergence is a method of SparseMatrix)
        attempt(dup, 4, L.UNSUPPORTED)
        attempt(mat, 129, L.UNSUPPORTED)
        attempt(neg, 4, L.BAD_PARAM)
        attempt(mat, 141, L.BAD_PARAM)
        attempt(mat, 4, L.BAD_PARAM, l1_ratio=1.5)
        attempt(mat, 4, L.BAD_PARAM, alpha_W=-1e-3)
        attempt(mat, 4, L.BAD_PARAM, max_iter=0)
        attempt(mat, 4, L.BAD_PARAM, tol=-1.0)
    finally:
        for x in (mat, dense, dup, neg):
            x.close()


def test_fp32_views_and_a_strided_w(gpu):
    """fp32 factor views, W a view of every second column of a wider tensor, updated in place: the start rounded to fp32 goes in,
    the iteration runs in fp64 and the result is rounded to fp32 once on the way out -- the restatement from the rounded start,
    to fp32's rounding"""
    import torch
    name = "k5"
    c = C.case(name)
    kw = dict(c["kw"], max_iter=10)
    W32, H32 = c["W0"].astype(np.float32), c["H0"].astype(np.float32)
    ref = R.fit(c["A"], W32.astype(np.float64), H32.astype(np.float64), **kw)
    dev = torch.device("cuda", 0)
    mat = _matrix(gpu, name)
    try:
        out = []
        for _ in range(2):
            wide = torch.full((c["A"].shape[0], 2 * c["k"]), -7.0, dtype=torch.float32, device=dev)
            W = wide[:, ::2]
            W.copy_(torch.from_numpy(W32))
            H = torch.from_numpy(H32).to(dev)
            r = gpu.nmf_kl(mat, W, H, inplace=True, **kw)
            assert r.W is W and r.H is H and bool((wide[:, 1::2] == -7.0).all())
            out.append((W.cpu().numpy().copy(), H.cpu().numpy().copy(), r))
    finally:
        mat.close()
    (Wg, Hg, r), (Wg2, Hg2, _) = out
    assert r.n_iter == ref["n_iter"] == 10 and abs(r.error - ref["error"]) <= 1e-12 * ref["error"]
    # one rounding to fp32 of a value that is right to 1e-12: half an ulp of fp32 and a little
    assert (np.abs(Wg - ref["W"]) <= 2.0 ** -24 * 1.001 * ref["W"]).all() and (np.abs(Hg - ref["H"]) <= 2.0 ** -24 * 1.001 * ref["H"]).all()
    assert np.array_equal(Wg, Wg2) and np.array_equal(Hg, Hg2)

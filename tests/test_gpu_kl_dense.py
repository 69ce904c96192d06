"""KL-divergence NMF on a dense resident matrix (smallk_amd.nmf_kl_dense, DenseMatrix.kl_divergence; smallk_amd/csrc/kl_dense.hip,
kl_dense.cpp) against the numpy restatement tests/kl_reference.py -- whose "stored entries" are the non-zeros of the
dense array: the same mathematics --, against scikit-learn's recorded result (tests/golden/kl_dense_sklearn.npz) and against the
sparse path on the same data.  That the cases hold these bars by themselves is checked on the CPU by tests/test_kl_dense_cpu.py.
Meant to pass under SMK_POISON=1 as well (the switch is read once per process, so no test here sets it).

Bars (u = 2^-53).  One H step / one W step by itself against the numpy.longdouble restatement, entry by entry and relative (every
summand is non-negative, so the bar holds for any summation order): 4 (k + L) u with L the rows swept -- m for H, n for W --, exact
zeros equal.  A fit: the restatement's n_iter and converged, factors within 1e-12 of the largest factor entry, W's zero pattern,
error_init and error within 1e-12 relative, the same bits on a second run.  The divergence: within 1e-12 (sum |a log(a / d)| +
sum a + sum WH) of the longdouble value."""
import functools
import os

import numpy as np
import pytest

import kl_cases as S
import kl_dense_cases as C
import kl_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kl_dense_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the restatement's fit, formed once per session (its quick summation order; test_kl_dense_cpu.py holds the orders together)"""
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], order="gemm", **c["kw"])


def _matrix(gpu, name, **kw):
    c = C.case(name)
    return gpu.DenseMatrix.from_host(c["A"], storage=kw.pop("storage", c["storage"]), **kw)


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
@pytest.mark.parametrize("name", C.STEP_CASES)
def test_one_step_of_each_side(gpu, name):
    c = C.case(name)
    E = R.Entries(c["A"])
    m, n = c["A"].shape
    l1h, l2h, l1w, l2w = _penalties(c)
    ld = np.longdouble
    kw = dict(c["kw"], tol=0.0, max_iter=1)
    mat = _matrix(gpu, name)
    try:
        h = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], update_W=False, **kw)
        both = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **kw)
    finally:
        mat.close()
    Href = R.step_h(E, c["W0"].astype(ld), c["H0"].astype(ld), l1h, l2h)
    assert np.array_equal(h.W, c["W0"]) and h.n_iter == 1 and not h.converged
    _check_step(h.H, Href, R.step_bar(c["k"], m), f"{name} H step (k {c['k']}, L {m})")
    # the W step from the device's own new H: what is compared is the W step alone
    assert np.array_equal(both.H, h.H)
    Wref = R.step_w(E, c["W0"].astype(ld), both.H.astype(ld), l1w, l2w)
    _check_step(both.W, Wref, R.step_bar(c["k"], n), f"{name} W step (k {c['k']}, L {n})")


# ---- whole fits --------------------------------------------------------------------------------------------------------------
def _compare_fit(r, ref, tag):
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    e0, e1 = abs(r.error_init - ref["error_init"]) / ref["error_init"], abs(r.error - ref["error"]) / ref["error"]
    print(f"fit {tag}: n_iter {r.n_iter} (reference {ref['n_iter']}), W {ew:.2e} H {eh:.2e} (bar {R.FIT_BAR:.0e}), error_init {e0:.2e} error {e1:.2e}")
    assert r.n_iter == ref["n_iter"]
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert np.array_equal(r.W == 0, ref["W"] == 0)
    assert e0 <= 1e-12 and e1 <= 1e-12


@pytest.mark.parametrize("name", list(C.CASES))
def test_fit(gpu, name):
    c, ref = C.case(name), _reference(name)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **c["kw"])
        r2 = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **c["kw"])
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


@pytest.mark.parametrize("name", ["k5", "k33"])
def test_dense_against_sparse(gpu, name):
    """the term-document cases of the sparse path (tests/kl_cases.py), once as a dense matrix and once as a CSC"""
    c = S.case(name)
    vals, rows, indptr, shape = c["csc"]
    dense, sparse = gpu.DenseMatrix.from_host(c["A"]), gpu.SparseMatrix(vals, rows, indptr, shape)
    try:
        rd = gpu.nmf_kl_dense(dense, c["W0"], c["H0"], **c["kw"])
        rs = gpu.nmf_kl(sparse, c["W0"], c["H0"], **c["kw"])
    finally:
        dense.close()
        sparse.close()
    top = max(rs.W.max(), rs.H.max())
    ew, eh = np.abs(rd.W - rs.W).max() / top, np.abs(rd.H - rs.H).max() / top
    print(f"dense against sparse {name}: n_iter {rd.n_iter} / {rs.n_iter}, W {ew:.2e} H {eh:.2e}")
    assert rd.n_iter == rs.n_iter == S.SKLEARN_N_ITER[name] and rd.converged == rs.converged
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert abs(rd.error - rs.error) <= 1e-12 * rs.error and abs(rd.error_init - rs.error_init) <= 1e-12 * rs.error_init


def test_bf16_storage_gives_what_fp32_storage_gives(gpu):
    """counts up to 255 are exact in bf16: the stored values are the same numbers, and so is the fit"""
    name = "d_k33"
    c, ref = C.case(name), _reference(name)
    assert c["A"].max() <= 255 and np.array_equal(c["A"], np.round(c["A"]))
    out = {}
    for storage in ("bf16", "f32"):
        mat = _matrix(gpu, name, storage=storage)
        try:
            out[storage] = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **c["kw"])
        finally:
            mat.close()
    _compare_fit(out["bf16"], ref, name + " bf16")
    top = max(out["f32"].W.max(), out["f32"].H.max())
    assert out["bf16"].n_iter == out["f32"].n_iter
    assert np.abs(out["bf16"].W - out["f32"].W).max() <= R.FIT_BAR * top and np.abs(out["bf16"].H - out["f32"].H).max() <= R.FIT_BAR * top


# ---- the divergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_k5", "d_k17_elastic", "d_k65", "d_k128", "d_spans_k8", "d_real_k6"])
def test_divergence(gpu, name):
    c = C.case(name)
    E = R.Entries(c["A"])
    ld = np.longdouble
    mat = _matrix(gpu, name)
    try:
        starts = [(c["W0"], c["H0"])]
        if name == "d_k5":
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
    """update_W=False leaves W bit for bit, gives the restatement's H, and reads the matrix once per iteration; a fit reads a
    stored copy twice per iteration"""
    import torch
    name = "d_k5"
    c = C.case(name)
    W = _reference(name)["W"]
    k = c["k"]
    H0 = np.full((k, c["A"].shape[1]), np.sqrt(c["X"].mean() / k))
    ref = R.fit(c["A"], W, H0, update_W=False, order="gemm", **c["kw"])
    dev = torch.device("cuda", 0)
    Wt, Ht = torch.from_numpy(W).to(dev), torch.from_numpy(H0).to(dev)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_kl_dense(mat, Wt, Ht, update_W=False, inplace=True, **c["kw"])
        passes, div = gpu.kl_dense_last_profile()
        gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **dict(c["kw"], max_iter=20))
        passes2, div2 = gpu.kl_dense_last_profile()
    finally:
        mat.close()
    assert np.array_equal(Wt.cpu().numpy(), W)
    assert r.n_iter == ref["n_iter"] > 1 and r.converged == ref["converged"]
    assert passes == r.n_iter and div == 1 + r.n_iter // 10 + (1 if r.n_iter % 10 else 0)
    assert (passes2, div2) == (40, 3)
    e = np.abs(Ht.cpu().numpy() - ref["H"]).max() / ref["H"].max()
    print(f"fold-in: {r.n_iter} iterations, {e:.2e} from the restatement")
    assert e <= R.FIT_BAR and abs(r.error - ref["error"]) <= 1e-12 * ref["error"]


# ---- views -------------------------------------------------------------------------------------------------------------------
def test_fp32_views_and_a_strided_w(gpu):
    """fp32 factor views, W a view of every second column of a wider tensor, updated in place: the start rounded to fp32 goes in,
    the iteration runs in fp64 and the result is rounded to fp32 once on the way out -- the restatement from the rounded start,
    to fp32's rounding"""
    import torch
    name = "d_k5"
    c = C.case(name)
    kw = dict(c["kw"], max_iter=10)
    W32, H32 = c["W0"].astype(np.float32), c["H0"].astype(np.float32)
    ref = R.fit(c["A"], W32.astype(np.float64), H32.astype(np.float64), order="gemm", **kw)
    dev = torch.device("cuda", 0)
    mat = _matrix(gpu, name)
    try:
        out = []
        for _ in range(2):
            wide = torch.full((c["A"].shape[0], 2 * c["k"]), -7.0, dtype=torch.float32, device=dev)
            W = wide[:, ::2]
            W.copy_(torch.from_numpy(W32))
            H = torch.from_numpy(H32).to(dev)
            r = gpu.nmf_kl_dense(mat, W, H, inplace=True, **kw)
            assert r.W is W and r.H is H and bool((wide[:, 1::2] == -7.0).all())
            out.append((W.cpu().numpy().copy(), H.cpu().numpy().copy(), r))
    finally:
        mat.close()
    (Wg, Hg, r), (Wg2, Hg2, _) = out
    assert r.n_iter == ref["n_iter"] == 10 and abs(r.error - ref["error"]) <= 1e-12 * ref["error"]
    # one rounding to fp32 of a value that is right to 1e-12: half an ulp of fp32 and a little
    assert (np.abs(Wg - ref["W"]) <= 2.0 ** -24 * 1.001 * ref["W"]).all() and (np.abs(Hg - ref["H"]) <= 2.0 ** -24 * 1.001 * ref["H"]).all()
    assert np.array_equal(Wg, Wg2) and np.array_equal(Hg, Hg2)


# ---- error returns -----------------------------------------------------------------------------------------------------------
def test_error_returns_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    c = C.case("d_k64")                    # 140 x 260: k = 129 is within min(m, n)
    s = S.case("k5")
    vals, rows, indptr, shape = s["csc"]

    def attempt(mat, k, code, divergence=True, **kw):
        W = torch.from_numpy(rng.random((mat.height, k))).to(dev)
        H = torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            gpu.nmf_kl_dense(mat, W, H, inplace=True, **kw)
        assert e.value.code == code, (kw, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())
        if divergence and not kw:          # refused for what the matrix or k is: the divergence by itself refuses alike
            with pytest.raises(L.SmallkError) as e:
                gpu.DenseMatrix.kl_divergence(mat, W, H)
            assert e.value.code == code, e.value
        return W, H

    mat = gpu.DenseMatrix.from_host(c["A"])
    sparse = gpu.SparseMatrix(vals, rows, indptr, shape)
    negA = c["A"].copy()
    negA[7, 11] = -1.0
    neg = gpu.DenseMatrix.from_host(negA)
    single = gpu.DenseMatrix.from_host(c["A"], single_copy=True)
    try:
        assert single.single_copy and not mat.single_copy
        attempt(sparse, 4, L.UNSUPPORTED)
        attempt(mat, 129, L.UNSUPPORTED)
        attempt(neg, 4, L.BAD_PARAM)
        attempt(mat, 141, L.BAD_PARAM)
        attempt(mat, 4, L.BAD_PARAM, l1_ratio=1.5)
        attempt(mat, 4, L.BAD_PARAM, alpha_W=-1e-3)
        attempt(mat, 4, L.BAD_PARAM, max_iter=0)
        attempt(mat, 4, L.BAD_PARAM, tol=-1.0)
        W, H = attempt(single, 4, L.UNSUPPORTED, divergence=False)
        # the same single copy serves the fold-in and the divergence, and gives what the two-copy matrix gives
        a = gpu.nmf_kl_dense(single, W, H, update_W=False, max_iter=10, tol=0.0)
        b = gpu.nmf_kl_dense(mat, W, H, update_W=False, max_iter=10, tol=0.0)
        assert a.n_iter == 10 and bool((a.H == b.H).all()) and bool((a.W == W).all()) and a.error == b.error
        assert single.kl_divergence(a.W, a.H) == mat.kl_divergence(b.W, b.H)
        # new contents are looked at again: the negative value goes, the refusal goes with it
        neg.upload(c["A"])
        assert gpu.nmf_kl_dense(neg, W, H, max_iter=1, tol=0.0).n_iter == 1
    finally:
        for x in (mat, sparse, neg, single):
            x.close()

"""Itakura-Saito and beta-divergence NMF on a dense resident matrix (smallk_amd.nmf_beta_dense, DenseMatrix.beta_divergence;
smallk_amd/csrc/beta_dense.hip, beta_dense.cpp) against the numpy restatement tests/beta_reference.py and against
scikit-learn's recorded result (tests/golden/beta_dense_sklearn.npz).  That the cases hold these bars by themselves is checked on
the CPU by tests/test_beta_dense_cpu.py.  Meant to pass under SMK_POISON=1 as well (the switch is read once per process, so no test
here sets it).

Bars (u = 2^-53).  One H step / one W step by itself against the numpy.longdouble restatement, entry by entry and relative (every
summand is non-negative, so the bar holds for any summation order): 4 (c k + L + 8 + P) u -- c = max(|beta - 2|, |beta - 1|, 1) the
amplification of d's rounding through the power, L the rows swept (m for H, n for W), 8 the fixed roundings of the quotients and the
update, P = 0 at beta = 0 and 16 for a general beta: an allowance for the device's power routine, a condition and not a measurement
--, exact zeros equal.  A fit: the restatement's n_iter and converged, factors within 1e-12 of the largest factor entry, the zero
patterns, error_init and error within 1e-12 relative, the same bits on a second run.  The divergence: within 1e-12 of the sum of the
absolute values of the terms D is formed from, against the longdouble value."""
import functools
import os

import numpy as np
import pytest

import beta_dense_cases as C
import beta_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_dense_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the float64 restatement's fit, formed once per session"""
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], **c["ref"])


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
    m, n = c["A"].shape
    beta = c["beta"]
    l1h, l2h, l1w, l2w = _penalties(c)
    ld = np.longdouble
    kw = dict(c["kw"], tol=0.0, max_iter=1)
    mat = _matrix(gpu, name)
    try:
        h = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], update_W=False, **kw)
        both = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **kw)
    finally:
        mat.close()
    Href = R.step_h(c["A"], c["W0"].astype(ld), c["H0"].astype(ld), beta, l1h, l2h)
    assert np.array_equal(h.W, c["W0"]) and h.n_iter == 1 and not h.converged
    _check_step(h.H, Href, R.step_bar(beta, c["k"], m), f"{name} H step (beta {beta}, k {c['k']}, L {m})")
    # the W step from the device's own new H: what is compared is the W step alone
    assert np.array_equal(both.H, h.H)
    Wref = R.step_w(c["A"], c["W0"].astype(ld), both.H.astype(ld), beta, l1w, l2w)
    _check_step(both.W, Wref, R.step_bar(beta, c["k"], n), f"{name} W step (beta {beta}, k {c['k']}, L {n})")


# ---- whole fits --------------------------------------------------------------------------------------------------------------
def _compare_fit(r, ref, tag):
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    e0, e1 = abs(r.error_init - ref["error_init"]) / ref["error_init"], abs(r.error - ref["error"]) / ref["error"]
    print(f"fit {tag}: n_iter {r.n_iter} (reference {ref['n_iter']}), W {ew:.2e} H {eh:.2e} (bar {R.FIT_BAR:.0e}), error_init {e0:.2e} error {e1:.2e}")
    assert r.n_iter == ref["n_iter"]
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR
    assert np.array_equal(r.W == 0, ref["W"] == 0) and np.array_equal(r.H == 0, ref["H"] == 0)
    assert e0 <= 1e-12 and e1 <= 1e-12


@pytest.mark.parametrize("name", list(C.CASES))
def test_fit(gpu, name):
    c, ref = C.case(name), _reference(name)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **c["kw"])
        r2 = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **c["kw"])
        d = mat.beta_divergence(r.W, r.H, c["beta"])
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


def test_itakura_saito_by_name(gpu):
    name = "is_k2"
    c = C.case(name)
    mat = _matrix(gpu, name)
    try:
        a = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **dict(c["kw"], beta_loss="itakura-saito"))
        b = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **c["kw"])
    finally:
        mat.close()
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and a.n_iter == b.n_iter == C.SKLEARN_N_ITER[name]


# ---- the divergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DIVERGENCE_CASES)
def test_divergence(gpu, name):
    c = C.case(name)
    ld = np.longdouble
    beta = c["beta"]
    mat = _matrix(gpu, name)
    try:
        starts = [(c["W0"], c["H0"])]
        if name == "is_k5":
            starts.append((_reference(name)["W"], _reference(name)["H"]))      # near the optimum: D is small beside its terms
        for W, H in starts:
            got = mat.beta_divergence(W, H, beta)
            D, mag, sums = R.divergence(c["A"], W.astype(ld), H.astype(ld), beta)
            bar = 1e-12 * float(mag)
            print(f"divergence {name}: D {got.divergence:.6e}, off by {abs(got.divergence - float(D)):.2e} (bar {bar:.2e})")
            assert got.beta == beta and abs(got.divergence - D) <= bar
            scale = abs(beta * (beta - 1.0)) if beta else 1.0               # the sums enter D divided by beta (beta - 1)
            for s_got, s_ref in zip(got.sums, sums):
                assert abs(s_got - s_ref) <= bar * max(scale, 1.0) * 4
            assert got == mat.beta_divergence(W, H, beta)
    finally:
        mat.close()


# ---- beta = 1 ----------------------------------------------------------------------------------------------------------------
def test_beta_one_is_nmf_kl_dense_bit_for_bit(gpu):
    import kl_dense_cases as K
    c = K.case("d_k16")
    mat = gpu.DenseMatrix.from_host(c["A"], storage=c["storage"])
    try:
        kl = gpu.nmf_kl_dense(mat, c["W0"], c["H0"], **c["kw"])
        for loss in (1.0, "kullback-leibler"):
            b = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], beta_loss=loss, **c["kw"])
            assert np.array_equal(kl.W, b.W) and np.array_equal(kl.H, b.H)
            assert (kl.n_iter, kl.converged, kl.error_init, kl.error) == (b.n_iter, b.converged, b.error_init, b.error)
        d1, dk = mat.beta_divergence(kl.W, kl.H, 1), mat.kl_divergence(kl.W, kl.H)
        assert d1.divergence == dk.divergence and d1.sums[:2] == (dk.a_log_ratio, dk.sum_wh)
    finally:
        mat.close()


# ---- bf16 storage ------------------------------------------------------------------------------------------------------------
def test_bf16_storage_gives_what_fp32_storage_gives(gpu):
    """is_k5's X rounded to bf16 (still strictly positive: its minimum is 0.0030): the stored values are the same numbers in
    either storage, and so is the fit"""
    import torch
    name = C.BF16_CASE
    c = C.case(name)
    A16 = torch.from_numpy(c["A"]).to(torch.bfloat16).to(torch.float64).numpy()
    assert A16.min() > 0 and not np.array_equal(A16, c["A"])
    ref = R.fit(A16, c["W0"], c["H0"], **c["ref"])
    assert ref["n_iter"] == 110 and min(ref["margins"]) >= 3e-3
    out = {}
    for storage in ("bf16", "f32"):
        mat = gpu.DenseMatrix.from_host(A16, storage=storage)
        try:
            out[storage] = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **c["kw"])
        finally:
            mat.close()
    _compare_fit(out["bf16"], ref, name + " bf16")
    assert np.array_equal(out["bf16"].W, out["f32"].W) and np.array_equal(out["bf16"].H, out["f32"].H)
    assert (out["bf16"].n_iter, out["bf16"].error) == (out["f32"].n_iter, out["f32"].error)


# ---- fold-in -----------------------------------------------------------------------------------------------------------------
def test_fold_in(gpu):
    """update_W=False leaves W bit for bit, gives the restatement's H, and reads the matrix once per iteration; a fit reads a
    stored copy twice per iteration"""
    import torch
    name = "is_k5"
    c = C.case(name)
    W = _reference(name)["W"]
    k = c["k"]
    H0 = np.full((k, c["A"].shape[1]), np.sqrt(c["X"].mean() / k))
    ref = R.fit(c["A"], W, H0, update_W=False, **c["ref"])
    dev = torch.device("cuda", 0)
    Wt, Ht = torch.from_numpy(W).to(dev), torch.from_numpy(H0).to(dev)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_beta_dense(mat, Wt, Ht, update_W=False, inplace=True, **c["kw"])
        passes, div = gpu.beta_dense_last_profile()
        gpu.nmf_beta_dense(mat, c["W0"], c["H0"], **dict(c["kw"], max_iter=20))
        passes2, div2 = gpu.beta_dense_last_profile()
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
    the iteration runs in fp64 and the result is rounded to fp32 once on the way out"""
    import torch
    name = "is_k5"
    c = C.case(name)
    kw = dict(c["kw"], max_iter=10)
    W32, H32 = c["W0"].astype(np.float32), c["H0"].astype(np.float32)
    ref = R.fit(c["A"], W32.astype(np.float64), H32.astype(np.float64), **dict(c["ref"], max_iter=10))
    dev = torch.device("cuda", 0)
    mat = _matrix(gpu, name)
    try:
        out = []
        for _ in range(2):
            wide = torch.full((c["A"].shape[0], 2 * c["k"]), -7.0, dtype=torch.float32, device=dev)
            W = wide[:, ::2]
            W.copy_(torch.from_numpy(W32))
            H = torch.from_numpy(H32).to(dev)
            r = gpu.nmf_beta_dense(mat, W, H, inplace=True, **kw)
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
    """the refusals of the C entry itself: the Python checks that would come first are stepped over where they would hide it"""
    import ctypes
    import torch
    import kl_cases as S
    from smallk_amd import _lib as L
    from smallk_amd import solver
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    c = C.case("is_k64")                    # 140 x 260: k = 129 is within min(m, n)
    s = S.case("k5")
    vals, rows, indptr, shape = s["csc"]

    def entry(mat, W, H, beta, **kw):
        """smk_nmf_beta_dense_device with no Python check before it"""
        return solver._penalised_fit("nmf_beta_dense", "DenseMatrix", "smk_nmf_beta_dense_device", L.KlStats, lambda st: (st.error_init, st.error),
                                     solver.KlResult, mat, W, H, alpha_W=kw.pop("alpha_W", 0.0), alpha_H="same", l1_ratio=kw.pop("l1_ratio", 0.0),
                                     tol=kw.pop("tol", 1e-4), max_iter=kw.pop("max_iter", 200), update_W=True, inplace=True,
                                     before_options=(ctypes.c_double(beta),))

    def attempt(mat, k, beta, code, match=None, divergence=True, **kw):
        W = torch.from_numpy(rng.random((mat.height, k))).to(dev)
        H = torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError, match=match) as e:
            entry(mat, W, H, beta, **kw)
        assert e.value.code == code, (kw, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())
        if divergence and not kw:          # refused for what the matrix, k or beta is: the divergence by itself refuses alike
            out = (ctypes.c_double * 4)()
            rc = L.lib().smk_matrix_beta_divergence_dense_device(mat._h, k, ctypes.c_double(beta), ctypes.c_void_p(W.data_ptr()), L.DT_F64, W.stride(0),
                                                                 W.stride(1), ctypes.c_void_p(H.data_ptr()), L.DT_F64, H.stride(0), H.stride(1), None, out)
            assert rc == code
        return W, H

    mat = gpu.DenseMatrix.from_host(c["A"])
    sparse = gpu.SparseMatrix(vals, rows, indptr, shape)
    negA, zeroA = c["A"].copy(), c["A"].copy()
    negA[7, 11] = -1.0
    zeroA[139, 259] = 0.0                  # the last entry: beside the padding, which is zeros and is not data
    neg, zero = gpu.DenseMatrix.from_host(negA), gpu.DenseMatrix.from_host(zeroA)
    single = gpu.DenseMatrix.from_host(c["A"], single_copy=True)
    try:
        assert single.single_copy and not mat.single_copy
        attempt(sparse, 4, 0.0, L.UNSUPPORTED)
        attempt(mat, 129, 0.0, L.UNSUPPORTED)
        attempt(mat, 4, 2.0, L.UNSUPPORTED, match="Frobenius")
        attempt(mat, 4, -0.5, L.BAD_PARAM)
        attempt(mat, 4, float("inf"), L.BAD_PARAM)
        attempt(mat, 4, float("nan"), L.BAD_PARAM)
        attempt(neg, 4, 0.0, L.BAD_PARAM, match="negative")
        attempt(neg, 4, 0.5, L.BAD_PARAM, match="negative")
        attempt(zero, 4, 0.0, L.BAD_PARAM, match="add a small value")
        attempt(mat, 141, 0.0, L.BAD_PARAM)
        attempt(mat, 4, 0.0, L.BAD_PARAM, l1_ratio=1.5)
        attempt(mat, 4, 0.0, L.BAD_PARAM, alpha_W=-1e-3)
        attempt(mat, 4, 0.0, L.BAD_PARAM, max_iter=0)
        attempt(mat, 4, 0.0, L.BAD_PARAM, tol=-1.0)
        W, H = attempt(single, 4, 0.0, L.UNSUPPORTED, divergence=False)
        # a stored zero is refused at beta <= 0 only; the strictly positive matrix is not refused (the padding is not data)
        assert gpu.nmf_beta_dense(zero, W, H, beta_loss=0.5, max_iter=1, tol=0.0).n_iter == 1
        assert gpu.nmf_beta_dense(mat, W, H, beta_loss=0, max_iter=1, tol=0.0).n_iter == 1
        # the same single copy serves the fold-in and the divergence, and gives what the two-copy matrix gives
        a = gpu.nmf_beta_dense(single, W, H, beta_loss=0, update_W=False, max_iter=10, tol=0.0)
        b = gpu.nmf_beta_dense(mat, W, H, beta_loss=0, update_W=False, max_iter=10, tol=0.0)
        assert a.n_iter == 10 and bool((a.H == b.H).all()) and bool((a.W == W).all()) and a.error == b.error
        assert single.beta_divergence(a.W, a.H, 0) == mat.beta_divergence(b.W, b.H, 0)
        # new contents are looked at again: the zero goes and the refusal goes with it, a zero comes and so does the refusal; the
        # KL entry's own record of a negative value follows the same contents
        zero.upload(c["A"])
        assert gpu.nmf_beta_dense(zero, W, H, beta_loss=0, max_iter=1, tol=0.0).n_iter == 1
        zero.upload(zeroA)
        with pytest.raises(L.SmallkError, match="add a small value"):
            gpu.nmf_beta_dense(zero, W, H, beta_loss=0, max_iter=1, tol=0.0)
        assert gpu.nmf_kl_dense(zero, W, H, max_iter=1, tol=0.0).n_iter == 1
        neg.upload(c["A"])
        assert gpu.nmf_beta_dense(neg, W, H, beta_loss=0, max_iter=1, tol=0.0).n_iter == 1
    finally:
        for x in (mat, sparse, neg, zero, single):
            x.close()

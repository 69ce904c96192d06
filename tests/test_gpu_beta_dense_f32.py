"""The fp32 form of the dense KL and Itakura-Saito solvers (nmf_kl_dense / nmf_beta_dense with precision="fp32";
smallk_amd/csrc/beta_dense_f32.hip, beta_dense_f32.cpp) against the numpy restatements tests/kl_reference.py and
tests/beta_reference.py.  Meant to pass under SMK_POISON=1 as well (the switch is read once per process, so no test here sets it).

Bars (u = 2^-24).  One H step / one W step from a start rounded to float32, against the numpy.longdouble restatement, entry by entry
and relative: the fp64 tests' own step_bar with u = 2^-24 in place of 2^-53 -- the same worst-case bound for sums of non-negative
terms with every rounding in fp32 --, exact zeros equal.  A 30-iteration fit: within 8 x the distance between the float64 and the
float32 restatement (two fp32 computations in different summation orders can each be that far from fp64), not below 16 u, for the
factors (max |difference| over the largest factor entry) and for `error` (relative).  The rest is exact."""
import functools

import numpy as np
import pytest

import beta_dense_cases as B
import beta_reference as BR
import kl_dense_cases as K
import kl_reference as KR

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
STEP_CASES = tuple(K.STEP_CASES) + tuple(n for n in B.STEP_CASES if B.CASES[n][4] == 0.0)
FIT_CASES = [("is_k16", "f32"), ("is_k64", "f32"), ("is_k65", "f32"), ("is_spans_k8", "f32"), ("is_k3_tile", "f32"),
             ("d_k16", "f32"), ("d_k65", "f32"), ("d_spans_k8", "f32"), ("d_k16", "bf16")]


def _case(name):
    """(the case, beta, its float32-rounded start as float64 arrays)"""
    c = K.case(name) if name.startswith("d_") else B.case(name)
    r32 = lambda x: x.astype(np.float32).astype(np.float64)
    return c, (1.0 if name.startswith("d_") else 0.0), r32(c["W0"]), r32(c["H0"])


def _run(gpu, mat, beta, W, H, precision="fp32", **kw):
    """the public call of that loss"""
    kw = {key: v for key, v in kw.items() if key != "beta_loss"}
    if beta == 1.0:
        return gpu.nmf_kl_dense(mat, W, H, precision=precision, **kw)
    return gpu.nmf_beta_dense(mat, W, H, beta_loss="itakura-saito", precision=precision, **kw)


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    err = np.asarray(np.abs(got.astype(np.longdouble) - ref) / np.where(live, ref, 1), dtype=np.float64)
    worst = err[live].max() if live.any() else 0.0
    print(f"{tag}: {worst / U24:.1f} u (bar {bar / U24:.0f} u), {int((~live).sum())} exact zeros")
    assert np.array_equal(got == 0, ref64 == 0)
    assert worst <= bar


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_of_each_side(gpu, name):
    c, beta, W0, H0 = _case(name)
    m, n = c["A"].shape
    k, ld = c["k"], np.longdouble
    kw = dict(c["kw"], tol=0.0, max_iter=1)
    mat = gpu.DenseMatrix.from_host(c["A"], storage=c["storage"])
    try:
        h = _run(gpu, mat, beta, W0, H0, update_W=False, **kw)
        both = _run(gpu, mat, beta, W0, H0, **kw)
    finally:
        mat.close()
    if beta == 1.0:
        E = KR.Entries(c["A"])
        step_h, step_w = (lambda W, H: KR.step_h(E, W, H, 0.0, 0.0)), (lambda W, H: KR.step_w(E, W, H, 0.0, 0.0))
        bar = lambda L: KR.step_bar(k, L) * 2.0 ** 29
    else:
        step_h, step_w = (lambda W, H: BR.step_h(c["A"], W, H, beta)), (lambda W, H: BR.step_w(c["A"], W, H, beta))
        bar = lambda L: BR.step_bar(beta, k, L) * 2.0 ** 29
    assert not any(c["kw"][p] for p in ("alpha_W", "alpha_H"))          # the step cases carry no penalties
    assert np.array_equal(h.W, W0) and h.n_iter == 1 and not h.converged
    _check_step(h.H, step_h(W0.astype(ld), H0.astype(ld)), bar(m), f"{name} H step (beta {beta}, k {k}, L {m})")
    # the W step from the device's own new H: what is compared is the W step alone
    assert np.array_equal(both.H, h.H) and np.array_equal(both.H, both.H.astype(np.float32))
    _check_step(both.W, step_w(W0.astype(ld), both.H.astype(ld)), bar(n), f"{name} W step (beta {beta}, k {k}, L {n})")


@functools.lru_cache(maxsize=None)
def _restatements(name):
    """the float64 and the float32 restatement of 30 iterations from the rounded start, formed once per session"""
    c, beta, W0, H0 = _case(name)
    if beta == 1.0:
        E = KR.Entries(c["A"])
        return tuple(KR.fit(E, W0, H0, tol=0.0, max_iter=30, dtype=dt) for dt in (np.float64, np.float32))
    return tuple(BR.fit(c["A"], W0, H0, beta=beta, tol=0.0, max_iter=30, dtype=dt) for dt in (np.float64, np.float32))


@pytest.mark.parametrize("name,storage", FIT_CASES)
def test_short_fit(gpu, name, storage):
    c, beta, W0, H0 = _case(name)
    ref64, ref32 = _restatements(name)
    mat = gpu.DenseMatrix.from_host(c["A"], storage=storage)
    try:
        r = _run(gpu, mat, beta, W0, H0, tol=0.0, max_iter=30)
        r2 = _run(gpu, mat, beta, W0, H0, tol=0.0, max_iter=30)
        f64 = _run(gpu, mat, beta, W0, H0, precision="fp64", tol=0.0, max_iter=1)
        d = mat.beta_divergence(r.W, r.H, beta)
    finally:
        mat.close()
    top = max(ref64["W"].max(), ref64["H"].max())
    dist = lambda a, b: max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / top
    rel = lambda a, b: abs(a - b) / ref64["error"]
    between, e_between = dist(ref32, ref64), rel(ref32["error"], ref64["error"])
    got, e_got = dist({"W": r.W, "H": r.H}, ref64), rel(r.error, ref64["error"])
    print(f"fit {name} {storage}: factors {got:.2e} from float64 (the float32 restatement {between:.2e}), error {e_got:.2e} ({e_between:.2e})")
    assert r.n_iter == 30 and not r.converged
    assert got <= max(8 * between, 16 * U24)
    assert e_got <= max(8 * e_between, 16 * U24)
    # exact: the error is the fp64 divergence of the returned factors, error_init the fp64 form's, the factors are fp32 numbers,
    # a second run gives the same bits
    assert d.error == r.error and r.error_init == f64.error_init
    assert np.array_equal(r.W, r.W.astype(np.float32)) and np.array_equal(r.H, r.H.astype(np.float32))
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.error_init, r.error) == (r2.error_init, r2.error)


@pytest.mark.parametrize("name", ["is_k16", "d_k16"])
def test_fold_in_and_views(gpu, name):
    """update_W=False leaves W bit for bit and reads the matrix once per iteration (a fit: twice); fp32 views, W a view of every
    second column of a wider tensor, updated in place, receive the fp64-view result rounded -- which is that result"""
    import torch
    c, beta, W0, H0 = _case(name)
    dev = torch.device("cuda", 0)
    mat = gpu.DenseMatrix.from_host(c["A"], storage=c["storage"])
    try:
        Wt, Ht = torch.from_numpy(c["W0"]).to(dev), torch.from_numpy(H0).to(dev)        # W not rounded: it must stay as it is
        f = _run(gpu, mat, beta, Wt, Ht, update_W=False, inplace=True, tol=0.0, max_iter=12)
        passes = gpu.beta_dense_f32_last_profile()
        r = _run(gpu, mat, beta, W0, H0, tol=0.0, max_iter=10)
        passes2 = gpu.beta_dense_f32_last_profile()
        wide = torch.full((c["A"].shape[0], 2 * c["k"]), -7.0, dtype=torch.float32, device=dev)
        W = wide[:, ::2]
        W.copy_(torch.from_numpy(W0.astype(np.float32)))
        H = torch.from_numpy(H0.astype(np.float32)).to(dev)
        v = _run(gpu, mat, beta, W, H, inplace=True, tol=0.0, max_iter=10)
    finally:
        mat.close()
    assert np.array_equal(Wt.cpu().numpy(), c["W0"]) and f.n_iter == 12 and passes == (12, 2) and passes2 == (20, 2)
    assert v.W is W and v.H is H and bool((wide[:, 1::2] == -7.0).all())
    assert np.array_equal(W.cpu().numpy(), r.W.astype(np.float32)) and np.array_equal(H.cpu().numpy(), r.H.astype(np.float32))
    assert np.array_equal(W.cpu().numpy().astype(np.float64), r.W) and v.error == r.error


def test_refusals_leave_the_factors_untouched(gpu):
    """the refusals of the C entry itself (the Python checks that would come first are stepped over), then those of the keyword"""
    import ctypes
    import torch
    import kl_cases as S
    from smallk_amd import _lib as L
    from smallk_amd import solver
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    c = B.case("is_k64")                    # 140 x 260: k = 129 is within min(m, n)
    negA, zeroA = c["A"].copy(), c["A"].copy()
    negA[7, 11] = -1.0
    zeroA[139, 259] = 0.0
    mats = {"dense": gpu.DenseMatrix.from_host(c["A"]), "sparse": gpu.SparseMatrix(*S.case("k5")["csc"]), "neg": gpu.DenseMatrix.from_host(negA),
            "zero": gpu.DenseMatrix.from_host(zeroA), "single": gpu.DenseMatrix.from_host(c["A"], single_copy=True)}

    def attempt(which, k, beta, code):
        mat = mats[which]
        W, H = torch.from_numpy(rng.random((mat.height, k))).to(dev), torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            solver._penalised_fit("nmf_beta_dense", "DenseMatrix", "smk_nmf_beta_dense_f32_device", L.KlStats, lambda st: (st.error_init, st.error),
                                  solver.KlResult, mat, W, H, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=5, update_W=True,
                                  inplace=True, before_options=(ctypes.c_double(beta),))
        assert e.value.code == code, (which, k, beta, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())
        return W, H

    try:
        for which, k, beta, code in (("dense", 4, 0.5, L.UNSUPPORTED), ("dense", 4, 3.0, L.UNSUPPORTED), ("sparse", 4, 0.0, L.UNSUPPORTED),
                                     ("dense", 129, 0.0, L.UNSUPPORTED), ("dense", 129, 1.0, L.UNSUPPORTED), ("single", 4, 1.0, L.UNSUPPORTED),
                                     ("zero", 4, 0.0, L.BAD_PARAM), ("neg", 4, 0.0, L.BAD_PARAM), ("neg", 4, 1.0, L.BAD_PARAM)):
            W, H = attempt(which, k, beta, code)
        # the single copy serves the fold-in, and gives what the two-copy matrix gives; a stored zero is served at beta = 1
        a = gpu.nmf_beta_dense(mats["single"], W, H, beta_loss=0, update_W=False, max_iter=5, tol=0.0, precision="fp32")
        b = gpu.nmf_beta_dense(mats["dense"], W, H, beta_loss=0, update_W=False, max_iter=5, tol=0.0, precision="fp32")
        assert a.n_iter == 5 and bool((a.H == b.H).all()) and a.error == b.error
        assert gpu.nmf_kl_dense(mats["zero"], W, H, max_iter=1, tol=0.0, precision="fp32").n_iter == 1
        W0, H0 = W.clone(), H.clone()
        for call, kw in ((gpu.nmf_beta_dense, dict(beta_loss=0.5, precision="fp32")), (gpu.nmf_beta_dense, dict(beta_loss=3, precision="fp32")),
                         (gpu.nmf_beta_dense, dict(beta_loss=0, precision="fp16")), (gpu.nmf_kl_dense, dict(precision="fp16"))):
            with pytest.raises(ValueError, match="precision"):
                call(mats["dense"], W, H, inplace=True, **kw)
        assert bool((W == W0).all()) and bool((H == H0).all())
    finally:
        for x in mats.values():
            x.close()


def test_fp64_is_the_call_without_the_keyword(gpu):
    c, beta, W0, H0 = _case("is_k16")
    mat = gpu.DenseMatrix.from_host(c["A"], storage=c["storage"])
    try:
        a = gpu.nmf_beta_dense(mat, W0, H0, beta_loss=0, max_iter=20)
        b = gpu.nmf_beta_dense(mat, W0, H0, beta_loss=0, max_iter=20, precision="fp64")
        ka, kb = gpu.nmf_kl_dense(mat, W0, H0, max_iter=20), gpu.nmf_kl_dense(mat, W0, H0, max_iter=20, precision="fp64")
    finally:
        mat.close()
    for x, y in ((a, b), (ka, kb)):
        assert np.array_equal(x.W, y.W) and np.array_equal(x.H, y.H) and (x.n_iter, x.error_init, x.error) == (y.n_iter, y.error_init, y.error)

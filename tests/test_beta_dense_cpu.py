"""The inputs of tests/test_gpu_beta_dense.py hold their bars by themselves: no device here.

* On every case of tests/beta_dense_cases.py the numpy restatement (tests/beta_reference.py) reproduces scikit-learn on the dense
  X -- live where sklearn imports, and the recorded result of the golden cases (tests/golden/beta_dense_sklearn.npz) -- with the
  same n_iter_ and factors within 1e-12 of the largest factor entry.
* The float64 restatement and the longdouble one agree in iteration count, zero patterns and, within FIT_BAR, the factors; at
  every check of the stopping rule the stop quantity stays 3e-3 tol away from tol (DESIGN 20's condition): what the GPU is held to
  is not decided by rounding.
* beta = 1 through the new restatement is tests/kl_reference.py's fit.
* The cases have the structure the GPU tests rely on, and the Python surface refuses what it can before any library call."""
import functools
import os
import warnings

import numpy as np
import pytest

import beta_dense_cases as C
import beta_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_dense_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _fit(name, dtype="float64"):
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], dtype=np.dtype(dtype), **c["ref"])


def _factor_diff(a, b):
    return max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / max(a["W"].max(), a["H"].max())


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_reproduces_live_sklearn(name):
    skd = pytest.importorskip("sklearn.decomposition")
    c = C.case(name)
    res = _fit(name)
    model = skd.NMF(n_components=c["k"], init="custom", solver="mu", **c["sk"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk = model.fit_transform(c["X"], W=c["Wsk0"].copy(), H=c["Hsk0"].copy())
    sk = {"W": model.components_.T, "H": Wsk.T}
    d = _factor_diff(sk, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {model.n_iter_}), factors {d:.2e} of the largest entry")
    assert res["n_iter"] == model.n_iter_ == C.SKLEARN_N_ITER[name]
    assert d <= 1e-12
    assert np.array_equal(sk["W"] == 0, res["W"] == 0) and np.array_equal(sk["H"] == 0, res["H"] == 0)
    assert abs(res["error"] - model.reconstruction_err_) <= 1e-12 * res["error"]


@pytest.mark.parametrize("name", C.GOLDEN_CASES)
def test_restatement_reproduces_the_recorded_sklearn_result(name):
    g = np.load(GOLDEN)
    c = C.case(name)
    assert np.array_equal(g[f"{name}/checksum"], [c["X"].sum(), c["W0"].sum(), c["H0"].sum()])
    res = _fit(name)
    d = _factor_diff({"W": g[f"{name}/W"], "H": g[f"{name}/H"]}, res)
    assert res["n_iter"] == int(g[f"{name}/n_iter"]) == C.SKLEARN_N_ITER[name]
    assert d <= 1e-12
    assert abs(res["error"] - float(g[f"{name}/reconstruction_err"])) <= 1e-12 * res["error"]


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_do_not_hang_on_rounding(name):
    """the margin property and the zero-pattern property, float64 against longdouble"""
    f64, ld = _fit(name), _fit(name, "longdouble")
    margin = min(f64["margins"] + ld["margins"])
    drift = _factor_diff(f64, ld)
    print(f"{name}: n_iter {f64['n_iter']}, float64 against longdouble {drift:.2e} (bar {R.FIT_BAR:.0e}), stop quantity to tol {margin:.2e} tol")
    assert ld["n_iter"] == f64["n_iter"] == C.SKLEARN_N_ITER[name] and ld["converged"] == f64["converged"]
    assert np.array_equal(ld["W"] == 0, f64["W"] == 0) and np.array_equal(ld["H"] == 0, f64["H"] == 0)
    assert abs(ld["error"] - f64["error"]) <= 1e-12 * f64["error"] and abs(ld["error_init"] - f64["error_init"]) <= 1e-12 * f64["error_init"]
    assert drift <= R.FIT_BAR
    assert margin >= 3e-3


def test_the_flush_has_work():
    """exact zeros made by the flush (beta < 1): in H (sklearn's W) from k = 16 on, in W too from k = 33 on"""
    assert int((_fit("is_k16")["H"] == 0).sum()) == 4 and C.case("is_k16")["A"].min() > 0
    for name in ("is_k33", "is_k64", "is_k65", "is_k128", "b05_k65"):
        assert (_fit(name)["W"] == 0).any() and (_fit(name)["H"] == 0).any()
    for name, c in C.CASES.items():
        if c[4] != 0:
            assert (_fit(name)["W"] == 0).any()


def test_single_steps_do_not_hang_on_rounding():
    """one H step and one W step by themselves: float64 stays within the GPU bar of the longdouble mode, equal zero patterns"""
    for name in C.STEP_CASES:
        c = C.case(name)
        m, n = c["A"].shape
        ld = np.longdouble
        b = c["beta"]
        Hl = np.asarray(R.step_h(c["A"], c["W0"].astype(ld), c["H0"].astype(ld), b), dtype=np.float64)
        Wl = np.asarray(R.step_w(c["A"], c["W0"].astype(ld), c["H0"].astype(ld), b), dtype=np.float64)
        Hd = R.step_h(c["A"], c["W0"].copy(), c["H0"].copy(), b)
        Wd = R.step_w(c["A"], c["W0"].copy(), c["H0"].copy(), b)
        assert (np.abs(Hd - Hl) <= R.step_bar(b, c["k"], m) * Hl).all() and np.array_equal(Hd == 0, Hl == 0)
        assert (np.abs(Wd - Wl) <= R.step_bar(b, c["k"], n) * Wl).all() and np.array_equal(Wd == 0, Wl == 0)


def test_beta_one_is_the_kl_restatement():
    import kl_dense_cases as K
    import kl_reference as KR
    c = K.case("d_k16")
    kl = KR.fit(c["A"], c["W0"], c["H0"], order="gemm", **c["kw"])
    b1 = R.fit(c["A"], c["W0"], c["H0"], beta=1.0, **c["kw"])
    assert b1["n_iter"] == kl["n_iter"] == K.SKLEARN_N_ITER["d_k16"] and b1["converged"] == kl["converged"]
    assert _factor_diff(kl, b1) <= R.FIT_BAR
    assert np.array_equal(kl["W"] == 0, b1["W"] == 0)
    assert abs(kl["error"] - b1["error"]) <= 1e-12 * kl["error"] and abs(kl["error_init"] - b1["error_init"]) <= 1e-12 * kl["error_init"]


def test_the_case_table_is_what_the_gpu_tests_expect():
    T = 64                                            # the kernel's tile
    for name, (ns, nf, k, seed, beta, alpha, l1_ratio, kind) in C.CASES.items():
        c = C.case(name)
        A = c["A"]
        assert A.shape == (nf, ns) and c["W0"].shape == (nf, k) and c["H0"].shape == (k, ns) and k <= min(A.shape)
        assert np.array_equal(A, A.astype(np.float32))                                  # fp32 storage holds every value
        if kind == "real":
            assert A.min() > 0 and (A != np.round(A)).mean() > 0.9                      # strictly positive: what beta = 0 needs
        else:
            assert beta > 0 and (A.sum(axis=1) == 0).any() and (A.sum(axis=0) == 0).any()   # a zero row, a zero column
            assert np.array_equal(A, np.round(A)) and A.max() <= 255
    shapes = {name: C.case(name)["A"].shape for name in C.CASES}
    assert shapes["is_k3_tile"] == (T, T)                                               # one exact tile
    assert shapes["is_k16"] == (T + 1, 2 * T + 1)                                       # one row and one column past a tile
    assert shapes["is_tall_k8"][0] == T - 1 and shapes[C.SPANS_CASE][0] == T - 1        # 63 rows
    assert C.CASES["is_k65"][2] == 65 and C.CASES["is_k128"][2] == 128                  # two 64-row groups of the factors
    m, n = shapes[C.SPANS_CASE]
    row_tiles = -(-n // T)
    per = -(-row_tiles // 32)
    assert row_tiles > 32 and per >= 2 and row_tiles % per != 0
    assert set(C.STEP_CASES) <= set(C.CASES) and set(C.GOLDEN_CASES) <= set(C.CASES) and set(C.DIVERGENCE_CASES) <= set(C.CASES)
    assert all(C.CASES[name][2] <= 33 for name in C.GOLDEN_CASES)
    assert {C.CASES[name][4] for name in C.GOLDEN_CASES} == {C.CASES[name][4] for name in C.CASES}        # every beta is recorded
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "kl_sklearn.npz"))
    # the bf16 case: X rounded to bf16 stays strictly positive
    bits = C.case(C.BF16_CASE)["A"].astype(np.float32).view(np.uint32)
    rounded = (((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    assert rounded.min() > 0


def test_python_surface_without_a_device():
    import smallk_amd
    from smallk_amd import _lib as L
    for name in ("nmf_beta_dense", "beta_dense_last_profile", "BetaDivergence"):
        assert callable(getattr(smallk_amd, name)) and name in smallk_amd.__all__
    assert callable(smallk_amd.DenseMatrix.beta_divergence)
    for sym in ("smk_nmf_beta_dense_device", "smk_matrix_beta_divergence_dense_device", "smk_beta_dense_last_profile", "smk_beta_dense_step_time"):
        assert sym in L.SYMBOLS and hasattr(L.lib(), sym)


def test_argument_checks_come_before_any_library_call():
    import smallk_amd
    from smallk_amd import solver
    W, H = np.ones((4, 2)), np.ones((2, 4))
    dense = object.__new__(smallk_amd.DenseMatrix)
    sparse = object.__new__(smallk_amd.SparseMatrix)
    for m in (dense, sparse):               # never created: no handle, so any library call on them fails as an AttributeError
        m.__dict__.update(height=4, ncols=4)
    with pytest.raises(ValueError, match="beta_loss must be one of"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss="euclid")
    with pytest.raises(ValueError, match="Frobenius"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss=2)
    with pytest.raises(ValueError, match="Frobenius"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss=2.0)
    with pytest.raises(ValueError, match="frobenius"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss="frobenius")
    with pytest.raises(ValueError, match=">= 0"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss=-0.5)
    with pytest.raises(ValueError, match=">= 0"):
        smallk_amd.nmf_beta_dense(dense, W, H, beta_loss=float("nan"))
    with pytest.raises(ValueError, match="DenseMatrix"):
        smallk_amd.nmf_beta_dense(sparse, W, H, beta_loss=0.5)
    with pytest.raises(ValueError, match="DenseMatrix"):
        smallk_amd.nmf_beta_dense(np.ones((4, 4)), W, H, beta_loss="itakura-saito")
    with pytest.raises(ValueError, match="DenseMatrix"):
        smallk_amd.DenseMatrix.beta_divergence(sparse, W, H, 0.5)
    with pytest.raises(ValueError, match="Frobenius"):
        smallk_amd.DenseMatrix.beta_divergence(dense, W, H, 2)
    assert solver._beta_of("t", "itakura-saito") == 0.0 and solver._beta_of("t", "kullback-leibler") == 1.0 and solver._beta_of("t", 3) == 3.0

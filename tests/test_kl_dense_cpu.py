"""The inputs of tests/test_gpu_kl_dense.py hold their bars by themselves: no device here.

* On every case of tests/kl_dense_cases.py the numpy restatement (tests/kl_reference.py, whose stored entries are the non-zeros of
  the dense array) reproduces scikit-learn on the dense X -- live where sklearn imports, else the recorded result of the k <= 33
  cases (tests/golden/kl_dense_sklearn.npz) -- with the same n_iter_ and factors within 1e-12 of the largest factor entry.
* The summation orders "pair" and "gemm" agree in iteration count, zero patterns and, within 1 / 8 of the GPU bar, the factors; at
  every check of the stopping rule the stop quantity stays 3e-3 tol away from tol (DESIGN 18's condition): what the GPU is held to
  is not decided by rounding.
* The cases have the structure the GPU tests rely on: a zero row and a zero column, counts that bf16 holds exactly, the tile edges,
  the span shape, the non-integer fp32 case.
* The Python surface that needs no device."""
import functools
import os
import warnings

import numpy as np
import pytest

import kl_dense_cases as C
import kl_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kl_dense_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _fit(name, order="pair"):
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], order=order, **c["kw"])


def _factor_diff(a, b):
    return max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / max(a["W"].max(), a["H"].max())


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_reproduces_sklearn(name):
    """live sklearn on the dense X where it imports; otherwise the recorded result (the golden cases only)"""
    c = C.case(name)
    res = _fit(name)
    try:
        import sklearn.decomposition as skd
    except ImportError:
        skd = None
    if skd is not None:
        model = skd.NMF(n_components=c["k"], init="custom", solver="mu", beta_loss="kullback-leibler", **c["sk"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Wsk = model.fit_transform(c["X"], W=c["Wsk0"].copy(), H=c["Hsk0"].copy())
        sk = {"W": model.components_.T, "H": Wsk.T, "n_iter": model.n_iter_, "error": model.reconstruction_err_}
    elif name in C.GOLDEN_CASES:
        g = np.load(GOLDEN)
        sk = {"W": g[f"{name}/W"], "H": g[f"{name}/H"], "n_iter": int(g[f"{name}/n_iter"]), "error": float(g[f"{name}/reconstruction_err"])}
    else:                                             # no sklearn here and no recorded factors: its recorded n_iter_ alone
        assert res["n_iter"] == C.SKLEARN_N_ITER[name]
        return
    d = _factor_diff(sk, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {sk['n_iter']}), factors {d:.2e} of the largest entry")
    assert res["n_iter"] == sk["n_iter"] == C.SKLEARN_N_ITER[name]
    assert d <= 1e-12
    assert abs(res["error"] - sk["error"]) <= 1e-12 * res["error"]


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
    """the margin property and the zero-pattern property"""
    pair, gemm = _fit(name), _fit(name, "gemm")
    margin = min(pair["margins"] + gemm["margins"])
    drift = _factor_diff(pair, gemm)
    print(f"{name}: n_iter {pair['n_iter']}, drift between orders {drift:.2e} (bar {R.FIT_BAR / 8:.2e}), stop quantity to tol {margin:.2e} tol")
    assert gemm["n_iter"] == pair["n_iter"] == C.SKLEARN_N_ITER[name] and gemm["converged"] == pair["converged"]
    assert np.array_equal(gemm["W"] == 0, pair["W"] == 0) and np.array_equal(gemm["H"] == 0, pair["H"] == 0)
    assert abs(gemm["error"] - pair["error"]) <= 1e-13 * pair["error"] and abs(gemm["error_init"] - pair["error_init"]) <= 1e-13 * pair["error_init"]
    assert drift <= R.FIT_BAR / 8
    assert margin >= 3e-3
    assert (pair["W"] == 0).any()                     # the flush of the W step has work


def test_single_steps_do_not_hang_on_rounding():
    """one H step and one W step by themselves: float64 stays within the GPU bar of the longdouble mode, equal zero patterns"""
    for name in C.STEP_CASES:
        c = C.case(name)
        E = R.Entries(c["A"])
        m, n = c["A"].shape
        ld = np.longdouble
        Hl = np.asarray(R.step_h(E, c["W0"].astype(ld), c["H0"].astype(ld), 0.0, 0.0), dtype=np.float64)
        Wl = np.asarray(R.step_w(E, c["W0"].astype(ld), c["H0"].astype(ld), 0.0, 0.0), dtype=np.float64)
        Hd = R.step_h(E, c["W0"].copy(), c["H0"].copy(), 0.0, 0.0)
        Wd = R.step_w(E, c["W0"].copy(), c["H0"].copy(), 0.0, 0.0)
        assert (np.abs(Hd - Hl) <= R.step_bar(c["k"], m) * Hl).all() and np.array_equal(Hd == 0, Hl == 0)
        assert (np.abs(Wd - Wl) <= R.step_bar(c["k"], n) * Wl).all() and np.array_equal(Wd == 0, Wl == 0)


def test_the_case_table_is_what_the_gpu_tests_expect():
    T = 64                                            # the kernel's tile
    for name, (ns, nf, k, seed, alpha, l1_ratio, kind) in C.CASES.items():
        c = C.case(name)
        A = c["A"]
        assert A.shape == (nf, ns) and c["W0"].shape == (nf, k) and c["H0"].shape == (k, ns) and k <= min(A.shape)
        assert (A.sum(axis=1) == 0).any() and (A.sum(axis=0) == 0).any()                # a zero row, a zero column
        assert (A >= 0).all() and np.array_equal(A, A.astype(np.float32))               # fp32 storage holds every value
        if kind == "counts":
            assert np.array_equal(A, np.round(A)) and A.max() <= 255                    # ... and so does bf16
            assert 0.15 < (A == 0).mean() < 0.25
        else:
            assert (A != np.round(A)).mean() > 0.9 and not np.array_equal(A, A.astype(np.float16))
    shapes = {name: C.case(name)["A"].shape for name in C.CASES}
    assert shapes["d_k3_l1"] == (T, T)                                                  # one exact tile
    assert shapes["d_k16"] == (T + 1, 2 * T + 1)                                        # one row and one column past a tile
    assert shapes["d_tall_k8"][0] == T - 1 and shapes[C.SPANS_CASE][0] == T - 1         # 63 rows
    assert C.CASES["d_k65"][2] == 65 and C.CASES["d_k128"][2] == 128                    # two 64-row groups of the factors
    # the span shape: the W step sweeps A' (n x m) in more row tiles than the launch has spans (at most 32), so a workgroup walks
    # several tiles and the last span is short
    m, n = shapes[C.SPANS_CASE]
    row_tiles = -(-n // T)
    per = -(-row_tiles // 32)
    assert row_tiles > 32 and per >= 2 and row_tiles % per != 0
    assert set(C.STEP_CASES) <= set(C.CASES) and set(C.GOLDEN_CASES) <= set(C.CASES)
    assert all(C.CASES[name][2] <= 33 for name in C.GOLDEN_CASES)
    assert os.path.getsize(GOLDEN) < 1 << 20
    for name in ("d_k128",):
        assert _fit(name)["n_iter"] == C.MAX_ITER and not _fit(name)["converged"]


def test_python_surface_without_a_device():
    import smallk_amd
    from smallk_amd import _lib as L
    for name in ("nmf_kl_dense", "kl_dense_last_profile"):
        assert callable(getattr(smallk_amd, name)) and name in smallk_amd.__all__
    assert callable(smallk_amd.DenseMatrix.kl_divergence)
    assert smallk_amd.SparseMatrix.kl_divergence is not smallk_amd.DenseMatrix.kl_divergence          # SparseMatrix keeps its own
    for sym in ("smk_nmf_kl_dense_device", "smk_matrix_kl_divergence_dense_device", "smk_kl_dense_last_profile", "smk_kl_dense_step_time"):
        assert sym in L.SYMBOLS and hasattr(L.lib(), sym)
    assert L.SYMBOLS["smk_nmf_kl_dense_device"] == L.SYMBOLS["smk_nmf_kl_device"]
    assert L.SYMBOLS["smk_matrix_kl_divergence_dense_device"] == L.SYMBOLS["smk_matrix_kl_divergence_device"]
    with pytest.raises(ValueError, match="DenseMatrix"):
        smallk_amd.nmf_kl_dense(np.ones((4, 4)), np.ones((4, 2)), np.ones((2, 4)))

"""The inputs of tests/test_gpu_kl.py hold their bars by themselves: no device here.

* The numpy restatement (tests/kl_reference.py) reproduces scikit-learn's recorded result (tests/golden/kl_sklearn.npz) to 1e-12 of
  the largest factor entry with the same n_iter, its recorded transform likewise, and, where sklearn imports, its live result.
* On every case of the GPU tests the three summation orders and the numpy.longdouble mode agree in iteration count and in the
  zero patterns, and in the factors within 1 / 8 of the GPU bar; at every check of the stopping rule the stop quantity stays
  1e-3 tol away from tol: what the GPU is held to is not decided by rounding.
* The cases have the structure the GPU tests rely on: an empty row and an empty column, long-column pieces on both sides (or, for
  the short case, none on the H side), the degenerate start.
* The estimator's argument checks that need no device."""
import functools
import os
import warnings

import numpy as np
import pytest

import kl_cases as C
import kl_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kl_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _fit(name, order="pair", dtype="float64"):
    c = C.case(name)
    return R.fit(c["A"], c["W0"], c["H0"], order=order, dtype=np.dtype(dtype), **c["kw"])


def _factor_diff(a, b):
    return max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / max(a["W"].max(), a["H"].max())


def _transform_start(name):
    c = C.case(name)
    return np.full((c["k"], c["A"].shape[1]), np.sqrt(c["X"].mean() / c["k"]))


@pytest.mark.parametrize("name", C.GOLDEN_CASES)
def test_restatement_reproduces_the_recorded_sklearn_result(name):
    g = np.load(GOLDEN)
    c = C.case(name)
    assert np.array_equal(g[f"{name}/checksum"], [c["X"].sum(), c["W0"].sum(), c["H0"].sum()])
    res = _fit(name)
    d = _factor_diff({"W": g[f"{name}/W"], "H": g[f"{name}/H"]}, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {int(g[f'{name}/n_iter'])}), factors {d:.2e} of the largest entry")
    assert res["n_iter"] == int(g[f"{name}/n_iter"]) == C.SKLEARN_N_ITER[name]
    assert d <= 1e-12
    assert abs(res["error"] - float(g[f"{name}/reconstruction_err"])) <= 1e-12 * res["error"]


def test_restatement_reproduces_the_recorded_transform():
    name = C.TRANSFORM_CASE
    g = np.load(GOLDEN)
    c = C.case(name)
    ref = R.fit(c["A"], g[f"{name}/W"], _transform_start(name), update_W=False, **c["kw"])
    want = g[f"{name}/transform_H"]
    d = np.abs(ref["H"] - want).max() / want.max()
    print(f"transform of {name}: {ref['n_iter']} iterations, {d:.2e}")
    assert d <= 1e-12 and np.array_equal(ref["W"], g[f"{name}/W"]) and ref["n_iter"] > 1


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_reproduces_live_sklearn(name):
    skd = pytest.importorskip("sklearn.decomposition")
    sp = pytest.importorskip("scipy.sparse")
    c = C.case(name)
    model = skd.NMF(n_components=c["k"], init="custom", solver="mu", beta_loss="kullback-leibler", **c["sk"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk = model.fit_transform(sp.csr_matrix(c["X"]), W=c["Wsk0"].copy(), H=c["Hsk0"].copy())
    res = _fit(name)
    d = _factor_diff({"W": model.components_.T, "H": Wsk.T}, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {model.n_iter_}), factors {d:.2e}")
    assert res["n_iter"] == model.n_iter_
    assert d <= 1e-12
    assert abs(res["error"] - model.reconstruction_err_) <= 1e-12 * res["error"]


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_do_not_hang_on_rounding(name):
    """the margin property and the zero-pattern property"""
    pair, seq, gemm = _fit(name), _fit(name, "seq"), _fit(name, "gemm")
    others = [seq, gemm]
    if C.case(name)["k"] <= 33:                       # the longdouble run of the two large ranks takes a minute and shows nothing more
        others.append(_fit(name, "pair", "longdouble"))
    margin = min(pair["margins"])
    drift = max(_factor_diff(pair, o) for o in others)
    print(f"{name}: n_iter {pair['n_iter']}, drift between orders {drift:.2e} (bar {R.FIT_BAR / 8:.2e}), stop quantity to tol {margin:.2e} tol")
    for o in others:
        assert o["n_iter"] == pair["n_iter"] and o["converged"] == pair["converged"]
        assert np.array_equal(o["W"] == 0, pair["W"] == 0) and np.array_equal(o["H"] == 0, pair["H"] == 0)
        assert abs(o["error"] - pair["error"]) <= 1e-13 * pair["error"] and abs(o["error_init"] - pair["error_init"]) <= 1e-13 * pair["error_init"]
    assert drift <= R.FIT_BAR / 8
    assert margin >= 1e-3
    assert (pair["W"] == 0).any()                     # the flush of the W step has work


def test_the_case_table_is_what_the_gpu_tests_expect():
    for name in C.CASES:
        c = C.case(name)
        A, (vals, rows, indptr, shape) = c["A"], c["csc"]
        assert (A.sum(axis=1) == 0).any() and (A.sum(axis=0) == 0).any()                # an empty row, an empty column
        assert shape == A.shape and len(vals) == indptr[-1] == (A != 0).sum() and (vals >= 1).all()
        dense = np.zeros(A.shape)
        for j in range(shape[1]):
            dense[rows[indptr[j]:indptr[j + 1]], j] = vals[indptr[j]:indptr[j + 1]]
        assert np.array_equal(dense, A)
        Lc, Lr = C.longest(A)
        if name == "short_k8":
            assert Lc <= C.SEG < Lr                   # no pieces on the H side
        elif name != "kmin_k30":
            assert Lc > C.SEG and Lr > C.SEG          # pieces on both sides
    assert C.case("kmin_k30")["k"] == min(C.case("kmin_k30")["A"].shape)
    d = C.case("degenerate_k4")
    assert (d["W0"][:, C.DEGENERATE_COMPONENT] == 0).all() and (d["H0"][:, C.DEGENERATE_COLUMN] == 0).all()
    assert d["A"][:, C.DEGENERATE_COLUMN].sum() > 0
    for name in ("k64", "k128"):
        assert _fit(name)["n_iter"] == C.MAX_ITER and not _fit(name)["converged"]
    for name, it in C.SKLEARN_N_ITER.items():
        assert _fit(name)["n_iter"] == it


def test_the_degenerate_start_meets_every_special_rule():
    """component 1 of W0 is zero: sum_i W[i, 1] = 0, the H step's denominator 0 becomes EPS, row 1 of H becomes zero, its sum 0
    becomes 1.0 in the W step; column 3 of H0 is zero: every dot product of its entries is clamped at EPS"""
    c = C.case("degenerate_k4")
    E = R.Entries(c["A"])
    W, H = c["W0"].copy(), c["H0"].copy()
    t, j = C.DEGENERATE_COMPONENT, C.DEGENERATE_COLUMN
    assert (R._dots(E, W, H, "pair")[E.j == j] == 0).all()
    R.step_h(E, W, H, 0.0, 0.0)
    assert (H[t] == 0).all() and (H[:, j] == 0).all() and np.isfinite(H).all()
    R.step_w(E, W, H, 0.0, 0.0)
    assert (W[:, t] == 0).all() and np.isfinite(W).all() and (np.delete(W, t, axis=1) > 0).any()


def test_single_steps_do_not_hang_on_rounding():
    """one H step and one W step by themselves: float64 in either order stays within the GPU bar of the longdouble mode, equal
    zero patterns"""
    for name in C.CASES:
        c = C.case(name)
        E = R.Entries(c["A"])
        Lc, Lr = C.longest(c["A"])
        ld = np.longdouble
        Hl = np.asarray(R.step_h(E, c["W0"].astype(ld), c["H0"].astype(ld), 0.0, 0.0), dtype=np.float64)
        Wl = np.asarray(R.step_w(E, c["W0"].astype(ld), c["H0"].astype(ld), 0.0, 0.0), dtype=np.float64)
        for order in ("pair", "seq"):
            Hd = R.step_h(E, c["W0"].copy(), c["H0"].copy(), 0.0, 0.0, order)
            Wd = R.step_w(E, c["W0"].copy(), c["H0"].copy(), 0.0, 0.0, order)
            assert (np.abs(Hd - Hl) <= R.step_bar(c["k"], Lc) * Hl).all() and np.array_equal(Hd == 0, Hl == 0)
            assert (np.abs(Wd - Wl) <= R.step_bar(c["k"], Lr) * Wl).all() and np.array_equal(Wd == 0, Wl == 0)


# ---- the estimator's argument checks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta_loss", ["kullback-leibler", 1, 1.0])
def test_estimator_accepts_the_pair(beta_loss):
    import smallk_amd
    est = smallk_amd.NMF(4, solver="mu", beta_loss=beta_loss, alpha_W=0.1, alpha_H=0.2, l1_ratio=0.5, tol=1e-3, max_iter=50)
    assert (est.solver, est.beta_loss) == ("mu", beta_loss)
    assert est._penalties() == {"alpha_W": 0.2, "alpha_H": 0.1, "l1_ratio": 0.5, "tol": 1e-3, "max_iter": 50}


@pytest.mark.parametrize("kw", [{"solver": "mu"}, {"beta_loss": "kullback-leibler"}, {"beta_loss": 1}, {"solver": "mu", "beta_loss": "frobenius"},
                                {"solver": "mu", "beta_loss": 2}, {"solver": "cd", "beta_loss": 1.0}, {"solver": "mu", "beta_loss": "itakura-saito"},
                                {"solver": "mu", "beta_loss": 0.5}, {"solver": "mu", "beta_loss": "kullback-leibler", "shuffle": True}])
def test_estimator_refuses_each_half_alone(kw):
    import smallk_amd
    with pytest.raises(ValueError):
        smallk_amd.NMF(**kw)


def test_estimator_refuses_a_dense_x_with_this_loss():
    """before anything touches a device: the KL path takes sparse input"""
    import smallk_amd
    est = smallk_amd.NMF(3, solver="mu", beta_loss="kullback-leibler", init="random")
    X = np.arange(40.0).reshape(8, 5)
    with pytest.raises(ValueError, match="sparse"):
        est.fit_transform(X)
    with pytest.raises(ValueError, match="sparse"):
        est.fit(X)
    est._W = None                     # as if fitted: transform refuses the dense X first
    with pytest.raises(ValueError, match="sparse"):
        est.transform(X)

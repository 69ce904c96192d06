"""The inputs of tests/test_gpu_cd.py hold their bars by themselves: no device here.

* The numpy restatement (tests/cd_reference.py) reproduces scikit-learn's recorded result (tests/golden/cd_sklearn.npz) and, where
  sklearn imports, its live result: the same n_iter, factors within 1e-13 of the largest entry.
* On every case of the GPU tests the two summation orders of the gradient and the numpy.longdouble mode agree in iteration
  count and zero pattern, and in the factors within 1 / 16 of the GPU bar: what the GPU is held to is not decided by rounding.
* Preconditions of every fit case: every pre-clamp value stays 2^-20 (relative to |x[t]| + |grad / G'[t,t]|) away from zero, no
  zero entry meets a gradient below 2^-20 of its column's largest, violation / violation_init stays 1e-6 tol away from tol in
  every iteration.  A case that misses one gets another seed in cd_reference.FIT_CASES, never another bar.
* The estimator's argument checks that need no device."""
import functools
import os
import warnings

import numpy as np
import pytest

import cd_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cd_sklearn.npz")


@functools.lru_cache(maxsize=None)
def _fit(name, order="seq", dtype="float64"):
    A, _, W0, H0, kw = R.fit_case(name)
    probe = R.Probe()
    res = R.fit(A, W0, H0, order=order, dtype=np.dtype(dtype), probe=probe, **kw)
    return res, probe, kw


def _top(res):
    return max(res["W"].max(), res["H"].max())


def _factor_diff(a, b):
    return max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / _top(a)


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_the_recorded_sklearn_result(name):
    g = np.load(GOLDEN)
    A, _, W0, H0, _ = R.fit_case(name)
    for key, v in (("A", A), ("W0", W0), ("H0", H0)):
        assert np.array_equal(g[f"{name}/{key}"].astype(np.float64), v), key
    res, _, _ = _fit(name)
    ref = {"W": g[f"{name}/W"], "H": g[f"{name}/H"]}
    d = _factor_diff(ref, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {int(g[f'{name}/n_iter'])}), factors {d:.2e} of the largest entry")
    assert res["n_iter"] == int(g[f"{name}/n_iter"])
    assert d <= 1e-13
    err = np.linalg.norm(A - res["W"] @ res["H"])
    assert abs(err - float(g[f"{name}/reconstruction_err"])) <= 1e-12 * err


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_live_sklearn(name):
    skd = pytest.importorskip("sklearn.decomposition")
    A, _, W0, H0, kw = R.fit_case(name)
    model = skd.NMF(n_components=W0.shape[1], init="custom", solver="cd", tol=kw["tol"], max_iter=kw["max_iter"], alpha_W=kw["alpha_H"],
                    alpha_H=kw["alpha_W"], l1_ratio=kw["l1_ratio"], shuffle=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk = model.fit_transform(np.ascontiguousarray(A.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
    res, _, _ = _fit(name)
    d = _factor_diff({"W": model.components_.T, "H": Wsk.T}, res)
    print(f"{name}: n_iter {res['n_iter']} (sklearn {model.n_iter_}), factors {d:.2e}")
    assert res["n_iter"] == model.n_iter_
    assert d <= 1e-13


def test_the_case_table_is_what_the_gpu_tests_expect():
    assert _fit(R.RUNS_TO_MAX_ITER)[0]["n_iter"] == R.FIT_MAX_ITER and not _fit(R.RUNS_TO_MAX_ITER)[0]["converged"]
    assert _fit("d96_plain")[0]["converged"]
    csc, D = R.fit_case("s300_sparse")[1], R.fit_case("s300_sparse")[0]
    vals, rows, indptr, shape = csc
    assert (D.sum(axis=1) == 0).any() and (D.sum(axis=0) == 0).any()                    # an empty row, an empty column
    assert any(len(set(rows[indptr[j]:indptr[j + 1]])) < indptr[j + 1] - indptr[j] for j in range(shape[1]))     # a duplicate
    for name in R.FIT_CASES:
        A, _, W0, H0, _ = R.fit_case(name)
        for v in (A, W0, H0):               # exact in fp32: the stored A is fp32, and one case hands fp32 factor views in
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)


@pytest.mark.parametrize("name", list(R.FIT_CASES))
def test_fit_cases_do_not_hang_on_rounding(name):
    seq, probe, kw = _fit(name)
    dot, _, _ = _fit(name, "dot")
    ld, _, _ = _fit(name, "dot", "longdouble")
    rd = min(abs(r - kw["tol"]) for r in seq["ratios"]) / kw["tol"]
    dd, dl = _factor_diff(seq, dot), _factor_diff(seq, ld)
    print(f"{name}: n_iter {seq['n_iter']}, seq/dot {dd:.2e}, seq/longdouble {dl:.2e} (bar {R.FIT_BAR / 16:.2e}), clamp margin {probe.clamp:.2e}, "
          f"zero-gradient margin {probe.zero_grad:.2e} (bar {R.MARGIN:.2e}), ratio to tol {rd:.2e}")
    for other in (dot, ld):
        assert other["n_iter"] == seq["n_iter"] and other["converged"] == seq["converged"]
        assert np.array_equal(other["W"] == 0, seq["W"] == 0) and np.array_equal(other["H"] == 0, seq["H"] == 0)
    assert dd <= R.FIT_BAR / 16 and dl <= R.FIT_BAR / 16
    assert probe.clamp >= R.MARGIN
    assert probe.zero_grad >= R.MARGIN
    assert rd >= 1e-6


def test_transform_case_does_not_hang_on_rounding():
    """update_W = False on the training data of a converged fit, from the constant start the estimator uses"""
    A, _, _, _, kw = R.fit_case("d96_plain")
    W = _fit("d96_plain")[0]["W"]
    k = W.shape[1]
    H0 = np.full((k, A.shape[1]), np.sqrt(A.mean() / k))
    runs = [R.fit(A, W, H0, update_W=False, order=o, dtype=np.dtype(d), **kw) for o, d in (("seq", "float64"), ("dot", "float64"), ("dot", "longdouble"))]
    for other in runs[1:]:
        assert other["n_iter"] == runs[0]["n_iter"]
        assert np.array_equal(other["H"] == 0, runs[0]["H"] == 0)
        assert np.abs(other["H"] - runs[0]["H"]).max() <= R.FIT_BAR / 16 * runs[0]["H"].max()
    assert np.array_equal(runs[0]["W"], W)


@pytest.mark.parametrize("reg", R.SWEEP_REGS)
@pytest.mark.parametrize("k", R.SWEEP_KS)
def test_sweep_cases_do_not_hang_on_rounding(k, reg):
    for N in R.SWEEP_NS:
        G, Rm, X, l1, l2 = R.sweep_case(k, N, reg)
        out, viol = [], []
        for order, dt in (("seq", np.float64), ("dot", np.float64), ("dot", np.longdouble)):
            x = np.array(X, dtype=dt)
            viol.append(float(R.sweep(x, G, Rm, l1, l2, order=order)))
            out.append(np.asarray(x, dtype=np.float64))
        top = np.abs(out[0]).max()
        for o, v in zip(out[1:], viol[1:]):
            assert np.array_equal(o == 0, out[0] == 0)
            assert np.abs(o - out[0]).max() <= R.sweep_bar(k) / 16 * top
            assert abs(v - viol[0]) <= R.sweep_bar(k) / 16 * viol[0]
        g0 = (G + l2 * np.eye(k)) @ X - (Rm - l1)
        if reg == "none" and k > 1 and N > 1:
            assert (g0[X == 0] > 0).any() and (g0[X == 0] < 0).any()          # exact zeros meet both signs of the gradient
        if reg == "l1":
            assert (out[0][:, 1::4] == 0).all() and ((out[0] != 0).any() or k * N == 1)          # whole columns end as zeros (N > 1), not all of them


@pytest.mark.parametrize("k, t0", [(3, 1), (17, 16), (65, 0)])
def test_zero_diagonal_case(k, t0):
    G, Rm, X, l1, l2 = R.sweep_case(k, 63, "none", zero_diag=t0)
    X[t0, ::2] = 0.0
    x = X.copy()
    viol = R.sweep(x, G, Rm, l1, l2)
    assert np.array_equal(x[t0], X[t0])
    pg = np.where(X[t0] == 0, np.minimum(-Rm[t0], 0), -Rm[t0])
    G2, x2 = np.delete(np.delete(G, t0, 0), t0, 1), np.delete(X, t0, 0)
    assert abs(viol - (R.sweep(x2, G2, np.delete(Rm, t0, 0), l1, l2) + np.abs(pg).sum())) <= 1e-12 * viol


# ---- the estimator's argument checks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"solver": "mu"}, {"beta_loss": "kullback-leibler"}, {"shuffle": True}, {"init": "nndsvdar"},
                                {"n_components": 0}, {"n_components": 2.5}, {"alpha_W": -1.0}, {"alpha_H": -0.5}, {"alpha_H": "both"},
                                {"l1_ratio": 1.5}, {"l1_ratio": -0.1}, {"tol": -1e-3}, {"max_iter": 0}, {"max_iter": 2.5}])
def test_estimator_refuses_what_it_does_not_do(kw):
    import smallk_amd
    with pytest.raises(ValueError):
        smallk_amd.NMF(**kw)


def test_estimator_keeps_its_arguments():
    import smallk_amd
    est = smallk_amd.NMF(7, init="custom", alpha_W=0.1, alpha_H=0.2, l1_ratio=0.5, tol=1e-5, max_iter=50, random_state=3)
    assert (est.n_components, est.init, est.solver, est.beta_loss, est.shuffle) == (7, "custom", "cd", "frobenius", False)
    # sklearn's alpha_W weighs W_sklearn = H', its alpha_H the components W'
    assert est._penalties() == {"alpha_W": 0.2, "alpha_H": 0.1, "l1_ratio": 0.5, "tol": 1e-5, "max_iter": 50}
    assert smallk_amd.NMF(3, alpha_W=0.25)._penalties()["alpha_W"] == 0.25
    with pytest.raises(AttributeError):
        est.components_
    with pytest.raises(ValueError):
        est._start(type("M", (), {"height": 4, "ncols": 9})(), 7, 1.0, None, None)          # custom without W and H

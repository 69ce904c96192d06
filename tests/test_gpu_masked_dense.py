"""Masked beta-divergence NMF on a dense resident matrix, NaN = not measured (smallk_amd.nmf_masked_dense,
DenseMatrix.masked_divergence; smallk_amd/csrc/masked_dense.hip, masked_dense.cpp) against the numpy restatement
tests/masked_dense_reference.py.  Meant to pass under SMK_POISON=1 as well.

Cases: beta = 0 on strictly positive draws (tests/beta_dense_cases.py's "real" kind), beta = 1 and 2 on counts with measured zeros,
bf16 cases on values rounded to bf16 first.  The mask removes 40 % at random and, on top, the last row's last entry, one whole row,
one whole column and the whole first 64 x 64 tile where the matrix goes on past it (on the 64 x 64 case that tile is the matrix, and a
matrix without a measured entry is a refusal, checked below).  2050 x 65 has 33 row tiles: 16 spans of two and one of one.

Bars (u = 2^-53).  One step by itself against the longdouble restatement, entry by entry and relative: 4 (c k + L + 8) u (every
summand is non-negative; c = max(|beta - 2|, |beta - 1|, 1), L the rows swept), exact zeros equal, no NaN.  A fit of 30 iterations:
factors within 1e-12 of the largest entry of the float64 restatement's, both zero patterns, error_init / error to 1e-12, the same
bits twice; with the default tol the restatement's n_iter and converged -- the seeds were chosen so that the restatement's stop
quantity stays 3e-3 tol away from tol at every check.  The divergence of the held-out matrix: within 1e-12 of the sum of the absolute
values of its terms, the count exact."""
import functools

import numpy as np
import pytest

import masked_dense_reference as R

pytestmark = pytest.mark.gpu

# name -> (m, n, k, beta, storage, seed)
CASES = {"fro_k3": (65, 63, 3, 2, "f32", 1), "kl_k5": (130, 67, 5, 1, "f32", 32), "is_k17": (67, 130, 17, 0, "f32", 3),
         "fro_k33_bf16": (129, 65, 33, 2, "bf16", 4), "kl_k16_bf16_tile": (64, 64, 16, 1, "bf16", 5), "is_k65": (200, 70, 65, 0, "f32", 6),
         "is_k5_spans": (2050, 65, 5, 0, "f32", 7)}
LD = np.longdouble


def _bf16(X):
    b = X.astype(np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name, masked=True):
    """dict: train / test (complementary NaNs; without ``masked`` train is X itself), W0, H0, k, beta, storage"""
    m, n, k, beta, storage, seed = CASES[name]
    rng = np.random.default_rng(seed)
    lam = rng.gamma(1.0, 1.0, (m, 4)) @ rng.gamma(1.0, 1.0, (4, n))
    lam *= 3.0 / lam.mean()
    X = (lam * rng.gamma(2.0, 0.5, (m, n))).astype(np.float32).astype(np.float64) if beta == 0 else np.minimum(rng.poisson(lam), 255).astype(np.float64)
    if storage == "bf16":
        X = _bf16(X)
    keep = rng.random((m, n)) >= 0.4
    keep[m - 1, n - 1] = keep[m // 3, :] = keep[:, n // 2] = False
    if m >= 64 and n >= 64 and m * n > 64 * 64:
        keep[:64, :64] = False
    if not masked:
        keep[...] = True
    avg = np.sqrt(X[keep].mean() / k)
    W0, H0 = avg * np.abs(rng.standard_normal((m, k))), avg * np.abs(rng.standard_normal((k, n)))
    return {"train": np.where(keep, X, np.nan), "test": np.where(keep, np.nan, X), "W0": W0, "H0": H0, "k": k, "beta": beta, "storage": storage}


@functools.lru_cache(maxsize=None)
def _reference(name, max_iter, tol):
    c = case(name)
    return R.fit(c["train"], c["W0"], c["H0"], beta=c["beta"], tol=tol, max_iter=max_iter)


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    worst = float((np.abs(got.astype(LD) - ref)[live] / ref[live]).max())
    print(f"{tag}: {worst / R.U53:.1f} u (bar {bar / R.U53:.0f} u), {int((~live).sum())} exact zeros")
    assert not np.isnan(got).any() and np.array_equal(got == 0, ref64 == 0) and worst <= bar


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_of_each_side(gpu, name):
    c = case(name)
    (m, n), k, beta = c["train"].shape, c["k"], c["beta"]
    mat = gpu.DenseMatrix.from_host(c["train"], storage=c["storage"])
    try:
        h = gpu.nmf_masked_dense(mat, c["W0"], c["H0"], beta_loss=beta, update_W=False, tol=0.0, max_iter=1)
        both = gpu.nmf_masked_dense(mat, c["W0"], c["H0"], beta_loss=beta, tol=0.0, max_iter=1)
    finally:
        mat.close()
    assert np.array_equal(h.W, c["W0"]) and np.array_equal(both.H, h.H) and h.n_iter == 1 and not h.converged
    _check_step(h.H, R.step_h(c["train"], c["W0"].astype(LD), c["H0"].astype(LD), beta), R.step_bar(beta, k, m), f"{name} H step")
    assert (h.H[:, n // 2] == 0).all()                    # the column without a measured entry
    # the W step from the device's own new H: what is compared is the W step alone
    _check_step(both.W, R.step_w(c["train"], c["W0"].astype(LD), both.H.astype(LD), beta), R.step_bar(beta, k, n), f"{name} W step")


@pytest.mark.parametrize("name", list(CASES))
def test_fit(gpu, name):
    c, ref, full = case(name), _reference(name, 30, 0.0), _reference(name, 200, 1e-4)
    assert min(full["margins"]) >= 3e-3
    mat = gpu.DenseMatrix.from_host(c["train"], storage=c["storage"])
    try:
        r, r2 = (gpu.nmf_masked_dense(mat, c["W0"], c["H0"], beta_loss=c["beta"], tol=0.0, max_iter=30) for _ in range(2))
        f = gpu.nmf_masked_dense(mat, c["W0"], c["H0"], beta_loss=c["beta"])
        d = mat.masked_divergence(r.W, r.H, c["beta"])
    finally:
        mat.close()
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    e0, e1 = abs(r.error_init - ref["error_init"]) / ref["error_init"], abs(r.error - ref["error"]) / ref["error"]
    print(f"fit {name}: W {ew:.2e} H {eh:.2e} (bar {R.FIT_BAR:.0e}), error_init {e0:.2e} error {e1:.2e}; default tol: n_iter {f.n_iter} (reference {full['n_iter']})")
    assert not np.isnan(r.W).any() and not np.isnan(r.H).any() and r.n_iter == 30
    assert ew <= R.FIT_BAR and eh <= R.FIT_BAR and e0 <= 1e-12 and e1 <= 1e-12
    assert np.array_equal(r.W == 0, ref["W"] == 0) and np.array_equal(r.H == 0, ref["H"] == 0)
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.error_init, r.error) == (r2.error_init, r2.error) and d.error == r.error
    assert (f.n_iter, f.converged) == (full["n_iter"], full["converged"])


@pytest.mark.parametrize("name", ["kl_k5", "kl_k16_bf16_tile", "is_k17", "is_k65", "is_k5_spans"])
def test_a_matrix_without_nan_is_the_existing_solver(gpu, name):
    c = case(name, masked=False)
    mat = gpu.DenseMatrix.from_host(c["train"], storage=c["storage"])
    try:
        got = gpu.nmf_masked_dense(mat, c["W0"], c["H0"], beta_loss=c["beta"])
        old = gpu.nmf_beta_dense(mat, c["W0"], c["H0"], beta_loss=c["beta"]) if c["beta"] == 0 else gpu.nmf_kl_dense(mat, c["W0"], c["H0"])
    finally:
        mat.close()
    top = max(old.W.max(), old.H.max())
    ew, eh = np.abs(got.W - old.W).max() / top, np.abs(got.H - old.H).max() / top
    print(f"{name} without NaN: n_iter {got.n_iter} / {old.n_iter}, W {ew:.2e} H {eh:.2e}")
    assert got.n_iter == old.n_iter and ew <= R.FIT_BAR and eh <= R.FIT_BAR


@pytest.mark.parametrize("name", list(CASES))
def test_masked_divergence_of_the_held_out_entries(gpu, name):
    c, ref = case(name), _reference(name, 30, 0.0)
    mat = gpu.DenseMatrix.from_host(c["test"], storage=c["storage"])
    try:
        got = [mat.masked_divergence(W, H, c["beta"]) for W, H in ((c["W0"], c["H0"]), (ref["W"], ref["H"]))]
    finally:
        mat.close()
    for g, (W, H) in zip(got, ((c["W0"], c["H0"]), (ref["W"], ref["H"]))):
        D, mag, cnt = R.divergence(c["test"], W.astype(LD), H.astype(LD), c["beta"])
        print(f"held-out {name}: D {g.divergence:.6e}, off by {abs(g.divergence - float(D)):.2e} (bar {1e-12 * float(mag):.2e}), count {g.count}")
        assert g.count == cnt == int((~np.isnan(c["test"])).sum()) and abs(g.divergence - D) <= 1e-12 * float(mag)
        assert g.mean == g.divergence / cnt and g.error == np.sqrt(2 * max(g.divergence, 0.0))


def test_refusals_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    A = 0.5 + rng.random((130, 131))
    A[rng.random(A.shape) < 0.4] = np.nan

    def changed(v, at=(7, 11)):
        B = A.copy()
        B[at] = v
        return gpu.DenseMatrix.from_host(B)

    mats = {"plain": gpu.DenseMatrix.from_host(A), "neg": changed(-1.0), "zero": changed(0.0), "empty": gpu.DenseMatrix.from_host(np.full(A.shape, np.nan)),
            "single": gpu.DenseMatrix.from_host(A, single_copy=True), "sparse": gpu.SparseMatrix.from_observed(np.nan_to_num(A), ~np.isnan(A))}

    def attempt(which, k, beta, exc, code=None, match=None):
        W, H = torch.from_numpy(rng.random((130, k))).to(dev), torch.from_numpy(rng.random((k, 131))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(exc, match=match) as e:
            gpu.nmf_masked_dense(mats[which], W, H, beta_loss=beta, inplace=True, max_iter=2)
        assert code is None or e.value.code == code
        assert bool((W == W0).all()) and bool((H == H0).all())
        return W, H

    try:
        attempt("plain", 4, 0.5, ValueError)
        attempt("sparse", 4, 2, ValueError)
        attempt("neg", 4, 2, L.SmallkError, L.BAD_PARAM, "negative")
        attempt("zero", 4, 0, L.SmallkError, L.BAD_PARAM, "add a small value")
        attempt("empty", 4, 1, L.SmallkError, L.BAD_PARAM, "no measured entry")
        attempt("plain", 129, 2, L.SmallkError, L.UNSUPPORTED)
        W, H = attempt("single", 4, 0, L.SmallkError, L.UNSUPPORTED, "single-copy")
        # what is refused is the data or the request, not NaN itself: a measured zero is served at beta = 1, the fold-in by a single copy
        assert gpu.nmf_masked_dense(mats["zero"], W, H, beta_loss=1, max_iter=1, tol=0.0).n_iter == 1
        a = gpu.nmf_masked_dense(mats["single"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0)
        b = gpu.nmf_masked_dense(mats["plain"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0)
        assert bool((a.H == b.H).all()) and a.error == b.error and gpu.masked_dense_last_profile() == (3, 2)
    finally:
        for x in mats.values():
            x.close()

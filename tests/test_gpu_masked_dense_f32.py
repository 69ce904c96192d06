"""The fp32 form of masked beta-divergence NMF on a dense matrix (nmf_masked_dense with precision="fp32";
smallk_amd/csrc/masked_dense_f32.hip, masked_dense_f32.cpp) against the numpy restatement
tests/masked_dense_reference.py, on the seven cases of tests/test_gpu_masked_dense.py.  Meant to pass under SMK_POISON=1 as well
(the switch is read once per process, so no test here sets it).

Bars (u = 2^-24).  One H step / one W step from a start rounded to float32, against the numpy.longdouble restatement, entry by entry
and relative: the fp64 test's step_bar with u = 2^-24 in place of 2^-53 -- the same worst-case bound for sums of non-negative terms
with every rounding in fp32 --, exact zeros equal, no NaN.  A 30-iteration fit: within 8 x the distance between the float64 and the
float32 restatement (two fp32 computations in different summation orders can each be that far from fp64), not below 16 u, for the
factors (max |difference| over the largest factor entry) and for `error` (relative).  The rest is exact."""
import functools

import numpy as np
import pytest

import masked_dense_reference as R
from test_gpu_masked_dense import CASES, case

pytestmark = pytest.mark.gpu

U24, LD = 2.0 ** -24, np.longdouble


def _start(c):
    """the float32-rounded start as float64 arrays"""
    return tuple(c[x].astype(np.float32).astype(np.float64) for x in ("W0", "H0"))


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    worst = float((np.abs(got.astype(LD) - ref)[live] / ref[live]).max())
    print(f"{tag}: {worst / U24:.1f} u (bar {bar / U24:.0f} u), {int((~live).sum())} exact zeros")
    assert not np.isnan(got).any() and np.array_equal(got == 0, ref64 == 0) and worst <= bar


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_of_each_side(gpu, name):
    c = case(name)
    (m, n), k, beta = c["train"].shape, c["k"], c["beta"]
    W0, H0 = _start(c)
    mat = gpu.DenseMatrix.from_host(c["train"], storage=c["storage"])
    try:
        h = gpu.nmf_masked_dense(mat, W0, H0, beta_loss=beta, update_W=False, tol=0.0, max_iter=1, precision="fp32")
        both = gpu.nmf_masked_dense(mat, W0, H0, beta_loss=beta, tol=0.0, max_iter=1, precision="fp32")
    finally:
        mat.close()
    assert np.array_equal(h.W, W0) and np.array_equal(both.H, h.H) and h.n_iter == 1 and not h.converged
    _check_step(h.H, R.step_h(c["train"], W0.astype(LD), H0.astype(LD), beta), R.step_bar(beta, k, m) * 2.0 ** 29, f"{name} H step")
    # the W step from the device's own new H: what is compared is the W step alone
    _check_step(both.W, R.step_w(c["train"], W0.astype(LD), both.H.astype(LD), beta), R.step_bar(beta, k, n) * 2.0 ** 29, f"{name} W step")
    assert (h.H[:, n // 2] == 0).all() and (both.W[m // 3, :] == 0).all()          # the column and the row without a measured entry


@functools.lru_cache(maxsize=None)
def _restatements(name):
    """the float64 and the float32 restatement of 30 iterations from the rounded start, formed once per session"""
    c = case(name)
    W0, H0 = _start(c)
    return tuple(R.fit(c["train"], W0, H0, beta=c["beta"], tol=0.0, max_iter=30, dtype=dt) for dt in (np.float64, np.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_short_fit(gpu, name):
    c, (ref64, ref32) = case(name), _restatements(name)
    W0, H0 = _start(c)
    kw = dict(beta_loss=c["beta"], tol=0.0, max_iter=30)
    mat = gpu.DenseMatrix.from_host(c["train"], storage=c["storage"])
    try:
        r = gpu.nmf_masked_dense(mat, W0, H0, precision="fp32", **kw)
        passes = gpu.masked_dense_f32_last_profile()
        r2 = gpu.nmf_masked_dense(mat, W0, H0, precision="fp32", **kw)
        f64 = gpu.nmf_masked_dense(mat, W0, H0, **kw)
        passes64 = gpu.masked_dense_last_profile()
        d = mat.masked_divergence(r.W, r.H, c["beta"])
    finally:
        mat.close()
    top = max(ref64["W"].max(), ref64["H"].max())
    dist = lambda a, b: max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / top
    rel = lambda a, b: abs(a - b) / ref64["error"]
    between, e_between = dist(ref32, ref64), rel(ref32["error"], ref64["error"])
    got, e_got = dist({"W": r.W, "H": r.H}, ref64), rel(r.error, ref64["error"])
    print(f"fit {name}: factors {got:.2e} from float64 (the float32 restatement {between:.2e}), error {e_got:.2e} ({e_between:.2e})")
    assert r.n_iter == 30 and not r.converged and not np.isnan(r.W).any() and not np.isnan(r.H).any()
    assert got <= max(8 * between, 16 * U24)
    assert e_got <= max(8 * e_between, 16 * U24)
    # exact: the error is the fp64 divergence of the returned factors, error_init the fp64 form's, the factors are fp32 numbers,
    # a second run gives the same bits, the passes are the fp64 form's
    assert d.error == r.error and r.error_init == f64.error_init and passes == passes64 == (60, 2)
    assert np.array_equal(r.W, r.W.astype(np.float32)) and np.array_equal(r.H, r.H.astype(np.float32))
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.error_init, r.error) == (r2.error_init, r2.error)


def test_refusals_and_the_keyword(gpu):
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

    def attempt(which, k, beta, exc, code=None, match=None, precision="fp32"):
        W, H = torch.from_numpy(rng.random((130, k))).to(dev), torch.from_numpy(rng.random((k, 131))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(exc, match=match) as e:
            gpu.nmf_masked_dense(mats[which], W, H, beta_loss=beta, inplace=True, max_iter=2, precision=precision)
        assert code is None or e.value.code == code
        assert bool((W == W0).all()) and bool((H == H0).all())
        return W, H

    try:
        attempt("plain", 4, 2, ValueError, match="precision", precision="fp16")
        attempt("plain", 4, 0.5, ValueError)
        attempt("sparse", 4, 2, ValueError)
        attempt("neg", 4, 2, L.SmallkError, L.BAD_PARAM, "negative")
        attempt("zero", 4, 0, L.SmallkError, L.BAD_PARAM, "add a small value")
        attempt("empty", 4, 1, L.SmallkError, L.BAD_PARAM, "no measured entry")
        attempt("plain", 129, 2, L.SmallkError, L.UNSUPPORTED, "k > 128")
        W, H = attempt("single", 4, 0, L.SmallkError, L.UNSUPPORTED, "single-copy")
        # the single copy's fold-in is served, with the plain matrix's bits
        a = gpu.nmf_masked_dense(mats["single"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0, precision="fp32")
        b = gpu.nmf_masked_dense(mats["plain"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0, precision="fp32")
        assert bool((a.H == b.H).all()) and a.error == b.error and gpu.masked_dense_f32_last_profile() == (3, 2)
        x, y = gpu.nmf_masked_dense(mats["plain"], W, H, beta_loss=1, max_iter=20), gpu.nmf_masked_dense(mats["plain"], W, H, beta_loss=1, max_iter=20, precision="fp64")
        assert bool((x.W == y.W).all()) and bool((x.H == y.H).all()) and (x.n_iter, x.error_init, x.error) == (y.n_iter, y.error_init, y.error)
    finally:
        for m_ in mats.values():
            m_.close()

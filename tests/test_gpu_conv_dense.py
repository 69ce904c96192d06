"""Convolutive NMF on a dense resident matrix (smallk_amd.nmf_conv_dense, DenseMatrix.conv_divergence; smallk_amd/csrc/conv_dense.hip,
conv_dense.cpp) against the numpy restatement tests/conv_dense_reference.py.  Meant to pass under SMK_POISON=1 as well.

The cases are the smallest shapes at which the kernel can go wrong.  t1: no lag, the existing solvers' iteration.  ragged: k padded per
lag (5 -> 8), the halo across two tile edges, ragged last tiles on both sides, in both storages.  full: inner dimension 128, the
limit, two 64-wide groups of the streamed factor.  longlag: T = 32, one tile, zeros entering over most of it.  tall / wide: the
streamed dimension has 16 row tiles against 2 column tiles, and the launch plan (residual_dense_shape: spans = min(32, row tiles,
ceil(4 CUs / column tiles))) splits it over S = 16 >= 2 spans on the H side / the W side respectively for any device of >= 8 CUs.

Bars (u = 2^-53).  One H step / one W step against the longdouble restatement, entry by entry and relative: DESIGN.md 21's
4 (c K + L + 8) u with K = T k + T in place of k, c = 2 at beta = 0 and 1 at beta = 1, L the streamed length; exact zeros equal.  A fit
of 30 iterations: factors within max(1e-12, 50 x the distance between the restatement's float64 and longdouble runs) of the largest
factor entry, error_init and error within 1e-12 relative, the same bits on a second call, error <= error_init."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_dense_reference as R

pytestmark = pytest.mark.gpu
LD = np.longdouble

CASES = {  # name: (m, n, k, T, storage)
    "t1": (64, 64, 4, 1, "f32"), "ragged": (70, 130, 5, 3, "f32"), "ragged_bf16": (70, 130, 5, 3, "bf16"), "full": (65, 95, 16, 8, "f32"),
    "longlag": (33, 40, 3, 32, "f32"), "tall": (1000, 70, 4, 4, "f32"), "wide": (70, 1000, 4, 4, "f32")}
BOTH = pytest.mark.parametrize("beta", [0, 1])
EACH = pytest.mark.parametrize("name", list(CASES))


@functools.lru_cache(maxsize=None)
def _case(name):
    """strictly positive data: Gamma noise plus a planted convolutive part, rounded to the storage type so that storage is exact"""
    m, n, k, T, storage = CASES[name]
    rng = np.random.default_rng(27)
    A = rng.gamma(2.0, 0.25, (m, n)) + R.model(rng.gamma(2.0, 0.5, (T, m, k)), rng.gamma(0.3, 1.0, (k, n)))
    A = torch.from_numpy(A).to(torch.bfloat16 if storage == "bf16" else torch.float32).double().numpy()
    return A, rng.uniform(0.1, 1.0, (T, m, k)), rng.uniform(0.1, 1.0, (k, n))


@functools.lru_cache(maxsize=None)
def _fits(name, beta):
    """the restatement's 30 iterations in float64 and, for the bar, their distance from the same in longdouble"""
    A, W0, H0 = _case(name)
    f, g = R.fit(A, W0, H0, beta, tol=0.0, max_iter=30), R.fit(A.astype(LD), W0.astype(LD), H0.astype(LD), beta, tol=0.0, max_iter=30)
    top = max(f["W"].max(), f["H"].max())
    return f, float(max(np.abs(f["W"] - g["W"]).max(), np.abs(f["H"] - g["H"]).max()) / top)


def _run(gpu, name, beta, mat=None, **kw):
    A, W0, H0 = _case(name)
    own = mat is None
    mat = gpu.DenseMatrix.from_host(A, storage=CASES[name][4]) if own else mat
    try:
        r = gpu.nmf_conv_dense(mat, torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda(), beta_loss=beta, **kw)
    finally:
        if own:
            mat.close()
    r.W, r.H = r.W.cpu().numpy(), r.H.cpu().numpy()
    return r


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    worst = float((np.abs(got.astype(LD) - ref) / np.where(live, ref, 1))[live].max())
    print(f"{tag}: {worst / R.U53:.1f} u (bar {bar / R.U53:.0f} u), {int((~live).sum())} exact zeros")
    assert np.array_equal(got == 0, ref64 == 0) and worst <= bar


@EACH
@BOTH
def test_one_step_of_each_side(gpu, name, beta):
    (A, W0, H0), (m, n, k, T, _) = _case(name), CASES[name]
    bar = lambda L: 4 * ((2 - beta) * (T * k + T) + L + 8) * R.U53
    h = _run(gpu, name, beta, tol=0.0, max_iter=1, update_W=False)
    both = _run(gpu, name, beta, tol=0.0, max_iter=1)
    assert np.array_equal(h.W, W0) and h.n_iter == 1 and not h.converged and np.array_equal(both.H, h.H)
    _check_step(h.H, R.step_h(A.astype(LD), W0.astype(LD), H0.astype(LD), beta), bar(m), f"{name} beta {beta} H step")
    # the W step from the device's own new H: what is compared is the W step alone
    _check_step(both.W, R.step_w(A.astype(LD), W0.astype(LD), both.H.astype(LD), beta), bar(n), f"{name} beta {beta} W step")


def _close(r, ref, dist, tag):
    top, bar = max(ref["W"].max(), ref["H"].max()), max(1e-12, 50 * dist)
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    assert ew <= bar and eh <= bar, f"{tag}: W {ew:.2e} H {eh:.2e}, bar {bar:.2e} (float64 to longdouble restatement {dist:.2e})"


@EACH
@BOTH
def test_fit_of_30_iterations(gpu, name, beta):
    (ref, dist), A = _fits(name, beta), _case(name)[0]
    mat = gpu.DenseMatrix.from_host(A, storage=CASES[name][4])
    try:
        r, r2 = _run(gpu, name, beta, mat, tol=0.0, max_iter=30), _run(gpu, name, beta, mat, tol=0.0, max_iter=30)
        d = mat.conv_divergence(torch.from_numpy(r.W).cuda(), torch.from_numpy(r.H).cuda(), beta)
    finally:
        mat.close()
    _close(r, ref, dist, f"{name} beta {beta}")
    assert r.n_iter == 30 and not r.converged and r.error <= r.error_init and d.error == r.error
    assert abs(r.error_init - ref["error_init"]) <= 1e-12 * ref["error_init"] and abs(r.error - ref["error"]) <= 1e-12 * ref["error"]
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.error_init, r.error) == (r2.error_init, r2.error)


@pytest.mark.parametrize("name", ["ragged_bf16", "full", "longlag"])
@BOTH
def test_divergence(gpu, name, beta):
    A, W0, H0 = _case(name)
    mat = gpu.DenseMatrix.from_host(A, storage=CASES[name][4])
    try:
        got = mat.conv_divergence(torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda(), beta)
    finally:
        mat.close()
    D, mag = R.divergence(A.astype(LD), W0.astype(LD), H0.astype(LD), beta)
    assert abs(got.divergence - D) <= 1e-12 * float(mag)


@BOTH
def test_no_lag_is_the_existing_solver(gpu, beta):
    A, W0, H0 = _case("t1")
    mat = gpu.DenseMatrix.from_host(A)
    try:
        r = _run(gpu, "t1", beta, mat)
        old = gpu.nmf_beta_dense(mat, W0[0], H0, beta_loss=beta)
    finally:
        mat.close()
    assert r.n_iter == old.n_iter and r.converged == old.converged
    _close(r, dict(W=old.W[None], H=old.H), _fits("t1", beta)[1], f"t1 beta {beta} against nmf_beta_dense")


@BOTH
def test_stopping_rule(gpu, beta):
    # chosen on the CPU, float64 and longdouble alike: on "ragged" the relative decrease per ten iterations runs 0.541, 0.0367, 0.0186
    # at beta = 0 and 0.592, 0.0386, 0.0375, 0.0408, 0.0331, 0.0264 at beta = 1, so tol = 0.03 stops at 30 / 60: the nearest value is
    # 10 % away from tol, rounding moves it by 1e-14
    ref = R.fit(*_case("ragged"), beta, tol=0.03, max_iter=200)
    r = _run(gpu, "ragged", beta, tol=0.03, max_iter=200)
    assert ref["n_iter"] == (60 if beta else 30) and ref["converged"]
    assert (r.n_iter, r.converged) == (ref["n_iter"], True)


def test_fold_in_on_a_single_copy(gpu):
    A = _case("ragged")[0]
    single = gpu.DenseMatrix.from_host(A, single_copy=True)
    try:
        a = _run(gpu, "ragged", 0, single, tol=0.0, max_iter=5, update_W=False)
        with pytest.raises(gpu._lib.SmallkError, match="single-copy") as e:
            _run(gpu, "ragged", 0, single, max_iter=1)
        assert e.value.code == gpu._lib.UNSUPPORTED
    finally:
        single.close()
    b = _run(gpu, "ragged", 0, tol=0.0, max_iter=5, update_W=False)
    assert np.array_equal(a.H, b.H) and np.array_equal(a.W, b.W) and a.error == b.error


def test_refusals_leave_the_factors_untouched(gpu):
    L, (A, W0, H0) = gpu._lib, _case("longlag")
    m, n, k = 33, 40, 3
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    mat, zero, neg = gpu.DenseMatrix.from_host(A), gpu.DenseMatrix.from_host(np.where(A > 5, 0, A)), gpu.DenseMatrix.from_host(-A)
    shard = gpu.DenseMatrix(m, 2 * n, col0=0, ncols=n)

    def refused(code, a, W, H, beta=0, **kw):
        W1, H1 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            gpu.nmf_conv_dense(a, W1, H1, beta_loss=beta, inplace=True, **kw)
        assert e.value.code == code and bool((W1 == W).all()) and bool((H1 == H).all())

    def direct(code, T, beta):          # what the Python layer never passes on: T < 1, another beta
        W, H, o, st = dev(W0), dev(H0), L.PenaltyOptions(0.0, 0.0, 0.0, 1e-4, 5, 1), L.KlStats()
        rc = L.lib().smk_nmf_conv_dense_device(mat._h, k, T, ctypes.c_double(beta), ctypes.byref(o), ctypes.c_void_p(W.data_ptr()), L.DT_F64, m * k, k, 1,
                                               ctypes.c_void_p(H.data_ptr()), L.DT_F64, n, 1, None, ctypes.byref(st))
        assert rc == code and np.array_equal(W.cpu().numpy(), W0) and np.array_equal(H.cpu().numpy(), H0)

    try:
        W, H = dev(W0), dev(H0)
        refused(L.UNSUPPORTED, mat, dev(np.ones((33, m, 4))), dev(np.ones((4, n))))        # 33 * 4 > 128
        refused(L.UNSUPPORTED, mat, dev(np.ones((9, m, 13))), dev(np.ones((13, n))))       # 9 * roundup(13, 4) > 128
        refused(L.BAD_PARAM, mat, dev(np.ones((41, m, 3))), dev(np.ones((3, n))))          # T > n
        refused(L.UNSUPPORTED, shard, W, H)
        refused(L.BAD_PARAM, neg, W, H, beta=1)
        refused(L.BAD_PARAM, zero, W, H, beta=0)
        assert gpu.nmf_conv_dense(zero, W, H, beta_loss=1, max_iter=1, tol=0.0).n_iter == 1
        refused(L.BAD_PARAM, mat, W, H, alpha_W=-1.0)
        direct(L.BAD_PARAM, 0, 0.0)
        direct(L.UNSUPPORTED, 32, 0.5)
        direct(L.UNSUPPORTED, 32, 2.0)
        direct(L.BAD_PARAM, 32, -1.0)
        for bad in ("frobenius", 2, 0.5, None, True):
            with pytest.raises(ValueError):
                gpu.nmf_conv_dense(mat, W, H, beta_loss=bad)
        for Wb, Hb in ((W[0], H), (W, H[:, :-1]), (W.cpu(), H), (W0, H0)):
            with pytest.raises(ValueError):
                gpu.nmf_conv_dense(mat, Wb, Hb, beta_loss=0)
            with pytest.raises(ValueError):
                mat.conv_divergence(Wb, Hb, 0)
    finally:
        for a in (mat, zero, neg, shard):
            a.close()

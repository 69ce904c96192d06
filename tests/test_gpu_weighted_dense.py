"""Weighted masked beta-divergence NMF on a dense resident matrix (smallk_amd.nmf_weighted_dense, DenseMatrix.weighted_divergence;
smallk_amd/csrc/weighted_dense.hip, weighted_dense.cpp) against the numpy restatement
tests/weighted_dense_reference.py.  Meant to pass under SMK_POISON=1 as well.

Cases: A, W0 and H0 are tests/test_gpu_masked_dense.case()'s draws at the shapes below -- each factor pitch once (k = 3, 5 and 16: 16;
17: 32; 33: 64; 128: 128, under both storages, whose weight tiles travel differently), each beta, the tile edges 63 / 65 / 67 / 130, and
2050 rows for spans of two tiles (the hand-over of the weight tile from one tile to the next).  The shapes keep one dimension below
64 or both at 130, so that the 64 x 64 tile of NaN of those draws leaves every row and column measured entries.  Weights: 2^e (0.25 +
U[0, 1)), e in -3 .. 3, rounded to the storage type, 20 % exact zeros, and column n / 2 + 1 and row m / 3 + 1 wholly 0 beside the
column n / 2 and row m / 3 of NaN.  case() asserts, on the CPU, that exactly those two columns and two rows have no measured entry of
positive weight: every other entry of H and W compared below has a positive reference denominator.

Bars (u = 2^-24).  One H step / one W step from a float32-rounded start against the numpy.longdouble restatement, entry by entry and
relative: 4 (c k + L + 10) u, the masked fp32 bar plus one more fp32 rounding in each of the two sums; exact zeros equal, no NaN.
Thirty iterations: within max(8 x the distance between the float64 and float32 restatements, 16 u), the masked fp32 test's rule.
The rest is exact."""
import functools
from unittest import mock

import numpy as np
import pytest

import masked_dense_reference as MR
import test_gpu_masked_dense as MD
import weighted_dense_reference as R

pytestmark = pytest.mark.gpu

# name -> (m, n, k, beta, storage, seed)
CASES = {"fro_k3": (65, 63, 3, 2, "f32", 1), "is_k17": (63, 130, 17, 0, "f32", 2), "kl_k33_bf16": (67, 63, 33, 1, "bf16", 3),
         "fro_k128": (130, 130, 128, 2, "f32", 4), "is_k128_bf16": (130, 130, 128, 0, "bf16", 5), "kl_k5_spans": (2050, 63, 5, 1, "f32", 6),
         "is_k16_bf16_spans": (2050, 63, 16, 0, "bf16", 7)}
U24, LD = 2.0 ** -24, np.longdouble


@functools.lru_cache(maxsize=None)
def case(name):
    """the masked test's dict for this file's shape (A is "train", the start rounded to float32) with the weights "V" """
    with mock.patch.dict(MD.CASES, {"weighted_" + name: CASES[name]}):
        c = dict(MD.case("weighted_" + name))
    (m, n), rng = c["train"].shape, np.random.default_rng(100 + CASES[name][5])
    V = (2.0 ** rng.integers(-3, 4, (m, n)) * (0.25 + rng.random((m, n)))).astype(np.float32).astype(np.float64)
    V = MD._bf16(V) if c["storage"] == "bf16" else V
    V[rng.random((m, n)) < 0.2] = 0.0
    V[m // 3 + 1, :] = V[:, n // 2 + 1] = 0.0
    live = ~np.isnan(c["train"]) & (V > 0)
    assert np.array_equal(np.flatnonzero(~live.any(0)), [n // 2, n // 2 + 1]) and np.array_equal(np.flatnonzero(~live.any(1)), [m // 3, m // 3 + 1])
    assert c["beta"] != 0 or not (c["train"] == 0).any()
    c.update(V=V, W0=c["W0"].astype(np.float32).astype(np.float64), H0=c["H0"].astype(np.float32).astype(np.float64))
    return c


class Pair:
    """A and V resident, closed together"""

    def __init__(self, gpu, A, V, storage="f32", **kw):
        self.A, self.V = gpu.DenseMatrix.from_host(A, storage=storage, **kw), gpu.DenseMatrix.from_host(V, storage=storage, **kw)

    def __enter__(self):
        return self.A, self.V

    def __exit__(self, *exc):
        self.A.close()
        self.V.close()


def _check_step(got, ref, bar, tag):
    ref64 = np.asarray(ref, dtype=np.float64)
    live = ref64 > 0
    worst = float((np.abs(got.astype(LD) - ref)[live] / ref[live]).max())
    print(f"{tag}: {worst / U24:.1f} u (bar {bar / U24:.0f} u), {int((~live).sum())} exact zeros")
    assert not np.isnan(got).any() and np.array_equal(got == 0, ref64 == 0) and worst <= bar


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_of_each_side(gpu, name):
    c = case(name)
    (m, n), k, beta, A, V, W0, H0 = c["train"].shape, c["k"], c["beta"], c["train"], c["V"], c["W0"], c["H0"]
    with Pair(gpu, A, V, c["storage"]) as (mat, wts):
        h = gpu.nmf_weighted_dense(mat, wts, W0, H0, beta_loss=beta, update_W=False, tol=0.0, max_iter=1)
        both = gpu.nmf_weighted_dense(mat, wts, W0, H0, beta_loss=beta, tol=0.0, max_iter=1)
    assert np.array_equal(h.W, W0) and np.array_equal(both.H, h.H) and h.n_iter == 1 and not h.converged
    bar = lambda L: MR.step_bar(beta, k, L) * 2.0 ** 29 + 8 * U24          # 4 (c k + L + 8) u + 4 . 2 u
    _check_step(h.H, R.step_h(A, V, W0.astype(LD), H0.astype(LD), beta), bar(m), f"{name} H step")
    # the W step from the device's own new H: what is compared is the W step alone
    _check_step(both.W, R.step_w(A, V, W0.astype(LD), both.H.astype(LD), beta), bar(n), f"{name} W step")
    # the column and the row of NaN, the column and the row of weight 0
    assert (h.H[:, n // 2:n // 2 + 2] == 0).all() and (both.W[m // 3:m // 3 + 2, :] == 0).all()


@functools.lru_cache(maxsize=None)
def _restatements(name):
    """the float64 and the float32 restatement of 30 iterations, formed once per session"""
    c = case(name)
    return tuple(R.fit(c["train"], c["V"], c["W0"], c["H0"], beta=c["beta"], max_iter=30, dtype=dt) for dt in (np.float64, np.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_short_fit(gpu, name):
    c, (ref64, ref32) = case(name), _restatements(name)
    kw = dict(beta_loss=c["beta"], tol=0.0, max_iter=30)
    with Pair(gpu, c["train"], c["V"], c["storage"]) as (mat, wts):
        r = gpu.nmf_weighted_dense(mat, wts, c["W0"], c["H0"], **kw)
        passes = gpu.weighted_dense_last_profile()
        r2 = gpu.nmf_weighted_dense(mat, wts, c["W0"], c["H0"], **kw)
        d = mat.weighted_divergence(wts, r.W, r.H, c["beta"])
    top = max(ref64["W"].max(), ref64["H"].max())
    dist = lambda a, b: max(np.abs(a["W"] - b["W"]).max(), np.abs(a["H"] - b["H"]).max()) / top
    rel = lambda a, b: abs(a - b) / ref64["error"]
    between, e_between = dist(ref32, ref64), rel(ref32["error"], ref64["error"])
    got, e_got = dist({"W": r.W, "H": r.H}, ref64), rel(r.error, ref64["error"])
    print(f"fit {name}: factors {got:.2e} from float64 (the float32 restatement {between:.2e}), error {e_got:.2e} ({e_between:.2e})")
    assert r.n_iter == 30 and not r.converged and not np.isnan(r.W).any() and not np.isnan(r.H).any()
    assert got <= max(8 * between, 16 * U24)
    assert e_got <= max(8 * e_between, 16 * U24)
    # exact: the error is the fp64 weighted divergence of the returned factors, whose mean is over the sum of the weights; the
    # factors are fp32 numbers; a second run gives the same bits
    D, mag, sw = R.divergence(c["train"], c["V"], r.W.astype(LD), r.H.astype(LD), c["beta"])
    assert d.error == r.error and passes == (60, 2) and d.count == int((~np.isnan(c["train"])).sum())
    # the masked divergence test's bar: 1e-12 of the sum of the absolute values of the terms
    assert abs(d.weight - float(sw)) <= 1e-12 * float(sw) and d.mean == d.divergence / d.weight and abs(d.divergence - float(D)) <= 1e-12 * float(mag)
    assert np.array_equal(r.W, r.W.astype(np.float32)) and np.array_equal(r.H, r.H.astype(np.float32))
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H) and (r.error_init, r.error) == (r2.error_init, r2.error)


@pytest.mark.parametrize("name", ["fro_k128", "kl_k33_bf16", "is_k17"])
def test_the_two_identities(gpu, name):
    c = case(name)
    (m, n), A, V, W0, H0 = c["train"].shape, c["train"], c["V"], c["W0"], c["H0"]
    kw = dict(beta_loss=c["beta"], max_iter=30)
    with Pair(gpu, A, np.ones_like(V), c["storage"]) as (mat, ones):
        one = gpu.nmf_weighted_dense(mat, ones, W0, H0, **kw)
        masked = gpu.nmf_masked_dense(mat, W0, H0, precision="fp32", **kw)
    assert np.array_equal(one.W, masked.W) and np.array_equal(one.H, masked.H)
    assert (one.error_init, one.error, one.n_iter, one.converged) == (masked.error_init, masked.error, masked.n_iter, masked.converged)
    with Pair(gpu, A, V, c["storage"]) as (mat, wts), Pair(gpu, A, 4 * V, c["storage"]) as (_, wts4):
        x, y = (gpu.nmf_weighted_dense(mat, v, W0, H0, tol=0.0, **kw) for v in (wts, wts4))
    assert np.array_equal(x.W, y.W) and np.array_equal(x.H, y.H)
    assert (x.H[:, n // 2:n // 2 + 2] == 0).all() and (x.W[m // 3:m // 3 + 2, :] == 0).all() and (x.H[:, :n // 2] > 0).any()


def test_refusals_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    A = 0.5 + rng.random((130, 131))
    A[rng.random(A.shape) < 0.4] = np.nan
    V = 0.25 + rng.random(A.shape)
    dense = gpu.DenseMatrix.from_host

    def changed(M, v, at=(7, 11)):
        B = M.copy()
        B[at] = v
        return dense(B)

    mats = {"A": dense(A), "V": dense(V), "A neg": changed(A, -1.0), "A zero": changed(A, 0.0), "A empty": dense(np.full(A.shape, np.nan)),
            "A single": dense(A, single_copy=True), "V single": dense(V, single_copy=True),
            "A sparse": gpu.SparseMatrix.from_observed(np.nan_to_num(A), ~np.isnan(A)), "V short": dense(V[:129]), "V narrow": dense(V[:, :130]),
            "V bf16": dense(V, storage="bf16"), "V neg": changed(V, -0.5), "V nan": changed(V, np.nan), "V inf": changed(V, np.inf),
            "V unmeasured": dense(np.where(np.isnan(A), 1.0, 0.0))}
    # (A, V, k, beta, exception, code, message)
    table = [("A", "V", 4, 0.5, ValueError, None, None), ("A sparse", "V", 4, 2, ValueError, None, None),
             ("A neg", "V", 4, 2, L.SmallkError, L.BAD_PARAM, "negative"), ("A zero", "V", 4, 0, L.SmallkError, L.BAD_PARAM, "add a small value"),
             ("A empty", "V", 4, 1, L.SmallkError, L.BAD_PARAM, "no measured entry"), ("A", "V", 129, 2, L.SmallkError, L.UNSUPPORTED, "k > 128"),
             ("A single", "V single", 4, 0, L.SmallkError, L.UNSUPPORTED, "single-copy"),
             ("A", "V short", 4, 2, L.SmallkError, L.BAD_PARAM, "height"), ("A", "V narrow", 4, 2, L.SmallkError, L.BAD_PARAM, "width"),
             ("A", "V bf16", 4, 2, L.SmallkError, L.BAD_PARAM, "storage type"), ("A", "V single", 4, 1, L.SmallkError, L.BAD_PARAM, "stored copies"),
             ("A", "V neg", 4, 1, L.SmallkError, L.BAD_PARAM, "a negative value, a NaN or an infinity"),
             ("A", "V nan", 4, 2, L.SmallkError, L.BAD_PARAM, "a negative value, a NaN or an infinity"),
             ("A", "V inf", 4, 0, L.SmallkError, L.BAD_PARAM, "a negative value, a NaN or an infinity"),
             ("A", "V unmeasured", 4, 2, L.SmallkError, L.BAD_PARAM, "positive weight")]
    try:
        for a, v, k, beta, exc, code, match in table:
            W, H = torch.from_numpy(rng.random((130, k))).to(dev), torch.from_numpy(rng.random((k, 131))).to(dev)
            W0, H0 = W.clone(), H.clone()
            with pytest.raises(exc, match=match) as e:
                gpu.nmf_weighted_dense(mats[a], mats[v], W, H, beta_loss=beta, inplace=True, max_iter=2)
            assert code is None or e.value.code == code, (a, v)
            assert bool((W == W0).all()) and bool((H == H0).all())
        # a stored zero in A is a measurement at beta = 1; the single copies serve the fold-in with the two-copy result's bits
        assert gpu.nmf_weighted_dense(mats["A zero"], mats["V"], W, H, beta_loss=1, max_iter=1, tol=0.0).n_iter == 1
        s = gpu.nmf_weighted_dense(mats["A single"], mats["V single"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0)
        b = gpu.nmf_weighted_dense(mats["A"], mats["V"], W, H, beta_loss=0, update_W=False, max_iter=3, tol=0.0)
        assert bool((s.H == b.H).all()) and s.error == b.error and gpu.weighted_dense_last_profile() == (3, 2)
    finally:
        for x in mats.values():
            x.close()

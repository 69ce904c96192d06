"""The entries that take W and H as strided views in device memory, through the C ABI (``smallk_amd._lib``, raw ctypes: the Python
wrappers would filter most of these inputs before the library sees them).

Part 1, the rejection table: what each of the nine entries answers to an input that is wrong in exactly one way -- the result code
and the text of ``smk_last_error()``.  m = 5, n = 7, k = 3.  The expected rows are literals, written down once from the source of
the entries; a rejected call launches nothing.  The view "one past its allocation" is a tensor of exactly rows x cols elements
passed with a column stride of rows + 1; it is the tail of a 20 MiB buffer allocated right after the caching allocator was
emptied, so that the tensor ends where its allocation ends (a 15-element tensor of its own would sit in the middle of a 2 MiB
segment of the caching allocator, which is all the runtime knows of; as in test_gpu_residual.py).

Part 2, views against contiguous fp64: each entry once with contiguous float64 factors and once with float32 tensors of the same
values handed in as non-contiguous views (W the transpose of a k x m tensor, H every second column of a k x 2n tensor), at
(m, n, k) = (19, 23, 3) [KP 8] and (19, 23, 17) [KP 32]: the pad edge of the resident layout, where a swapped stride pair or a
missing zero fill of the workspace shows.  The values are drawn as float32 and widened for the first run, so both runs compute on
the same fp64 numbers: the float32 results equal the rounded float64 results bit for bit, scalars and statistics are equal, and
the columns of the 2n-wide tensor that the view skips keep their sentinel."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, K = 5, 7, 3
BAD_PARAM = -3
F64, F32, BF16, UNKNOWN = 0, 1, 2, 9

# ---- part 1 ----------------------------------------------------------------------------------------------------------------
# entry -> its name in the texts, its views as (name in the text, rows, cols, is an output), the text for a null view (None: the
# view check's own "null pointer"), the text for a wrong element type, whether k is an argument and whether k > min(m, n) is checked
ENTRIES = {
    "set_factors": dict(prefix="smk_solver_set_factors_device", views=(("W0", M, K, False), ("H0", K, N, False)), null=None,
                        dtype="smk_solver_set_factors_device: factors are fp64 or fp32", has_k=False, kmin=False, options=False),
    "get_factors": dict(prefix="smk_solver_get_factors_device", views=(("W", M, K, True), ("H", K, N, True)), null=None,
                        dtype="smk_solver_get_factors_device: factors are fp64 or fp32", has_k=False, kmin=False, options=False),
    "residual": dict(prefix="smk_matrix_residual_device", views=(("W", M, K, False), ("H", K, N, False)),
                     null="smk_matrix_residual_device: null matrix or factor",
                     dtype="smk_matrix_residual_device: factors are fp64 or fp32", has_k=True, kmin=False, options=False),
    "svd": dict(prefix="smk_matrix_svd_device", views=(("U", M, K, True), ("V", N, K, True)), null=None,
                dtype="smk_matrix_svd_device: U and V are fp64 or fp32", has_k=True, kmin=True, options=False),
    "nndsvd": dict(prefix="smk_matrix_nndsvd_device", views=(("W", M, K, True), ("H", K, N, True)), null=None,
                   dtype="smk_matrix_nndsvd_device: W and H are fp64 or fp32", has_k=True, kmin=True, options=False),
    "nmf_cd": dict(prefix="smk_nmf_cd_device", views=(("W", M, K, True), ("H", K, N, True)), null="smk_nmf_cd_device: null argument",
                   dtype="smk_nmf_cd_device: W and H are fp64 or fp32", has_k=True, kmin=True, options=True),
    "nmf_kl": dict(prefix="smk_nmf_kl_device", views=(("W", M, K, True), ("H", K, N, True)), null="smk_nmf_kl_device: null argument",
                   dtype="smk_nmf_kl_device: W and H are fp64 or fp32", has_k=True, kmin=True, options=True),
    "kl_divergence": dict(prefix="smk_matrix_kl_divergence_device", views=(("W", M, K, False), ("H", K, N, False)),
                          null="smk_matrix_kl_divergence_device: null argument",
                          dtype="smk_matrix_kl_divergence_device: W and H are fp64 or fp32", has_k=True, kmin=True, options=False),
    "labels": dict(prefix="smk_labels_device", views=(("H", K, N, False),), null="smk_labels_device: null factor",
                   dtype="smk_labels_device: factors are fp64 or fp32", has_k=True, kmin=False, options=False),
    "top_terms": dict(prefix="smk_top_terms_device", views=(("W", M, K, False),), null="smk_top_terms_device: null factor",
                      dtype="smk_top_terms_device: factors are fp64 or fp32", has_k=True, kmin=False, options=False),
}
OPTION_ROWS = [(dict(alpha_w=-1.0), ": alpha_w and alpha_h must be >= 0"), (dict(alpha_h=-1.0), ": alpha_w and alpha_h must be >= 0"),
               (dict(alpha_w=math.nan), ": alpha_w and alpha_h must be >= 0"), (dict(l1_ratio=1.5), ": l1_ratio must lie in [0, 1]"),
               (dict(l1_ratio=-0.5), ": l1_ratio must lie in [0, 1]"), (dict(tol=-1.0), ": tol must be >= 0"),
               (dict(max_iter=0), ": max_iter < 1")]


def _rows():
    """(id, entry, what to change, expected text); every row expects SMK_BAD_PARAM"""
    out = []
    for name, e in ENTRIES.items():
        for i, (vname, rows, cols, output) in enumerate(e["views"]):
            what = f"{e['prefix']}({vname})"
            out.append((f"{name}-{vname}-null", name, ("view", i, "null"), e["null"] or what + ": null pointer"))
            out.append((f"{name}-{vname}-bf16", name, ("view", i, "bf16"), e["dtype"]))
            out.append((f"{name}-{vname}-unknown-dtype", name, ("view", i, "unknown"), e["dtype"]))
            out.append((f"{name}-{vname}-negative-stride", name, ("view", i, "negative"), what + ": negative stride"))
            if output:
                out.append((f"{name}-{vname}-zero-stride", name, ("view", i, "zero"), what + ": the elements of an output overlap"))
                out.append((f"{name}-{vname}-equal-strides", name, ("view", i, "equal"), what + ": the elements of an output overlap"))
            out.append((f"{name}-{vname}-host-pointer", name, ("view", i, "host"), what + ": not a pointer to memory of the current device"))
            out.append((f"{name}-{vname}-past-allocation", name, ("view", i, "past"), what + ": the strided extent leaves the allocation"))
        if e["has_k"]:
            out.append((f"{name}-k0", name, ("k", 0), e["prefix"] + ": k < 1"))
        if e["kmin"]:
            out.append((f"{name}-k-above-min", name, ("k", min(M, N) + 1), e["prefix"] + ": k exceeds min(m, n)"))
        if e["options"]:
            for j, (change, text) in enumerate(OPTION_ROWS):
                out.append((f"{name}-option-{j}-{next(iter(change))}", name, ("option", change), e["prefix"] + text))
    return out


ROWS = _rows()


def _view(t):
    code = {"torch.float64": F64, "torch.float32": F32}[str(t.dtype)]
    return [C.c_void_p(t.data_ptr()), code, int(t.stride(0)), int(t.stride(1))]


def _options(kind, **change):
    o = dict(alpha_w=0.01, alpha_h=0.02, l1_ratio=0.5, tol=0.0, max_iter=3, update_w=1)
    o.update(change)
    return kind(o["alpha_w"], o["alpha_h"], o["l1_ratio"], o["tol"], o["max_iter"], o["update_w"])


class Bench:
    """the handles one shape needs and one caller per entry: views are [pointer, element type, row stride, column stride]"""

    def __init__(self, gpu, torch, m, n, k, seed=5):
        self.S, self.L, self.lib, self.torch = gpu, gpu._lib, gpu._lib.lib(), torch
        self.m, self.n, self.k = m, n, k
        rng = np.random.default_rng(seed)
        self.dense = gpu.DenseMatrix.from_host(rng.random((m, n)).astype(np.float32).astype(np.float64))
        mask = rng.random((m, n)) < 0.3
        mask[np.arange(m), np.arange(m) % n] = True            # no empty row
        mask[np.arange(n) % m, np.arange(n)] = True            # no empty column
        vals = np.where(mask, rng.random((m, n)) + 0.1, 0.0)
        indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.uint32)
        indices = np.concatenate([np.nonzero(mask[:, j])[0] for j in range(n)]).astype(np.uint32)
        data = np.concatenate([vals[mask[:, j], j] for j in range(n)])
        self.sparse = gpu.SparseMatrix(data, indices, indptr, (m, n))
        self.solver = gpu.NmfSolver(self.dense, gpu.make_options(m, n, k, "MU"))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        self.solver.close()
        self.sparse.close()
        self.dense.close()

    def svd_options(self, k):
        return self.L.SvdOptions(int(k), 2, 1, 7, None, F64, 0, 0)

    def set_factors(self, v, k=None, o=None):
        return self.lib.smk_solver_set_factors_device(self.solver._h, *v[0], *v[1], self.stream), None

    def get_factors(self, v, k=None, o=None):
        return self.lib.smk_solver_get_factors_device(self.solver._h, 0, *v[0], *v[1], self.stream), None

    def residual(self, v, k, o=None):
        r, a = C.c_double(0), C.c_double(0)
        col = self.torch.zeros(self.n, dtype=self.torch.float64, device="cuda")
        rc = self.lib.smk_matrix_residual_device(self.dense._h, k, *v[0], *v[1], self.stream, C.byref(r), C.byref(a), C.c_void_p(col.data_ptr()))
        return rc, (r.value, a.value, col)

    def svd(self, v, k, o=None):
        S = (C.c_double * max(k, 1))()
        return self.lib.smk_matrix_svd_device(self.dense._h, C.byref(self.svd_options(k)), *v[0], S, *v[1], self.stream), list(S)

    def nndsvd(self, v, k, o=None):
        return self.lib.smk_matrix_nndsvd_device(self.dense._h, C.byref(self.svd_options(k)), self.L.NNDSVD, *v[0], *v[1], self.stream), None

    def nmf_cd(self, v, k, o=None):
        st = self.L.CdStats()
        o = o or _options(self.L.CdOptions)
        rc = self.lib.smk_nmf_cd_device(self.dense._h, k, C.byref(o), *v[0], *v[1], self.stream, C.byref(st))
        return rc, (st.iterations, st.converged, st.violation_init, st.violation)

    def nmf_kl(self, v, k, o=None):
        st = self.L.KlStats()
        o = o or _options(self.L.KlOptions)
        rc = self.lib.smk_nmf_kl_device(self.sparse._h, k, C.byref(o), *v[0], *v[1], self.stream, C.byref(st))
        return rc, (st.iterations, st.converged, st.error_init, st.error)

    def kl_divergence(self, v, k, o=None):
        out = (C.c_double * 3)()
        return self.lib.smk_matrix_kl_divergence_device(self.sparse._h, k, *v[0], *v[1], self.stream, out), list(out)

    def labels(self, v, k, o=None):
        lab = self.torch.zeros(self.n, dtype=self.torch.int32, device="cuda")
        return self.lib.smk_labels_device(*v[0], k, self.n, self.stream, C.c_void_p(lab.data_ptr()), None), lab

    def top_terms(self, v, k, o=None):
        terms = self.torch.zeros((max(k, 1), 2), dtype=self.torch.int32, device="cuda")
        return self.lib.smk_top_terms_device(*v[0], self.m, k, 2, self.stream, C.c_void_p(terms.data_ptr())), terms


@pytest.fixture(scope="module")
def table(gpu):
    torch = pytest.importorskip("torch")
    b = Bench(gpu, torch, M, N, K)
    torch.cuda.empty_cache()
    b.own = torch.zeros(20 * 2 ** 20 // 8, dtype=torch.float64, device="cuda")       # an allocation of its own: it ends where the tensor ends
    b.host = np.zeros(64)
    b.good = {(r, c): torch.rand((r, c), dtype=torch.float64, device="cuda") + 0.1 for r, c in ((M, K), (K, N), (N, K))}
    yield b
    b.close()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_rejection_table(table, row):
    _, name, change, text = row
    b, e = table, ENTRIES[name]
    views = [_view(b.good[(rows, cols)]) for _, rows, cols, _ in e["views"]]
    k, o = K, None
    if change[0] == "view":
        _, i, how = change
        _, rows, cols, _ = e["views"][i]
        v = views[i]
        if how == "null":
            v[0] = None
        elif how == "bf16":
            v[1] = BF16
        elif how == "unknown":
            v[1] = UNKNOWN
        elif how == "negative":
            v[2] = -v[2]
        elif how == "zero":
            v[2] = 0
        elif how == "equal":
            v[2] = v[3] = 1
        elif how == "host":
            v[0] = C.c_void_p(b.host.ctypes.data)
        elif how == "past":              # exactly rows x cols elements, the last of them the last of the allocation; column stride rows + 1
            v[0] = C.c_void_p(b.own.data_ptr() + (b.own.numel() - rows * cols) * 8)
            v[2], v[3] = 1, rows + 1
    elif change[0] == "k":
        k = change[1]
    else:
        o = _options(b.L.CdOptions if name == "nmf_cd" else b.L.KlOptions, **change[1])
    rc, _ = getattr(b, name)(views, k, o)
    got = b.lib.smk_last_error().decode()
    print(f"{row[0]}: rc {rc}, {got!r}")
    assert rc == BAD_PARAM
    assert got.startswith(e["prefix"])
    assert got == text


# ---- part 2 ----------------------------------------------------------------------------------------------------------------
SHAPES = [(19, 23, 3), (19, 23, 17)]
SENTINEL = -7.0


@pytest.fixture(scope="module", params=SHAPES, ids=["k3_kp8", "k17_kp32"])
def bench(gpu, request):
    torch = pytest.importorskip("torch")
    m, n, k = request.param
    b = Bench(gpu, torch, m, n, k)
    g = torch.Generator().manual_seed(11)
    b.W32 = (torch.rand((m, k), generator=g, dtype=torch.float32) + 0.1).cuda()
    b.H32 = (torch.rand((k, n), generator=g, dtype=torch.float32) + 0.1).cuda()
    yield b
    b.close()


def _contiguous(b):
    """the start as contiguous float64 tensors"""
    return b.W32.double().contiguous(), b.H32.double().contiguous(), None


def _strided(b):
    """the same values as float32: W the transpose of a k x m tensor, H every second column of a k x 2n tensor of sentinels"""
    torch = b.torch
    W = b.W32.t().contiguous().t()
    wide = torch.full((b.k, 2 * b.n), SENTINEL, dtype=torch.float32, device="cuda")
    wide[:, ::2] = b.H32
    H = wide[:, ::2]
    assert W.stride() == (1, b.m) and H.stride() == (2 * b.n, 2)
    return W, H, wide


def _both_ways(b, run):
    """run(W, H) -> scalars, once per layout; compares what it left in W and H and what it returned"""
    torch = b.torch
    W64, H64, _ = _contiguous(b)
    s64 = run(W64, H64)
    W32, H32, wide = _strided(b)
    s32 = run(W32, H32)
    torch.cuda.synchronize()
    assert torch.equal(W32, W64.float()) and torch.equal(H32, H64.float())
    assert bool((wide[:, 1::2] == SENTINEL).all())
    return s64, s32


def test_residual_of_views(bench):
    b = bench

    def run(W, H):
        rc, (r, a, col) = b.residual([_view(W), _view(H)], b.k)
        assert rc == 0, b.lib.smk_last_error()
        return r, a, col

    (r64, a64, c64), (r32, a32, c32) = _both_ways(b, run)
    print(f"residual k {b.k}: {r64!r} / {r32!r}, ||A||^2 {a64!r} / {a32!r}")
    assert (r64, a64) == (r32, a32) and r64 > 0 and a64 > 0
    assert b.torch.equal(c64, c32)


@pytest.mark.parametrize("entry", ["nmf_cd", "nmf_kl"])
def test_fit_of_views(bench, entry):
    b = bench

    def run(W, H):
        rc, stats = getattr(b, entry)([_view(W), _view(H)], b.k)
        assert rc == 0, b.lib.smk_last_error()
        return stats

    s64, s32 = _both_ways(b, run)
    print(f"{entry} k {b.k}: {s64} / {s32}")
    assert s64 == s32 and s64[0] == 3


def test_nndsvd_into_views(bench):
    b = bench

    def run(W, H):
        W.fill_(SENTINEL)
        H.fill_(SENTINEL)
        rc, _ = b.nndsvd([_view(W), _view(H)], b.k)
        assert rc == 0, b.lib.smk_last_error()
        assert not bool((W == SENTINEL).any()) and not bool((H == SENTINEL).any())
        return None

    _both_ways(b, run)


def test_set_then_get_factors_through_views(bench):
    b = bench
    torch = b.torch

    def run(W, H):
        rc, _ = b.set_factors([_view(W), _view(H)])
        assert rc == 0, b.lib.smk_last_error()
        W.fill_(SENTINEL)
        H.fill_(SENTINEL)
        rc, _ = b.get_factors([_view(W), _view(H)])
        assert rc == 0, b.lib.smk_last_error()
        return None

    W64, H64, _ = _contiguous(b)
    _both_ways(b, run)
    # ... and what came back is what went in (the strided run equals the contiguous one: _both_ways)
    run(W64, H64)
    torch.cuda.synchronize()
    assert torch.equal(W64, b.W32.double()) and torch.equal(H64, b.H32.double())

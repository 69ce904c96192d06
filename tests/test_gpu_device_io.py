"""GPU tests of the device-tensor entries: a torch tensor in GPU memory becomes the resident matrix, the start of a solver or
the destination of its factors without a visit to the host.  Everything is compared bit for bit with the host path fed the same
values (the host path is what the rest of the suite pins against the oracle); the one-shot call is also compared with the oracle.

Shapes: the smallest at which a 64 x 64 tile kernel with 4-element accesses can go wrong -- one element, one row / column that
crosses a tile edge, one element short of / past a tile in either direction, exactly one tile, and (257, 131): several tiles
with ragged edges in both directions."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import make_golden as mg
from test_gpu_parity import TOL, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(1, 1), (1, 65), (65, 1), (63, 65), (64, 64), (257, 131)]
DTYPES = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LAYOUTS = ("row_major", "col_major", "offset_slice", "every_other_column", "expanded_row")
# values that tell the rounding rules apart (all >= 0: the matrices also go through one MU step)
SPECIALS = [0.0, 65504.0,                          # exact zero, the fp16 maximum
            2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24,   # fp16 subnormals
            1 + 2.0 ** -24,                        # a tie in fp32 (to even: 1)
            1 + 2.0 ** -24 + 2.0 ** -40,           # just above it (up in fp32)
            1 + 2.0 ** -8,                         # exact in fp32, a tie in bf16 (to even: 1)
            1 + 2.0 ** -8 + 2.0 ** -20,            # exact in fp32, up in bf16
            1 + 2.0 ** -8 + 2.0 ** -30,            # fp32 first makes it the tie above: 1 in bf16, 1 + 2^-7 if rounded in one step
            1 + 3 * 2.0 ** -8, 0.0, 3.0000001, 1e-3, 0.3333333333333333]


def values(rows, cols, seed):
    rng = np.random.default_rng(seed)
    v = rng.random(rows * cols) * 3.0
    v[rng.random(rows * cols) < 0.1] = 0.0
    idx = rng.permutation(rows * cols)[:len(SPECIALS)]
    v[idx] = SPECIALS[:len(idx)]
    return v.reshape(rows, cols)


def lay_out(x, layout):
    """the CPU tensor x on the GPU as a view with the given memory layout; the surroundings of a view hold 7s"""
    rows, cols = x.shape
    if layout == "row_major":
        return x.cuda()
    if layout == "col_major":
        return x.cuda().t().contiguous().t()
    if layout == "offset_slice":            # X[1:, 3:] of a tensor with an odd pitch: aligned to the element and nothing more
        pitch = cols + 3 + (1 - (cols + 3) % 2)
        big = torch.full((rows + 1, pitch), 7.0, dtype=x.dtype, device="cuda")
        big[1:, 3:3 + cols] = x.cuda()
        return big[1:, 3:3 + cols]
    if layout == "every_other_column":      # X[:, ::2]: no unit stride
        big = torch.full((rows, 2 * cols), 7.0, dtype=x.dtype, device="cuda")
        big[:, ::2] = x.cuda()
        return big[:, ::2]
    if layout == "expanded_row":            # stride 0
        return x[:1, :].cuda().expand(rows, cols)
    raise AssertionError(layout)


def mu_step(gpu, D, W0, H0):
    s = gpu.NmfSolver(D, gpu.make_options(D.height, D.ncols, W0.shape[1], "MU", min_iter=1, max_iter=1))
    s.set_factors(W0, H0)
    s.iterate(1)
    out = s.factors()
    s.close()
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_stored_bits(gpu, rows, cols, dtype):
    """every layout x storage x single_copy: the adopted matrix holds what the host path stores for the same values, and its
    stored transpose serves one MU step exactly as the host-uploaded one does"""
    x = torch.from_numpy(values(rows, cols, rows * 1000 + cols)).to(DTYPES[dtype])
    k = min(3, rows, cols)
    W0 = oracle.fill_uniform(rows, k, 43) + 0.01
    H0 = oracle.fill_uniform(k, cols, 44) + 0.01
    for layout in LAYOUTS:
        t = lay_out(x, layout)
        assert tuple(t.shape) == (rows, cols)
        want = t.cpu().double().numpy()
        if layout != "expanded_row":
            assert np.array_equal(want, x.double().numpy())
        for storage, quant in (("f32", 0), ("bf16", 1)):
            for single in (False, True):
                tag = (layout, storage, single, t.stride())
                D = gpu.DenseMatrix.from_device(t, storage=storage, single_copy=single)
                Hst = gpu.DenseMatrix.from_host(want, storage=storage, single_copy=single)
                assert D.single_copy == single
                got = D.download()
                assert np.array_equal(got, oracle.quantize(want, quant)), tag
                assert np.array_equal(got, Hst.download()), tag
                Wd, Hd = mu_step(gpu, D, W0, H0)
                Wh, Hh = mu_step(gpu, Hst, W0, H0)
                assert np.array_equal(Wd, Wh) and np.array_equal(Hd, Hh), tag
                D.close()
                Hst.close()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_to_device_round_trip(gpu, storage):
    m, n = 257, 131
    D = gpu.DenseMatrix.from_host(np.minimum(values(m, n, 5), 1000.0), storage=storage)     # inside fp16's range in either storage
    want = D.download()
    row_major = D.to_device(torch.float32)
    assert row_major.dtype == torch.float32 and row_major.is_contiguous() and row_major.is_cuda
    assert np.array_equal(row_major.cpu().numpy().astype(np.float64), want)
    col_major = torch.empty((n, m), dtype=torch.float32, device="cuda").t()
    assert D.to_device(out=col_major) is col_major and col_major.stride() == (1, m)
    assert np.array_equal(col_major.cpu().numpy().astype(np.float64), want)
    # a destination that is aligned to its element only, and the other element types (fp64 holds every stored value exactly)
    big = torch.full((m + 1, n + 4), 7.0, dtype=torch.float32, device="cuda")
    D.to_device(out=big[1:, 3:3 + n])
    assert np.array_equal(big[1:, 3:3 + n].cpu().numpy().astype(np.float64), want)
    assert (big[0] == 7).all() and (big[:, :3] == 7).all() and (big[:, 3 + n:] == 7).all()
    assert np.array_equal(D.to_device(torch.float64).cpu().numpy(), want)
    assert np.array_equal(D.to_device(torch.float16).cpu().numpy(), want.astype(np.float32).astype(np.float16))
    if storage == "bf16":
        assert np.array_equal(D.to_device(torch.bfloat16).double().cpu().numpy(), want)
    D.close()


def as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "row_major" else t.t().contiguous().t()


@pytest.mark.parametrize("alg", ["HALS", "BPP"])
@pytest.mark.parametrize("k", [3, 16, 33])
def test_factors_in_and_out(gpu, alg, k):
    """set_factors_device / factors_device against a twin solver that took the same values through the host entries: 5
    iterations, identical bits (padded ranks 8, 16 and 64: k < KP and k = KP)"""
    m, n = 257, 131
    A = mg.make_A(m, n, k, True, 0)
    W0 = oracle.fill_uniform(m, k, 43)
    H0 = oracle.fill_uniform(k, n, 44)
    D = gpu.DenseMatrix.from_host(A)
    opts = gpu.make_options(m, n, k, alg, min_iter=5, max_iter=5)
    host, dev = gpu.NmfSolver(D, opts), gpu.NmfSolver(D, opts)

    def host_run(w0, h0):
        host.set_factors(w0, h0)
        host.iterate(5)
        return host.factors()

    Wh, Hh = host_run(W0, H0)
    assert np.isfinite(Wh).all() and np.isfinite(Hh).all()
    for layout in ("row_major", "col_major"):
        tW, tH = as_layout(W0, layout), as_layout(H0, layout)
        assert tW.dtype == torch.float64 and tW.stride() == ((k, 1) if layout == "row_major" else (1, m))
        dev.set_factors_device(tW, tH)
        dev.iterate(5)
        Wd, Hd = dev.factors_device(dtype=torch.float64)
        assert Wd.is_cuda and tuple(Wd.shape) == (m, k) and tuple(Hd.shape) == (k, n)
        assert np.array_equal(Wd.cpu().numpy(), Wh) and np.array_equal(Hd.cpu().numpy(), Hh), layout
        W32, H32 = dev.factors_device(dtype=torch.float32)
        assert W32.dtype == torch.float32
        assert np.array_equal(W32.cpu().numpy(), Wh.astype(np.float32)) and np.array_equal(H32.cpu().numpy(), Hh.astype(np.float32))
    # fp32 tensors in = the host path fed the widened values
    W0f, H0f = W0.astype(np.float32), H0.astype(np.float32)
    Wh, Hh = host_run(W0f.astype(np.float64), H0f.astype(np.float64))
    dev.set_factors_device(as_layout(W0f, "row_major"), as_layout(H0f, "col_major"))
    dev.iterate(5)
    Wd, Hd = dev.factors_device()
    assert Wd.dtype == torch.float64
    assert np.array_equal(Wd.cpu().numpy(), Wh) and np.array_equal(Hd.cpu().numpy(), Hh)
    # the final NormalizeAndScale in front of the copy
    Wn, Hn = host.factors(normalize=True)
    Wdn, Hdn = dev.factors_device(normalize=True)
    assert np.array_equal(Wdn.cpu().numpy(), Wn) and np.array_equal(Hdn.cpu().numpy(), Hn)
    assert np.allclose(np.linalg.norm(Wn, axis=0), 1.0, atol=1e-9)
    host.close()
    dev.close()
    D.close()


@pytest.mark.parametrize("alg", ["HALS", "BPP"])
def test_new_contents_under_a_live_solver(gpu, alg):
    """adopt() into a matrix that already has a solver: scale and norms are measured again, as after upload()"""
    m, n, k = 256, 192, 12
    A1 = mg.make_A(m, n, k, True, 0)
    A2 = np.asfortranarray(np.ldexp(A1[::-1, :].copy(), 10))
    W0 = oracle.fill_uniform(m, k, 43)
    H0 = oracle.fill_uniform(k, n, 44)
    opts = gpu.make_options(m, n, k, alg, min_iter=3, max_iter=3)
    Dh = gpu.DenseMatrix.from_host(A1)
    Dd = gpu.DenseMatrix.from_device(torch.from_numpy(np.ascontiguousarray(A1)).cuda())
    sh, sd = gpu.NmfSolver(Dh, opts), gpu.NmfSolver(Dd, opts)
    for A, h0 in ((A1, H0), (A2, np.ldexp(H0, 10))):
        Dh.upload(A)
        sh.set_factors(W0, h0)
        sh.iterate(3)
        Wh, Hh = sh.factors()
        Dd.adopt(torch.from_numpy(np.ascontiguousarray(A)).cuda())
        sd.set_factors_device(as_layout(W0, "row_major"), as_layout(h0, "row_major"))
        sd.iterate(3)
        Wd, Hd = sd.factors_device()
        assert np.isfinite(Wh).all() and np.abs(Hh).max() > 0
        assert np.array_equal(Wd.cpu().numpy(), Wh) and np.array_equal(Hd.cpu().numpy(), Hh)
    for o in (sh, sd, Dh, Dd):
        o.close()


@pytest.mark.parametrize("alg", ["MU", "HALS", "BPP"])
@pytest.mark.parametrize("m,n,k,planted", mg.CASES)
def test_nmf_device_matches_the_oracle(gpu, m, n, k, planted, alg):
    iters = 5
    A = mg.make_A(m, n, k, planted, 0)                     # exact in fp32
    W0 = oracle.fill_uniform(m, k, 43)
    H0 = oracle.fill_uniform(k, n, 44)
    ref = oracle.nmf(A, W0, H0, alg, min_iter=iters, max_iter=iters)
    tA = torch.from_numpy(np.ascontiguousarray(A.astype(np.float32))).cuda()
    assert tA.dtype == torch.float32 and tA.is_contiguous()
    got = gpu.nmf_device(tA, as_layout(W0, "row_major"), as_layout(H0, "row_major"), alg, min_iter=iters, max_iter=iters, storage="f32")
    assert got.result == 0 and got.iteration_count == iters
    assert got.W.is_cuda and got.H.is_cuda and got.W.dtype == torch.float64
    eW, eH = rel(got.W.cpu().numpy(), ref.W), rel(got.H.cpu().numpy(), ref.H)
    print(f"nmf_device {alg} {m}x{n} k={k}: relW={eW:.3e} relH={eH:.3e}")
    assert eW < TOL and eH < TOL


# ---- sparse -----------------------------------------------------------------------------------------------------------------
def sparse_case():
    """300 x 200, about 5 % dense, an empty column (7), an empty row (11), a column of 100 entries (3)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(11)
    M = np.where(rng.random((300, 200)) < 0.05, rng.random((300, 200)) + 0.1, 0.0)
    M[:100, 3] = rng.random(100) + 0.1
    M[:, 7] = 0.0
    M[11, :] = 0.0
    S = sp.csc_matrix(M)
    assert S.indptr[8] == S.indptr[7] and S.indptr[4] - S.indptr[3] > 64 and not (S.indices == 11).any()
    return S


def download_csc(gpu, Sm, transposed):
    nc = Sm.height if transposed else Sm.ncols
    co, ri, va = np.zeros(nc + 1, np.uint32), np.zeros(Sm.nnz, np.uint32), np.zeros(Sm.nnz)
    gpu._lib.check(gpu._lib.lib().smk_matrix_download_csc(Sm._h, int(transposed), co.ctypes.data_as(C.POINTER(C.c_uint)),
                                                          ri.ctypes.data_as(C.POINTER(C.c_uint)),
                                                          va.ctypes.data_as(C.POINTER(C.c_double))), "smk_matrix_download_csc")
    return co, ri, va


@pytest.mark.parametrize("val_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
def test_sparse_from_device(gpu, idx_dtype, val_dtype):
    import scipy.sparse as sp
    S = sparse_case()
    data = S.data.astype(val_dtype)
    S = sp.csc_matrix((data.astype(np.float64), S.indices, S.indptr), shape=S.shape)      # what the device path must hold
    ref = gpu.SparseMatrix.from_scipy(S)
    co = torch.from_numpy(S.indptr.astype(idx_dtype)).cuda()
    ri = torch.from_numpy(S.indices.astype(idx_dtype)).cuda()
    va = torch.from_numpy(data).cuda()
    got = gpu.SparseMatrix.from_device(co, ri, va, S.shape)
    assert (got.height, got.ncols, got.nnz) == (300, 200, S.nnz)
    for transposed in (False, True):
        for a, b in zip(download_csc(gpu, got, transposed), download_csc(gpu, ref, transposed)):
            assert np.array_equal(a, b), transposed
    # the one-shot call on a sparse CSC tensor = nmf_sparse on the same data, bit for bit
    k = 8
    W0 = oracle.fill_uniform(300, k, 43)
    H0 = oracle.fill_uniform(k, 200, 44)
    want = gpu.nmf_sparse(S, W0, H0, "BPP", min_iter=5, max_iter=5)
    tS = torch.sparse_csc_tensor(co, ri, va, size=S.shape)
    res = gpu.nmf_device(tS, as_layout(W0, "row_major"), as_layout(H0, "row_major"), "BPP", min_iter=5, max_iter=5)
    assert res.result == want.result == 0 and res.iteration_count == want.iteration_count == 5
    assert np.array_equal(res.W.cpu().numpy(), want.W) and np.array_equal(res.H.cpu().numpy(), want.H)
    got.close()
    ref.close()


def test_sparse_bad_index_arrays_are_refused_by_the_check(gpu):
    """The validation kernel reads the index arrays inside their stated lengths and nothing else; none of these inputs reaches
    a gather."""
    S = sparse_case()
    va = torch.from_numpy(S.data).cuda()

    def attempt(indptr, indices):
        return gpu.SparseMatrix.from_device(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), va, S.shape)

    bad_row = S.indices.copy()
    bad_row[S.nnz // 2] = 300                                  # == height
    not_monotone = S.indptr.copy()
    not_monotone[5], not_monotone[6] = not_monotone[6] + 1, not_monotone[5]
    assert not_monotone[6] < not_monotone[5]
    short_span = S.indptr.copy()
    short_span[-1] -= 1
    for indptr, indices, word in ((S.indptr, bad_row, "row index"), (not_monotone, S.indices, "monotone"),
                                  (short_span, S.indices, "nnz")):
        with pytest.raises(gpu._lib.SmallkError) as e:
            attempt(indptr, indices)
        assert e.value.code == gpu._lib.BAD_PARAM and word in str(e.value), str(e.value)
    ok = attempt(S.indptr, S.indices)
    assert ok.nnz == S.nnz
    ok.close()


def test_from_device_is_ordered_after_the_producer_stream(gpu):
    """Functional coverage of the stream contract (it cannot prove the ordering): the tensor is still being produced on a
    side stream when from_device is called there without a synchronise."""
    m, n = 257, 131
    side = torch.cuda.Stream()
    base = torch.arange(m * n, dtype=torch.float32).reshape(m, n) % 7
    want = base.clone()
    for _ in range(10):                                        # small integers: exact in every type and on every device
        want = want * 2 + 1
        want = want % 1021
    with torch.cuda.stream(side):
        x = base.cuda(non_blocking=True)
        for _ in range(10):
            x = x * 2 + 1
            x = x % 1021
        D = gpu.DenseMatrix.from_device(x)
        back = D.to_device(torch.float32)
    assert np.array_equal(D.download(), want.double().numpy())
    assert torch.equal(back.cpu(), want)
    D.close()


def test_rejections_without_a_launch(gpu):
    L = gpu._lib
    m, n = 33, 17
    good = torch.rand((m, n), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        gpu.DenseMatrix.from_device(good.cpu())
    with pytest.raises(TypeError):
        gpu.DenseMatrix.from_device(torch.ones((m, n), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu.DenseMatrix.from_device(torch.ones(m, device="cuda"))
    D = gpu.DenseMatrix(m, n)
    with pytest.raises(ValueError):
        D.adopt(torch.ones((n, m), device="cuda"))
    host = np.ones((m, n), order="F")
    vp = C.c_void_p
    adopt = L.lib().smk_matrix_adopt_device
    for args, word in (((vp(host.ctypes.data), L.DT_F64, 1, m), "device"),          # a numpy host pointer
                       ((None, L.DT_F32, n, 1), "null"),
                       ((vp(good.data_ptr()), 9, n, 1), "element type"),
                       ((vp(good.data_ptr()), L.DT_F32, -n, 1), "negative"),
                       ((vp(good.data_ptr()), L.DT_F32, 1 << 40, 1), "allocation")):   # rows 2^40 elements apart
        assert adopt(D._h, *args, None) == L.BAD_PARAM, word
        assert word in L.lib().smk_last_error().decode(), (word, L.lib().smk_last_error())
    out = torch.empty((m, n), dtype=torch.float32, device="cuda")
    assert L.lib().smk_matrix_copy_to_device(D._h, vp(out.data_ptr()), L.DT_F32, 0, 1, None) == L.BAD_PARAM      # overlapping output
    s = gpu.NmfSolver(D, gpu.make_options(m, n, 4, "HALS"))
    W0 = torch.rand((m, 4), dtype=torch.float64, device="cuda")
    H0 = torch.rand((4, n), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        s.set_factors_device(W0.to(torch.float16), H0)
    with pytest.raises(ValueError):
        s.set_factors_device(W0, H0.cpu())
    with pytest.raises(ValueError):
        s.set_factors_device(W0, H0[:, :5])
    # ... and the handles still work
    D.adopt(good)
    assert np.array_equal(D.download(), good.cpu().double().numpy())
    s.set_factors_device(W0, H0)
    s.iterate(2)
    W, H = s.factors_device()
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    s.close()
    D.close()


def test_device_example_runs():
    """examples/device_nmf.py: factors a torch tensor and keeps the factors on the device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "device_nmf.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "nmf_device: result 0" in r.stdout and "W (4096, 16) on cuda:0" in r.stdout and "fp32 factors on cuda:0" in r.stdout

"""GPU tests of the fold-in step (smk_solver_project_h, NmfSolver.project, transform): H = argmin_{H >= 0} ||A - W H||_F, W fixed.

The expected H is the fp64 oracle's block pivoting, ``oracle.nnls_blockpivot(W'W, W'A~, zeros)``, with A~ the STORED values of
the resident matrix (``D.download()`` / the CSC values), so the rounding of the storage type is no part of the comparison.  W is
``uniform_host(m, k, seed)``: full column rank and well conditioned at these shapes, so the minimiser is unique.

Bar: the project's parity bar and measure (tests/test_gpu_parity.py): ||H - H_ref||_F / ||H_ref||_F <= 1e-4.  project() takes the
accurate product form on dense A, so the distance is summation order only; the measured maxima are printed (DESIGN.md 14 lists
them) and anything above 1e-8 is reported as a finding by FINDING below, which this suite asserts too."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

TOL = 1e-4
FINDING = 1e-8
M, N = 257, 131
SEG = 64


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dense_values(seed):
    rng = np.random.default_rng(seed)
    v = rng.random((M, N)) * 3.0
    v[rng.random((M, N)) < 0.1] = 0.0
    return v


def sparse_case(seed=5):
    """the shape of test_gpu_residual.py's sparse case: 300 x 200 with an empty column, an empty row, columns of exactly SEG,
    SEG + 1 and 3 SEG + 5 entries and row indices in no order inside a column"""
    m, n = 300, 200
    rng = np.random.default_rng(seed)
    rows_ok = np.array([r for r in range(m) if r != 5])
    lens = rng.integers(1, 24, n)
    lens[0], lens[10], lens[11], lens[12] = 0, SEG, SEG + 1, 3 * SEG + 5
    cols = [(rng.permutation(rows_ok)[:lens[j]], rng.random(lens[j]) * 2.0 + 0.1) for j in range(n)]
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum([len(c[0]) for c in cols])
    indices = np.concatenate([c[0] for c in cols]).astype(np.uint32)
    data = np.concatenate([c[1] for c in cols])
    dense = np.zeros((m, n))
    dense[indices.astype(np.int64), np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))] = data
    return data, indices, indptr, (m, n), dense


def reference(W, A):
    k = W.shape[1]
    ok, X, _, _ = oracle.nnls_blockpivot(W.T @ W, W.T @ A, np.zeros((k, A.shape[1])))
    assert ok
    return X


def bpp(gpu, A, k):
    return gpu.NmfSolver(A, gpu.make_options(A.height, A.ncols, k, "BPP", min_iter=100, max_iter=100, normalize=False))


def check_project(gpu, torch, A, stored, k, tag):
    m, n = stored.shape
    W = gpu.uniform_host(m, k, 100 + k)
    want = reference(W, stored)
    dW = torch.from_numpy(np.ascontiguousarray(W)).cuda()
    s = bpp(gpu, A, k)
    s.set_factors_device(dW, torch.zeros((k, n), dtype=torch.float64, device="cuda"))
    s.project()
    Wback, H = s.factors_device()
    err = rel(H.cpu().numpy(), want)
    print(tag, "k", k, "rel H", err)
    assert err <= TOL, (tag, k, err)
    assert err <= FINDING, (tag, k, err, "above the summation-order level: a finding, see DESIGN.md 14")
    assert bool((H >= 0).all())
    assert torch.equal(Wback, dW), "W must come back bit for bit"
    assert s.iteration_count == 0
    # another warm start, the same minimiser
    s.set_factors_device(dW, torch.from_numpy(np.ascontiguousarray(gpu.uniform_host(k, n, 200 + k))).cuda())
    s.project()
    H2 = s.factors_device()[1]
    assert rel(H2.cpu().numpy(), want) <= TOL and rel(H2.cpu().numpy(), H.cpu().numpy()) <= TOL
    assert s.iteration_count == 0
    s.close()
    # transform = the explicit sequence, bit for bit; from a numpy W too
    assert torch.equal(gpu.transform(A, dW), H)
    assert torch.equal(gpu.transform(A, W), H)
    return err


@pytest.mark.parametrize("k", [3, 9, 33, 130])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_project_dense(gpu, k, storage):
    torch = pytest.importorskip("torch")
    D =gpu.DenseMatrix.from_host(dense_values(3), storage=storage)
    check_project(gpu, torch, D, D.download(), k, ("dense", storage))
    D.close()


@pytest.mark.parametrize("k", [3, 9, 33])
def test_project_sparse(gpu, k):
    torch = pytest.importorskip("torch")
    data, indices, indptr, shape, dense = sparse_case()
    S = gpu.SparseMatrix(data, indices, indptr, shape)
    check_project(gpu, torch, S, dense, k, ("sparse",))
    S.close()


def test_project_after_iterations_keeps_w_and_the_count(gpu):
    """in the middle of a run: W and the iteration count stay, H becomes the minimiser for that W, and the run goes on"""
    torch = pytest.importorskip("torch")
    k = 9
    D = gpu.DenseMatrix.from_host(dense_values(4))
    s = bpp(gpu, D, k)
    s.set_factors(gpu.uniform_host(M, k, 1) + 0.01, (gpu.uniform_host(k, N, 2) + 0.01) * (2.0 / k))
    s.iterate(3)
    assert s.sync() == 0
    W3 = s.factors_device()[0]
    s.project()
    W, H = s.factors_device()
    assert torch.equal(W, W3) and s.iteration_count == 3
    assert rel(H.cpu().numpy(), reference(W.cpu().numpy(), D.download())) <= FINDING
    s.iterate(1)
    assert s.sync() == 0 and s.iteration_count == 4
    s.close()
    D.close()


def test_project_needs_a_bpp_solver_with_factors(gpu):
    L = gpu._lib
    D = gpu.DenseMatrix.from_host(dense_values(5))
    for alg, ready in (("HALS", True), ("MU", True), ("BPP", False)):
        s = gpu.NmfSolver(D, gpu.make_options(M, N, 9, alg))
        if ready:
            s.set_factors(gpu.uniform_host(M, 9, 1), gpu.uniform_host(9, N, 2))
        with pytest.raises(L.SmallkError) as e:
            s.project()
        assert e.value.code == L.BAD_PARAM and L.lib().smk_last_error()
        s.close()
    D.close()


def test_classify_the_training_set(gpu):
    """Factor a planted 512 x 256 matrix at k = 8 (20 BPP iterations), fold the same matrix in with the trained W: the labels
    must be those of the trained H in at least 95 % of the columns.  With this seed the fp64 oracle's route (oracle.nmf, then
    oracle.nnls_blockpivot from zeros) gives 100 %, checked on the CPU; the trained H is not the minimiser for the final W (W was
    updated after it), which is what the 5 % allow for."""
    torch = pytest.importorskip("torch")
    m, n, k, seed = 512, 256, 8, 7
    A = oracle.fill_planted(m, n, seed, k, quant=0)
    D = gpu.DenseMatrix.from_host(A)
    s = bpp(gpu, D, k)
    s.set_factors(oracle.fill_uniform(m, k, seed + 1) + 0.01, (oracle.fill_uniform(k, n, seed + 2) + 0.01) * (2.0 / k))
    s.iterate(20)
    assert s.sync() == 0
    W, H = s.factors_device()
    trained = gpu.labels_device(H)
    assert torch.equal(trained, s.labels_device(normalize=False))
    folded = gpu.labels_device(gpu.transform(D, W))
    share = float((trained == folded).double().mean())
    print("labels kept by the fold-in:", share)
    assert share >= 0.95
    s.close()
    D.close()

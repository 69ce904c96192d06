"""GPU tests of the reconstruction error ||A - W H||_F^2 (smk_matrix_residual, smk_matrix_residual_device, smk_solver_residual).

The reference is plain numpy fp64 on the stored values (``D.download()``): ``R = A - W @ H``, ``(R * R).sum()``,
``(R * R).sum(0)``, ``(A * A).sum()``.  No oracle is involved except to choose which algorithms the descent test keeps.

Shapes: the smallest at which a kernel with 64 x 64 tiles and padded operands can go wrong -- one element, a row / column that
crosses a tile edge, one short of / past a tile, exactly one tile, several tiles with ragged edges both ways; ranks 1, 9, 64
everywhere and, on (257, 131), every padded-rank class and two groups of 64 factor rows.

Bars of the comparison with numpy (u = 2^-53): ``a_sq`` is a sum of N <= 257 * 131 exact squares, worst case N u = 3.7e-12
relative -> 1e-11.  A term of ``resid_sq`` carries about (k + 2) u (|a| + |wh|) / |r| = 6e-14 of its own plus the sum's N u
-> 1e-10, with W and H unrelated to A so that the residual is of the size of A (no cancellation)."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 65), (65, 1), (63, 65), (64, 64), (129, 257), (257, 131)]
RANKS = [1, 9, 64]
MORE_RANKS = [2, 7, 8, 16, 33, 65, 130]          # on (257, 131): every KP class, and two groups of 64
CASES = [(m, n, k) for (m, n) in SHAPES for k in RANKS] + [(257, 131, k) for k in MORE_RANKS]
SPECIALS = [0.0, 65504.0, 2.0 ** -24, 1 + 2.0 ** -24, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.0000001, 1e-3, 0.3333333333333333]


def values(rows, cols, seed):
    """random data in [0, 3) with a tenth of exact zeros and a few values that tell the rounding rules of the storage types apart"""
    rng = np.random.default_rng(seed)
    v = rng.random(rows * cols) * 3.0
    v[rng.random(rows * cols) < 0.1] = 0.0
    idx = rng.permutation(rows * cols)[:len(SPECIALS)]
    v[idx] = SPECIALS[:len(idx)]
    return v.reshape(rows, cols)


def factors(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.random((m, k))), np.asfortranarray(rng.random((k, n)))


def numpy_ref(A, W, H):
    R = A - W @ H
    return (R * R).sum(), (A * A).sum(), (R * R).sum(0)


def close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


def check_against(res, want, tag, r_tol=1e-10, a_tol=1e-11):
    r, a, cols = want
    print(tag, "resid_sq", res.resid_sq, r, "a_sq", res.a_sq, a)
    assert close(res.a_sq, a, a_tol), (tag, res.a_sq, a)
    assert close(res.resid_sq, r, r_tol), (tag, res.resid_sq, r)
    got = np.asarray(res.col_resid_sq)
    assert got.shape == cols.shape, tag
    assert np.all(np.abs(got - cols) <= r_tol * np.abs(cols)), (tag, np.max(np.abs(got - cols) / np.maximum(cols, 1e-300)))


def storages(k):
    return ("f32", "bf16") if k <= 64 else ("f32",)


@pytest.mark.parametrize("m,n,k", CASES)
def test_exact_fit_is_exactly_zero(gpu, m, n, k):
    """A = W H in small integers (exact in either storage): every pad row, pad column and factor row k .. KP-1 that leaked into
    a tile would show as a non-zero residual; ||A||^2 is an integer below 2^53, the same in any order of summation"""
    rng = np.random.default_rng(m * 1000 + n * 10 + k)
    top = 3 if k <= 64 else 2              # entries <= 4 k are exact in bf16 up to k = 64; above that entries in {0, 1}, fp32 storage
    W = np.asfortranarray(rng.integers(0, top, (m, k)).astype(np.float64))
    H = np.asfortranarray(rng.integers(0, top, (k, n)).astype(np.float64))
    A = W @ H
    a_sq = float((A.astype(np.int64) ** 2).sum())
    for storage in storages(k):
        for single in (False, True):
            D = gpu.DenseMatrix.from_host(A, storage=storage, single_copy=single)
            assert np.array_equal(D.download(), A)
            res = D.residual(W, H, per_column=True)
            assert res.resid_sq == 0.0, (storage, single, res.resid_sq)
            assert np.all(res.col_resid_sq == 0.0), (storage, single, res.col_resid_sq.max())
            assert res.a_sq == a_sq, (storage, single, res.a_sq, a_sq)
            assert res.relative == 0.0 or (a_sq == 0.0 and np.isnan(res.relative))       # (an all-zero A has no relative error)
            if single:
                assert D.single_copy, "the residual must not make a single-copy matrix build its transpose"
            D.close()


@pytest.mark.parametrize("m,n,k", CASES)
def test_against_numpy(gpu, m, n, k):
    A0 = values(m, n, m * 1000 + n)
    W, H = factors(m, n, k, 7 * m + n + k)
    for storage in storages(k):
        for single in (False, True):
            D = gpu.DenseMatrix.from_host(A0, storage=storage, single_copy=single)
            want = numpy_ref(D.download(), W, H)
            check_against(D.residual(W, H, per_column=True), want, (m, n, k, storage, single))
            plain = D.residual(W, H)
            assert plain.col_resid_sq is None and close(plain.resid_sq, want[0], 1e-10)
            if want[1] > 0:
                assert close(gpu.relative_error(D, W, H), np.sqrt(want[0] / want[1]), 1e-10)
            else:                              # (1, 1): the one stored value is an exact zero
                assert np.isnan(gpu.relative_error(D, W, H))
            if single:
                assert D.single_copy
            D.close()


def test_host_leading_dimensions(gpu):
    """the C entry with leading dimensions larger than the factor (what a caller with padded buffers passes)"""
    m, n, k = 63, 65, 9
    D = gpu.DenseMatrix.from_host(values(m, n, 3))
    W, H = factors(m, n, k, 4)
    Wp = np.full((m + 5, k), 7.0, order="F")
    Hp = np.full((k + 3, n), 7.0, order="F")
    Wp[:m], Hp[:k] = W, H
    r, a = C.c_double(0), C.c_double(0)
    dp = C.POINTER(C.c_double)
    L = gpu._lib
    L.check(L.lib().smk_matrix_residual(D._h, k, Wp.ctypes.data_as(dp), m + 5, Hp.ctypes.data_as(dp), k + 3, C.byref(r), C.byref(a), None),
            "smk_matrix_residual")
    want = numpy_ref(D.download(), W, H)
    assert close(r.value, want[0], 1e-10) and close(a.value, want[1], 1e-11)
    D.close()


def lay_out(torch, x, layout):
    rows, cols = x.shape
    if layout == "row_major":
        return x.cuda()
    if layout == "col_major":
        return x.cuda().t().contiguous().t()
    pitch = cols + 3 + (1 - (cols + 3) % 2)          # offset_slice: X[1:, 3:] of a tensor with an odd pitch, 7s around it
    big = torch.full((rows + 1, pitch), 7.0, dtype=x.dtype, device="cuda")
    big[1:, 3:3 + cols] = x.cuda()
    return big[1:, 3:3 + cols]


@pytest.mark.parametrize("m,n,k", [(257, 131, 9), (63, 65, 64), (1, 1, 1), (257, 131, 130)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_device_factors(gpu, m, n, k, dtype):
    """the same through smk_matrix_residual_device: fp32 factors are widened exactly, and numpy uses the widened values"""
    torch = pytest.importorskip("torch")
    td = {"f64": torch.float64, "f32": torch.float32}[dtype]
    W, H = factors(m, n, k, 11)
    tW, tH = torch.from_numpy(np.ascontiguousarray(W)).to(td), torch.from_numpy(np.ascontiguousarray(H)).to(td)
    D = gpu.DenseMatrix.from_host(values(m, n, 12), storage="bf16" if k <= 64 else "f32")
    want = numpy_ref(D.download(), tW.double().numpy(), tH.double().numpy())
    for layout in ("row_major", "col_major", "offset_slice"):
        dW, dH = lay_out(torch, tW, layout), lay_out(torch, tH, layout)
        res = D.residual(dW, dH, per_column=True)
        assert isinstance(res.col_resid_sq, torch.Tensor) and res.col_resid_sq.is_cuda and res.col_resid_sq.dtype == torch.float64
        res.col_resid_sq = res.col_resid_sq.cpu().numpy()
        check_against(res, want, (m, n, k, dtype, layout))
        assert D.residual(dW, dH).col_resid_sq is None
    D.close()


# ---- sparse -----------------------------------------------------------------------------------------------------------
SEG = 64              # entries per segment of the gather plans (the library's default)


def sparse_case(seed=5, dup=0):
    """300 x 200 in CSC with an empty column (0), an empty row (5), columns of exactly SEG, SEG + 1 and 3 SEG + 5 entries and
    row indices in no order inside a column; dup: that many stored entries repeated (the repeats add up)"""
    m, n = 300, 200
    rng = np.random.default_rng(seed)
    rows_ok = np.array([r for r in range(m) if r != 5])
    lens = rng.integers(1, 24, n)
    lens[0], lens[10], lens[11], lens[12] = 0, SEG, SEG + 1, 3 * SEG + 5
    cols = []
    for j in range(n):
        ri = rng.permutation(rows_ok)[:lens[j]]
        cols.append((ri, rng.random(lens[j]) * 2.0 + 0.1))
    if dup:
        for j in rng.permutation(np.arange(1, n))[:dup]:
            ri, va = cols[j]
            t = rng.integers(0, len(ri))
            at = rng.integers(0, len(ri) + 1)          # the repeat goes anywhere in the column
            cols[j] = (np.insert(ri, at, ri[t]), np.insert(va, at, rng.random() + 0.5))
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum([len(c[0]) for c in cols])
    indices = np.concatenate([c[0] for c in cols]).astype(np.uint32)
    data = np.concatenate([c[1] for c in cols])
    dense = np.zeros((m, n))
    np.add.at(dense, (indices.astype(np.int64), np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))), data)
    return data, indices, indptr, (m, n), dense


def sparse_terms(A, W, H):
    """the three sums per column and the bar 1e-12 (a_sq + 2 |S_ap| + ||W H||^2): each fp64 sum loses a few N u relative to
    its own size and the result is their difference"""
    P = W @ H
    a = (A * A).sum(0)
    s = (A * P).sum(0)
    q = (P * P).sum(0)
    R = A - P
    return (R * R).sum(0), a, 1e-12 * (a + 2 * np.abs(s) + q)


def check_sparse(res, A, W, H, tag, a_tol=1e-11):
    cols, a, bar = sparse_terms(A, W, H)
    got = np.asarray(res.col_resid_sq)
    print(tag, "resid_sq", res.resid_sq, cols.sum(), "bar", bar.sum(), "worst column", np.max(np.abs(got - cols) / np.maximum(bar, 1e-300)))
    assert close(res.a_sq, a.sum(), a_tol), (tag, res.a_sq, a.sum())
    assert abs(res.resid_sq - cols.sum()) <= bar.sum(), (tag, res.resid_sq, cols.sum(), bar.sum())
    assert np.all(got >= 0.0), tag
    assert np.all(np.abs(got - cols) <= bar), (tag, np.max(np.abs(got - cols) / np.maximum(bar, 1e-300)))


@pytest.fixture(scope="module")
def sparse_plain():
    return sparse_case()


@pytest.fixture(scope="module")
def sparse_dup():
    return sparse_case(dup=40)


@pytest.mark.parametrize("k", [2, 3, 9, 32, 33, 130])
def test_sparse_against_numpy(gpu, sparse_plain, k):
    data, indices, indptr, (m, n), A = sparse_plain
    S = gpu.SparseMatrix(data, indices, indptr, (m, n))
    W, H = factors(m, n, k, 20 + k)
    check_sparse(S.residual(W, H, per_column=True), A, W, H, ("sparse", k))
    S.close()


def test_sparse_device_factors(gpu, sparse_plain):
    torch = pytest.importorskip("torch")
    data, indices, indptr, (m, n), A = sparse_plain
    S = gpu.SparseMatrix(data, indices, indptr, (m, n))
    W, H = factors(m, n, 9, 31)
    tW, tH = torch.from_numpy(np.ascontiguousarray(W)).float(), torch.from_numpy(np.ascontiguousarray(H)).float()
    res = S.residual(tW.cuda(), tH.cuda().t().contiguous().t(), per_column=True)
    res.col_resid_sq = res.col_resid_sq.cpu().numpy()
    check_sparse(res, A, tW.double().numpy(), tH.double().numpy(), "sparse, fp32 tensors")
    S.close()


def test_sparse_one_entry(gpu):
    S = gpu.SparseMatrix(np.array([3.0]), np.array([0]), np.array([0, 1]), (1, 1))
    for k in (1, 3):
        W, H = factors(1, 1, k, 40 + k)
        check_sparse(S.residual(W, H, per_column=True), np.array([[3.0]]), W, H, ("1 x 1", k))
    S.close()


@pytest.mark.parametrize("k", [3, 33])
def test_sparse_duplicates_add_up(gpu, sparse_dup, k):
    """the resident CSC keeps repeated entries and every product adds them up: ||A||^2 and the residual are those of the
    matrix with the repeats summed, through the host entry and through the device entry"""
    torch = pytest.importorskip("torch")
    data, indices, indptr, (m, n), A = sparse_dup
    assert len(data) == sparse_case()[0].size + 40
    W, H = factors(m, n, k, 50 + k)
    S = gpu.SparseMatrix(data, indices, indptr, (m, n))
    T = gpu.SparseMatrix.from_device(torch.from_numpy(indptr.astype(np.int64)).cuda(), torch.from_numpy(indices.astype(np.int32)).cuda(),
                                     torch.from_numpy(data).cuda(), (m, n))
    for M, tag in ((S, "create_sparse"), (T, "from_device")):
        check_sparse(M.residual(W, H, per_column=True), A, W, H, ("duplicates", tag, k))
        check_sparse(M.residual(W, H, per_column=True), A, W, H, ("duplicates, cached record", tag, k))
        M.close()


@pytest.mark.parametrize("k", [9, 33])
def test_sparse_exact_fit(gpu, k):
    """A = W H in integers with every entry stored: the three sums cancel to rounding, and what is left is not negative"""
    m, n = 70, 90
    rng = np.random.default_rng(k)
    W = np.asfortranarray(rng.integers(0, 3, (m, k)).astype(np.float64))
    H = np.asfortranarray(rng.integers(0, 3, (k, n)).astype(np.float64))
    A = W @ H
    indptr = np.arange(n + 1, dtype=np.uint32) * m
    indices = np.tile(np.arange(m, dtype=np.uint32), n)
    S = gpu.SparseMatrix(A.flatten(order="F"), indices, indptr, (m, n))
    res = S.residual(W, H, per_column=True)
    print("exact fit", k, res.resid_sq, res.a_sq)
    assert res.a_sq == float((A * A).sum())
    assert 0.0 <= res.resid_sq <= 1e-12 * res.a_sq
    assert np.all(res.col_resid_sq >= 0.0)
    S.close()


# ---- the solver route --------------------------------------------------------------------------------------------------
def start(m, n, k, seed=43):
    return oracle.fill_uniform(m, k, seed) + 0.01, (oracle.fill_uniform(k, n, seed + 1) + 0.01) * (2.0 / k)


@pytest.fixture(scope="module")
def planted():
    return oracle.fill_planted(257, 131, 7, 9, quant=0)


def solver_on(gpu, M, alg, k, W0, H0):
    s = gpu.NmfSolver(M, gpu.make_options(M.height, M.ncols, k, alg, min_iter=100, max_iter=100, normalize=False))
    s.set_factors(W0, H0)
    return s


@pytest.mark.parametrize("alg,k", [("MU", 9), ("HALS", 9), ("BPP", 9), ("MU", 33), ("HALS", 33), ("BPP", 33), ("RANK2", 2)])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_solver_route_and_non_interference(gpu, planted, sparse_plain, alg, k, kind):
    if kind == "dense":
        A = planted
        M = gpu.DenseMatrix.from_host(A)
        A = M.download()
    else:
        data, indices, indptr, shape, A = sparse_plain
        M = gpu.SparseMatrix(data, indices, indptr, shape)
    m, n = A.shape
    W0, H0 = start(m, n, k)
    if kind == "sparse":
        H0 = H0 * A.mean() + 0.01
    s = solver_on(gpu, M, alg, k, W0, H0)
    s.iterate(3)
    assert s.sync() == 0
    got = s.residual(per_column=True)
    W, H = s.factors(normalize=False)
    via_matrix = M.residual(W, H, per_column=True)
    want = numpy_ref(A, W, H)
    print(alg, k, kind, got.resid_sq, via_matrix.resid_sq, want[0])
    assert got.a_sq == via_matrix.a_sq
    assert close(got.resid_sq, via_matrix.resid_sq, 1e-10) and close(got.resid_sq, want[0], 1e-10)
    assert np.all(np.abs(got.col_resid_sq - via_matrix.col_resid_sq) <= 1e-10 * via_matrix.col_resid_sq)
    assert np.all(np.abs(got.col_resid_sq - want[2]) <= 1e-10 * want[2])
    count = gpu._lib.lib().smk_solver_iteration_count
    assert count(s._h) == 3
    s.close()
    # a residual after every iteration changes nothing: same bits as an undisturbed run
    a, b = solver_on(gpu, M, alg, k, W0, H0), solver_on(gpu, M, alg, k, W0, H0)
    for _ in range(6):
        a.iterate(1)
        assert a.sync() == 0
        a.residual()
    b.iterate(6)
    assert b.sync() == 0
    assert count(a._h) == count(b._h) == 6
    Wa, Ha = a.factors()
    Wb, Hb = b.factors()
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb)
    a.close()
    b.close()
    M.close()


def test_solver_with_a_communicator_is_refused(gpu, planted):
    L = gpu._lib
    D = gpu.DenseMatrix.from_host(planted)
    comm = gpu.Comm.init_local(1)[0]
    s = gpu.NmfSolver(D, gpu.make_options(257, 131, 9, "HALS"))
    s.attach_comm(comm)
    s.set_factors(*start(257, 131, 9))
    with pytest.raises(L.SmallkError) as e:
        s.residual()
    assert e.value.code == L.UNSUPPORTED
    s.close()
    comm.close()
    D.close()


def test_column_shard_returns_its_local_sums(gpu, planted):
    """a plain column shard without a communicator: the caller adds the squares"""
    W, H = factors(257, 131, 9, 60)
    whole = gpu.DenseMatrix.from_host(planted)
    want = whole.residual(W, H, per_column=True)
    r = a = 0.0
    for c0, nc in ((0, 70), (70, 61)):
        D = gpu.DenseMatrix(257, 131, col0=c0, ncols=nc)
        D.upload(planted[:, c0:c0 + nc])
        part = D.residual(W, H[:, c0:c0 + nc], per_column=True)
        assert np.allclose(part.col_resid_sq, want.col_resid_sq[c0:c0 + nc], rtol=1e-12, atol=0.0)
        r, a = r + part.resid_sq, a + part.a_sq
        D.close()
    assert close(r, want.resid_sq, 1e-12) and close(a, want.a_sq, 1e-12)
    whole.close()


@pytest.mark.parametrize("alg", ["BPP", "HALS", "MU"])
def test_descent(gpu, planted, alg):
    """Exact block coordinate descent never increases ||A - W H||^2.  The oracle's own sequences on these inputs ((257, 131)
    planted data, k = 9, 10 iterations) were computed on the CPU first: BPP, HALS and MU are all non-increasing within 1e-9
    relative here (MU's epsilon in the denominators and HALS' reset of zero columns did not step up on this data), so all three
    are kept.  The device sequence may step up by 1e-7 relative: the product forms the solver itself uses are good to 1e-8."""
    D = gpu.DenseMatrix.from_host(planted)
    s = solver_on(gpu, D, alg, 9, *start(257, 131, 9))
    seq = []
    for _ in range(10):
        s.iterate(1)
        assert s.sync() == 0
        seq.append(s.residual().resid_sq)
    print(alg, seq)
    for before, after in zip(seq, seq[1:]):
        assert after <= before * (1 + 1e-7), (alg, seq)
    assert seq[-1] < seq[0]
    s.close()
    D.close()


def test_same_bits_on_every_run(gpu, sparse_plain):
    A0 = values(257, 131, 70)
    for k in (9, 130):
        W, H = factors(257, 131, k, 71)
        D = gpu.DenseMatrix.from_host(A0, storage="f32")
        one, two = D.residual(W, H, per_column=True), D.residual(W, H, per_column=True)
        assert one.resid_sq == two.resid_sq and one.a_sq == two.a_sq and np.array_equal(one.col_resid_sq, two.col_resid_sq)
        D.close()
    data, indices, indptr, (m, n), _ = sparse_plain
    S = gpu.SparseMatrix(data, indices, indptr, (m, n))
    for k in (9, 130):
        W, H = factors(m, n, k, 72)
        one, two = S.residual(W, H, per_column=True), S.residual(W, H, per_column=True)
        assert one.resid_sq == two.resid_sq and one.a_sq == two.a_sq and np.array_equal(one.col_resid_sq, two.col_resid_sq)
    S.close()


def test_bad_arguments(gpu):
    """SMK_BAD_PARAM with an error text, from the C entries themselves (the Python layer refuses most of these earlier)"""
    torch = pytest.importorskip("torch")
    L = gpu._lib
    lib = L.lib()
    m, n, k = 65, 63, 9
    D = gpu.DenseMatrix.from_host(values(m, n, 80))
    W, H = factors(m, n, k, 81)
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    r, a = C.c_double(0), C.c_double(0)
    host = lambda kk, W_, ldW, H_, ldH, r_=C.byref(r), a_=C.byref(a): lib.smk_matrix_residual(
        D._h, kk, W_.ctypes.data_as(dp), ldW, H_.ctypes.data_as(dp), ldH, r_, a_, None)
    assert host(k, W, m, H, k) == L.OK
    # (each attempt is made inside the loop: smk_last_error() speaks of the last call)
    for attempt, word in ((lambda: host(0, W, m, H, k), "k < 1"),
                          (lambda: host(k, np.asfortranarray(W[:-1]), m - 1, H, k), "leading dimension"),     # W with m - 1 rows
                          (lambda: host(k, W, m, np.asfortranarray(H[:-1]), k - 1), "leading dimension"),
                          (lambda: host(k, W, m, H, k, None), "null output"),
                          (lambda: host(k, W, m, H, k, C.byref(r), None), "null output")):
        rc = attempt()
        assert rc == L.BAD_PARAM, (word, rc)
        assert word in lib.smk_last_error().decode(), (word, lib.smk_last_error())
    assert host(4096, W, m, H, 4096) == L.UNSUPPORTED and lib.smk_last_error()
    dW, dH = torch.from_numpy(np.ascontiguousarray(W)).cuda(), torch.from_numpy(np.ascontiguousarray(H)).cuda()
    dev = lambda kk, wp, hp, wdt=L.DT_F64: lib.smk_matrix_residual_device(D._h, kk, wp, wdt, k, 1, hp, L.DT_F64, n, 1, None, C.byref(r), C.byref(a), None)
    assert dev(k, vp(dW.data_ptr()), vp(dH.data_ptr())) == L.OK
    Wh = np.ascontiguousarray(W)
    for attempt, word in ((lambda: dev(0, vp(dW.data_ptr()), vp(dH.data_ptr())), "k < 1"),
                          (lambda: dev(k, vp(Wh.ctypes.data), vp(dH.data_ptr())), "device"),     # a host pointer
                          (lambda: dev(k, vp(dW.data_ptr()), vp(dH.data_ptr()), L.DT_BF16), "fp64 or fp32"),
                          (lambda: dev(k, None, vp(dH.data_ptr())), "null")):
        rc = attempt()
        assert rc == L.BAD_PARAM, (word, rc)
        assert word in lib.smk_last_error().decode(), (word, lib.smk_last_error())
    # the Python layer: shapes that do not fit the matrix never reach the library
    for bad_w, bad_h in ((W[:-1], H), (W, H[:, :-1]), (dW[:-1], dH), (dW, dH[:, :-1])):
        with pytest.raises(ValueError):
            D.residual(bad_w, bad_h)
    D.close()


def test_device_factor_one_column_short_leaves_its_allocation(gpu):
    """H with one column too few, through the C entry: the k x n view runs past the end of the allocation.  The buffer is 20 MiB
    allocated right after the caching allocator was emptied, so that it is an allocation of its own and ends where the tensor ends."""
    torch = pytest.importorskip("torch")
    L = gpu._lib
    k, n = 64, 40961                      # 64 x 40960 doubles = 20 MiB
    D = gpu.DenseMatrix(1, n)
    D.fill_uniform(1)
    torch.cuda.empty_cache()
    H = torch.zeros((n - 1, k), dtype=torch.float64, device="cuda")          # column-major k x (n - 1)
    W = torch.zeros((1, k), dtype=torch.float64, device="cuda")
    r, a = C.c_double(0), C.c_double(0)
    vp = C.c_void_p
    rc = L.lib().smk_matrix_residual_device(D._h, k, vp(W.data_ptr()), L.DT_F64, k, 1, vp(H.data_ptr()), L.DT_F64, 1, k, None,
                                            C.byref(r), C.byref(a), None)
    assert rc == L.BAD_PARAM, rc
    assert "allocation" in L.lib().smk_last_error().decode(), L.lib().smk_last_error()
    D.close()

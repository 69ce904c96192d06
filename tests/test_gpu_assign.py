"""GPU tests of the labelling entries (smk_labels_device, smk_top_terms_device, smk_solver_labels, smk_solver_top_terms).

The expected values are the library's own host functions on the same fp64 values (fp32 tensors are widened exactly and the host
functions get the widened values): ``flatclust.compute_assignments``, ``compute_fuzzy_assignments`` and ``top_terms``.  Where
the host function refuses a shape the device entry takes (labels with k > n) it is given the same matrix with columns of zeros
appended, which changes no column it is asked about; every top-terms case has m >= k, the host function's rule.  Everything is
compared exactly: labels and term indices as integers, memberships bit for bit wherever the host's value is not NaN (and NaN
where it is).

Shapes: one element; k below, at and above the 16-row strip of the labels kernel; n past the 256 columns of a workgroup; k > n;
for top terms one row, fewer rows than maxterms, two row chunks (300), many chunks with a ragged last tile (4099, 70001), three
topic groups (k = 33) and nine (k = 130), the cap of the in-LDS selection (256: several merge levels) and one above it."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

LABEL_SHAPES = [(1, 1), (2, 5), (9, 257), (16, 64), (33, 131), (130, 70), (64, 3)]
# (m, k, maxterms); 257 = the cap of the in-LDS selection + 1: the radix sort route
TERM_SHAPES = [(1, 1, 1), (3, 3, 5), (300, 9, 5), (4099, 33, 64), (70001, 3, 256), (70001, 3, 257), (2050, 130, 5)]


def host_labels(H):
    from smallk_amd import flatclust
    k, n = H.shape
    Hp = np.hstack([H, np.zeros((k, k - n))]) if k > n else H
    return flatclust.compute_assignments(Hp)[:n].astype(np.int64), flatclust.compute_fuzzy_assignments(H)


def host_terms(W, maxterms):
    from smallk_amd import flatclust
    m, k = W.shape
    assert m >= k                            # (the host function's rule; every case here obeys it)
    out = flatclust.top_terms(W, maxterms).reshape(k, maxterms).astype(np.int64)
    out[:, min(maxterms, m):] = -1
    return out


def h_input(kind, k, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.random((k, n))
    if kind == "ties":                       # four levels: most columns hold their maximum more than once
        return np.floor(rng.random((k, n)) * 4.0) / 4.0
    H = rng.random((k, n))                   # "zero_column"
    H[:, n // 2] = 0.0
    return H


def lay_out(torch, x, layout):
    """x: a CPU tensor; the same values on the GPU in the layout asked for"""
    rows, cols = x.shape
    if layout == "row_major":
        return x.cuda().contiguous()
    if layout == "col_major":
        return x.cuda().t().contiguous().t()
    big = torch.full((2 * rows + 1, 2 * cols + 3), 7.0, dtype=x.dtype, device="cuda")       # "slice": no unit stride at all
    big[1::2, 3::2] = x.cuda()
    return big[1::2, 3::2]


def check_labels(got, P, H, tag):
    want, wantP = host_labels(H)
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == want.shape and np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:5])
    if P is not None:
        assert tuple(P.shape) == H.shape and P.t().is_contiguous(), tag             # (k, n) with document-major memory
        P = P.cpu().numpy()
        nan = np.isnan(wantP)
        assert np.array_equal(np.isnan(P), nan), tag
        assert np.array_equal(P[~nan].view(np.uint32), np.asarray(wantP)[~nan].view(np.uint32)), tag


@pytest.mark.parametrize("k,n", LABEL_SHAPES)
@pytest.mark.parametrize("kind", ["random", "ties", "zero_column"])
def test_labels_and_memberships(gpu, k, n, kind):
    torch = pytest.importorskip("torch")
    H64 = h_input(kind, k, n, 1000 * k + n)
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(H64).to(dtype)
        H = t.double().numpy()
        for layout in ("col_major", "row_major", "slice"):
            d = lay_out(torch, t, layout)
            labels, P = gpu.labels_device(d, memberships=True)
            assert labels.dtype == torch.int32 and labels.is_cuda and P.dtype == torch.float32
            check_labels(labels, P, H, (k, n, kind, dtype, layout))
            only = gpu.labels_device(d)
            assert torch.equal(only, labels)
            again, Pagain = gpu.labels_device(d, memberships=True)
            assert torch.equal(again, labels) and np.array_equal(Pagain.cpu().numpy().view(np.uint32), P.cpu().numpy().view(np.uint32))
    if kind == "zero_column":
        assert int(labels[n // 2]) == 0 and bool(torch.isnan(P[:, n // 2]).all())


def w_input(kind, m, k, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((m, k))
    if kind == "constant":                   # every entry equal: the order is the index order, across every chunk of rows
        W[:, 0] = 0.5
        W[:, k - 1] = 0.0
    elif kind == "ties":
        W = np.floor(W * 4.0) / 4.0
    elif kind == "zeros":                    # +0.0 and -0.0 compare equal: the index decides
        W[:, 0] = np.where(rng.random(m) < 0.5, 0.0, -0.0)
        W[:, k - 1] = np.where(rng.random(m) < 0.7, W[:, k - 1], -0.0)
    elif kind == "ascending":                # the largest entries are the last rows: every row enters the selection
        W[:, 0] = np.arange(m) / m
        W[:, k - 1] = np.sort(W[:, k - 1])
    return W


@pytest.fixture(scope="module")
def term_cases():
    """inputs and the host's answers, computed once"""
    cache = {}

    def get(m, k, maxterms, kind):
        key = (m, k, maxterms, kind)
        if key not in cache:
            W = w_input(kind, m, k, 7 * m + k + maxterms)
            cache[key] = (W, host_terms(W, maxterms))
        return cache[key]
    return get


@pytest.mark.parametrize("m,k,maxterms", TERM_SHAPES)
@pytest.mark.parametrize("kind", ["random", "constant", "ties", "zeros", "ascending"])
def test_top_terms(gpu, term_cases, m, k, maxterms, kind):
    torch = pytest.importorskip("torch")
    W, want = term_cases(m, k, maxterms, kind)
    t = torch.from_numpy(W)
    layouts = ("row_major", "col_major") if m > 4099 else ("row_major", "col_major", "slice")
    for layout in layouts:
        d = lay_out(torch, t, layout)
        got = gpu.top_terms_device(d, maxterms)
        assert got.dtype == torch.int32 and tuple(got.shape) == (k, maxterms)
        g = got.cpu().numpy().astype(np.int64)
        assert np.array_equal(g, want), (m, k, maxterms, kind, layout, np.argwhere(g != want)[:5])
        assert torch.equal(gpu.top_terms_device(d, maxterms), got)


@pytest.mark.parametrize("m,k,maxterms", [(300, 9, 5), (4099, 33, 64), (70001, 3, 257)])
def test_top_terms_fp32(gpu, m, k, maxterms):
    """fp32 factors are widened exactly; rounding to fp32 makes ties, which the host breaks by index on the widened values"""
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(w_input("random", m, k, 5 * m + k)).float()
    want = host_terms(t.double().numpy(), maxterms)
    for layout in ("row_major", "col_major"):
        got = gpu.top_terms_device(lay_out(torch, t, layout), maxterms).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), (m, k, maxterms, layout)


# ---- the solver route --------------------------------------------------------------------------------------------------
def start(m, n, k, seed=43):
    return oracle.fill_uniform(m, k, seed) + 0.01, (oracle.fill_uniform(k, n, seed + 1) + 0.01) * (2.0 / k)


@pytest.fixture(scope="module")
def planted():
    return oracle.fill_planted(257, 131, 7, 9, quant=0)


def solver_on(gpu, M, k, W0, H0):
    s = gpu.NmfSolver(M, gpu.make_options(M.height, M.ncols, k, "BPP", min_iter=100, max_iter=100, normalize=False))
    s.set_factors(W0, H0)
    return s


@pytest.mark.parametrize("k", [9, 33])
def test_solver_route_and_non_interference(gpu, planted, k):
    """k = 9 has KP = 16 and k = 33 has KP = 64: a pad row of the resident H or Wt that became a candidate would show as a label
    or a term index the host does not give"""
    torch = pytest.importorskip("torch")
    m, n = planted.shape
    M = gpu.DenseMatrix.from_host(planted)
    W0, H0 = start(m, n, k)
    # labelling after every iteration changes nothing: the same bits as an undisturbed run
    a, b = solver_on(gpu, M, k, W0, H0), solver_on(gpu, M, k, W0, H0)
    for _ in range(3):
        a.iterate(1)
        assert a.sync() == 0
        a.labels_device(normalize=False, memberships=True)
        a.top_terms_device(5, normalize=False)
    b.iterate(3)
    assert b.sync() == 0
    assert a.iteration_count == b.iteration_count == 3
    Wa, Ha = a.factors()
    Wb, Hb = b.factors()
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb)
    a.iterate(1)
    b.iterate(1)
    assert a.sync() == 0 and b.sync() == 0
    assert all(np.array_equal(x, y) for x, y in zip(a.factors(), b.factors()))
    # the values: the host functions on the factors as factors() returns them
    for normalize in (False, True):
        labels, P = a.labels_device(normalize=normalize, memberships=True)
        W, H = a.factors(normalize=normalize)          # (after the labels: with normalize, the solver entry is what normalises)
        check_labels(labels, P, H, ("solver", k, normalize))
        for maxterms in (5, 64, 257):
            got = a.top_terms_device(maxterms, normalize=normalize)
            assert tuple(got.shape) == (k, maxterms)
            assert np.array_equal(got.cpu().numpy().astype(np.int64), host_terms(W, maxterms)), (k, normalize, maxterms)
    # normalising for the labels is what factors(normalize=True) does: the next iteration is the same as after that call
    b.factors(normalize=True)
    a.iterate(1)
    b.iterate(1)
    assert a.sync() == 0 and b.sync() == 0
    assert all(np.array_equal(x, y) for x, y in zip(a.factors(), b.factors()))
    a.close()
    b.close()
    M.close()


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    """SMK_BAD_PARAM with an error text from the C entries themselves, and nothing written"""
    torch = pytest.importorskip("torch")
    L = gpu._lib
    lib = L.lib()
    vp = C.c_void_p
    k, n, m, mt = 9, 65, 70, 5
    H = torch.rand((n, k), dtype=torch.float64, device="cuda")           # column-major k x n
    W = torch.rand((m, k), dtype=torch.float64, device="cuda")
    labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    P = torch.full((n, k), -7.0, dtype=torch.float32, device="cuda")
    terms = torch.full((k, mt), -7, dtype=torch.int32, device="cuda")
    Hh, lh = np.zeros((n, k)), np.zeros(n, dtype=np.int32)
    lab = lambda hp=vp(H.data_ptr()), dt=L.DT_F64, kk=k, nn=n, out=vp(labels.data_ptr()): lib.smk_labels_device(
        hp, dt, 1, k, kk, nn, None, out, vp(P.data_ptr()))
    top = lambda wp=vp(W.data_ptr()), dt=L.DT_F64, kk=k, mm=m, t=mt, out=vp(terms.data_ptr()): lib.smk_top_terms_device(
        wp, dt, k, 1, mm, kk, t, None, out)
    for attempt, word in ((lambda: lab(hp=vp(Hh.ctypes.data)), "device"),            # a CPU pointer as the factor
                          (lambda: lab(out=vp(lh.ctypes.data)), "device"),           # ... as the output
                          (lambda: lab(hp=None), "null"),
                          (lambda: lab(kk=0), "k < 1"),
                          (lambda: lab(nn=0), "n < 1"),
                          (lambda: lab(dt=L.DT_BF16), "fp64 or fp32"),
                          (lambda: top(wp=vp(Hh.ctypes.data)), "device"),
                          (lambda: top(kk=0), "k < 1"),
                          (lambda: top(mm=0), "m < 1"),
                          (lambda: top(t=0), "maxterms < 1"),
                          (lambda: top(dt=L.DT_BF16), "fp64 or fp32")):
        rc = attempt()
        assert rc == L.BAD_PARAM, (word, rc)
        assert word in lib.smk_last_error().decode(), (word, lib.smk_last_error())
    assert bool((labels == -7).all()) and bool((P == -7.0).all()) and bool((terms == -7).all())
    assert lab() == L.OK and top() == L.OK
    assert not bool((labels == -7).any()) and not bool((terms == -7).any())


def test_view_that_leaves_its_allocation(gpu):
    """H with one column too few through the C entry.  The buffer is 20 MiB allocated right after the caching allocator was
    emptied, so that it is an allocation of its own and ends where the tensor ends (as in test_gpu_residual.py)."""
    torch = pytest.importorskip("torch")
    L = gpu._lib
    k, n = 64, 40961
    torch.cuda.empty_cache()
    H = torch.zeros((n - 1, k), dtype=torch.float64, device="cuda")
    labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    vp = C.c_void_p
    rc = L.lib().smk_labels_device(vp(H.data_ptr()), L.DT_F64, 1, k, k, n, None, vp(labels.data_ptr()), None)
    assert rc == L.BAD_PARAM, rc
    assert "allocation" in L.lib().smk_last_error().decode(), L.lib().smk_last_error()
    rc = L.lib().smk_top_terms_device(vp(H.data_ptr()), L.DT_F64, k, 1, n, k, 5, None, vp(labels.data_ptr()))
    assert rc == L.BAD_PARAM, rc
    assert "allocation" in L.lib().smk_last_error().decode(), L.lib().smk_last_error()
    assert bool((labels == -7).all())

"""The tree router on the device (smk_tree_router_*, smk_tree_route_device, TreeRouter) against the numpy
restatement of the descent (tree_route_reference.py) on the hand-built cases of tree_route_cases.py and on fitted trees.

The result is discrete, and test_tree_route_cpu.py shows every decision of every case clear of rounding by a margin >= 1e-6, so
leaves and depths must be EQUAL.  h differs from the restatement by summation order only (sixteen lanes and a butterfly against
storage order): it must agree within 16 x the fp64-versus-long-double difference of the restatement, relative to max(h0, h1).
That difference was measured on the CPU as 2.212e-15 (kept as 2.22e-15 in test_tree_route_cpu.py, which asserts it), so the bar is
3.55e-14; its floor, 64 * 2^-53 = 7.1e-15, lies below.  A fitted tree has a rounding scale of its own (nearly parallel siblings:
3.0e-14 between the two restatements on the second planted case), measured in the same way inside test_fitted_tree and used
there with the same factor and floor.  Nothing here is taken from the device's own output.  Measured on the device: h of the
hand-built cases differs from the restatement by at most 1.3e-15 of max(h0, h1) (chain9, m = 200), on the fitted trees by 6.1e-16
(bar 1.4e-14) and 3.9e-14 (bar 4.8e-13)."""
import ctypes as C

import numpy as np
import pytest

import tree_route_cases as cases
import tree_route_reference as ref
from hier_cases import planted
from test_tree_route_cpu import FLOOR, MARGIN, ORACLE_CASES, h_bar, rel_h_difference

pytestmark = pytest.mark.gpu
NONE = ref.NONE
SENTINEL = -77


def router_of(gpu, c):
    return gpu.TreeRouter(c["left"], c["right"], c["topics"], c["valid"])


def check_against(got, want, n, what, bar=None):
    """got: (leaf, depth, h) tensors of a call over the first n documents; want: the restatement's over all of them; bar: for h,
    relative to max(h0, h1) (the hand-built cases' unless given)"""
    bar = h_bar() if bar is None else bar
    leaf, depth, h = (x.cpu().numpy() for x in got)
    assert leaf.dtype == np.int32 and depth.dtype == np.int32 and h.dtype == np.float64 and h.shape == (n, 2)
    assert np.array_equal(leaf, want[0][:n]), what
    assert np.array_equal(depth, want[1][:n]), what
    wh = want[2][:n]
    err = np.max(np.abs(h - wh), axis=1)
    top = np.max(wh, axis=1)
    worst = float(np.max(err / np.maximum(top, np.finfo(np.float64).tiny)))
    print(f"{what}: h differs by at most {worst:.3e} of max(h0, h1); bar {bar:.3e}")
    assert np.all(err <= bar * top), (what, worst)


@pytest.mark.parametrize("name,m", cases.all_cases())
def test_exact_on_every_case(gpu, name, m):
    """every width of every case: equal leaves and depths, h within the rounding bar; labels alone give the same leaves"""
    c = cases.case(name, m)
    want = cases.expected(name, m)
    r = router_of(gpu, c)
    assert (r.pairs, r.max_depth) == ref.structure(c["left"], c["right"]) and r.table_bytes == r.pairs * m * 16
    for n in cases.WIDTHS:
        A = gpu.SparseMatrix.from_scipy(cases.scipy_columns(c, n))
        got = r.route(A, details=True)
        check_against(got, want, n, f"{name} m={m} n={n}")
        assert np.array_equal(r.route(A).cpu().numpy(), want[0][:n])
        A.close()
    r.close()


@pytest.mark.parametrize("name", cases.TREES)
def test_empty_document_goes_right(gpu, name):
    c = cases.case(name, 37)
    empty = int(np.nonzero(np.diff(c["colptr"]) == 0)[0][0])
    r = router_of(gpu, c)
    leaf, depth, h = (x.cpu().numpy() for x in r.route(cases.scipy_columns(c, 17), details=True))
    want_leaf, want_depth = cases.rightmost(c["left"], c["right"])
    assert (leaf[empty], depth[empty]) == (want_leaf, want_depth) and tuple(h[empty]) == (0.0, 0.0)
    assert want_depth == {"root_pair": 1, "balanced3": 3, "chain9": 1, "slots22": 2}[name]


def tree_arrays_of(tree):
    nodes = tree.nodes
    left = np.array([nd.left for nd in nodes], dtype=np.uint32)
    right = np.array([nd.right for nd in nodes], dtype=np.uint32)
    valid = np.array([nd.is_valid for nd in nodes], dtype=np.int32)
    return left, right, np.stack([nd.topic_vector for nd in nodes], axis=1), valid


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_fitted_tree(gpu, case, tmp_path):
    """a tree trained on the first n of n + 64 planted columns: the training columns land where the search put them, the fresh
    ones where the restatement puts them, and the router is the same however it was made"""
    m, n, topics, seed, tiny, clusters = case
    A, _ = planted(m, n + 64, topics, seed, sparse=True, tiny=tiny)
    A = A.tocsc()
    A.sort_indices()
    A_train, A_new = A[:, :n], A[:, n:]
    tree = gpu.hier_nmf2(A_train, clusters, seed=seed)
    want = tree.get_assignments()
    inside = want != NONE
    got = tree.assign(A_train)
    assert got.dtype == np.uint32 and np.array_equal(got[inside], want[inside]) and not (got == NONE).any()
    assert sorted(np.nonzero(~inside)[0].tolist()) == sorted(tree.get_outliers().tolist())
    left, right, T, valid = tree_arrays_of(tree)
    assert all(left[q] == NONE and valid[q] for q in got)
    # fresh columns against the restatement on the tree's own topic vectors
    leaf, depth, h, margins = ref.route(A_new.indptr, A_new.indices, A_new.data, left, right, T)
    worst = min(min(mj) for mj in margins)
    print(f"{case}: {int(inside.sum())} of {n} training documents are not outliers; smallest margin of the fresh columns {worst:.3e}")
    assert worst >= MARGIN
    # h: the bar is this tree's own rounding scale, measured as the hand-built cases' was (fp64 against long double of the
    # restatement, times 16, the same floor).  Siblings low in a fitted tree are nearly parallel (cosine 0.987 in the second
    # case), and their 2 x 2 solve amplifies rounding: 3.0e-14 between the two restatements there, 9.0e-16 in the first case.
    leaf_l, depth_l, h_l, _ = ref.route(A_new.indptr, A_new.indices, A_new.data, left, right, T, np.longdouble)
    assert np.array_equal(leaf, leaf_l) and np.array_equal(depth, depth_l)
    bar = max(16 * rel_h_difference(h, h_l), FLOOR)
    r1 = tree.router()
    D = gpu.SparseMatrix.from_scipy(A_new)
    out1 = r1.route(D, details=True)
    check_against(out1, (leaf, depth, h), 64, f"fresh columns of {case}", bar)
    # the same router from the arrays read through node(), and from a file
    r2 = gpu.TreeRouter(left, right, T, valid)
    assert (r1.pairs, r1.max_depth, r1.table_bytes) == (r2.pairs, r2.max_depth, r2.table_bytes)
    assert same_bits(out1, r2.route(D, details=True))
    path = tmp_path / "router.npz"
    r1.save(path)
    r3 = gpu.TreeRouter.load(path)
    for key in ("left", "right", "valid", "topics"):
        assert getattr(r1, key).tobytes(order="F") == getattr(r3, key).tobytes(order="F") == getattr(r2, key).tobytes(order="F"), key
    assert same_bits(out1, r3.route(D, details=True))
    D.close()


def test_two_runs_give_the_same_bits(gpu):
    c = cases.case("chain9", 200)
    r = router_of(gpu, c)
    A = gpu.SparseMatrix.from_scipy(cases.scipy_columns(c, 257))
    first = r.route(A, details=True)
    assert same_bits(first, r.route(A, details=True))
    assert same_bits(first, router_of(gpu, c).route(A, details=True))          # and from tables packed again


def test_caller_stream_is_honoured(gpu):
    """functional coverage of the stream contract (it cannot prove the ordering): the matrix is made and routed on a side stream
    without a synchronise, and the results are consumed there"""
    import torch
    c = cases.case("balanced3", 200)
    n = 257
    S = cases.scipy_columns(c, n)
    r = router_of(gpu, c)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        co = torch.from_numpy(S.indptr.astype(np.int64)).cuda(non_blocking=True)
        ri = torch.from_numpy(S.indices.astype(np.int32)).cuda(non_blocking=True)
        va = torch.from_numpy(S.data.astype(np.float64)).cuda(non_blocking=True) * 2.0 * 0.5
        A = gpu.SparseMatrix.from_device(co, ri, va, (200, n))
        got = r.route(A, details=True)
        counts = torch.bincount(got[0].long(), minlength=14)
    side.synchronize()
    check_against(got, cases.expected("balanced3", 200), n, "on a side stream")
    assert counts.cpu().tolist() == np.bincount(cases.expected("balanced3", 200)[0][:n], minlength=14).tolist()


def raw_route(gpu, router, A, n):
    """smk_tree_route_device into outputs filled with a sentinel: (rc, message, leaf, depth, h)"""
    import torch
    from smallk_amd import _lib as L
    leaf = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    depth = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    h = torch.full((n, 2), float(SENTINEL), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = L.lib().smk_tree_route_device(router._h if router is not None else None, A._h if A is not None else None, None,
                                       C.c_void_p(leaf.data_ptr()), C.c_void_p(depth.data_ptr()), C.c_void_p(h.data_ptr()))
    text = (L.lib().smk_last_error() or b"").decode()
    torch.cuda.synchronize()
    return rc, text, leaf.cpu().numpy(), depth.cpu().numpy(), h.cpu().numpy()


def untouched(out):
    return (out[2] == SENTINEL).all() and (out[3] == SENTINEL).all() and (out[4] == float(SENTINEL)).all()


def test_refusals_leave_the_outputs_alone(gpu):
    from smallk_amd import _lib as L
    c = cases.case("balanced3", 37)
    r = router_of(gpu, c)
    n = 17
    good = gpu.SparseMatrix.from_scipy(cases.scipy_columns(c, n))
    # (the same call succeeds on the right input, and then does write)
    out = raw_route(gpu, r, good, n)
    assert out[0] == L.OK and np.array_equal(out[2], cases.expected("balanced3", 37)[0][:n]) and not (out[3] == SENTINEL).any()
    dense = gpu.DenseMatrix.from_host(np.asfortranarray(np.random.default_rng(0).random((37, n))))
    out = raw_route(gpu, r, dense, n)
    assert out[0] == L.UNSUPPORTED and "sparse input only" in out[1] and untouched(out)
    with pytest.raises(L.SmallkError) as e:
        r.route(dense)
    assert e.value.code == L.UNSUPPORTED
    tall = gpu.SparseMatrix.from_scipy(cases.scipy_columns(cases.case("balanced3", 200), n))
    out = raw_route(gpu, r, tall, n)
    assert out[0] == L.BAD_PARAM and untouched(out)
    out = raw_route(gpu, None, good, n)
    assert out[0] == L.BAD_PARAM and untouched(out)
    out = raw_route(gpu, r, None, n)
    assert out[0] == L.BAD_PARAM and untouched(out)
    # a cyclic structure and a zero topic vector are refused when the router is made: there is nothing to route with
    left, right = c["left"].copy(), c["right"].copy()
    left[6], right[6] = 0, 1
    with pytest.raises(L.SmallkError) as e:
        gpu.TreeRouter(left, right, c["topics"], c["valid"])
    assert e.value.code == L.BAD_PARAM and "(node 0)" in str(e.value)
    h = C.c_void_p()
    T = np.asfortranarray(c["topics"])
    args = (C.c_int64(37), 14, left.ctypes.data_as(C.POINTER(C.c_uint)), right.ctypes.data_as(C.POINTER(C.c_uint)),
            c["valid"].ctypes.data_as(C.POINTER(C.c_int)), T.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(37), C.byref(h))
    assert L.lib().smk_tree_router_create(*args) == L.BAD_PARAM and not h.value
    for node in (9, 0):                      # a right and a left sibling
        T = c["topics"].copy(order="F")
        T[:, node] = 0.0
        with pytest.raises(L.SmallkError) as e:
            gpu.TreeRouter(c["left"], c["right"], T, c["valid"])
        assert e.value.code == L.FAILURE and "pair" in str(e.value) and f"nodes {node - node % 2} and {node - node % 2 + 1}" in str(e.value)
    for x in (good, dense, tall):
        x.close()


def test_profile_reports_one_launch_over_the_entries(gpu):
    from smallk_amd import _lib as L
    c = cases.case("slots22", 200)
    r = router_of(gpu, c)
    for n in (65, 257):
        S = cases.scipy_columns(c, n)
        r.route(S, details=True)
        launches, entries = C.c_int(-1), C.c_int64(-1)
        assert L.lib().smk_tree_route_last_profile(C.byref(launches), C.byref(entries)) == L.OK
        assert (launches.value, entries.value) == (1, S.nnz)
    ms = C.c_double(-1.0)
    A = gpu.SparseMatrix.from_scipy(cases.scipy_columns(c, 257))
    L.check(L.lib().smk_tree_route_time(r._handle(), A._h, 5, C.byref(ms)), "smk_tree_route_time")
    assert ms.value > 0.0

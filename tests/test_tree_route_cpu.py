"""The tree router without a GPU: the conditions the fixtures of tree_route_cases.py must meet for the GPU test to
be exact, the numpy restatement of the descent (tree_route_reference.py) on the fp64 oracle's trees, fp64 against long double,
the structure check through the C ABI and -- compiled by itself under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/tree_route/check_sim.cpp) -- as a stand-alone program, and the file round trip of a saved router.

ROUNDING_SCALE below is the largest relative difference |h_fp64 - h_longdouble| / max(h0, h1) over every document of every case
(measured by test_fp64_against_long_double, which asserts it): the GPU test's bar for h is 16 x that, floored at 64 * 2^-53."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tree_route_cases as cases
import tree_route_reference as ref
from hier_cases import planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
MARGIN = 1e-6
NONE = ref.NONE
# measured: 2.212e-15 (chain9, m = 200), written here rounded up; test_fp64_against_long_double asserts that the measurement
# stays at or below it.  The bar that follows: 16 x 2.22e-15 = 3.55e-14 (the floor, 64 * 2^-53 = 7.1e-15, lies below it).
ROUNDING_SCALE = 2.22e-15
FLOOR = 64 * 2.0 ** -53


def h_bar():
    """the GPU test's bar for h relative to max(h0, h1): 16 x the fp64-versus-long-double difference, at least 64 * 2^-53"""
    return max(16 * ROUNDING_SCALE, FLOOR)


def rel_h_difference(h, hl):
    top = np.maximum(np.max(hl, axis=1), np.finfo(np.float64).tiny).astype(np.longdouble)
    return float(np.max(np.max(np.abs(h.astype(np.longdouble) - hl), axis=1) / top))


@pytest.mark.parametrize("name,m", cases.all_cases())
def test_fixture_conditions(name, m):
    """every decision of every document is clear of rounding, the descents cover the tree, the edge shapes are present"""
    c = cases.case(name, m)
    leaf, depth, h, margins = cases.expected(name, m)
    assert len(margins) == max(cases.WIDTHS) and all(len(mj) == d for mj, d in zip(margins, depth))
    worst = min(min(mj) for mj in margins)
    print(f"{name} m={m}: smallest margin {worst:.3e}, leaves reached {sorted(set(leaf.tolist()))}")
    assert worst >= MARGIN
    counts = np.diff(c["colptr"])
    assert set([0, 1, 15, 16, 17, 31, 32, 33, m]) <= set(counts[:15].tolist())     # within the smallest call that has several documents
    assert counts[0] > 0 and (c["rowidx"] == m - 1).any()
    assert all(c["left"][q] == NONE for q in leaf) and set(leaf.tolist()) <= set(c["leaves"])
    if name == "balanced3":
        assert set(leaf.tolist()) == set(c["leaves"]) and len(c["leaves"]) == 8 and set(depth.tolist()) == {3}
    if name == "chain9":
        assert 9 in depth.tolist() and 16 in leaf.tolist()                        # the deepest leaf (left at every level)
    if name == "slots22":
        assert len(c["left"]) == 22 and int(c["valid"].sum()) == 10
    # the document without entries: right at every level, h = (0, 0)
    empty = int(np.nonzero(counts == 0)[0][0])
    assert (leaf[empty], depth[empty]) == cases.rightmost(c["left"], c["right"]) and tuple(h[empty]) == (0.0, 0.0)
    # documents do not all follow their target: the noise decides some, and that is fine -- but most do
    assert np.mean(leaf == c["target"]) > 0.5


def test_fp64_against_long_double():
    """identical leaves and depths on all cases; the largest relative difference of h is the rounding scale of the GPU test"""
    scale = 0.0
    for name, m in cases.all_cases():
        leaf, depth, h, _ = cases.expected(name, m)
        leaf_l, depth_l, h_l, _ = cases.expected(name, m, True)
        assert np.array_equal(leaf, leaf_l) and np.array_equal(depth, depth_l), (name, m)
        scale = max(scale, rel_h_difference(h, h_l))
    print(f"largest |h_fp64 - h_longdouble| / max(h0, h1): {scale:.3e}; bar of the GPU test {h_bar():.3e}")
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:          # (where long double is wider than double)
        assert 0.0 < scale <= ROUNDING_SCALE


ORACLE_CASES = [(300, 400, 6, 2, 0, 6), (150, 260, 3, 4, 5, 5)]          # the two sparse cases of test_gpu_hierclust.py


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_restatement_on_the_oracle_trees(case):
    """the training columns down the fp64 oracle's own tree land where the search put them -- every one that is not an outlier"""
    from oracle import hierclust as oh
    m, n, topics, seed, tiny, clusters = case
    A, _ = planted(m, n, topics, seed, sparse=True, tiny=tiny)
    tree, _ = oh.hier_nmf2(A, clusters, seed=seed)
    left = np.array([nd.left for nd in tree.nodes], dtype=np.uint32)
    right = np.array([nd.right for nd in tree.nodes], dtype=np.uint32)
    T = np.stack([nd.topic_vector for nd in tree.nodes], axis=1)
    A = A.tocsc()
    A.sort_indices()
    leaf, depth, h, margins = ref.route(A.indptr, A.indices, A.data, left, right, T)
    want = np.array(tree.assignments, dtype=np.int64)
    inside = want != NONE
    worst = min(min(mj) for mj in margins)
    print(f"{case}: {int(inside.sum())} of {n} documents are not outliers, smallest margin {worst:.3e}")
    assert np.array_equal(leaf[inside], want[inside])
    assert sorted(np.nonzero(~inside)[0].tolist()) == sorted(tree.outliers) and len(tree.outliers) == tiny       # the far-off cluster
    assert worst >= MARGIN


def _check(left, right, valid):
    from smallk_amd import _lib as L
    left, right = np.ascontiguousarray(left, dtype=np.uint32), np.ascontiguousarray(right, dtype=np.uint32)
    valid = np.ascontiguousarray(valid, dtype=np.int32)
    pairs, depth = C.c_int(-7), C.c_int(-7)
    rc = L.lib().smk_tree_router_check(len(left), left.ctypes.data_as(C.POINTER(C.c_uint)), right.ctypes.data_as(C.POINTER(C.c_uint)),
                                       valid.ctypes.data_as(C.POINTER(C.c_int)), C.byref(pairs), C.byref(depth))
    return rc, pairs.value, depth.value, (L.lib().smk_last_error() or b"").decode()


def bad_structures():
    """(what, the node the message must name, left, right, valid): each a balanced tree with one thing wrong"""
    out = []
    for what, node, edit in (("cycle", 0, lambda l, r, v: (l.__setitem__(6, 0), r.__setitem__(6, 1))),
                             ("two parents", 2, lambda l, r, v: r.__setitem__(1, 2)),
                             ("one child", 3, lambda l, r, v: l.__setitem__(3, NONE)),
                             ("child index", 5, lambda l, r, v: r.__setitem__(5, 14)),
                             ("missing root", 1, lambda l, r, v: v.__setitem__(1, 0)),
                             ("invalid child", 2, lambda l, r, v: v.__setitem__(7, 0))):
        l, r, v = (x.copy() for x in cases.links("balanced3"))
        edit(l, r, v)
        out.append((what, node, l, r, v))
    return out


def test_structure_check_through_the_library():
    """smk_tree_router_check needs no device: the right pairs / max_depth for every case, BAD_PARAM naming the node otherwise"""
    from smallk_amd import _lib as L
    want = {"root_pair": (1, 1), "balanced3": (7, 3), "chain9": (9, 9), "slots22": (5, 4)}
    for name in cases.TREES:
        left, right, valid = cases.links(name)
        assert ref.structure(left, right) == want[name]
        assert _check(left, right, valid)[:3] == (L.OK,) + want[name], name
    for what, node, l, r, v in bad_structures():
        rc, pairs, depth, text = _check(l, r, v)
        assert rc == L.BAD_PARAM and (pairs, depth) == (-7, -7) and f"(node {node})" in text, (what, text)
    # a tree of one node, and the Python wrapper
    assert _check([NONE], [NONE], [1])[0] == L.BAD_PARAM
    from smallk_amd.hierclust import check_tree_structure
    assert check_tree_structure(*cases.links("chain9")) == (9, 9)
    with pytest.raises(L.SmallkError) as e:
        check_tree_structure(*bad_structures()[0][2:])
    assert e.value.code == L.BAD_PARAM


def test_structure_check_alone_under_the_sanitizers(tmp_path):
    """tree_route_check.h compiles without HIP; the good and the bad structures through it under ASan + UBSan"""
    exe = tmp_path / "check_sim"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "tree_route", "check_sim.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    good = [cases.links(name) for name in cases.TREES]
    bad = [s[2:] for s in bad_structures()]
    huge = (np.array([NONE - 1, NONE], dtype=np.uint32), np.array([5, NONE], dtype=np.uint32), np.ones(2, dtype=np.int32))     # links far outside
    lines = ["%d %s" % (len(l), " ".join("%d %d %d" % t for t in zip(l.tolist(), r.tolist(), v.tolist()))) for l, r, v in good + bad + [huge]]
    lines.append("1 4294967295 4294967295 1")
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=120, env=ENV)
    text = r.stdout[-3000:] + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-4000:]
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "check_sim: done %d" % len(lines), text[-3000:]
    want = [(1, 1), (7, 3), (9, 9), (5, 4)]
    for line, (pairs, depth), (l, rr, v) in zip(out, want, good):
        words = line.split()
        assert words[:3] == ["ok", str(pairs), str(depth)], line
        bar = words.index("|")
        pair_nodes, child_pair = [int(w) for w in words[3:bar]], [int(w) for w in words[bar + 1:]]
        assert len(pair_nodes) == 2 * pairs and len(child_pair) == len(l) and pair_nodes[:2] == [0, 1]
        for q, p in enumerate(child_pair):           # the pair of a split is the pair of its children; leaves and unopened slots have none
            if v[q] and l[q] != NONE:
                assert pair_nodes[2 * p:2 * p + 2] == [int(l[q]), int(rr[q])], (line, q)
            else:
                assert p == -1, (line, q)
    for line, (what, node, *_), in zip(out[len(good):], bad_structures()):
        assert line.startswith("bad ") and f"(node {node})" in line, (what, line)
    assert out[len(good) + len(bad)].startswith("bad ") and out[len(good) + len(bad) + 1].startswith("bad ")


def test_saved_router_round_trips_bit_for_bit(tmp_path):
    """file level only: the four arrays of a router come back from the .npz with the same bits (garbage slots included)"""
    from smallk_amd import TreeRouter, _lib as L
    c = cases.case("slots22", 37)
    r = TreeRouter(c["left"], c["right"], c["topics"], c["valid"])
    assert (r.pairs, r.max_depth, r.table_bytes, r.m, r.node_count) == (5, 4, 5 * 37 * 16, 37, 22)
    path = tmp_path / "router.npz"
    r.save(path)
    back = TreeRouter.load(path)
    for key in ("left", "right", "valid", "topics"):
        a, b = getattr(r, key), getattr(back, key)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="F") == b.tobytes(order="F"), key
        assert np.array_equal(np.asarray(c[key]), a)
    assert (back.pairs, back.max_depth) == (r.pairs, r.max_depth)
    with pytest.raises(L.SmallkError):
        TreeRouter(*bad_structures()[1][2:4], c["topics"][:, :14], bad_structures()[1][4])

"""HierNMF2 host mirror: ``Clust`` / ``ClustSparse`` + ``Tree<T>`` behind the C ABI.

Reference surface: hierclust/include/clust.hpp:27-58 (ClustOptions, ClustStats, Clust, ClustSparse),
hierclust/include/tree.hpp (Tree<T>), pysmallk's ``TreeResults`` (smallk_lib.pyx:399-420: ``write``,
``write_assignments``, ``get_assignments``).  All numeric work happens in libsmallk_amd.so on the
GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L

NONE = 0xFFFFFFFF


@dataclass
class TreeNode:
    priority: float
    parent: int
    left: int
    right: int
    is_valid: bool
    is_left_child: bool
    is_leaf: bool
    docs: np.ndarray
    topic_vector: np.ndarray
    term_indices: list


class TreeResults:
    """Owns an ``smk_tree``; mirrors pysmallk's TreeResults plus read access to the nodes."""

    def __init__(self, handle, stats):
        self._h = handle
        self.nmf_count, self.max_count = stats.nmf_count, stats.max_count

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            L.lib().smk_tree_destroy(h)

    @property
    def node_count(self):
        return L.lib().smk_tree_node_count(self._h)

    def node(self, q) -> TreeNode:
        l = L.lib()
        info = L.TreeNodeInfo()
        L.check(l.smk_tree_get_node(self._h, q, C.byref(info)), "smk_tree_get_node")
        docs = np.zeros(max(info.doc_count, 1), dtype=np.uint32)
        l.smk_tree_node_docs(self._h, q, docs.ctypes.data_as(C.POINTER(C.c_uint)))
        topic = np.zeros(l.smk_tree_term_count(self._h))
        l.smk_tree_node_topic(self._h, q, topic.ctypes.data_as(C.POINTER(C.c_double)))
        terms = (C.c_int * 4096)()
        nt = l.smk_tree_node_terms(self._h, q, terms)
        return TreeNode(info.priority, info.parent, info.left_child, info.right_child, bool(info.is_valid),
                        bool(info.is_left_child), bool(info.is_leaf), docs[:info.doc_count], topic,
                        [terms[i] for i in range(nt)])

    @property
    def nodes(self):
        return [self.node(q) for q in range(self.node_count)]

    def get_assignments(self):
        n = L.lib().smk_tree_doc_count(self._h)
        out = np.zeros(n, dtype=np.uint32)
        L.lib().smk_tree_assignments(self._h, out.ctypes.data_as(C.POINTER(C.c_uint)))
        return out

    def get_outliers(self):
        cnt = L.lib().smk_tree_outliers(self._h, None)
        out = np.zeros(max(cnt, 1), dtype=np.uint32)
        L.lib().smk_tree_outliers(self._h, out.ctypes.data_as(C.POINTER(C.c_uint)))
        return out[:cnt]

    def flat_factors(self):
        """(W m x k, H k x n) of the flat clustering run with ``flat=True`` (ClustFlat)."""
        l = L.lib()
        m, n = l.smk_tree_term_count(self._h), l.smk_tree_doc_count(self._h)
        k = sum(1 for q in range(self.node_count) if self.node(q).is_leaf)
        W = np.zeros((m, k), order="F")
        H = np.zeros((k, n), order="F")
        L.check(l.smk_tree_flat_factors(self._h, W.ctypes.data_as(C.POINTER(C.c_double)), m,
                                        H.ctypes.data_as(C.POINTER(C.c_double)), k), "smk_tree_flat_factors")
        return W, H

    def router(self) -> "TreeRouter":
        """A ``TreeRouter`` of this tree (its links and topic vectors, read through the node accessors): new documents down the
        tree on the device.  It lives on without the tree and can be saved."""
        h = C.c_void_p()
        L.check(L.lib().smk_tree_router_from_tree(self._h, C.byref(h)), "smk_tree_router_from_tree")
        return TreeRouter._from_handle(h)

    def assign(self, A_new):
        """Leaf nodes of new documents (the columns of a sparse matrix with this tree's terms as rows), a numpy uint32 array in
        the convention of ``get_assignments``: the index of the leaf node.  Routing never returns NONE: every document reaches a
        leaf.  The training outliers that ``get_assignments`` marks NONE are a property of the search (``trial_split`` sets
        small far-off subsets aside), not of the routing rule, so a training outlier routed again lands on a leaf.  The device
        tables are packed for this call; keep ``router()`` for more than one batch."""
        return self.router().route(A_new).cpu().numpy().astype(np.uint32)

    def write_assignments(self, filepath):
        return L.lib().smk_tree_write_assignments(self._h, str(filepath).encode()) == L.OK

    def write(self, filepath, dictionary, form="JSON"):
        terms = (C.c_char_p * len(dictionary))(*[str(t).encode() for t in dictionary])
        fmt = 0 if str(form).upper() == "XML" else 1
        return L.lib().smk_tree_write(self._h, str(filepath).encode(), fmt, terms, len(dictionary)) == L.OK


_up = C.POINTER(C.c_uint)
_ip = C.POINTER(C.c_int)


def check_tree_structure(left, right, valid=None):
    """(pairs, max_depth) of a tree given by its links, or SmallkError(BAD_PARAM) naming the node (``smk_tree_router_check``;
    host code, no GPU).  pairs: splits plus the root pair; max_depth: decisions on the longest descent."""
    left, right = np.ascontiguousarray(left, dtype=np.uint32), np.ascontiguousarray(right, dtype=np.uint32)
    if left.ndim != 1 or right.shape != left.shape:
        raise ValueError("check_tree_structure: left and right are 1-D arrays of one length")
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.int32)
    if v is not None and v.shape != left.shape:
        raise ValueError("check_tree_structure: valid has one entry per node")
    pairs, depth = C.c_int(), C.c_int()
    L.check(L.lib().smk_tree_router_check(len(left), left.ctypes.data_as(_up), right.ctypes.data_as(_up),
                                          v.ctypes.data_as(_ip) if v is not None else None, C.byref(pairs), C.byref(depth)),
            "smk_tree_router_check")
    return pairs.value, depth.value


class TreeRouter:
    """New documents down a fitted HierNMF2 tree, on the device.

    ``left`` / ``right``: the child links per node (``NONE`` = 0xFFFFFFFF for a leaf), ``topics``: (m, node_count) float64, column
    q the topic vector of node q, ``valid``: per node whether the search opened it (None: every node).  Nodes 0 and 1 are the
    roots, as HierNMF2 numbers them; invalid or unreachable nodes are ignored whatever they hold.  The structure is checked on
    the host when the object is made (SmallkError BAD_PARAM names the node).

    The rule is the training code's: at a split with child topic vectors w_l, w_r document a goes left iff h0 > h1, where
    (h0, h1) = argmin_{h >= 0} ||a - [w_l w_r] h|| by the closed-form rank-2 solve.  Routing never returns NONE: every
    document reaches a leaf; a document without entries goes right at every level.  The outliers of a training run are a
    property of the search (``trial_split``), not of this rule.

    The device tables hold the two topic vectors of every sibling pair interleaved: ``table_bytes`` = pairs * m * 16 (an 8-leaf
    tree over 10^6 terms: 7 pairs, 112 MB).  They are built when the object is made if the library is initialised, else by the
    first ``route``; a pair whose 2 x 2 Gram matrix is singular (a zero topic vector) is SmallkError FAILURE there."""

    def __init__(self, left, right, topics, valid=None):
        self._h = None
        self.left = np.ascontiguousarray(left, dtype=np.uint32).copy()
        self.right = np.ascontiguousarray(right, dtype=np.uint32).copy()
        t = np.asarray(topics, dtype=np.float64)
        if t.ndim != 2 or self.left.ndim != 1 or t.shape[1] != len(self.left) or self.right.shape != self.left.shape or t.shape[0] < 1:
            raise ValueError("TreeRouter: left and right have node_count entries, topics is (m, node_count)")
        self.topics = np.asfortranarray(t).copy(order="F")
        self.valid = np.ones(len(self.left), dtype=np.int32) if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.int32)
        if self.valid.shape != self.left.shape:
            raise ValueError("TreeRouter: valid has one entry per node")
        self.m, self.node_count = int(t.shape[0]), len(self.left)
        self.pairs, self.max_depth = check_tree_structure(self.left, self.right, self.valid)
        from .solver import is_initialized
        if is_initialized():
            self._handle()

    @classmethod
    def _from_handle(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        m, nc, pairs, depth, tb = C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        L.check(L.lib().smk_tree_router_sizes(handle, C.byref(m), C.byref(nc), C.byref(pairs), C.byref(depth), C.byref(tb)), "smk_tree_router_sizes")
        self.m, self.node_count, self.pairs, self.max_depth = m.value, nc.value, pairs.value, depth.value
        self.left = np.zeros(nc.value, dtype=np.uint32)
        self.right = np.zeros(nc.value, dtype=np.uint32)
        self.valid = np.zeros(nc.value, dtype=np.int32)
        self.topics = np.zeros((m.value, nc.value), order="F")
        L.check(L.lib().smk_tree_router_download(handle, self.left.ctypes.data_as(_up), self.right.ctypes.data_as(_up), self.valid.ctypes.data_as(_ip),
                                                 self.topics.ctypes.data_as(C.POINTER(C.c_double)), m.value), "smk_tree_router_download")
        return self

    def _handle(self):
        if not self._h:
            from .solver import initialize, is_initialized
            if not is_initialized():
                initialize(-1)
            h = C.c_void_p()
            L.check(L.lib().smk_tree_router_create(self.m, self.node_count, self.left.ctypes.data_as(_up), self.right.ctypes.data_as(_up),
                                                   self.valid.ctypes.data_as(_ip), self.topics.ctypes.data_as(C.POINTER(C.c_double)),
                                                   self.m, C.byref(h)), "smk_tree_router_create")
            self._h = h
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            L.lib().smk_tree_router_destroy(h)

    __del__ = close

    @property
    def table_bytes(self):
        """bytes of the interleaved topic tables on the device: pairs * m * 16"""
        return self.pairs * self.m * 16

    def save(self, path):
        """The router as an .npz file (left, right, topics, valid) for a later process."""
        with open(path, "wb") as f:
            np.savez(f, left=self.left, right=self.right, topics=self.topics, valid=self.valid)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["left"], z["right"], z["topics"], z["valid"])

    def route(self, A_new, *, details=False):
        """The leaf of every column of ``A_new`` (a resident ``SparseMatrix`` with m rows, or a scipy sparse matrix, which is
        uploaded): an int32 torch tensor (n,) on the GPU, the leaf node's index in the tree's own numbering (what
        ``get_assignments`` uses), never NONE.  With ``details`` also ``depth`` (int32: decisions taken) and ``h`` (n, 2) float64:
        (h0, h1) of the last decision.  One launch; the same bits on every run.  A dense ``A_new`` is SmallkError UNSUPPORTED."""
        import torch
        from .solver import SparseMatrix
        h = self._handle()
        own = None
        if hasattr(A_new, "tocsc"):
            own = A_new = SparseMatrix.from_scipy(A_new)
        if not hasattr(A_new, "_h") or not hasattr(A_new, "ncols"):
            raise TypeError(f"TreeRouter.route: expected a SparseMatrix or a scipy sparse matrix, got {type(A_new).__name__}")
        n = int(A_new.ncols)
        dev = torch.device("cuda", L.lib().smk_current_device())
        leaf = torch.empty(n, dtype=torch.int32, device=dev)
        depth = torch.empty(n, dtype=torch.int32, device=dev) if details else None
        hh = torch.empty((n, 2), dtype=torch.float64, device=dev) if details else None
        try:
            L.check(L.lib().smk_tree_route_device(h, A_new._h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.c_void_p(leaf.data_ptr()),
                                                  C.c_void_p(depth.data_ptr()) if details else None,
                                                  C.c_void_p(hh.data_ptr()) if details else None), "smk_tree_route_device")
        finally:
            if own is not None:
                own.close()
        return (leaf, depth, hh) if details else leaf


def make_clust_options(m, n, num_clusters, *, tol=1e-4, min_iter=5, max_iter=5000, maxterms=5, unbalanced=0.1,
                       trial_allowance=3, verbose=False, flat=False, prog_est=L.PROG_PG_RATIO):
    """The option set smallk::HierNmf2 uses (smallk/src/smallk.cpp:755-772)."""
    o = L.ClustOptions()
    o.nmf = L.Options(tol, L.ALG_RANK2, prog_est, m, n, 2, min_iter, max_iter, 1, 1, 0, 1)
    o.maxterms, o.unbalanced, o.trial_allowance = maxterms, unbalanced, trial_allowance
    o.num_clusters, o.verbose, o.flat = num_clusters, int(verbose), int(flat)
    return o


def hier_nmf2(A, num_clusters, *, seed=0, draws=0, initdir="", storage="f32", **kw) -> TreeResults:
    """Clust (dense ndarray) / ClustSparse (scipy.sparse matrix) -> TreeResults.  A may also be a
    ``DenseMatrix`` / ``SparseMatrix`` that is already resident in HBM (no upload, ``storage`` ignored)."""
    l = L.lib()
    resident = hasattr(A, "_h") and hasattr(A, "height")       # a DenseMatrix / SparseMatrix already in HBM
    m, n = (A.height, A.ncols) if resident else A.shape
    o = make_clust_options(m, n, num_clusters, **kw)
    tree = C.c_void_p()
    stats = L.ClustStats()
    dr = C.c_uint64(draws)
    idir = initdir.encode() if initdir else None
    if resident:
        rc = l.smk_clust_resident(C.byref(o), A._h, seed, C.byref(dr), idir, C.byref(tree), C.byref(stats))
    elif hasattr(A, "tocsc"):
        a = A.tocsc()
        a.sort_indices()
        co = np.ascontiguousarray(a.indptr, dtype=np.uint32)
        ri = np.ascontiguousarray(a.indices, dtype=np.uint32)
        va = np.ascontiguousarray(a.data, dtype=np.float64)
        rc = l.smk_clust_sparse(C.byref(o), a.nnz, co.ctypes.data_as(C.POINTER(C.c_uint)),
                                ri.ctypes.data_as(C.POINTER(C.c_uint)), va.ctypes.data_as(C.POINTER(C.c_double)),
                                seed, C.byref(dr), idir, C.byref(tree), C.byref(stats))
    else:
        a = np.asfortranarray(A, dtype=np.float64)
        st = L.STORE_BF16 if str(storage).lower() == "bf16" else L.STORE_F32
        rc = l.smk_clust_dense(C.byref(o), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], st, seed,
                               C.byref(dr), idir, C.byref(tree), C.byref(stats))
    if rc != L.OK and tree:            # FLATCLUST_FAILURE hands the tree back; this wrapper raises instead
        l.smk_tree_destroy(tree)
    L.check(rc, "smk_clust")
    res = TreeResults(tree, stats)
    res.draws = dr.value
    return res


def priority(w_parent, w_child) -> float:
    """compute_priority (clust_hier_util.hpp:105-173); host-side, no GPU needed."""
    wp = np.ascontiguousarray(w_parent, dtype=np.float64).ravel()
    wc = np.asfortranarray(w_child, dtype=np.float64)
    return L.lib().smk_clust_priority(wp.ctypes.data_as(C.POINTER(C.c_double)),
                                      wc.ctypes.data_as(C.POINTER(C.c_double)), len(wp))

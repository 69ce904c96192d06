"""The descent of a document down a HierNMF2 tree, restated in numpy (what smk_tree_route_device computes).

At the pair (l, r) -- first the roots (0, 1), then the children of the node just chosen -- the document a goes to l iff h0 > h1,
(h0, h1) = argmin_{h >= 0} ||a - [w_l w_r] h||: tree_partition's rule.  The solve is the closed-form rank-2 solve of
smallk_amd/csrc/rank2_math.h, side 0 (one fast Givens rotation, cosine or sine branch, then the optimal active set), written
out again here and not read from the header.  Every sum runs in storage order: the Gram entries over the rows, the dot products
over the document's stored entries.  ``dtype`` is numpy.float64 or numpy.longdouble (the thresholds stay those of fp64)."""
import numpy as np

NONE = 0xFFFFFFFF
EPS = np.finfo(np.float64).eps


def _seq_sum(x, dtype):
    return np.cumsum(x, dtype=dtype)[-1] if len(x) else dtype(0)


def prepare(a00, a01, a11):
    """what depends on the 2 x 2 Gram matrix only (r2_prepare, side 0)"""
    one = type(a00)(1)
    a10 = a01
    bad = bool(abs(a00) < EPS and abs(a01) < EPS)
    cosine = bool(abs(a00) >= abs(a01))
    if cosine:
        t = -a10 / a00
        a2, b2, d2 = a00 - t * a10, a01 - t * a11, a11 + t * a01
    else:
        t = -a00 / a10
        a2, b2, d2 = -a10 + t * a00, -a11 + t * a01, a01 + t * a11
    if abs(d2 / a2) < EPS:
        bad = True
    return dict(t=t, b2=b2, inv_a2=one / a2, inv_d2=one / d2, inv0=one / a00, inv1=one / a11, sq0=np.sqrt(a00), sq1=np.sqrt(a11),
                cosine=cosine, bad=bad)


def apply(s, b0, b1):
    """one right-hand side -> the non-negative solution (r2_apply, side 0)"""
    t = s["t"]
    if s["cosine"]:
        e2, f2 = b0 - t * b1, b1 + t * b0
    else:
        e2, f2 = -b1 + t * b0, b0 + t * b1
    x1 = f2 * s["inv_d2"]
    x0 = (e2 - s["b2"] * x1) * s["inv_a2"]
    if x0 <= 0 or x1 <= 0:
        v1, v2 = b0 * s["inv0"], b1 * s["inv1"]
        if v1 * s["sq0"] >= v2 * s["sq1"]:
            v2 = type(v2)(0)
        else:
            v1 = type(v1)(0)
        x0, x1 = v1, v2
    return x0, x1


def margin(h0, h1):
    """|h0 - h1| / max(h0, h1) of one decision; inf for h = (0, 0) exactly (a document without entries: no rounding takes part)"""
    top = max(h0, h1)
    return float("inf") if top == 0 else float(abs(h0 - h1) / top)


def route(colptr, rowidx, val, left, right, topics, dtype=np.float64):
    """leaf (int32), depth (int32), h (n x 2, dtype) and margins (one list per document, one entry per decision) of the columns of
    the CSC (colptr, rowidx, val) down the tree (left, right, topics m x node_count).  Only nodes on a descent are read."""
    topics = np.asarray(topics, dtype=np.float64)
    n = len(colptr) - 1
    solves = {}

    def solve_of(l, r):
        if (l, r) not in solves:
            wl, wr = topics[:, l].astype(dtype), topics[:, r].astype(dtype)
            solves[(l, r)] = prepare(_seq_sum(wl * wl, dtype), _seq_sum(wl * wr, dtype), _seq_sum(wr * wr, dtype))
        return solves[(l, r)]

    leaf, depth = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    h = np.zeros((n, 2), dtype=dtype)
    margins = []
    for j in range(n):
        rows = np.asarray(rowidx[colptr[j]:colptr[j + 1]], dtype=np.int64)
        a = np.asarray(val[colptr[j]:colptr[j + 1]], dtype=np.float64).astype(dtype)
        l, r, d, mj = 0, 1, 0, []
        while True:
            s = solve_of(l, r)
            b0 = _seq_sum(a * topics[rows, l].astype(dtype), dtype)
            b1 = _seq_sum(a * topics[rows, r].astype(dtype), dtype)
            h0, h1 = apply(s, b0, b1)
            mj.append(margin(h0, h1))
            node = l if h0 > h1 else r
            d += 1
            if left[node] == NONE:
                break
            l, r = int(left[node]), int(right[node])
        leaf[j], depth[j], h[j, 0], h[j, 1] = node, d, h0, h1
        margins.append(mj)
    return leaf, depth, h, margins


def structure(left, right, valid=None):
    """(pairs, max_depth) of the forest under the roots 0 and 1: splits + the root pair, decisions on the longest descent"""
    pairs, deepest, todo = 1, 1, [(0, 1), (1, 1)]
    while todo:
        q, d = todo.pop()
        deepest = max(deepest, d)
        if left[q] != NONE:
            pairs += 1
            todo += [(int(left[q]), d + 1), (int(right[q]), d + 1)]
    return pairs, deepest

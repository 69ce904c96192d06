"""Hand-built trees and documents for the tree router's tests (CPU and GPU): deterministic, small, at the edges of the kernel's
launch shape.  Trees are numbered as HierNMF2 numbers them: roots 0 and 1, a split opens the next two free slots (left, right).
Documents are sparse columns drawn from the topic vectors on the path to a target leaf plus noise, so that a descent is decided
by the data at every level.  tree_route_reference.route gives what the device must return."""
import functools

import numpy as np

import tree_route_reference as ref

NONE = ref.NONE
HEIGHTS = (37, 200)
TREES = ("root_pair", "balanced3", "chain9", "slots22")
WIDTHS = (1, 15, 16, 17, 63, 64, 65, 257)           # documents per call: the edges of a wave (4) and of a workgroup (16)
SEED = 20


def links(name):
    """(left, right, valid) of a tree; slots22 has 22 slots of which the search opened 10, the others hold garbage links"""
    splits = {"root_pair": [], "balanced3": [0, 1, 2, 3, 4, 5], "chain9": [0, 2, 4, 6, 8, 10, 12, 14], "slots22": [1, 2, 0, 5]}[name]
    count = 22 if name == "slots22" else 2 + 2 * len(splits)
    left, right = np.full(count, NONE, dtype=np.uint32), np.full(count, NONE, dtype=np.uint32)
    valid = np.zeros(count, dtype=np.int32)
    valid[:2] = 1
    active = 2
    for q in splits:
        left[q], right[q] = active, active + 1
        valid[active:active + 2] = 1
        active += 2
    for q in range(active, count):                  # never opened: links that would be refused if anything read them
        left[q], right[q] = q, (q * 7) % count
    return left, right, valid


def leaves_under(left, right, q):
    return [q] if left[q] == NONE else leaves_under(left, right, left[q]) + leaves_under(left, right, right[q])


def path_to(left, right, leaf):
    """the nodes chosen on the way to `leaf`, root first"""
    parent = {}
    for q in range(len(left)):
        if left[q] != NONE and left[q] < len(left) and q not in (left[q], right[q]):
            parent.setdefault(int(left[q]), q)
            parent.setdefault(int(right[q]), q)
    out = [leaf]
    while out[-1] not in (0, 1):
        out.append(parent[out[-1]])
    return out[::-1]


@functools.lru_cache(maxsize=None)
def case(name, m):
    """dict(left, right, valid, topics (m x node_count), colptr, rowidx, val (257 documents), target)"""
    rng = np.random.default_rng([SEED, TREES.index(name), m])
    left, right, valid = links(name)
    count = len(left)
    reach = [q for q in range(count) if valid[q]]
    leaves = [q for q in reach if left[q] == NONE]
    own = {q: 0.02 * rng.random(m) for q in reach}
    for q in leaves:                                 # a leaf's own terms
        idx = rng.choice(m, size=max(3, m // 6), replace=False)
        own[q][idx] += rng.random(len(idx)) + 0.3
    topics = 1e6 * rng.standard_normal((m, count))  # garbage where the search never went
    for q in reach:
        under = leaves_under(left, right, q)
        topics[:, q] = np.mean([own[u] for u in under], axis=0) + (0.0 if q in leaves else 0.02 * rng.random(m))
    edge = [17, 0, 1, 15, 16, 31, 32, 33, m]         # entries per document: the edges of the 16-entry chunk (the first one is not empty:
                                                     # a call over one document needs a matrix with an entry)
    colptr, rowidx, val, target = [0], [], [], []
    for j in range(max(WIDTHS)):
        leaf = leaves[j % len(leaves)] if j >= len(edge) else leaves[int(rng.integers(len(leaves)))]
        cnt = edge[j] if j < len(edge) else int(rng.integers(1, m + 1))
        x = sum((1.0 + i) * topics[:, q] for i, q in enumerate(path_to(left, right, leaf))) * (0.5 + rng.random()) + 0.05 * rng.random(m)
        rows = np.sort(np.argsort(-(x * (0.6 + 0.4 * rng.random(m))), kind="stable")[:cnt])
        if j == 3 and m - 1 not in rows:
            rows[-1] = m - 1                          # an entry in the last row of the tables
        rowidx += [int(r) for r in rows]
        val += [float(v) for v in x[rows]]
        colptr.append(len(rowidx))
        target.append(leaf)
    return dict(left=left, right=right, valid=valid, topics=np.asfortranarray(topics), colptr=np.array(colptr, dtype=np.int64),
                rowidx=np.array(rowidx, dtype=np.int64), val=np.array(val), target=np.array(target), leaves=leaves, m=m)


@functools.lru_cache(maxsize=None)
def expected(name, m, long_double=False):
    """(leaf, depth, h, margins) of the 257 documents of a case; a call over the first n documents must return their first n"""
    c = case(name, m)
    return ref.route(c["colptr"], c["rowidx"], c["val"], c["left"], c["right"], c["topics"], np.longdouble if long_double else np.float64)


def rightmost(left, right):
    """(leaf, depth) of the descent that goes right at every level"""
    q, d = 1, 1
    while left[q] != NONE:
        q, d = int(right[q]), d + 1
    return q, d


def scipy_columns(c, n):
    import scipy.sparse as sp
    p = c["colptr"][:n + 1]
    return sp.csc_matrix((c["val"][:p[-1]], c["rowidx"][:p[-1]], p), shape=(c["m"], n))


def all_cases():
    return [(name, m) for name in TREES for m in HEIGHTS]

"""smk_tree_route_device at size: new documents drawn like tools/vocabulary_rate.py's corpus, routed down HierNMF2 trees fitted on
documents of that kind.  Kernel time is taken from device events (smk_tree_route_time, the minimum of three windows) and compared
with two things that are not the code under test:

  1. the floor: one plain rank-2 gather of the same entries (smk_matrix_sparse_product, k = 2) times the mean depth -- a descent
     gathers a 16-byte pair per entry and level, and so does that product;
  2. the only route there was: the scores of all nodes from one sparse product at k = node_count, a download, and the descent in
     numpy on the host.

    python tools/route_rate.py [--terms 1048576] [--train-docs 200000] [--new-docs 200000] [--per-doc 85] [--leaves 8 64]
                               [--reps 5] [--out profiles/route_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_descent(P, left, right, T):
    """the descent in numpy from the scores P (node_count x n) of every node: the leaf of every document"""
    import tree_route_reference as ref
    none = ref.NONE
    n = P.shape[1]
    node = np.full(n, -1, dtype=np.int64)
    l, r = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    live = np.arange(n)
    solves = {}
    sibling = {0: 1}
    sibling.update({int(left[q]): int(right[q]) for q in range(len(left)) if left[q] != none})
    while live.size:
        go_left = np.zeros(live.size, dtype=bool)
        for pl in np.unique(l[live]):
            pl, pr = int(pl), sibling[int(pl)]
            if (pl, pr) not in solves:
                wl, wr = T[:, pl], T[:, pr]
                solves[(pl, pr)] = ref.prepare(np.cumsum(wl * wl)[-1], np.cumsum(wl * wr)[-1], np.cumsum(wr * wr)[-1])
            s = solves[(pl, pr)]
            sel = l[live] == pl
            b0, b1 = P[pl, live[sel]], P[pr, live[sel]]
            t = s["t"]
            e2, f2 = (b0 - t * b1, b1 + t * b0) if s["cosine"] else (-b1 + t * b0, b0 + t * b1)
            x1 = f2 * s["inv_d2"]
            x0 = (e2 - s["b2"] * x1) * s["inv_a2"]
            act = (x0 <= 0) | (x1 <= 0)
            first = (b0 * s["inv0"]) * s["sq0"] >= (b1 * s["inv1"]) * s["sq1"]
            x0 = np.where(act, np.where(first, b0 * s["inv0"], 0.0), x0)
            x1 = np.where(act, np.where(first, 0.0, b1 * s["inv1"]), x1)
            go_left[sel] = x0 > x1
        node[live] = np.where(go_left, l[live], r[live])
        split = left[node[live]] != none
        live = live[split]
        l[live], r[live] = left[node[live]], right[node[live]]
    return node


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--terms", type=int, default=1 << 20)
    ap.add_argument("--train-docs", type=int, default=200000)
    ap.add_argument("--new-docs", type=int, default=200000)
    ap.add_argument("--per-doc", type=int, default=85)
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--leaves", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")

    import scipy.sparse as sp
    import smallk_amd
    from smallk_amd import _lib as L
    from smallk_amd.preprocess import preprocess
    from smallk_amd.synthetic import term_counts
    smallk_amd.initialize(0)
    lib = L.lib()
    t = time.time()
    docs = a.train_docs + a.new_docs
    A = term_counts(a.terms, docs, a.per_doc * docs, 1, dup_frac=0.0, sigma=a.sigma)
    fit = preprocess(a.terms, docs, A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data)
    del A
    _, _, cp, rows, scores = fit.download()
    S = sp.csc_matrix((scores, rows, cp), shape=(fit.height, fit.width))
    train, new = S[:, :fit.width // 2], S[:, fit.width // 2:]
    m = fit.height
    say(f"corpus: term_counts({a.terms} terms, {docs} documents, {a.per_doc} entries per document, seed 1, sigma {a.sigma}) after "
        f"preprocess: {m} terms x {fit.width} documents, {S.nnz} entries of tf-idf; trained on the first {train.shape[1]} "
        f"({train.nnz} entries), routed: the other {new.shape[1]} ({new.nnz} entries) ({time.time() - t:.1f} s)")
    fit.close()
    A_train = smallk_amd.SparseMatrix.from_scipy(train)
    A_new = smallk_amd.SparseMatrix.from_scipy(new)
    n, nnz = new.shape[1], new.nnz

    X2 = np.asfortranarray(np.random.default_rng(3).random((2, m)))
    floor = min(A_new.product(X2, reps=a.reps)[1] for _ in range(3))
    say(f"plain rank-2 gather of the routed entries (smk_matrix_sparse_product, k = 2, minimum of three windows of {a.reps}): "
        f"{floor:.3f} ms = {nnz * 28 / (floor * 1e-3) / 1e12:.2f} TB/s of index, value and 16-byte operand traffic")

    for want in a.leaves:
        t = time.time()
        tree = smallk_amd.hier_nmf2(A_train, want, seed=11)
        nodes = tree.nodes
        leaves = [q for q, nd in enumerate(nodes) if nd.is_leaf]
        r = tree.router()
        say()
        say(f"tree asked for {want} leaves: {len(leaves)} leaves, {r.pairs} pairs, at most {r.max_depth} decisions, tables "
            f"{r.table_bytes / 1e6:.0f} MB (fit {time.time() - t:.1f} s, {tree.nmf_count} factorisations)")
        leaf, depth, _ = r.route(A_new, details=True)
        depth_mean = float(depth.double().mean().item())
        ms = []
        for _ in range(3):
            v = C.c_double()
            L.check(lib.smk_tree_route_time(r._handle(), A_new._h, a.reps, C.byref(v)), "smk_tree_route_time")
            ms.append(v.value)
        kern = min(ms)
        say(f"  smk_tree_route_device: kernel {kern:.3f} ms (minimum of three windows of {a.reps}: {', '.join('%.3f' % x for x in ms)}); "
            f"mean depth {depth_mean:.2f}; {nnz * depth_mean / (kern * 1e-3) / 1e9:.1f} G entry-levels/s")
        say(f"  1. floor = {floor:.3f} ms x mean depth {depth_mean:.2f} = {floor * depth_mean:.3f} ms; kernel / floor = {kern / (floor * depth_mean):.2f}")
        # 2. the only route there was
        left, right, T = r.left, r.right, r.topics
        k = r.node_count
        if k >= 3:
            X = np.asfortranarray(T.T)
            t0 = time.perf_counter()
            P = A_new.product(X)
            t1 = time.perf_counter()
            host = host_descent(P, left, right, T)
            t2 = time.perf_counter()
            prod_ms = min(A_new.product(X, reps=a.reps)[1] for _ in range(2))
            same = int((host == leaf.cpu().numpy()).sum())
            say(f"  2. scores of all {k} nodes by one sparse product: kernel {prod_ms:.3f} ms, the call with upload and download "
                f"{(t1 - t0) * 1e3:.0f} ms, numpy descent {(t2 - t1) * 1e3:.0f} ms: {(t2 - t0) * 1e3:.0f} ms in all; routing kernel / "
                f"product kernel = {kern / prod_ms:.2f}, whole old route / routing kernel = {(t2 - t0) * 1e3 / kern:.0f}; "
                f"{same} of {n} leaves agree")
        r.close()
        del tree


if __name__ == "__main__":
    main()

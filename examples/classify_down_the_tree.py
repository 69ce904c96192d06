#!/usr/bin/env python3
"""Raw term counts in, leaves of a topic hierarchy out: fit the term set and idf on one batch of documents, grow a HierNMF2 tree on
the fit's matrix, save its router, and -- as a later process would -- load the router and the vocabulary and send a later batch of
raw counts down the tree.  After its upload the new batch never returns to the host.

``preprocess`` prunes and scores the training counts; ``hier_nmf2`` grows the tree; ``tree.router()`` keeps what routing needs
(the links and the topic vectors) and ``save`` / ``TreeRouter.load`` carry it across processes as ``Vocabulary.save`` / ``.load``
carry the term set; ``Vocabulary.apply`` turns the later batch into the matrix of the trained term space and ``route`` returns
the leaf of every document: at each split the document goes to the child whose topic vector takes the larger coefficient in the
non-negative rank-2 fit, the rule the tree was grown with.

    python examples/classify_down_the_tree.py
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import smallk_amd
from smallk_amd.preprocess import Vocabulary, preprocess
from smallk_amd.synthetic import term_counts


def main():
    smallk_amd.initialize(0)
    m, n, clusters = 5000, 3000, 8
    A = term_counts(m, n, 20 * n, 3, dup_frac=0.05).tocsc()
    n_train = 2 * n // 3
    train, new = A[:, :n_train], A[:, n_train:]

    fit = preprocess(m, n_train, train.indptr, train.indices, train.data)
    A_fit = fit.matrix()
    tree = smallk_amd.hier_nmf2(A_fit, clusters, seed=7)
    leaves = [q for q, nd in enumerate(tree.nodes) if nd.is_leaf]
    print(f"fit: {m} terms x {n_train} documents -> {fit.height} x {fit.width}; tree: {len(leaves)} leaves {leaves}, "
          f"{tree.nmf_count} factorisations, {len(tree.get_outliers())} outliers")

    with tempfile.TemporaryDirectory() as d:
        router = tree.router()
        print(f"router: {router.pairs} sibling pairs, at most {router.max_depth} decisions, {router.table_bytes / 1e6:.2f} MB of tables")
        router.save(os.path.join(d, "router.npz"))
        fit.vocabulary().save(os.path.join(d, "vocabulary.npz"))
        # the training documents land where the search put them (its outliers aside: routing sends those to a leaf too)
        mine = router.route(A_fit).cpu().numpy()
        want = tree.get_assignments()
        inside = want != smallk_amd.hierclust.NONE
        print(f"training documents on their own leaf: {int((mine[inside] == want[inside]).sum())} of {int(inside.sum())}")
        del router, tree

        # a later process: the two files, a batch of raw counts in the original term numbering
        router = smallk_amd.TreeRouter.load(os.path.join(d, "router.npz"))
        vocab = Vocabulary.load(os.path.join(d, "vocabulary.npz"))
    applied = vocab.apply(new, min_terms=1)
    A_new = applied.matrix()
    leaf, depth, h = router.route(A_new, details=True)
    sizes = torch.bincount(leaf.long(), minlength=router.node_count)
    print(f"new documents: {new.shape[1]} raw, {applied.width} with a known term; routed on {leaf.device}: "
          f"{ {q: int(sizes[q]) for q in leaves} } per leaf, mean depth {depth.double().mean().item():.2f}")
    for x in (A_new, A_fit, applied, vocab, fit, router):
        x.close()


if __name__ == "__main__":
    main()

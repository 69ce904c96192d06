"""Synthetic sparse inputs of the bench workloads and tests (host side, numpy/scipy; the reference's data sets --
smallk_data/reuters.mtx, Makefile:28 -- are not in the tree).

term_document(m, n, nnz, seed): a term-by-document count matrix in the shape of the reference's Reuters example
  (sphinx/source/pages_smallkAPI.rst:58-143: 12411 terms x 7984 documents): document lengths log-normal, terms drawn from a
  Zipf law (exponent 1.0) -- a few terms occur in thousands of documents, most in a handful -- tf weights 1 + log(count), every
  row and column non-empty (an empty row or column makes W'W or HH' singular under block pivoting).
community_graph(n, degree, communities, seed): the symmetric adjacency of tools/c5_hier.py (C5's shape): `communities` planted
  groups, 85 % of the edges inside a group, unit weights (duplicates summed)."""
import numpy as np
import scipy.sparse as sp


def term_document(m, n, nnz, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.lognormal(mean=0.0, sigma=0.6, size=n)
    lens = np.maximum(1, np.round(lens * (1.25 * nnz / lens.sum()))).astype(np.int64)   # duplicates collapse: draw ~25 % more
    p = 1.0 / np.arange(1, m + 1, dtype=np.float64)
    p /= p.sum()
    cdf = np.cumsum(p)
    total = int(lens.sum())
    terms = np.searchsorted(cdf, rng.random(total), side="right").astype(np.int64)
    terms = np.minimum(terms, m - 1)
    perm = rng.permutation(m)                           # frequent terms are not the first rows
    docs = np.repeat(np.arange(n, dtype=np.int64), lens)
    A = sp.coo_matrix((np.ones(total), (perm[terms], docs)), shape=(m, n)).tocsc()
    A.sum_duplicates()
    A.data = 1.0 + np.log(A.data)
    # every term occurs somewhere, every document has a term
    rows_missing = np.flatnonzero(np.diff(A.tocsr().indptr) == 0)
    if rows_missing.size:
        extra = sp.coo_matrix((np.ones(rows_missing.size), (rows_missing, rng.integers(0, n, rows_missing.size))), shape=(m, n))
        A = (A + extra).tocsc()
    A.sort_indices()
    return A


def community_graph(n, degree=16, communities=16, seed=0):
    rng = np.random.default_rng(seed)
    comm = rng.integers(0, communities, size=n)
    order = np.argsort(comm, kind="stable")
    starts = np.searchsorted(comm[order], np.arange(communities + 1))
    nnz_half = n * degree // 2
    src = rng.integers(0, n, size=nnz_half)
    intra = rng.random(nnz_half) < 0.85
    dst = rng.integers(0, n, size=nnz_half)
    c = comm[src[intra]]
    dst[intra] = order[starts[c] + (rng.random(int(intra.sum())) * (starts[c + 1] - starts[c])).astype(np.int64)]
    A = sp.coo_matrix((np.ones(nnz_half), (src, dst)), shape=(n, n))
    A = (A + A.T).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A, comm


def term_counts(m, n, nnz, seed=0, *, dup_frac=0.02, sigma=1.3, zipf_s=1.05, chains=0, chain_len=4):
    """A raw term-count matrix for preprocess_tf (scipy CSC, float64 counts, rows sorted inside columns): terms drawn from a
    Zipf law (exponent `zipf_s`, frequent terms scattered over the rows), document lengths log-normal (`sigma`; a few per cent
    of the documents at 80 entries per document, a quarter at 20, come out shorter than 5 distinct terms, and pruning rare
    terms shortens more of them, so the pruning loop runs for several iterations), and a fraction `dup_frac` of the documents exact copies of other documents.  About `nnz`
    stored entries; seeded.
    chains > 0 replaces the last chains * (2 chain_len + 1) documents by pruning chains for the default thresholds (a document
    with 5 terms dropped, 3 occurrences per term): a 4-term document holds one of 3 occurrences of a chain term, whose
    loss in the next iteration shortens the next document of the chain to 4 terms, and so on: each chain link is one more
    iteration of the loop.  The chain terms are the rarest `chains * chain_len` Zipf ranks, kept out of the other documents."""
    rng = np.random.default_rng(seed)
    lens = rng.lognormal(mean=0.0, sigma=sigma, size=n)
    lens = np.maximum(1, np.round(lens * (1.35 * nnz / lens.sum()))).astype(np.int64)      # repeated terms collapse into counts
    p = 1.0 / np.arange(1, m + 1, dtype=np.float64) ** zipf_s
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    perm = rng.permutation(m).astype(np.int64)
    ndup = int(round(dup_frac * n))
    dup_cols = np.sort(rng.choice(n, size=ndup, replace=False)) if ndup else np.zeros(0, dtype=np.int64)
    lens[dup_cols] = 0
    total = int(lens.sum())
    reserved = chains * chain_len
    terms = perm[np.minimum(np.searchsorted(cdf, rng.random(total), side="right"), m - 1 - reserved)]
    docs = np.repeat(np.arange(n, dtype=np.int64), lens)
    key, counts = np.unique(docs * m + terms, return_counts=True)          # sorted by (doc, term): CSC order
    col = key // m
    row = key % m
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=cp[1:])
    if ndup:
        # each duplicate copies a random non-duplicate document
        src_pool = np.setdiff1d(np.arange(n), dup_cols)
        src = rng.choice(src_pool, size=ndup)
        seg_len = np.diff(cp)
        seg_len[dup_cols] = seg_len[src]
        cp2 = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(seg_len, out=cp2[1:])
        srcmap = np.arange(n)
        srcmap[dup_cols] = src
        owner = np.repeat(np.arange(n), seg_len)
        pos = np.arange(cp2[-1]) - cp2[owner] + cp[srcmap[owner]]
        row, counts, cp = row[pos], counts[pos], cp2
    if chains:
        L = chain_len
        k0 = n - chains * (2 * L + 1)
        cols = []
        for k in range(chains):
            u = perm[m - reserved + k * L: m - reserved + (k + 1) * L]
            common = lambda cnt: list(perm[rng.choice(200, size=cnt, replace=False)])
            cols.append(common(3) + [u[0]])                                 # short from the start
            for j in range(L):                                              # 3 common terms + u[j] (+ u[j + 1])
                cols.append(common(4 if j == L - 1 else 3) + [u[j]] + ([u[j + 1]] if j + 1 < L else []))
            for j in range(L):                                              # a long document holds the third occurrence
                cols.append(common(30) + [u[j]])
        lens_c = np.array([len(c) for c in cols], dtype=np.int64)
        order = [np.argsort(c) for c in cols]
        row = np.concatenate([row[:cp[k0]]] + [np.asarray(c, dtype=np.int64)[o] for c, o in zip(cols, order)])
        counts = np.concatenate([counts[:cp[k0]], np.ones(int(lens_c.sum()), dtype=counts.dtype)])
        cp = np.concatenate([cp[:k0 + 1], cp[k0] + np.cumsum(lens_c)])
    return sp.csc_matrix((counts.astype(np.float64), row.astype(np.int32), cp), shape=(m, n))

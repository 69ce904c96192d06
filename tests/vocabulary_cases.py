"""Vocabulary.apply restated in numpy, and the corpora of the vocabulary tests.

``restate_apply`` is built on ``preprocess_cases.counts_of`` and the scoring lines of ``preprocess_cases.restate``: the counts
of the fit's input conversion, the stable row sort, the entries of pruned terms removed and the rest renumbered in order,
``(1 + log(count)) * idf[row]`` with the column's squares summed in entry order, NaN written as the x86 default NaN.
"""
import functools

import numpy as np

import preprocess_cases as pc

PRUNED = 0xFFFFFFFF

# (m, n, per, seed): synthetic.term_counts(m, n, n * per, seed, dup_frac=0.05), fitted with the default options on the first
# 2n // 3 columns and applied to the rest
CORPORA = [(2000, 600, 12, 1), (5000, 3000, 20, 3), (300, 130, 8, 4), (30000, 20000, 12, 5)]
# what the restatement gives on them: surviving terms, fit documents, new documents, empty new documents, new documents with
# fewer than 5 survivors, new columns of at least 65 entries, iterations of the fit
EXPECTED = {(2000, 600, 12, 1): (311, 226, 200, 1, 83, 5, 2), (5000, 3000, 20, 3): (2066, 1416, 1000, 5, 285, 54, 2),
            (300, 130, 8, 4): (52, 28, 44, 5, 30, 0, 2), (30000, 20000, 12, 5): (7051, 7558, 6667, 113, 2863, 159, 3)}


def vocab_of(ref, height_in, boolean_mode=0):
    """the vocabulary of a restated fit (preprocess_cases.restate): its terms and the idf of its final matrix"""
    df = np.bincount(ref["rows"].astype(np.int64), minlength=ref["height"])
    with np.errstate(divide="ignore", invalid="ignore"):
        idf = np.log(float(ref["width"]) / df.astype(np.float64))
    return dict(term=ref["term"].astype(np.uint32), idf=idf, height_in=int(height_in), boolean_mode=int(boolean_mode))


def old_to_new(vocab):
    out = np.full(vocab["height_in"], PRUNED, dtype=np.int64)
    out[vocab["term"].astype(np.int64)] = np.arange(vocab["term"].size)
    return out


def restate_apply(vocab, cp, rows, data, min_terms=0, boolean_mode=-1):
    """dict(ok, term, doc, cp, rows, counts, scores, height, width, survivors); ok False (with width and survivors, the
    sizes before the drop) when every column was dropped.  survivors: entries in surviving terms per INPUT column."""
    cp = np.asarray(cp, dtype=np.int64).copy()
    cp -= cp[0]
    w_in = cp.size - 1
    rows = np.asarray(rows, dtype=np.int64)[: cp[-1]].copy()
    bm = vocab["boolean_mode"] if boolean_mode == -1 else boolean_mode
    counts = pc.counts_of(np.asarray(data)[: cp[-1]], bm)
    # SortRows: by row inside each column (stable; the identity on a column that arrives sorted)
    col = pc._col_of(cp)
    order = np.lexsort((rows, col))
    rows, counts = rows[order], counts[order]
    # entries of pruned terms leave, the others are renumbered in place
    new_row = old_to_new(vocab)[rows]
    alive = new_row != PRUNED
    survivors = np.bincount(col[alive], minlength=w_in)
    keep_c = survivors >= min_terms
    h = int(vocab["term"].size)
    if not keep_c.any():
        return dict(ok=False, height=h, width=w_in, nnz=int(survivors.sum()), survivors=survivors)
    ek = alive & keep_c[col]
    rows, counts = new_row[ek], counts[ek]
    doc = np.flatnonzero(keep_c)
    w = doc.size
    cp = np.zeros(w + 1, dtype=np.int64)
    np.cumsum(survivors[keep_c], out=cp[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 1.0 + np.log(counts.astype(np.float64))
        s = s * vocab["idf"][rows]
        col = pc._col_of(cp)
        sq = s * s
        nonempty = np.diff(cp) > 0
        sums = np.zeros(w)
        if rows.size:
            sums[nonempty] = np.add.reduceat(sq, cp[:-1][nonempty])
        D = 1.0 / np.sqrt(sums)
        s = s * D[col]
    s[np.isnan(s)] = pc.X86_NAN
    return dict(ok=True, term=vocab["term"], doc=doc.astype(np.uint32), cp=cp.astype(np.uint32), rows=rows.astype(np.uint32),
                counts=counts, scores=s, height=h, width=w, survivors=survivors)


def split(cp, rows, data, nfit):
    """the CSC arrays of the first nfit columns and of the rest"""
    cp = np.asarray(cp, dtype=np.int64)
    e = cp[nfit]
    return (cp[: nfit + 1].copy(), rows[:e], data[:e]), (cp[nfit:] - e, rows[e:], data[e:])


@functools.lru_cache(maxsize=None)
def corpus(m, n, per, seed):
    """dict(m, nfit, fit=(cp, rows, data), new=(cp, rows, data), ref=the restated fit, vocab)"""
    from smallk_amd.synthetic import term_counts
    A = term_counts(m, n, n * per, seed, dup_frac=0.05)
    nfit = 2 * n // 3
    fit, new = split(A.indptr, A.indices.astype(np.int64), A.data.astype(np.float64), nfit)
    ref = pc.restate(m, nfit, *fit)
    return dict(m=m, nfit=nfit, fit=fit, new=new, ref=ref, vocab=vocab_of(ref, m) if ref["ok"] else None)


@functools.lru_cache(maxsize=None)
def messy_corpus(seed=9, m=1500, n=500, per=14):
    """fractional and negative values (counts 0 among them) and rows that are not sorted inside some columns, the way
    test_gpu_preprocess._corpus makes them for seed % 3 == 0 and seed % 4 == 1; default fit options on the whole matrix"""
    from smallk_amd.synthetic import term_counts
    rng = np.random.default_rng(seed)
    A = term_counts(m, n, n * per, seed, dup_frac=0.05)
    cp, rows, data = A.indptr.astype(np.int64), A.indices.astype(np.int64).copy(), A.data.astype(np.float64)
    data = data + rng.uniform(-2.5, 0.9, size=data.size) * (rng.random(data.size) < 0.2)
    for c in rng.choice(n, size=min(n, 200), replace=False):
        s, e = cp[c], cp[c + 1]
        p = rng.permutation(e - s)
        rows[s:e], data[s:e] = rows[s:e][p], data[s:e][p]
    ref = pc.restate(m, n, cp, rows, data)
    return dict(m=m, nfit=n, fit=(cp, rows, data), new=None, ref=ref, vocab=vocab_of(ref, m))


@functools.lru_cache(maxsize=None)
def long_corpus(seed=6, m=4000, n=300, per=14, lengths=(800, 1100, 1500)):
    """a fit whose input holds documents of 800, 1100 and 1500 distinct terms (first, middle and last column), so that columns
    of more than 768 entries survive the fit: the fill pass keeps 4 x 64 entries in flight per load stage, three stages deep"""
    from smallk_amd.synthetic import term_counts
    rng = np.random.default_rng(seed)
    A = term_counts(m, n, n * per, seed, dup_frac=0.05)
    cp, rows, data = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)
    cols = [(rows[cp[j]:cp[j + 1]], data[cp[j]:cp[j + 1]]) for j in range(n)]
    for at, length in zip((0, n // 2, n - 1), lengths):
        cols[at] = (np.sort(rng.choice(m, size=length, replace=False)), rng.integers(1, 5, size=length).astype(np.float64))
    cp, rows, data = pc._csc(m, n, cols)
    ref = pc.restate(m, n, cp, rows, data)
    return dict(m=m, nfit=n, fit=(cp, rows, data), new=None, ref=ref, vocab=vocab_of(ref, m))


SUPER = 256                                     # entries a wave of the fill pass loads per stage
SUPER_LENGTHS = (256, 257, 512, 513, 768, 769, 1024, 1025, 1300)
SUPER_H_IN = 2 * 1300


def superchunk_case(seed=8):
    """(vocab, cols): even terms survive, odd ones are pruned; the entry at position i of a column is term 2i or 2i + 1, at
    random, except around every multiple of 256, where positions e - 2 .. e + 1 are kept, pruned, pruned, kept in the columns
    of even index and pruned, kept, kept, pruned in the others.  One column per length of SUPER_LENGTHS, then one of 1025
    entries that all survive and one of 1025 that are all pruned."""
    rng = np.random.default_rng(seed)
    term = np.arange(0, SUPER_H_IN, 2, dtype=np.uint32)
    vocab = dict(term=term, idf=rng.uniform(0.2, 3.0, size=term.size), height_in=SUPER_H_IN, boolean_mode=0)
    cols = []
    for j, length in enumerate(SUPER_LENGTHS):
        odd = rng.integers(0, 2, size=length)
        for e in range(SUPER, length + 2, SUPER):
            for off, b in zip((-2, -1, 0, 1), (0, 1, 1, 0)):
                if 0 <= e + off < length:
                    odd[e + off] = b ^ (j & 1)
        cols.append((2 * np.arange(length) + odd, rng.integers(1, 6, size=length).astype(np.float64)))
    cols.append((2 * np.arange(1025), rng.integers(1, 6, size=1025).astype(np.float64)))
    cols.append((2 * np.arange(1025) + 1, rng.integers(1, 6, size=1025).astype(np.float64)))
    return vocab, cols


def stats(c):
    """the figures of EXPECTED for a corpus, plus the out-of-vocabulary fraction and the longest new column"""
    cp, rows, data = c["new"]
    out = restate_apply(c["vocab"], cp, rows, data, 0)
    lens = np.diff(cp)
    surv = out["survivors"]
    return dict(terms=c["ref"]["height"], fit_docs=c["ref"]["width"], new_docs=cp.size - 1, empty=int((surv == 0).sum()),
                short=int((surv < 5).sum()), long_cols=int((lens >= 65).sum()), iterations=len(c["ref"]["log"]),
                oov=1.0 - surv.sum() / max(1, int(cp[-1])), longest=int(lens.max()))


def csc(cols):
    """list of (rows, values) per column -> (cp, rows, data)"""
    return pc._csc(0, len(cols), cols)

"""Vocabulary.apply at size: new documents drawn like tools/preprocess_rate.py's corpus, scored against a vocabulary fitted on
that corpus.  Reports the input upload and the device phase separately (as smk_preprocess_result_timing gives them), the
minimum bytes of the passes against 8 TB/s, the device entry on arrays that are already in GPU memory, and the only route there
was before: download term_indices, select and renumber the rows with scipy, tf-idf with numpy on the host, SparseMatrix(...).

    python tools/vocabulary_rate.py [--docs 1000000] [--terms 1048576] [--nnz 100000000] [--new-docs 200000]
                                    [--new-nnz 20000000] [--reps 5] [--out profiles/vocabulary_rate.txt]
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

HBM = 8.0e12


def host_route(smk, fit, idf, width_in, cp, rows, data, min_terms):
    """what a caller had to do without the vocabulary: (seconds by step, the resident matrix)"""
    import scipy.sparse as sp
    from smallk_amd import _lib as L
    t = [time.perf_counter()]
    term = np.zeros(fit.height, dtype=np.uint32)                        # term_indices alone
    L.check(L.lib().smk_preprocess_result_download(fit._h, term.ctypes.data_as(C.POINTER(C.c_uint)), None, None, None, None),
            "smk_preprocess_result_download")
    t.append(time.perf_counter())
    A = sp.csc_matrix((np.trunc(np.maximum(data, 0.0)), rows, cp), shape=(width_in, cp.size - 1))
    R = A[term.astype(np.int64), :].tocsc()                             # surviving rows, renumbered
    R.sort_indices()
    keep = np.diff(R.indptr) >= min_terms
    R = R[:, keep]
    t.append(time.perf_counter())
    s = (1.0 + np.log(R.data)) * idf[R.indices]
    lens = np.diff(R.indptr)
    sums = np.add.reduceat(s * s, R.indptr[:-1][lens > 0])
    D = np.zeros(R.shape[1])
    D[lens > 0] = 1.0 / np.sqrt(sums)
    s = s * np.repeat(D, lens)
    t.append(time.perf_counter())
    M = smk.SparseMatrix(s, R.indices, R.indptr, R.shape)
    t.append(time.perf_counter())
    return np.diff(t), M, (R.indptr, R.indices, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--terms", type=int, default=1 << 20)
    ap.add_argument("--nnz", type=int, default=100000000)
    ap.add_argument("--new-docs", type=int, default=200000)
    ap.add_argument("--new-nnz", type=int, default=20000000)
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--dup-frac", type=float, default=0.02)
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--min-terms", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    import torch
    import smallk_amd
    from smallk_amd.preprocess import preprocess
    from smallk_amd.synthetic import term_counts
    smallk_amd.initialize(0)
    t = time.time()
    A = term_counts(a.terms, a.docs, a.nnz, 1, dup_frac=a.dup_frac, sigma=a.sigma, chains=a.chains)
    fit = preprocess(a.terms, A.shape[1], A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data)
    say(f"fit: {A.shape[0]} terms x {A.shape[1]} documents, {A.nnz} entries (term_counts seed 1, sigma {a.sigma}, dup_frac "
        f"{a.dup_frac}, chains {a.chains}) -> {fit.height} x {fit.width}, {fit.nnz} entries in {fit.iterations} iterations "
        f"(corpus and fit in {time.time() - t:.1f} s)")
    del A
    V = fit.vocabulary()
    B = term_counts(a.terms, a.new_docs, a.new_nnz, 2, dup_frac=a.dup_frac, sigma=a.sigma)
    cp, rows, data = B.indptr.astype(np.uint32), B.indices.astype(np.uint32), B.data
    width, nnz = cp.size - 1, rows.size
    del B

    res = V.apply(cp, rows, data, width, min_terms=a.min_terms)         # warm-up
    say(f"new documents: {a.terms} terms x {width} documents, {nnz} entries (seed 2) -> {res.width} documents, {res.nnz} entries "
        f"in the vocabulary ({100.0 * (1 - res.nnz / nnz):.1f} % out of vocabulary), min_terms {a.min_terms}")
    up, dev, call = [], [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        r = V.apply(cp, rows, data, width, min_terms=a.min_terms)
        call.append((time.perf_counter() - t) * 1e3)
        up.append(r.upload_ms)
        dev.append(r.device_ms)
        r.close()
    up, dev, call = np.array(up), np.array(dev), np.array(call)
    say(f"smk_vocabulary_apply over {a.reps} runs after a warm-up: upload (the input copies) {np.median(up):.2f} ms (min "
        f"{up.min():.2f}, max {up.max():.2f}); device phase {np.median(dev):.2f} ms (min {dev.min():.2f}, max {dev.max():.2f}); the "
        f"whole call {np.median(call):.2f} ms (min {call.min():.2f}, max {call.max():.2f}: also the checks of the input and the "
        f"allocations)")
    passes = [("convert: rows + values in, pairs out", (4 + 8 + 8) * nnz),
              ("count: pairs in, one gathered map word per entry", (8 + 4) * nnz),
              ("fill and score: pairs in, a map word per entry; per survivor an idf, pair and score out, score in and out",
               (8 + 4) * nnz + (8 + 8 + 8 + 8 + 8) * res.nnz)]
    total = sum(b for _, b in passes)
    say("minimum bytes per pass (the two passes of the vocabulary: "
        f"{(passes[1][1] + passes[2][1]) / nnz:.1f} bytes per input entry here):")
    for name, b in passes:
        say(f"  {name:<100s} {b / 1e9:7.3f} GB  ({b / HBM * 1e3:.3f} ms at 8 TB/s)")
    say(f"  together: {total / 1e9:.3f} GB = {total / HBM * 1e3:.3f} ms at 8 TB/s; measured device phase {np.median(dev):.2f} ms = "
        f"{total / (np.median(dev) * 1e-3) / HBM * 100:.1f} % of 8 TB/s")

    d = torch.device("cuda", 0)
    tcp, trows = (torch.from_numpy(x.astype(np.int32)).to(d) for x in (cp, rows))
    tdata = torch.from_numpy(data).to(d)
    dd = []
    rd = V.apply(tcp, trows, tdata, min_terms=a.min_terms)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(rd.download(), res.download()))
    for _ in range(a.reps):
        r = V.apply(tcp, trows, tdata, min_terms=a.min_terms)
        dd.append(r.device_ms)
        r.close()
    dd = np.array(dd)
    say(f"smk_vocabulary_apply_device on the same arrays in GPU memory (int32, fp64): {np.median(dd):.2f} ms (min {dd.min():.2f}, max "
        f"{dd.max():.2f}), the index check included; result {'identical to' if same else 'DIFFERENT from'} the host entry's")
    del tcp, trows, tdata

    idf = V.idf
    steps, M, (hcp, hrows, hs) = host_route(smallk_amd, fit, idf, a.terms, cp, rows, data, a.min_terms)      # warm-up
    _, _, dcp, drows, ds = res.download()
    agree = np.array_equal(hcp, dcp) and np.array_equal(hrows, drows) and np.allclose(hs, ds, rtol=1e-13, atol=0)
    M.close()
    runs = []
    for _ in range(a.reps):
        steps, M, _ = host_route(smallk_amd, fit, idf, a.terms, cp, rows, data, a.min_terms)
        M.close()
        runs.append(steps * 1e3)
    runs = np.array(runs)
    tot = runs.sum(1)
    med = np.median(runs, 0)
    say(f"host route over {a.reps} runs after a warm-up: {np.median(tot):.0f} ms (min {tot.min():.0f}, max {tot.max():.0f}) = download "
        f"{med[0]:.0f} + scipy row selection {med[1]:.0f} + numpy tf-idf {med[2]:.0f} + SparseMatrix(...) {med[3]:.0f} ms; its "
        f"matrix {'agrees with' if agree else 'DIFFERS from'} the device's (integer counts, rows sorted)")
    t = time.perf_counter()
    M = res.matrix()
    say(f"device route to the same resident matrix: apply {np.median(call):.2f} ms + PreprocessResult.matrix() "
        f"{(time.perf_counter() - t) * 1e3:.2f} ms")
    M.close()
    if not (same and agree):
        sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

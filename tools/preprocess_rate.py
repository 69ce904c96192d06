"""preprocess_tf on the device at size: iterations and sizes, the time of smk_preprocess split into the input upload and the
device phase (uploaded input -> resident result), the minimum bytes of each pass against 8 TB/s, a structure check against
the numpy restatement, and the command line tool's split into load, preprocessing and write.

    python tools/preprocess_rate.py [--docs 1000000] [--terms 1048576] [--nnz 100000000] [--reps 5] [--no-check]
                                    [--cli-nnz 19500000] [--out profiles/preprocess_rate.txt]

The kernel table comes from a separate run: rocprofv3 --kernel-trace --stats -- python tools/preprocess_rate.py --reps 1
--no-check --cli-nnz 0.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12


def pass_bytes(nnz0, w0, h0, log):
    """minimum bytes of each pass (entries are 8-byte (row, count) pairs, offsets and flags 4 bytes)"""
    rows = [("upload (host -> device): rows 4 + values 8 per entry, offsets", 12 * nnz0 + 4 * (w0 + 1))]
    dev = [("convert: rows + values in, pairs out", (4 + 8 + 8) * nnz0), ("row statistics: pairs in", 8 * nnz0)]
    h, w, n = h0, w0, nnz0
    for i, (h1, w1, n1) in enumerate(log):
        if h1 != h:
            dev.append((f"[{i + 1}] row compaction: pairs in twice, kept pairs out", 16 * n + 8 * n1))
        dev.append((f"[{i + 1}] column length test + hash: pairs in once", 8 * n1))
        if w1 != w:
            dev.append((f"[{i + 1}] column compaction: kept pairs out, in", 16 * n1))
        h, w, n = h1, w1, n1
    dev.append(("scores: pairs in, scores out (two sweeps)", (8 + 8 + 8 + 8) * n))
    return rows, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--terms", type=int, default=1 << 20)
    ap.add_argument("--nnz", type=int, default=100000000)
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--dup-frac", type=float, default=0.02)
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--cli-nnz", type=int, default=19500000)      # drawn: ~1.6e7 entries written after collapse and pruning
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    import smallk_amd
    from smallk_amd.preprocess import preprocess
    from smallk_amd.synthetic import term_counts
    smallk_amd.initialize(0)
    t = time.time()
    A = term_counts(a.terms, a.docs, a.nnz, 1, dup_frac=a.dup_frac, sigma=a.sigma, chains=a.chains)
    say(f"corpus: {A.shape[0]} terms x {A.shape[1]} documents, {A.nnz} entries (term_counts seed 1, sigma {a.sigma}, "
        f"dup_frac {a.dup_frac}, chains {a.chains}; generated in {time.time() - t:.1f} s)")
    cp, rows, data = A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data
    del A
    up, dev, call = [], [], []
    res = preprocess(a.terms, len(cp) - 1, cp, rows, data)          # warm-up
    log = res.log
    for _ in range(a.reps):
        t = time.perf_counter()
        r = preprocess(a.terms, len(cp) - 1, cp, rows, data)
        call.append((time.perf_counter() - t) * 1e3)
        up.append(r.upload_ms)
        dev.append(r.device_ms)
        assert r.log == log
        r.close()
    say(f"iterations: {len(log)}")
    for i, (h, w, n) in enumerate(log):
        say(f"\t[{i + 1}] height: {h}, width: {w}, nonzeros: {n}")
    up, dev, call = np.array(up), np.array(dev), np.array(call)
    say(f"smk_preprocess over {a.reps} runs after a warm-up: upload (the input copies) {np.median(up):.2f} ms (min {up.min():.2f}, "
        f"max {up.max():.2f}); device phase {np.median(dev):.2f} ms (min {dev.min():.2f}, max {dev.max():.2f}); the whole call "
        f"{np.median(call):.2f} ms (min {call.min():.2f}, max {call.max():.2f}: also the checks of the input, the offset "
        f"rebasing and the allocation of the working set)")
    up_rows, dev_rows = pass_bytes(len(rows), len(cp) - 1, a.terms, log)
    total = sum(b for _, b in dev_rows)
    say("minimum bytes per pass:")
    for name, b in up_rows:
        say(f"  {name:<58s} {b / 1e9:8.3f} GB  -> {b / 1e9 / (np.median(up) * 1e-3):.1f} GB/s measured")
    for name, b in dev_rows:
        say(f"  {name:<58s} {b / 1e9:8.3f} GB  ({b / HBM * 1e3:.3f} ms at 8 TB/s)")
    say(f"  device passes together: {total / 1e9:.3f} GB = {total / HBM * 1e3:.3f} ms at 8 TB/s; measured device phase "
        f"{np.median(dev):.2f} ms = {total / (np.median(dev) * 1e-3) / HBM * 100:.1f} % of 8 TB/s")

    if not a.no_check:
        import preprocess_cases as pc
        t = time.time()
        ref = pc.restate(a.terms, len(cp) - 1, cp, rows, data)
        term, doc, rcp, rrows, _ = res.download()
        ok = (ref["log"] == log and np.array_equal(term, ref["term"]) and np.array_equal(doc, ref["doc"])
              and np.array_equal(rcp, ref["cp"]) and np.array_equal(rrows, ref["rows"]))
        say(f"structure against the restatement: {'identical' if ok else 'DIFFERENT'} ({time.time() - t:.1f} s)")
        if not ok:
            sys.exit(1)
    res.close()

    if a.cli_nnz > 0:
        import preprocess_cases as pc
        docs = max(1, a.cli_nnz // 100)
        B = term_counts(a.terms, docs, a.cli_nnz, 2, dup_frac=a.dup_frac, sigma=a.sigma, chains=a.chains // 10)
        with tempfile.TemporaryDirectory() as tmp:
            indir, outdir = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            os.makedirs(outdir)
            pc.write_input_dir(indir, B.shape[0], B.shape[1], B.indptr, B.indices, B.data)
            tool = os.path.join(ROOT, "smallk_amd", "bin", "preprocess_tf")
            p = subprocess.run([tool, "--indir", indir, "--outdir", outdir], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr
            grab = lambda pat: re.search(pat + r": (\S+)s\.", p.stdout).group(1)
            load, proc = grab("Input file load time"), grab("Processing time")
            written = int(re.search(r"New nonzero count: (\d+)", p.stdout).group(1))
            write, strings = grab("Output file write time"), grab(r"Dictionary \+ documents write time")
            mb = os.path.getsize(os.path.join(outdir, "reduced_matrix.mtx")) / 1e6
            say(f"preprocess_tf on {B.shape[0]} x {B.shape[1]}, {B.nnz} input entries: load {load} s, preprocessing {proc} s, "
                f"write reduced_matrix.mtx {write} s ({written} entries, {mb:.0f} MB), dictionary + documents {strings} s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

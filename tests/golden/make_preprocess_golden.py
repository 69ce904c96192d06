"""Records the reference preprocess_tf on the corpora of tests/preprocess_cases.py into ref_preprocess_results.npz.

    python tests/golden/make_preprocess_golden.py --ref-bin PATH

PATH is the reference tool, built outside this repository from the smallk sources (standard library only) as a release
build (-DNDEBUG: with assertions on, the tool stops at `assert(sum_sq > 0.0)`, preprocess.cpp:219, on a column whose sum of
squares is NaN or 0 -- the idf = 0 case after a run that stopped at max_iter), with SRC the top of the smallk source tree:

    g++ -std=c++11 -O2 -DNDEBUG -ISRC/common/include -ISRC/preprocessor/include -o preprocess_tf SRC/preprocessor/src/{main,command_line,preprocess}.cpp SRC/common/src/{term_frequency_matrix,spooky_v2,xxhash,matrix_market_file,utils,constants,system_posix}.cpp

For every case the recorder keeps the input, the options, the tool's "[i] height: ..." lines, the three output files at
--precision 4 and the matrix at --precision 17 (or, for a case where every column is pruned, that no file was written).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import preprocess_cases as pc  # noqa: E402


def run(ref_bin, indir, outdir, opts, precision):
    os.makedirs(outdir, exist_ok=True)
    cmd = [ref_bin, "--indir", indir, "--outdir", outdir, "--maxiter", str(opts["max_iter"]),
           "--docs_per_term", str(opts["docs_per_term"]), "--terms_per_doc", str(opts["terms_per_doc"]),
           "--boolean_mode", str(opts["boolean_mode"]), "--precision", str(precision)]
    p = subprocess.run(cmd, capture_output=True, text=True, check=True)
    log = [ln for ln in p.stdout.split("\n") if ln.startswith("\t[")]
    files = {}
    for name in ("reduced_matrix.mtx", "reduced_dictionary.txt", "reduced_documents.txt"):
        path = os.path.join(outdir, name)
        files[name] = open(path).read() if os.path.exists(path) else None
    return log, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_preprocess_results.npz"))
    a = ap.parse_args()
    arrays = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (h, w, cp, rows, data, opts) in pc.fixture_cases().items():
            indir = os.path.join(tmp, name, "in")
            pc.write_input_dir(indir, h, w, cp, rows, data)
            log, f4 = run(a.ref_bin, indir, os.path.join(tmp, name, "p4"), opts, 4)
            _, f17 = run(a.ref_bin, indir, os.path.join(tmp, name, "p17"), opts, 17)
            ok = f4["reduced_matrix.mtx"] is not None
            b = lambda s: np.frombuffer((s or "").encode(), dtype=np.uint8)
            arrays.update({f"{name}/shape": np.array([h, w], dtype=np.int64), f"{name}/cp": np.asarray(cp, dtype=np.int64),
                           f"{name}/rows": np.asarray(rows, dtype=np.int64), f"{name}/data": np.asarray(data, dtype=np.float64),
                           f"{name}/opts": np.array([opts["max_iter"], opts["docs_per_term"], opts["terms_per_doc"],
                                                     opts["boolean_mode"]], dtype=np.int64),
                           f"{name}/ok": np.array([ok]), f"{name}/log": b("\n".join(log)),
                           f"{name}/mtx4": b(f4["reduced_matrix.mtx"]), f"{name}/dict4": b(f4["reduced_dictionary.txt"]),
                           f"{name}/docs4": b(f4["reduced_documents.txt"]), f"{name}/mtx17": b(f17["reduced_matrix.mtx"])})
            names.append(name)
            print(f"{name}: {h} x {w}, {int(cp[-1])} entries, {len(log)} iterations, ok={ok}")
    arrays["names"] = np.array(names)
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()

"""preprocess_tf on the MI355X: the reference tool's recorded outputs through the C ABI, the Python class and the command
line tool; seeded corpora (one of them at 2e7 entries) against the numpy restatement; run-to-run bits; the handoff of the
resident result to the clustering."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import preprocess_cases as pc
from test_preprocess_cpu import GOLD, PRINTED, assert_scores_match, reference_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "smallk_amd", "bin", "preprocess_tf")


@pytest.fixture(scope="module")
def smk():
    import smallk_amd
    smallk_amd.initialize(0)
    return smallk_amd


def device_run(smk, h, w, cp, rows, data, **opts):
    from smallk_amd.preprocess import preprocess
    return preprocess(h, w, cp, rows, data, **opts)


def assert_matches_restatement(res, ref):
    assert res.ok == ref["ok"]
    assert res.log == ref["log"]
    if not ref["ok"]:
        return
    term, doc, cp, rows, scores = res.download()
    assert np.array_equal(term, ref["term"])
    assert np.array_equal(doc, ref["doc"])
    assert np.array_equal(cp, ref["cp"])
    assert np.array_equal(rows, ref["rows"])
    assert_scores_match(scores, ref["scores"])


@pytest.mark.parametrize("name", sorted(GOLD))
def test_fixture_through_abi(smk, name):
    g = GOLD[name]
    res = device_run(smk, g["height"], g["width"], g["cp"], g["rows"], g["data"], **g["opts"])
    assert pc.log_lines(res.log) == g["log"]
    assert res.ok == g["ok"]
    if not g["ok"]:
        return
    term, doc, cp, rows, scores = res.download()
    rterm, rdoc, rcp, rrows, rscores = reference_arrays(g)
    assert np.array_equal(term, rterm) and np.array_equal(doc, rdoc)
    assert np.array_equal(cp, rcp) and np.array_equal(rows, rrows)
    assert_scores_match(scores, rscores, atol=PRINTED)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_fixture_through_python_class(smk, name, tmp_path, capsys):
    g = GOLD[name]
    p = smk.Preprocessor()
    p.load_matrix(height=g["height"], width=g["width"], nz=int(g["cp"][-1]), buffer=g["data"].tolist(),
                  row_indices=g["rows"].tolist(), col_offsets=g["cp"].tolist())
    p.load_dictionary(dictionary=[f"term{i}" for i in range(g["height"])])
    p.load_documents(documents=[f"doc{i}" for i in range(g["width"])])
    o = g["opts"]
    out = p.preprocess(maxiter=o["max_iter"], docsperterm=o["docs_per_term"], termsperdoc=o["terms_per_doc"],
                       boolean_mode=o["boolean_mode"])
    assert out is None
    if not g["ok"]:
        assert "ERROR: preprocess()" in capsys.readouterr().out
        return
    assert p.get_reduced_dictionary() == [t for t in g["dict4"].split("\n") if t]
    assert p.get_reduced_documents() == [t for t in g["docs4"].split("\n") if t]
    _, _, rcp, rrows, rscores = reference_arrays(g)
    assert p.get_reduced_col_offsets() == rcp.tolist()
    assert p.get_reduced_row_indices() == rrows.tolist()
    assert_scores_match(np.array(p.get_reduced_scores()), rscores, atol=PRINTED)
    p.write_output(str(tmp_path / "m.mtx"), str(tmp_path / "d.txt"), str(tmp_path / "c.txt"))
    assert open(tmp_path / "m.mtx").read() == g["mtx4"]
    assert open(tmp_path / "d.txt").read() == g["dict4"]
    assert open(tmp_path / "c.txt").read() == g["docs4"]


@pytest.mark.parametrize("name", sorted(GOLD))
def test_fixture_through_cli(name, tmp_path):
    g = GOLD[name]
    indir, outdir = tmp_path / "in", tmp_path / "out"
    pc.write_input_dir(str(indir), g["height"], g["width"], g["cp"], g["rows"], g["data"])
    os.makedirs(outdir)
    o = g["opts"]
    p = subprocess.run([TOOL, "--indir", str(indir), "--outdir", str(outdir), "--maxiter", str(o["max_iter"]),
                        "--docs_per_term", str(o["docs_per_term"]), "--terms_per_doc", str(o["terms_per_doc"]),
                        "--boolean_mode", str(o["boolean_mode"])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert [ln for ln in p.stdout.split("\n") if ln.startswith("\t[")] == g["log"]
    if not g["ok"]:
        assert os.listdir(outdir) == []
        assert "no output files will be written" in p.stderr
        return
    assert open(outdir / "reduced_matrix.mtx").read() == g["mtx4"]
    assert open(outdir / "reduced_dictionary.txt").read() == g["dict4"]
    assert open(outdir / "reduced_documents.txt").read() == g["docs4"]


def _corpus(seed):
    from smallk_amd.synthetic import term_counts
    rng = np.random.default_rng(seed)
    n = int(rng.choice([50, 300, 2000, 20000, 100000]))
    m = int(rng.choice([100, 1000, 5000, 30000]))
    per_doc = float(rng.choice([6, 12, 40]))
    A = term_counts(m, n, int(n * per_doc), seed, dup_frac=float(rng.choice([0.0, 0.05, 0.3])))
    opts = dict(max_iter=int(rng.choice([1, 2, 1000])), docs_per_term=int(rng.integers(1, 6)),
                terms_per_doc=int(rng.integers(1, 8)), boolean_mode=int(rng.integers(0, 2)))
    cp, rows, data = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    if seed % 3 == 0:                                   # fractional and negative values (counts 0 among them)
        data = data + rng.uniform(-2.5, 0.9, size=data.size) * (rng.random(data.size) < 0.2)
    if seed % 4 == 1:                                   # rows not sorted inside the columns (ABI input)
        rows = rows.copy()
        data = np.array(data, copy=True)
        for c in rng.choice(n, size=min(n, 500), replace=False):
            s, e = cp[c], cp[c + 1]
            p = rng.permutation(e - s)
            rows[s:e], data[s:e] = rows[s:e][p], data[s:e][p]
    return m, n, cp, rows, data, opts


@pytest.mark.parametrize("seed", range(20))
def test_seeded_corpus_against_restatement(smk, seed):
    m, n, cp, rows, data, opts = _corpus(seed)
    ref = pc.restate(m, n, cp, rows, data, **opts)
    res = device_run(smk, m, n, cp, rows, data, **opts)
    assert_matches_restatement(res, ref)


@pytest.mark.parametrize("survivor", [0, 4])
def test_lone_column_is_unique(smk, survivor):
    m, n, cp, rows, data = pc.lone_column(survivor)
    ref = pc.restate(m, n, cp, rows, data, max_iter=1)
    res = device_run(smk, m, n, cp, rows, data, max_iter=1)
    assert_matches_restatement(res, ref)
    assert res.download()[1].tolist() == [survivor]


def test_two_calls_same_bits(smk):
    m, n, cp, rows, data, opts = _corpus(7)
    a = device_run(smk, m, n, cp, rows, data, **opts).download()
    b = device_run(smk, m, n, cp, rows, data, **opts).download()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_many_identical_documents(smk):
    # 5000 copies of one document among 2000 others: one survivor, the copy with the largest index (O(g) comparisons)
    rng = np.random.default_rng(3)
    base = (np.sort(rng.choice(400, size=20, replace=False)), rng.integers(1, 4, size=20).astype(float))
    cols = []
    for k in range(7000):
        if k % 7 < 5:
            cols.append(base)
        else:
            r = np.sort(rng.choice(400, size=12, replace=False))
            cols.append((r, rng.integers(1, 4, size=12).astype(float)))
    cp, rows, data = pc._csc(400, len(cols), cols)
    ref = pc.restate(400, len(cols), cp, rows, data)
    res = device_run(smk, 400, len(cols), cp, rows, data)
    assert_matches_restatement(res, ref)


def test_handoff_to_clustering(smk):
    from smallk_amd import _lib as L
    from smallk_amd.synthetic import term_counts
    A = term_counts(3000, 2000, 60000, 11, dup_frac=0.05)
    res = device_run(smk, A.shape[0], A.shape[1], A.indptr, A.indices, A.data)
    assert res.ok
    term, doc, rcp, rrows, scores = res.download()
    A1 = res.matrix()
    A2 = smk.SparseMatrix(scores, rrows, rcp, (res.height, res.width))
    for tr, size in ((0, res.width), (1, res.height)):
        got = []
        for A in (A1, A2):
            co = np.zeros(size + 1, dtype=np.uint32)
            ri = np.zeros(res.nnz, dtype=np.uint32)
            va = np.zeros(res.nnz)
            L.check(L.lib().smk_matrix_download_csc(A._h, tr, co.ctypes.data_as(C.POINTER(C.c_uint)),
                                                    ri.ctypes.data_as(C.POINTER(C.c_uint)),
                                                    va.ctypes.data_as(C.POINTER(C.c_double))), "download_csc")
            got.append((co.tobytes(), ri.tobytes(), va.tobytes()))
        assert got[0] == got[1]
    import scipy.sparse as sp
    t1 = smk.hier_nmf2(A1, 4, seed=5, maxterms=5)
    t2 = smk.hier_nmf2(sp.csc_matrix((scores, rrows, rcp), shape=(res.height, res.width)), 4, seed=5, maxterms=5)
    assert np.array_equal(t1.get_assignments(), t2.get_assignments())
    assert t1.node_count == t2.node_count > 1
    for a, b in zip(t1.nodes, t2.nodes):
        assert np.array_equal(a.docs, b.docs)
        assert a.topic_vector.tobytes() == b.topic_vector.tobytes()


def test_at_size_structure(smk):
    from smallk_amd.synthetic import term_counts
    A = term_counts(2 ** 18, 250000, 2 * 10 ** 7, 7, dup_frac=0.02, sigma=1.8)
    ref = pc.restate(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)
    res = device_run(smk, A.shape[0], A.shape[1], A.indptr, A.indices, A.data)
    assert res.log == ref["log"]
    term, doc, cp, rows, scores = res.download()
    assert np.array_equal(term, ref["term"]) and np.array_equal(doc, ref["doc"])
    assert np.array_equal(cp, ref["cp"]) and np.array_equal(rows, ref["rows"])

"""A fitted vocabulary on the MI355X: new documents scored against the numpy restatement (tests/vocabulary_cases.py), a fit's
own documents bit for bit, hand-built shapes around the 64-entry chunk and the 256-entry load stages, the two ways to make a vocabulary, the host and the
device entry, run-to-run bits, the error paths, and the hand-over of the applied matrix to transform."""
import ctypes as C

import numpy as np
import pytest

import preprocess_cases as pc
import vocabulary_cases as vc
from test_preprocess_cpu import assert_scores_match

pytestmark = pytest.mark.gpu

MAX_ITER = 1000
_fits = {}


@pytest.fixture(scope="module")
def smk():
    import smallk_amd
    smallk_amd.initialize(0)
    return smallk_amd


def fit_of(smk, name, c):
    """the device fit of a corpus (default options) and its vocabulary, made once; converged, with terms and documents pruned"""
    if name not in _fits:
        from smallk_amd.preprocess import preprocess
        cp, rows, data = c["fit"]
        res = preprocess(c["m"], c["nfit"], cp, rows, data, max_iter=MAX_ITER)
        assert res.ok and res.iterations < MAX_ITER
        assert res.height < c["m"] and res.width < c["nfit"]                       # the fit pruned terms and documents
        _fits[name] = (res, res.vocabulary())
    return _fits[name]


def assert_non_vacuous(c, key):
    s = vc.stats(c)
    assert s["oov"] > 0 and s["short"] >= 1
    if key[0] != 300:
        assert s["longest"] > 64


def downloaded_matrix(smk, A, width, nnz):
    from smallk_amd import _lib as L
    co = np.zeros(width + 1, dtype=np.uint32)
    ri = np.zeros(nnz, dtype=np.uint32)
    va = np.zeros(nnz)
    up = C.POINTER(C.c_uint)
    L.check(L.lib().smk_matrix_download_csc(A._h, 0, co.ctypes.data_as(up), ri.ctypes.data_as(up), va.ctypes.data_as(C.POINTER(C.c_double))),
            "smk_matrix_download_csc")
    return co, ri, va


def assert_matches(out, ref):
    """an applied result against the restatement: integers exactly, scores as the fit's tests compare them"""
    assert out.ok == ref["ok"]
    assert (out.height, out.width) == (ref["height"], ref["width"])
    assert out.log == [] and out.iterations == 0
    if not ref["ok"]:
        assert out.nnz == ref["nnz"]
        return None
    got = out.download()
    term, doc, cp, rows, scores = got
    assert np.array_equal(term, ref["term"])
    assert np.array_equal(doc, ref["doc"])
    assert np.array_equal(cp, ref["cp"])
    assert np.array_equal(rows, ref["rows"])
    assert_scores_match(scores, ref["scores"])
    nan = np.isnan(scores)
    assert (scores[nan].view(np.uint64) == 0xFFF8000000000000).all()
    return got


@pytest.mark.parametrize("min_terms", [0, 1, 5])
@pytest.mark.parametrize("key", vc.CORPORA)
def test_new_documents_against_restatement(smk, key, min_terms):
    c = vc.corpus(*key)
    assert_non_vacuous(c, key)
    res, V = fit_of(smk, key, c)
    fit_term = res.download()[0]
    assert np.array_equal(fit_term, c["vocab"]["term"])
    cp, rows, data = c["new"]
    ref = vc.restate_apply(c["vocab"], cp, rows, data, min_terms)
    out = V.apply(cp, rows, data, cp.size - 1, min_terms=min_terms)
    term, doc, ocp, orows, scores = assert_matches(out, ref)
    assert np.array_equal(term, fit_term)
    assert out.upload_ms > 0 and out.device_ms > 0
    A = out.matrix()
    co, ri, va = downloaded_matrix(smk, A, out.width, out.nnz)
    assert co.tobytes() == ocp.tobytes() and ri.tobytes() == orows.tobytes() and va.tobytes() == scores.tobytes()
    A.close()


def _assert_own_documents_bitwise(smk, name, c):
    res, V = fit_of(smk, name, c)
    term, doc, fcp, frows, fscores = res.download()
    cp, rows, data = c["fit"]
    out = V.apply(cp, rows, data, c["nfit"], min_terms=0)
    assert out.ok and out.width == c["nfit"]
    _, adoc, acp, arows, ascores = out.download()
    assert np.array_equal(adoc, np.arange(c["nfit"]))
    assert doc.size > 0
    # the fit's columns, gathered out of the applied matrix in one go
    starts, lens = acp[:-1][doc].astype(np.int64), np.diff(acp.astype(np.int64))[doc]
    assert np.array_equal(lens, np.diff(fcp.astype(np.int64)))
    pos = np.repeat(starts - fcp[:-1].astype(np.int64), lens) + np.arange(fcp[-1], dtype=np.int64)
    assert np.array_equal(arows[pos], frows)
    assert np.array_equal(ascores[pos].view(np.uint64), fscores.view(np.uint64))


@pytest.mark.parametrize("key", vc.CORPORA[:2])
def test_fit_documents_reproduce_bit_for_bit(smk, key):
    _assert_own_documents_bitwise(smk, key, vc.corpus(*key))


def test_fit_documents_reproduce_bit_for_bit_unsorted_fractional(smk):
    c = vc.messy_corpus()
    cp, rows, data = c["fit"]
    assert (np.diff(rows)[np.diff(pc._col_of(cp)) == 0] < 0).any() and (data < 0).any() and (c["ref"]["counts"] == 0).any()
    _assert_own_documents_bitwise(smk, "messy", c)


def test_fit_documents_reproduce_bit_for_bit_long_columns(smk):
    # fit columns of more than 768 and more than 1024 entries: every load stage of the fill pass carries live entries
    c = vc.long_corpus()
    lens = np.diff(c["ref"]["cp"].astype(np.int64))
    assert (lens > 3 * vc.SUPER).sum() >= 2 and lens.max() > 4 * vc.SUPER
    _assert_own_documents_bitwise(smk, "long", c)
    res, _ = fit_of(smk, "long", c)
    assert np.array_equal(np.diff(res.download()[2].astype(np.int64)), lens)


# ---- hand-built shapes ------------------------------------------------------------------------------------------------------
# terms 0 .. 199: 60 .. 129, 150 .. 159 and the odd ones from 161 on are pruned; 0 and 199 are kept (199 by hand)
H_IN = 200
PRUNED_TERMS = np.r_[60:130, 150:160, 161:199:2]
KEPT_TERMS = np.setdiff1d(np.arange(H_IN), PRUNED_TERMS)


def _edge_vocab(idf_zero_at=None):
    rng = np.random.default_rng(5)
    idf = rng.uniform(0.2, 3.0, size=KEPT_TERMS.size)
    if idf_zero_at is not None:
        idf[idf_zero_at] = 0.0
    return dict(term=KEPT_TERMS.astype(np.uint32), idf=idf, height_in=H_IN, boolean_mode=0)


def _device_vocab(smk, vocab):
    return smk.Vocabulary(vocab["term"], vocab["idf"], vocab["height_in"], vocab["boolean_mode"])


def _random_column(rng, length):
    r = np.sort(rng.choice(H_IN, size=length, replace=False))
    return r, rng.integers(1, 6, size=length).astype(float)


def _check(smk, vocab, cols, min_terms, V=None):
    cp, rows, data = vc.csc(cols)
    ref = vc.restate_apply(vocab, cp, rows, data, min_terms)
    V = V or _device_vocab(smk, vocab)
    out = V.apply(cp, rows, data, len(cols), min_terms=min_terms)
    assert_matches(out, ref)
    return ref, out


@pytest.mark.parametrize("min_terms", [0, 1])
def test_column_lengths_around_the_chunk(smk, min_terms):
    rng = np.random.default_rng(11)
    vocab = _edge_vocab()
    assert vocab["term"][0] == 0 and vocab["term"][-1] == H_IN - 1
    all_pruned = (PRUNED_TERMS[:40], np.full(40, 2.0))
    ends = (np.array([0, H_IN - 1]), np.array([3.0, 1.0]))                                    # terms 0 and height_in - 1
    # survivors exactly at positions 0 and 64: term 0, then 63 pruned terms, term 130, then two pruned ones
    r = np.r_[0, 60:123, 130, 150, 151]
    assert r.size == 67 and np.isin(r[[0, 64]], KEPT_TERMS).all() and np.isin(np.delete(r, [0, 64]), PRUNED_TERMS).all()
    two = (r, np.arange(1.0, 68.0))
    cols = [all_pruned] + [_random_column(rng, n) for n in (0, 1, 63, 64)] + [two, all_pruned] + \
           [_random_column(rng, n) for n in (65, 128, 129)] + [ends, all_pruned]
    ref, out = _check(smk, vocab, cols, min_terms)
    surv = ref["survivors"]
    assert surv[0] == surv[6] == surv[-1] == 0 and surv[5] == 2 and surv[-2] == 2
    assert ref["width"] == (len(cols) if min_terms == 0 else int((surv >= 1).sum()))
    assert (np.diff(ref["cp"].astype(np.int64)) > 64).any()                                   # a kept column of more than one chunk


@pytest.mark.parametrize("min_terms", [0, 1])
def test_column_lengths_around_the_load_stages(smk, min_terms):
    # the fill pass loads 256 entries per stage, three stages ahead: columns that end at, and one past, 1 .. 4 stages, and one
    # of about five, with a survivor and a pruned entry on both sides of every multiple of 256
    vocab, cols = vc.superchunk_case()
    kept_map = vc.old_to_new(vocab) != vc.PRUNED
    for r, _ in cols[:len(vc.SUPER_LENGTHS)]:
        kept = kept_map[r]
        for e in range(vc.SUPER, len(r) - 1, vc.SUPER):
            assert kept[e - 2] != kept[e - 1] and kept[e] != kept[e + 1]
    ref, out = _check(smk, vocab, cols, min_terms)
    assert [int(x) for x in np.diff(vc.csc(cols)[0])] == list(vc.SUPER_LENGTHS) + [1025, 1025]
    assert ref["survivors"][-2] == 1025 and ref["survivors"][-1] == 0
    assert ref["width"] == len(cols) - (1 if min_terms else 0)
    # the same columns in reverse order and unsorted inside (the sort path), through the device entry's bits as well
    import torch
    rng = np.random.default_rng(9)
    shuffled = []
    for r, v in cols[::-1]:
        p = rng.permutation(len(r))
        shuffled.append((r[p], v[p]))
    ref2, out2 = _check(smk, vocab, shuffled, min_terms)
    assert np.array_equal(ref2["survivors"], ref["survivors"][::-1])
    cp, rows, data = vc.csc(shuffled)
    dev = torch.device("cuda", 0)
    V = _device_vocab(smk, vocab)
    devr = V.apply(torch.from_numpy(cp).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(data).to(dev), min_terms=min_terms)
    assert _bytes(devr) == _bytes(out2)


def test_width_one_and_no_entries(smk):
    rng = np.random.default_rng(12)
    vocab = _edge_vocab()
    V = _device_vocab(smk, vocab)
    _check(smk, vocab, [_random_column(rng, 70)], 1, V)
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    ref, out = _check(smk, vocab, [empty, empty, empty], 0, V)
    assert out.nnz == 0 and out.width == 3 and out.download()[2].tolist() == [0, 0, 0, 0]
    ref, out = _check(smk, vocab, [empty], 0, V)
    assert out.nnz == 0 and out.width == 1


def test_identity_and_one_term_vocabularies(smk):
    rng = np.random.default_rng(13)
    cols = [_random_column(rng, n) for n in (5, 64, 90, 0, 130)]
    ident = dict(term=np.arange(H_IN, dtype=np.uint32), idf=rng.uniform(0.1, 2.0, size=H_IN), height_in=H_IN, boolean_mode=0)
    ref, _ = _check(smk, ident, cols, 0)
    assert np.array_equal(ref["survivors"], [5, 64, 90, 0, 130])
    term = int(cols[1][0][10])
    one = dict(term=np.array([term], dtype=np.uint32), idf=np.array([0.75]), height_in=H_IN, boolean_mode=0)
    for mt in (0, 1):
        ref, out = _check(smk, one, cols, mt)
        assert ref["survivors"].max() == 1 and 1 <= ref["survivors"].sum() < len(cols)
        if mt == 1:
            assert np.abs(out.download()[4] - 1.0).max() <= 2.0 ** -52                         # a one-entry column normalises to 1


def test_idf_zero_and_count_zero(smk):
    rng = np.random.default_rng(14)
    vocab = _edge_vocab(idf_zero_at=3)                                                         # term 3: idf 0
    r1 = np.array([1, 3, 7, 70])
    cols = [(r1, np.array([2.0, 5.0, 1.0, 4.0])),                                              # an idf of 0: that score is 0
            (np.array([2, 5, 9]), np.array([0.0, 3.0, 2.0])),                                  # a count of 0: -inf, the sum inf, D 0
            (np.array([3, 8]), np.array([-1.5, 2.0])),                                         # a count of 0 at idf 0: -inf * 0, all NaN
            _random_column(rng, 66)]
    ref, out = _check(smk, vocab, cols, 0)
    s = out.download()[4]
    cp = ref["cp"]
    assert s[cp[0] + 1] == 0.0 and np.isfinite(s[cp[0]:cp[1]]).all()
    assert np.isnan(s[cp[1]]) and (s[cp[1] + 1:cp[2]] == 0.0).all()
    assert np.isnan(s[cp[2]:cp[3]]).all() and cp[3] - cp[2] == 2
    # boolean mode turns the same input into counts of 1
    cpi, rows, data = vc.csc(cols)
    V = _device_vocab(smk, vocab)
    refb = vc.restate_apply(vocab, cpi, rows, data, 0, boolean_mode=1)
    assert np.isfinite(refb["scores"]).all()
    assert_matches(V.apply(cpi, rows, data, len(cols), boolean_mode=1), refb)


# ---- one vocabulary, two ways; two entries; two runs -------------------------------------------------------------------------
def _bytes(out):
    return tuple(a.tobytes() for a in out.download())


def test_vocabulary_from_result_and_from_arrays_agree(smk, tmp_path):
    key = vc.CORPORA[0]
    c = vc.corpus(*key)
    res, V = fit_of(smk, key, c)
    assert (V.height_in, V.height, V.boolean_mode) == (c["m"], res.height, 0)
    term, idf = V.term_indices, V.idf
    assert np.array_equal(term, res.download()[0])
    assert_scores_match(idf, c["vocab"]["idf"])
    V2 = smk.Vocabulary(term, idf, V.height_in, V.boolean_mode)
    V.save(str(tmp_path / "v.npz"))
    V3 = smk.Vocabulary.load(str(tmp_path / "v.npz"))
    cp, rows, data = c["new"]
    a = _bytes(V.apply(cp, rows, data, cp.size - 1, min_terms=1))
    for other in (V2, V3):
        assert other.term_indices.tobytes() == term.tobytes() and other.idf.tobytes() == idf.tobytes()
        assert _bytes(other.apply(cp, rows, data, cp.size - 1, min_terms=1)) == a
    applied = V.apply(cp, rows, data, cp.size - 1, min_terms=1)
    from smallk_amd import _lib as L
    with pytest.raises(L.SmallkError) as e:                                                    # an applied result keeps no idf
        applied.vocabulary()
    assert e.value.code == L.FAILURE


@pytest.mark.parametrize("idx,val", [("int32", "float64"), ("int64", "float64"), ("int32", "float32"), ("int64", "float32")])
def test_host_and_device_entries_agree(smk, idx, val):
    import torch
    key = vc.CORPORA[0]
    c = vc.corpus(*key)
    _, V = fit_of(smk, key, c)
    cp, rows, data = c["new"]
    assert np.array_equal(data, data.astype(np.float32).astype(np.float64)) and np.array_equal(data, np.floor(data))
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    host = V.apply(cp, rows, data, cp.size - 1, min_terms=1)
    devr = V.apply(t(cp, idx), t(rows, idx), t(data, val), min_terms=1)
    assert _bytes(devr) == _bytes(host)
    assert devr.upload_ms == 0 and devr.device_ms > 0
    if (idx, val) == ("int64", "float64"):
        A = torch.sparse_csc_tensor(t(cp, idx), t(rows, idx), t(data, val), size=(c["m"], cp.size - 1))
        assert _bytes(V.apply(A, min_terms=1)) == _bytes(host)
        import scipy.sparse as sp
        assert _bytes(V.apply(sp.csc_matrix((data, rows, cp), shape=(c["m"], cp.size - 1)), min_terms=1)) == _bytes(host)


def test_device_entry_sorts_and_handles_no_entries(smk):
    import torch
    c = vc.messy_corpus()
    _, V = fit_of(smk, "messy", c)
    cp, rows, data = c["fit"]
    dev = torch.device("cuda", 0)
    host = V.apply(cp, rows, data, cp.size - 1, min_terms=0)
    devr = V.apply(torch.from_numpy(cp).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(data).to(dev), min_terms=0)
    assert _bytes(devr) == _bytes(host)
    none = V.apply(torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                   torch.zeros(0, dtype=torch.float64, device=dev), min_terms=0)
    assert none.ok and (none.width, none.nnz) == (3, 0)


def test_two_applies_same_bits(smk):
    key = vc.CORPORA[1]
    c = vc.corpus(*key)
    _, V = fit_of(smk, key, c)
    cp, rows, data = c["new"]
    assert _bytes(V.apply(cp, rows, data, cp.size - 1)) == _bytes(V.apply(cp, rows, data, cp.size - 1))


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(smk):
    import torch
    from smallk_amd import _lib as L
    vocab = _edge_vocab()
    V = _device_vocab(smk, vocab)
    cp, rows, data = vc.csc([(np.array([1, 2, H_IN]), np.ones(3))])
    with pytest.raises(L.SmallkError) as e:
        V.apply(cp, rows, data, 1)
    assert e.value.code == L.BAD_PARAM and "row index" in str(e.value)
    dev = torch.device("cuda", 0)
    with pytest.raises(L.SmallkError) as e:
        V.apply(torch.from_numpy(cp).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(data).to(dev))
    assert e.value.code == L.BAD_PARAM and "row index" in str(e.value)
    for term in ([3, 3, 5], [3, 2, 5], [1, 2, H_IN]):
        with pytest.raises(L.SmallkError) as e:
            smk.Vocabulary(term, [1.0, 1.0, 1.0], H_IN)
        assert e.value.code == L.BAD_PARAM
    with pytest.raises(L.SmallkError) as e:
        smk.Vocabulary([], [], H_IN)
    assert e.value.code == L.BAD_PARAM
    o = L.ApplyOptions(0, -1)
    h = C.c_void_p()
    co, ri, va = np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.ones(1)
    up = C.POINTER(C.c_uint)
    rc = L.lib().smk_vocabulary_apply(None, C.byref(o), 1, 1, co.ctypes.data_as(up), ri.ctypes.data_as(up),
                                      va.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    assert rc == L.BAD_PARAM and not h.value


def test_failed_fit_has_no_vocabulary(smk):
    from smallk_amd import _lib as L
    from smallk_amd.preprocess import preprocess
    m, n, cp, rows, data = pc._all_pruned()
    res = preprocess(m, n, cp, rows, data)
    assert not res.ok
    with pytest.raises(L.SmallkError) as e:
        res.vocabulary()
    assert e.value.code == L.FAILURE


def test_every_document_dropped(smk):
    key = vc.CORPORA[2]
    c = vc.corpus(*key)
    _, V = fit_of(smk, key, c)
    cp, rows, data = c["new"]
    most = int(vc.restate_apply(c["vocab"], cp, rows, data, 0)["survivors"].max())
    ref = vc.restate_apply(c["vocab"], cp, rows, data, most + 1)
    out = V.apply(cp, rows, data, cp.size - 1, min_terms=most + 1)
    assert not out.ok and not ref["ok"]
    assert (out.height, out.width, out.nnz) == (ref["height"], cp.size - 1, ref["nnz"])
    with pytest.raises(RuntimeError):
        out.download()
    assert V.apply(cp, rows, data, cp.size - 1, min_terms=most).ok


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_applied_matrix_is_the_one_transform_needs(smk):
    import torch
    key = vc.CORPORA[1]
    c = vc.corpus(*key)
    res, V = fit_of(smk, key, c)
    k = 8
    A_fit = res.matrix()
    solver = smk.NmfSolver(A_fit, smk.make_options(res.height, res.width, k, "BPP", min_iter=20, max_iter=20))
    solver.set_factors_uniform(1, 2)
    solver.iterate(20)
    solver.sync()
    W, _ = solver.factors_device(normalize=True)
    solver.close()
    cp, rows, data = c["new"]
    out = V.apply(cp, rows, data, cp.size - 1, min_terms=1)
    ref = vc.restate_apply(c["vocab"], cp, rows, data, 1)
    term, doc, ocp, orows, scores = assert_matches(out, ref)
    A1 = out.matrix()
    A2 = smk.SparseMatrix(scores, ref["rows"], ref["cp"], (ref["height"], ref["width"]))
    H1 = smk.transform(A1, W)
    H2 = smk.transform(A2, W)
    assert tuple(H1.shape) == (k, ref["width"]) and float(H1.sum()) > 0
    assert torch.equal(H1.view(torch.int64), H2.view(torch.int64))
    for A in (A1, A2, A_fit):
        A.close()

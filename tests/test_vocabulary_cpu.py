"""The vocabulary entries without a GPU: the numpy restatement of apply (tests/vocabulary_cases.py) against the restatement of
the fit on the fit's own input, the corpora's figures, the declarations, and the .npz round trip of a saved vocabulary."""
import os
import re

import numpy as np
import pytest

import preprocess_cases as pc
import vocabulary_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITY = {"smk_preprocess_result_vocabulary": 2, "smk_vocabulary_create": 6, "smk_vocabulary_destroy": 1, "smk_vocabulary_sizes": 4,
         "smk_vocabulary_download": 3, "smk_vocabulary_apply": 8, "smk_vocabulary_apply_device": 12}


def test_entries_are_declared_and_bound():
    """header, binding table and shared object agree, argument for argument"""
    import smallk_amd
    header = open(os.path.join(ROOT, "include", "smallk_amd.h")).read()
    lib = smallk_amd._lib.lib()
    for name, arity in ARITY.items():
        decl = re.search(r"\b(?:int|void) %s\(([^;]*?)\);" % name, header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity, (name, decl.group(1))
        res, args = smallk_amd._lib.SYMBOLS[name]
        assert len(args) == arity, (name, len(args))
        assert hasattr(lib, name), name
    assert "Vocabulary" in smallk_amd.__all__
    from smallk_amd.preprocess import Preprocessor, PreprocessResult, Vocabulary
    assert smallk_amd.Vocabulary is Vocabulary
    assert callable(PreprocessResult.vocabulary) and callable(Preprocessor.vocabulary)
    for name in ("apply", "save", "load", "term_indices", "idf"):
        assert hasattr(Vocabulary, name), name


@pytest.mark.parametrize("key", vc.CORPORA)
def test_corpora_have_the_stated_figures(key):
    c = vc.corpus(*key)
    s = vc.stats(c)
    assert (s["terms"], s["fit_docs"], s["new_docs"], s["empty"], s["short"], s["long_cols"], s["iterations"]) == vc.EXPECTED[key]
    assert s["oov"] > 0.1 and c["ref"]["height"] < c["m"] and c["ref"]["width"] < c["nfit"]


def _assert_own_documents(c, boolean_mode=0):
    """apply (min_terms 0) on the fit's input: column j of the result is the fit's column of document j, bit for bit"""
    ref = c["ref"]
    cp, rows, data = c["fit"]
    out = vc.restate_apply(c["vocab"], cp, rows, data, 0)
    assert out["ok"] and out["width"] == c["nfit"] and np.array_equal(out["doc"], np.arange(c["nfit"]))
    assert np.array_equal(out["term"], ref["term"])
    assert ref["width"] > 0
    for jf, j in enumerate(ref["doc"]):
        a0, a1 = out["cp"][j], out["cp"][j + 1]
        f0, f1 = ref["cp"][jf], ref["cp"][jf + 1]
        assert np.array_equal(out["rows"][a0:a1], ref["rows"][f0:f1])
        assert out["scores"][a0:a1].view(np.uint64).tolist() == ref["scores"][f0:f1].view(np.uint64).tolist()


@pytest.mark.parametrize("key", vc.CORPORA)
def test_restatement_reproduces_the_fit_on_its_own_documents(key):
    _assert_own_documents(vc.corpus(*key))


def test_restatement_reproduces_the_fit_on_unsorted_fractional_input():
    c = vc.messy_corpus()
    cp, rows, data = c["fit"]
    assert (np.diff(rows)[np.diff(pc._col_of(cp)) == 0] < 0).any()           # a column arrives unsorted
    assert (data < 0).any() and (c["ref"]["counts"] == 0).any()
    assert len(c["ref"]["log"]) < 1000
    _assert_own_documents(c)


def test_long_corpus_has_fit_columns_beyond_three_load_stages():
    c = vc.long_corpus()
    ref = c["ref"]
    assert len(ref["log"]) < 1000 and ref["height"] < c["m"] and ref["width"] < c["nfit"]
    lens = np.diff(ref["cp"].astype(np.int64))
    assert (lens > 3 * vc.SUPER).sum() >= 2 and lens.max() > 4 * vc.SUPER
    assert {0, c["nfit"] // 2, c["nfit"] - 1} <= set(ref["doc"].tolist())
    _assert_own_documents(c)


def test_superchunk_case_has_both_kinds_on_both_sides_of_every_edge():
    vocab, cols = vc.superchunk_case()
    assert [len(r) for r, _ in cols[:len(vc.SUPER_LENGTHS)]] == list(vc.SUPER_LENGTHS)
    kept_map = vc.old_to_new(vocab) != vc.PRUNED
    for r, _ in cols[:len(vc.SUPER_LENGTHS)]:
        assert (np.diff(r) > 0).all() and r.max() < vocab["height_in"]
        kept = kept_map[r]
        for e in range(vc.SUPER, len(r) - 1, vc.SUPER):
            assert kept[e - 2] != kept[e - 1] and kept[e] != kept[e + 1] and kept[e - 1] == kept[e]
    out = vc.restate_apply(vocab, *vc.csc(cols), 0)
    assert out["survivors"][-2] == 1025 and out["survivors"][-1] == 0


def test_restatement_min_terms_and_failure():
    c = vc.corpus(*vc.CORPORA[2])
    cp, rows, data = c["new"]
    surv = vc.restate_apply(c["vocab"], cp, rows, data, 0)["survivors"]
    for mt in (0, 1, 5):
        out = vc.restate_apply(c["vocab"], cp, rows, data, mt)
        assert np.array_equal(out["doc"], np.flatnonzero(surv >= mt))
        assert np.array_equal(np.diff(out["cp"].astype(np.int64)), surv[surv >= mt])
        assert (out["rows"] < out["height"]).all()
    out = vc.restate_apply(c["vocab"], cp, rows, data, int(surv.max()) + 1)
    assert not out["ok"] and out["nnz"] == surv.sum()


def test_count_of_zero_gives_the_x86_nan_column():
    vocab = dict(term=np.array([0, 2], dtype=np.uint32), idf=np.array([0.5, 0.25]), height_in=3, boolean_mode=0)
    cp, rows, data = vc.csc([(np.array([0, 1, 2]), np.array([0.0, 4.0, 2.0]))])
    # -inf squared makes the sum inf and D 0: -inf * 0 is the NaN, a finite score times 0 is 0
    out = vc.restate_apply(vocab, cp, rows, data, 0)
    assert out["rows"].tolist() == [0, 1]
    assert out["scores"].view(np.uint64).tolist() == [0xFFF8000000000000, 0]
    # with an idf of 0 the raw score is already -inf * 0: the sum is NaN and with it the whole column
    vocab["idf"] = np.array([0.0, 0.25])
    out = vc.restate_apply(vocab, cp, rows, data, 0)
    assert out["scores"].view(np.uint64).tolist() == [0xFFF8000000000000] * 2


class _HostVocabulary:
    """a Vocabulary whose device arrays are host arrays: save / load need nothing else of it"""

    def __init__(self, term_indices, idf, height_in, boolean_mode=0):
        self._arrays = np.asarray(term_indices, dtype=np.uint32), np.asarray(idf, dtype=np.float64)
        self.height_in, self.boolean_mode, self.height = int(height_in), int(boolean_mode), len(term_indices)

    def _download(self):
        return self._arrays


def test_save_load_round_trip_is_bitwise(tmp_path):
    from smallk_amd.preprocess import Vocabulary
    term = np.array([0, 3, 4, 9, 4000000000], dtype=np.uint32)
    idf = np.array([0.0, np.inf, np.nan, 1.0 / 3.0, -0.0])
    path = str(tmp_path / "vocab.npz")
    Vocabulary.save(_HostVocabulary(term, idf, 4000000001, 1), path)
    got = Vocabulary.load.__func__(_HostVocabulary, path)
    t2, i2 = got._download()
    assert t2.dtype == np.uint32 and t2.tobytes() == term.tobytes()
    assert i2.dtype == np.float64 and i2.tobytes() == idf.tobytes()
    assert (got.height_in, got.boolean_mode) == (4000000001, 1)

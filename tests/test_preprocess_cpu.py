"""preprocess_tf without a GPU: the numpy restatement (tests/preprocess_cases.py) against the reference tool's recorded
outputs (tests/golden/ref_preprocess_results.npz), and the argument paths of smallk_amd/bin/preprocess_tf, which end before
the device is touched."""
import os
import subprocess

import numpy as np
import pytest

import preprocess_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "smallk_amd", "bin", "preprocess_tf")
GOLD = pc.load_golden()


def reference_arrays(g):
    """(term, doc, cp, rows, scores) of a recorded run: the indices from the written files, scores at precision 17"""
    term = np.array([int(t[4:]) for t in g["dict4"].split("\n") if t], dtype=np.uint32)
    doc = np.array([int(t[3:]) for t in g["docs4"].split("\n") if t], dtype=np.uint32)
    h, w, n, r, c, v = pc.parse_mtx(g["mtx17"])
    cp = np.zeros(w + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=w), out=cp[1:])
    assert (np.diff(c) >= 0).all()
    return term, doc, cp.astype(np.uint32), r.astype(np.uint32), v


def assert_scores_match(got, ref, rel=1e-14, atol=0.0):
    """finite values within rel (plus atol), non-finite values in the same places and equal"""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    assert (np.isnan(got) == np.isnan(ref)).all()
    assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all()
    assert np.all(np.abs(got[fin] - ref[fin]) <= rel * np.abs(ref[fin]) + atol)


# the recorded scores are printed with 17 decimals: half a unit of the last one on top of the relative bound
PRINTED = 5e-18


def test_fixture_set_covers_the_cases():
    assert len(GOLD) >= 12
    assert any(not g["ok"] for g in GOLD.values())
    assert any(len(g["log"]) >= 3 for g in GOLD.values())
    assert any(g["opts"]["boolean_mode"] for g in GOLD.values())
    assert os.path.getsize(pc.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", sorted(GOLD))
def test_restatement_reproduces_reference(name):
    g = GOLD[name]
    r = pc.restate(g["height"], g["width"], g["cp"], g["rows"], g["data"], **g["opts"])
    assert pc.log_lines(r["log"]) == g["log"]
    assert r["ok"] == g["ok"]
    if not g["ok"]:
        assert g["mtx4"] == "" and g["dict4"] == "" and g["docs4"] == ""
        return
    term, doc, cp, rows, scores = reference_arrays(g)
    assert np.array_equal(r["term"], term)
    assert np.array_equal(r["doc"], doc)
    assert np.array_equal(r["cp"], cp)
    assert np.array_equal(r["rows"], rows)
    assert_scores_match(r["scores"], scores, atol=PRINTED)


def test_fixture_idf_zero_gives_nan():
    # stopped at max_iter 1 with a row in every surviving document: idf = 0, and the column holding a count 0 there is NaN
    g = GOLD["idf_zero_maxiter"]
    assert "-nan" in g["mtx4"] and " 0.0000\n" in g["mtx4"]
    assert "inf" not in g["mtx4"]


def test_restatement_keeps_a_lone_column_that_is_not_the_first():
    # the reference reads a stale mask entry when one column is left after column pruning: it keeps the column only when it was
    # column 0 (fixture lone_column_kept); here the lone column is always unique
    for survivor in (0, 4):
        r = pc.restate(*pc.lone_column(survivor), max_iter=1)
        assert r["ok"] and r["doc"].tolist() == [survivor]
        assert len(r["log"]) == 1 and r["log"][0][1:] == (1, 8)


def test_restatement_keeps_largest_duplicate():
    # documents {0, 2, 5} identical, {1, 4} identical: 3, 4 and 5 survive
    a = (np.arange(8), np.ones(8))
    b = (np.arange(8, 16), np.full(8, 2.0))
    c = (np.arange(16, 24), np.full(8, 3.0))
    cp, rows, data = pc._csc(30, 6, [a, b, a, c, b, a])
    # docs_per_term 1: every term survives row pruning (each is in at most 3 of the 6 documents)
    r = pc.restate(30, 6, cp, rows, data, docs_per_term=1)
    assert r["doc"].tolist() == [3, 4, 5]


def test_restatement_nan_is_x86_default_nan():
    # a zero count gives -inf * idf, the column sum is inf and the scaling 1/inf = 0: -inf * 0 is NaN with the sign bit set
    cols = [(np.arange(6), np.r_[0.0, np.full(5, 2.0)])] + [(np.arange(6, 12), np.full(6, 1.0 + k)) for k in range(4)]
    cols += [(np.arange(0, 12, 2), np.full(6, 3.0))]
    cp, rows, data = pc._csc(12, 6, cols)
    r = pc.restate(12, 6, cp, rows, data, docs_per_term=1)
    s = r["scores"]
    assert np.isnan(s).any()
    assert (np.signbit(s[np.isnan(s)])).all()


def run_tool(*args, cwd=None):
    return subprocess.run([TOOL, *args], capture_output=True, text=True, cwd=cwd)


def test_cli_no_arguments_prints_usage():
    p = run_tool()
    assert p.returncode == 0
    assert p.stdout == ("\nUsage: " + TOOL + "\n          --indir  <path> \n        [--outdir  (defaults to current directory)] \n"
                        "        [--docs_per_term  3] \n        [--terms_per_doc  5] \n        [--maxiter  1000] \n"
                        "        [--precision  4] \n        [--boolean_mode  0] \n\n")


def test_cli_missing_indir():
    p = run_tool("--maxiter", "5")
    assert p.returncode == 255
    assert p.stderr == "preprocessor error: required command line argument --indir not found\n"


@pytest.mark.parametrize("flag,value", [("--maxiter", "0"), ("--docs_per_term", "0"), ("--terms_per_doc", "0"),
                                        ("--precision", "0"), ("--boolean_mode", "-1")])
def test_cli_invalid_values(flag, value, tmp_path):
    # the reference's message; its parser throws and lets the exception end the process, this tool returns -1 instead
    p = run_tool("--indir", str(tmp_path), flag, value)
    assert p.returncode != 0
    assert p.stderr == "Invalid value specified for command-line argument " + flag + "\n"


def test_cli_missing_directories(tmp_path):
    missing = str(tmp_path / "nope")
    p = run_tool("--indir", missing)
    assert p.returncode == 255
    assert p.stderr == f"\npreprocessor: the specified input directory {missing} does not exist.\n"
    p = run_tool("--indir", str(tmp_path), "--outdir", missing)
    assert p.returncode == 255
    assert p.stderr == f"\npreprocessor: the specified output directory {missing} does not exist.\n"


def test_cli_missing_input_files_and_size_checks(tmp_path):
    p = run_tool("--indir", str(tmp_path))
    assert p.returncode == 255
    assert p.stderr == f"\npreprocessor: could not open dictionary file {tmp_path}/dictionary.txt\n"
    cp, rows, data = pc._csc(6, 3, [(np.arange(5), np.ones(5))] * 3)
    pc.write_input_dir(str(tmp_path), 6, 3, cp, rows, data)
    with open(tmp_path / "dictionary.txt", "w") as f:
        f.write("a\nb\n")
    p = run_tool("--indir", str(tmp_path))
    assert p.returncode == 255
    assert p.stderr.endswith("\npreprocessor error: expected 6 terms in the dictionary; found 2.\n")
    pc.write_input_dir(str(tmp_path), 6, 3, cp, rows, data)
    with open(tmp_path / "documents.txt", "w") as f:
        f.write("a\n")
    p = run_tool("--indir", str(tmp_path))
    assert p.returncode == 255
    assert p.stderr.endswith("\npreprocessor error: expected 3 strings in the documents file; found 1.\n")

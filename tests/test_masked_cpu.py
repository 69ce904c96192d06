"""Masked coordinate descent without a GPU: that the numpy restatement tests/masked_reference.py is the iteration the
issue states, and that the cases of tests/masked_cases.py hold the bars of tests/test_gpu_masked.py by themselves -- no iteration
count, no zero pattern hangs on a rounding -- so that a device result off the bar is the device's doing."""
import functools
import os
import re

import numpy as np
import pytest

import cd_reference
import masked_cases as MC
import masked_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("seq", np.float64), ("pair", np.float64), ("pair", np.longdouble))


@functools.lru_cache(maxsize=None)
def _fits(name):
    """the three modes' fits, each with the factors after the first H sweep and the first W sweep"""
    c = MC.case(name)
    out = []
    for order, dt in MODES:
        first = {}
        r = R.fit(c["csc"], c["W0"], c["H0"], order=order, dtype=dt, after_first=lambda Wt, H, first=first: first.update(W=np.array(Wt.T), H=np.array(H)),
                  **c["kw"])
        out.append(dict(r, first=first))
    return out


def test_the_pattern_cases_sit_on_the_edges():
    for name in MC.PATTERN_CASES:
        c = MC.case(name)
        data, rows, indptr, (m, n) = c["csc"]
        col_counts, row_counts = np.diff(indptr), np.bincount(rows, minlength=m)
        for cnt, r, col in zip(MC.EDGE_COUNTS, c["srows"], c["scols"]):
            assert row_counts[r] == cnt and col_counts[col] == cnt, (name, cnt)
        assert col_counts.max() >= 200 and row_counts.max() >= 200 and col_counts.min() == 0 and row_counts.min() == 0
        assert (data == 0).mean() >= 0.05, name
        assert np.array_equal(data, MC.f32(data)) and np.array_equal(c["W0"], MC.f32(c["W0"])) and np.array_equal(c["H0"], MC.f32(c["H0"]))
        assert 260 <= m <= 400 and 90 <= n <= 300 and c["k"] <= min(m, n)
    d = MC.case("k5_degenerate")
    assert (d["W0"][:, MC.DEGENERATE_ZERO_COLUMN] == 0).mean() > 0.9 and (d["H0"] == 0).mean() > 0.1 and d["kw"]["alpha_H"] == 0.0
    assert sorted(MC.case(n)["k"] for n in ("k2", "k5", "k16", "k17", "k33", "k64", "k128")) == [2, 5, 16, 17, 33, 64, 128]


def test_full_mask_is_the_dense_iteration():
    """every entry stored: the restatement against cd_reference's fit of the same dense matrix"""
    c = MC.case(MC.FULL_MASK)
    assert c["csc"][0].size == c["dense"].size
    ref = cd_reference.fit(c["dense"], c["W0"], c["H0"], **c["kw"])
    top = max(ref["W"].max(), ref["H"].max())
    for got in _fits(MC.FULL_MASK)[:2]:
        ew, eh = np.abs(got["W"] - ref["W"]).max() / top, np.abs(got["H"] - ref["H"]).max() / top
        print(f"full mask: n_iter {got['n_iter']} (dense {ref['n_iter']}), W {ew:.2e} H {eh:.2e}")
        assert got["n_iter"] == ref["n_iter"] and got["converged"] == ref["converged"] and ref["converged"]
        assert ew <= MC.FIT_BAR and eh <= MC.FIT_BAR
        assert abs(got["violation"] - ref["violation"]) <= 1e-9 * ref["violation"]


@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_the_case_holds_its_bars_by_itself(name):
    fits = _fits(name)
    ld = fits[2]
    tol = MC.case(name)["kw"]["tol"]
    top = max(ld["W"].max(), ld["H"].max())
    for f in fits:
        assert f["n_iter"] == ld["n_iter"] and f["converged"] == ld["converged"]
        assert np.array_equal(f["W"] == 0, ld["W"] == 0) and np.array_equal(f["H"] == 0, ld["H"] == 0)
        assert all(abs(r - tol) >= MC.MARGIN * tol for r in f["ratios"]), name
        dev = max(np.abs(f["W"] - ld["W"]).max(), np.abs(f["H"] - ld["H"]).max()) / top
        assert dev <= MC.FIT_BAR / 16, (name, dev)           # the restatement itself uses a sixteenth of the GPU's bar at most
    dh = max(np.abs(f["first"]["H"] - ld["first"]["H"]).max() for f in fits[:2]) / ld["first"]["H"].max()
    dw = max(np.abs(f["first"]["W"] - ld["first"]["W"]).max() for f in fits[:2]) / ld["first"]["W"].max()
    print(f"{name}: n_iter {ld['n_iter']}, one sweep float64 against longdouble: H {dh:.2e} W {dw:.2e} (recorded {MC.SWEEP_DEVIATION[name]})")
    assert dh <= MC.SWEEP_DEVIATION[name][0] and dw <= MC.SWEEP_DEVIATION[name][1]
    for f in fits:
        assert np.array_equal(f["first"]["H"] == 0, ld["first"]["H"] == 0) and np.array_equal(f["first"]["W"] == 0, ld["first"]["W"] == 0)


def test_degenerate_start_rules():
    """hess == 0 (a zero column of W0, l2 = 0): that coordinate of H stays where the column meets zero rows only, its projected
    gradient still counts; a coordinate at zero moves only against a negative gradient"""
    c = MC.case("k5_degenerate")
    z = MC.DEGENERATE_ZERO_COLUMN
    first = _fits("k5_degenerate")[0]["first"]
    mask = c["mask"]
    stays = np.array([mask[:, j].any() and (c["W0"][mask[:, j], z] == 0).all() for j in range(mask.shape[1])])
    assert stays.sum() > 100 and np.array_equal(first["H"][z, stays], c["H0"][z, stays])
    assert (first["H"][z, ~stays & mask.any(axis=0)] != c["H0"][z, ~stays & mask.any(axis=0)]).any()
    assert (first["W"][:, z] > 0).any()                        # the W sweep sees the new H: its hess is not zero


def test_planted_case_states_the_gap():
    """fitting the observed entries recovers the held-out ones; the zero-filled fit (nmf_cd on the sparse matrix) does not"""
    c = MC.case(MC.PLANTED)
    ld = _fits(MC.PLANTED)[0]
    r, a = R.masked_residual(c["test_csc"], ld["W"], ld["H"])[:2]
    held = np.sqrt(r / a)
    zero_filled = np.where(c["seen"], c["dense"], 0.0)
    zf = cd_reference.fit(zero_filled, c["W0"], c["H0"], **c["kw"])
    r0, a0 = R.masked_residual(c["test_csc"], zf["W"], zf["H"])[:2]
    print(f"planted: held-out relative error {held:.3e} after {ld['n_iter']} iterations; zero-filled fit {np.sqrt(r0 / a0):.3f}")
    assert ld["converged"] and held <= 1e-3
    assert np.sqrt(r0 / a0) >= 0.3


def test_holdout_split_partitions_the_stored_entries():
    import scipy.sparse as sp
    from smallk_amd.solver import holdout_split
    c = MC.case("k5")
    data, rows, indptr, shape = c["csc"]
    assert (data == 0).sum() > 100
    for src in (c["csc"], sp.csc_matrix((data, rows.astype(np.int32), indptr.astype(np.int32)), shape=shape)):
        train, test = holdout_split(src, 0.3, seed=11)
        again = holdout_split(src, 0.3, seed=11)
        other = holdout_split(src, 0.3, seed=12)
        for p, q in zip(train + test, again[0] + again[1]):
            assert np.array_equal(p, q)
        assert not np.array_equal(other[1][1], test[1]) or not np.array_equal(other[1][2], test[2])
        assert train[3] == test[3] == shape and test[0].size == round(0.3 * data.size) and train[0].size + test[0].size == data.size
        # the two parts together are the stored entries, each once, stored zeros included
        col = lambda t: np.repeat(np.arange(shape[1]), np.diff(t[2]))
        key = lambda t: col(t).astype(np.int64) * shape[0] + t[1]
        allk = np.concatenate([key(train), key(test)])
        allv = np.concatenate([train[0], test[0]])
        order = np.argsort(allk, kind="stable")
        assert np.array_equal(allk[order], key(c["csc"])) and np.array_equal(allv[order], data)
        assert (train[0] == 0).sum() + (test[0] == 0).sum() == (data == 0).sum() and (test[0] == 0).sum() > 0
        for t in (train, test):
            assert all(np.all(np.diff(t[1][t[2][j]:t[2][j + 1]].astype(np.int64)) > 0) for j in range(shape[1]))
    empty, everything = holdout_split(c["csc"], 1.0, seed=1)
    assert empty[0].size == 0 and everything[0].size == data.size
    with pytest.raises(ValueError):
        holdout_split(c["csc"], 1.5, seed=1)


def test_from_observed_keeps_masked_in_zeros(monkeypatch):
    """the triple that reaches the library holds the zeros where X == 0 and the mask is true"""
    from smallk_amd import solver
    seen = {}

    def fake_init(self, data, indices, indptr, shape, **kw):
        seen.update(data=np.asarray(data), indices=np.asarray(indices), indptr=np.asarray(indptr), shape=tuple(shape))

    monkeypatch.setattr(solver.SparseMatrix, "__init__", fake_init)
    monkeypatch.setattr(solver.SparseMatrix, "close", lambda self: None)
    c = MC.case("k5")
    X, mask = c["dense"], c["mask"]
    solver.SparseMatrix.from_observed(X, mask)
    data, rows, indptr, shape = c["csc"]
    assert np.array_equal(seen["data"], data) and np.array_equal(seen["indices"], rows) and np.array_equal(seen["indptr"], indptr)
    assert seen["shape"] == shape and (seen["data"] == 0).sum() == (X[mask] == 0).sum() > 100
    with pytest.raises(ValueError):
        solver.SparseMatrix.from_observed(X, mask.astype(np.int8))
    with pytest.raises(ValueError):
        solver.SparseMatrix.from_observed(X, mask[:, :-1])


def test_the_new_symbols_are_declared_and_exported():
    import smallk_amd
    from smallk_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "smallk_amd.h")).read()
    lib = L.lib()
    for name in ("smk_nmf_masked_device", "smk_matrix_masked_residual_device", "smk_masked_last_profile", "smk_masked_step_time"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    assert "smk_masked_stats" in header and [f for f, _ in L.MaskedStats._fields_] == ["iterations", "converged", "violation_init", "violation", "error"]
    for name in ("nmf_masked", "masked_last_profile", "MaskedResult", "MaskedResidual", "holdout_split"):
        assert hasattr(smallk_amd, name) and name in smallk_amd.__all__
    assert hasattr(smallk_amd.SparseMatrix, "masked_residual") and hasattr(smallk_amd.SparseMatrix, "from_observed")

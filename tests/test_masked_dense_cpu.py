"""What masked dense NMF does on the host, without a GPU: the held-out split, the NaN that marks "not measured" and
its way through the rounding to bf16, and the ValueErrors raised before any library call."""
import numpy as np
import pytest

from smallk_amd import solver


def test_holdout_split_dense():
    rng = np.random.default_rng(3)
    X = rng.random((37, 23))
    X[rng.random(X.shape) < 0.2] = np.nan
    X[4, 5] = 0.0                                             # a measured zero is a measurement
    measured = ~np.isnan(X)
    train, test = solver.holdout_split_dense(X, 0.3, seed=9)
    assert train.shape == test.shape == X.shape and train.dtype == test.dtype == np.float64
    in_train, in_test = ~np.isnan(train), ~np.isnan(test)
    assert not (in_train & in_test).any() and np.array_equal(in_train | in_test, measured)
    assert int(in_test.sum()) == int(round(0.3 * measured.sum()))
    assert np.array_equal(train[in_train], X[in_train]) and np.array_equal(test[in_test], X[in_test])
    again = solver.holdout_split_dense(X, 0.3, seed=9)
    assert np.array_equal(again[0], train, equal_nan=True) and np.array_equal(again[1], test, equal_nan=True)
    assert not np.array_equal(solver.holdout_split_dense(X, 0.3, seed=10)[1], test, equal_nan=True)
    with pytest.raises(ValueError):
        solver.holdout_split_dense(X, 1.5, seed=0)


def test_from_observed_writes_the_canonical_nan(monkeypatch):
    seen = {}
    monkeypatch.setattr(solver.DenseMatrix, "from_host", classmethod(lambda cls, A, **kw: seen.update(A=A, kw=kw)))
    X, mask = np.arange(6.0).reshape(2, 3), np.array([[True, False, True], [False, True, True]])
    solver.DenseMatrix.from_observed(X, mask, storage="bf16")
    assert seen["kw"] == {"storage": "bf16"} and seen["A"].shape == (2, 3) and X[0, 1] == 1.0           # X itself is not written
    assert np.array_equal(np.isnan(seen["A"]), ~mask) and np.array_equal(seen["A"][mask], X[mask])
    assert (seen["A"][~mask].astype(np.float32).view(np.uint32) == 0x7FC00000).all()
    for bad in (np.ones((2, 3)), mask[:, :2]):
        with pytest.raises(ValueError):
            solver.DenseMatrix.from_observed(X, bad)


def test_the_canonical_nan_survives_the_rounding_to_bf16():
    """f32_to_bf16_rne adds 0x7FFF and the lowest kept bit, then shifts: restated in integer operations"""
    rne = lambda b: ((np.uint32(b) + np.uint32(0x7FFF) + ((np.uint32(b) >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) & np.uint32(0xFFFF)
    assert np.array([np.nan], dtype=np.float32).view(np.uint32)[0] == 0x7FC00000
    assert rne(0x7FC00000) == 0x7FC0                         # still a NaN in bf16
    assert rne(0x7FFFFFFF) == 0x8000                         # a full payload wraps to -0: why adopted tensors must carry the canonical one


def test_value_errors_come_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(solver.L, "lib", no_library)
    dense, sparse = object.__new__(solver.DenseMatrix), object.__new__(solver.SparseMatrix)
    dense.height, dense.ncols = sparse.height, sparse.ncols = 4, 5
    W, H = np.ones((4, 2)), np.ones((2, 5))
    for loss in (0.5, 3, "poisson", True, None, float("nan")):
        with pytest.raises(ValueError, match="beta_loss"):
            solver.nmf_masked_dense(dense, W, H, beta_loss=loss)
        with pytest.raises(ValueError, match="beta_loss"):
            dense.masked_divergence(W, H, loss)
    with pytest.raises(ValueError, match="DenseMatrix"):
        solver.nmf_masked_dense(sparse, W, H, beta_loss="itakura-saito")
    with pytest.raises(ValueError, match="DenseMatrix"):
        sparse.masked_divergence(W, H, 2)
    with pytest.raises(ValueError):
        solver.nmf_masked_dense(dense, W, np.ones((3, 5)))
    for x in (dense, sparse):                               # no handle: nothing for __del__ to release
        x._h = None

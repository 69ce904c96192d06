"""CPU tests of the labelling and fold-in entries (smk_labels_device, smk_top_terms_device, smk_solver_labels,
smk_solver_top_terms, smk_solver_project_h; labels_device, top_terms_device, transform): the declarations, and the argument
checks that run in Python before the library is called."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITY = {"smk_labels_device": 9, "smk_top_terms_device": 9, "smk_solver_labels": 5, "smk_solver_top_terms": 5, "smk_solver_project_h": 1}


def test_entries_are_declared_and_bound():
    """header, binding table and shared object agree, argument for argument"""
    import smallk_amd
    header = open(os.path.join(ROOT, "include", "smallk_amd.h")).read()
    lib = smallk_amd._lib.lib()
    for name, arity in ARITY.items():
        decl = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity, (name, decl.group(1))
        res, args = smallk_amd._lib.SYMBOLS[name]
        assert len(args) == arity, (name, len(args))
        assert hasattr(lib, name), name
    for name in ("labels_device", "top_terms_device", "transform"):
        assert callable(getattr(smallk_amd, name)) and name in smallk_amd.__all__
    for name in ("labels_device", "top_terms_device", "project"):
        assert hasattr(smallk_amd.NmfSolver, name)


def shell_matrix(height, ncols):
    """a DenseMatrix without a device behind it: any call that reaches the library fails on the null handle"""
    import smallk_amd
    D = smallk_amd.DenseMatrix.__new__(smallk_amd.DenseMatrix)
    D.height, D.ncols, D.width_global, D._h = height, ncols, ncols, None
    return D


def test_python_checks_come_before_the_library(monkeypatch):
    """CPU tensors, wrong ranks, element types that are not float64 / float32, things that are no tensors and maxterms < 1 are
    ValueErrors, and the library is not even loaded for them"""
    torch = pytest.importorskip("torch")
    import smallk_amd
    L = smallk_amd._lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", no_library)
    H = torch.ones((3, 4), dtype=torch.float64)
    W = torch.ones((5, 3), dtype=torch.float64)
    for bad in (H, H.float()):
        with pytest.raises(ValueError, match="GPU memory"):
            smallk_amd.labels_device(bad)
        with pytest.raises(ValueError, match="GPU memory"):
            smallk_amd.labels_device(bad, memberships=True)
    with pytest.raises(ValueError, match="GPU memory"):
        smallk_amd.top_terms_device(W, 5)
    for bad in (H[0], H[None], torch.ones(())):
        with pytest.raises(ValueError, match="dimensions"):
            smallk_amd.labels_device(bad)
        with pytest.raises(ValueError, match="dimensions"):
            smallk_amd.top_terms_device(bad, 5)
    for bad in (H.to(torch.int32), H.to(torch.int64), H.to(torch.float16), H.to(torch.bfloat16), H > 0):
        with pytest.raises(ValueError, match="dtype"):
            smallk_amd.labels_device(bad)
        with pytest.raises(ValueError, match="dtype"):
            smallk_amd.top_terms_device(bad, 5)
    for bad in (H.numpy(), [[1.0, 2.0]], None):
        with pytest.raises(ValueError, match="torch tensor"):
            smallk_amd.labels_device(bad)
        with pytest.raises(ValueError, match="torch tensor"):
            smallk_amd.top_terms_device(bad, 5)
    with pytest.raises(ValueError, match="empty"):
        smallk_amd.labels_device(torch.ones((0, 4), dtype=torch.float64))
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="maxterms"):
            smallk_amd.top_terms_device(W, bad)
    s = smallk_amd.NmfSolver.__new__(smallk_amd.NmfSolver)
    s._h, s.k = None, 3
    with pytest.raises(ValueError, match="maxterms"):
        s.top_terms_device(0)
    s._h = None                # (nothing to destroy)


def test_transform_checks_come_before_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    import smallk_amd
    L = smallk_amd._lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", no_library)
    D = shell_matrix(5, 4)
    W = np.ones((5, 3))
    with pytest.raises(ValueError, match="resident"):
        smallk_amd.transform(np.ones((5, 4)), W)
    for bad in (W[:-1], W[:, 0], np.ones((5, 3, 1)), np.ones((5, 0))):
        with pytest.raises(ValueError, match=r"transform\(W\)"):
            smallk_amd.transform(D, bad)
    with pytest.raises(ValueError, match="real numbers"):
        smallk_amd.transform(D, W.astype(complex))
    with pytest.raises(ValueError, match="GPU memory"):
        smallk_amd.transform(D, torch.ones((5, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="dtype"):
        smallk_amd.transform(D, torch.ones((5, 3), dtype=torch.int32))
    for bad in (np.ones((3, 5)), np.ones((2, 4)), np.ones(4)):
        with pytest.raises(ValueError, match=r"transform\(H0\)"):
            smallk_amd.transform(D, W, H0=bad)

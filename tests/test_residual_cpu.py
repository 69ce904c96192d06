"""CPU tests of the reconstruction-error entries (smk_matrix_residual, smk_matrix_residual_device, smk_solver_residual,
DenseMatrix.residual, NmfSolver.residual, relative_error): the declarations, the arithmetic of the result type, the argument
checks that run in Python before the library is called, and that the package still imports without torch."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITY = {"smk_matrix_residual": 9, "smk_matrix_residual_device": 14, "smk_solver_residual": 4}


def test_entries_are_declared_and_bound():
    """header, binding table and shared object agree, argument for argument (tests/test_abi.py then checks that every declared
    symbol is exported)"""
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
    assert hasattr(smallk_amd.DenseMatrix, "residual") and smallk_amd.SparseMatrix.residual is smallk_amd.DenseMatrix.residual
    assert hasattr(smallk_amd.NmfSolver, "residual")
    assert callable(smallk_amd.relative_error) and "relative_error" in smallk_amd.__all__


def test_residual_arithmetic():
    from smallk_amd import Residual
    r = Residual(4.0, 16.0)
    assert r.norm == 2.0 and r.relative == 0.5 and r.col_resid_sq is None
    assert Residual(0.0, 9.0).relative == 0.0 and Residual(0.0, 9.0).norm == 0.0
    assert Residual(2.0, 8.0).relative == math.sqrt(0.25)
    assert math.isnan(Residual(0.0, 0.0).relative) and math.isnan(Residual(3.0, 0.0).relative)
    assert Residual(3.0, 0.0).norm == math.sqrt(3.0)
    cols = np.array([1.0, 3.0])
    assert Residual(4.0, 16.0, cols).col_resid_sq is cols


def shell_matrix(height, ncols):
    """a DenseMatrix without a device behind it: any call that reaches the library fails on the null handle"""
    import smallk_amd
    D = smallk_amd.DenseMatrix.__new__(smallk_amd.DenseMatrix)
    D.height, D.ncols, D._h = height, ncols, None
    return D


def test_python_checks_reject_bad_factors_before_the_library():
    import smallk_amd
    L = smallk_amd._lib
    was = L.lib().smk_is_initialized()
    D = shell_matrix(5, 4)
    W, H = np.ones((5, 3)), np.ones((3, 4))
    for bad_w, bad_h in ((W[:-1], H), (W, H[:, :-1]), (W, np.ones((2, 4))), (np.ones((5, 0)), np.ones((0, 4))), (W[:, 0], H), (W, H[0])):
        with pytest.raises(ValueError, match="residual"):
            D.residual(bad_w, bad_h)
        with pytest.raises(ValueError, match="residual"):
            smallk_amd.relative_error(D, bad_w, bad_h)
    with pytest.raises(TypeError, match="real numbers"):
        D.residual(W.astype(complex), H)
    with pytest.raises(TypeError, match="real numbers"):
        D.residual(W, np.array([["a"] * 4] * 3))
    assert L.lib().smk_is_initialized() == was


def test_python_checks_reject_tensors_before_the_library():
    """mixed host / device factors, integer tensors, tensors of the wrong shape and tensors that are not in GPU memory"""
    torch = pytest.importorskip("torch")
    import smallk_amd
    L = smallk_amd._lib
    was = L.lib().smk_is_initialized()
    D = shell_matrix(5, 4)
    W, H = torch.ones((5, 3), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="both"):
        D.residual(W, H.numpy())
    with pytest.raises(TypeError, match="both"):
        D.residual(W.numpy(), H)
    with pytest.raises(ValueError, match="do not match"):
        D.residual(W[:-1], H)
    with pytest.raises(ValueError, match="do not match"):
        D.residual(W, H[:, :-1])
    with pytest.raises(TypeError, match="dtype"):
        D.residual(W.to(torch.int32), H.to(torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        D.residual(W, H.to(torch.int64))
    with pytest.raises(TypeError, match="dtype"):
        D.residual(W.to(torch.float16), H.to(torch.float16))
    with pytest.raises(ValueError, match="GPU memory"):
        D.residual(W, H)
    assert L.lib().smk_is_initialized() == was


def test_import_does_not_pull_in_torch():
    code = ("import sys; sys.path.insert(0, %r); import smallk_amd, numpy as np; smallk_amd._lib.lib(); "
            "D = smallk_amd.DenseMatrix.__new__(smallk_amd.DenseMatrix); D.height, D.ncols, D._h = 3, 2, None\n"
            "try:\n    D.residual(np.ones((2, 1)), np.ones((1, 2)))\nexcept ValueError:\n    pass\n"
            "assert smallk_amd.Residual(1.0, 4.0).relative == 0.5\n"
            "sys.exit(3 if 'torch' in sys.modules else 0)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])

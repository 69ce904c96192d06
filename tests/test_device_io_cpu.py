"""CPU tests of the device-tensor entries (smk_*_device, DenseMatrix.from_device, ...): what can be said without a GPU --
the declarations, that the package still imports without torch, the argument checks in front of the library, and the 64-bit
extent arithmetic behind the pointer checks."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["smk_matrix_adopt_device", "smk_matrix_copy_to_device", "smk_matrix_create_sparse_device",
               "smk_solver_set_factors_device", "smk_solver_get_factors_device", "smk_strided_extent_fits"]


def test_new_entries_are_declared_and_bound():
    """header, binding table and shared object agree (tests/test_abi.py then checks that every declared symbol is exported)"""
    import smallk_amd
    header = open(os.path.join(ROOT, "include", "smallk_amd.h")).read()
    lib = smallk_amd._lib.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in smallk_amd._lib.SYMBOLS, name
        assert hasattr(lib, name), name
    for enum in ("SMK_DT_F64 = 0", "SMK_DT_F32 = 1", "SMK_DT_BF16 = 2", "SMK_DT_F16 = 3", "SMK_IDX_I32 = 0", "SMK_IDX_I64 = 1"):
        assert enum in header, enum
    L = smallk_amd._lib
    assert (L.DT_F64, L.DT_F32, L.DT_BF16, L.DT_F16, L.IDX_I32, L.IDX_I64) == (0, 1, 2, 3, 0, 1)
    for name in ("from_device", "adopt", "to_device"):
        assert hasattr(smallk_amd.DenseMatrix, name), name
    assert hasattr(smallk_amd.NmfSolver, "set_factors_device") and hasattr(smallk_amd.NmfSolver, "factors_device")
    assert callable(smallk_amd.nmf_device)


def test_import_does_not_pull_in_torch():
    code = ("import sys; sys.path.insert(0, %r); import smallk_amd; smallk_amd._lib.lib(); "
            "assert hasattr(smallk_amd.DenseMatrix, 'from_device'); "
            "sys.exit(3 if 'torch' in sys.modules else 0)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])


def test_python_checks_reject_host_tensors_before_the_library():
    """a CPU tensor, a wrong rank and a wrong dtype raise from Python; the library is never initialised by them"""
    torch = pytest.importorskip("torch")
    import smallk_amd
    L = smallk_amd._lib
    was = L.lib().smk_is_initialized()
    cpu = torch.ones((4, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="GPU memory"):
        smallk_amd.DenseMatrix.from_device(cpu)
    with pytest.raises(ValueError, match="dimensions"):
        smallk_amd.DenseMatrix.from_device(torch.ones(5))
    with pytest.raises(TypeError, match="dtype"):
        smallk_amd.DenseMatrix.from_device(torch.ones((4, 3), dtype=torch.int32))
    with pytest.raises(TypeError, match="torch.Tensor"):
        smallk_amd.DenseMatrix.from_device([[1.0, 2.0]])
    with pytest.raises(ValueError, match="GPU memory"):
        smallk_amd.SparseMatrix.from_device(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.tensor([1.0, 2.0]), (2, 2))
    with pytest.raises(TypeError, match="dtype"):
        smallk_amd.SparseMatrix.from_device(torch.tensor([0.0, 1.0, 2.0]), torch.tensor([0, 1]), torch.tensor([1.0, 2.0]), (2, 2))
    with pytest.raises(ValueError, match="GPU memory"):
        smallk_amd.nmf_device(cpu, torch.ones((4, 2)), torch.ones((2, 3)), "MU")
    assert L.lib().smk_is_initialized() == was


def fits(rows, cols, rs, cs, es, offset, alloc):
    import smallk_amd
    return smallk_amd._lib.lib().smk_strided_extent_fits(rows, cols, rs, cs, es, offset, alloc)


def test_extent_arithmetic():
    # ordinary views: column-major 5 x 3 with leading dimension 7 ends at element 2 * 7 + 4 = 18 -> 19 elements
    assert fits(5, 3, 1, 7, 4, 0, 19 * 4) == 1
    assert fits(5, 3, 1, 7, 4, 0, 19 * 4 - 1) == 0
    assert fits(5, 3, 7, 1, 8, 16, 16 + (4 * 7 + 3) * 8) == 1          # row-major, offset into the allocation
    assert fits(5, 3, 7, 1, 8, 16, 16 + (4 * 7 + 3) * 8 - 8) == 0
    # X[:, ::2]: the last element sits at (rows - 1) ld + 2 (cols - 1)
    assert fits(4, 3, 10, 2, 2, 0, (3 * 10 + 4 + 1) * 2) == 1
    assert fits(4, 3, 10, 2, 2, 0, (3 * 10 + 4) * 2) == 0
    # stride 0 (expand): one row of 6 elements read 1000 times
    assert fits(1000, 6, 0, 1, 4, 0, 24) == 1
    assert fits(1000, 6, 0, 1, 4, 0, 23) == 0
    assert fits(1000, 6, 0, 0, 2, 0, 2) == 1
    # a view that ends exactly at the end of the allocation is accepted, one element further is not
    assert fits(8, 8, 1, 8, 4, 256 - 64 * 4, 256) == 1
    assert fits(8, 8, 1, 8, 4, 256 - 64 * 4 + 4, 256) == 0
    assert fits(9, 8, 1, 8, 4, 0, 256) == 0 and fits(8, 8, 1, 9, 4, 0, 256) == 0
    # 2^40 elements: 2^43 bytes of fp64, far past 32 bits, still exact
    n = 1 << 40
    assert fits(n, 1, 1, n, 8, 0, n * 8) == 1
    assert fits(n, 1, 1, n, 8, 0, n * 8 - 1) == 0
    assert fits(1 << 20, 1 << 20, 1, 1 << 20, 2, 0, n * 2) == 1
    assert fits(1 << 20, 1 << 20, 1, 1 << 20, 2, 2, n * 2) == 0
    # products that leave 64 bits are refused, not wrapped
    assert fits(n, n, n, 1, 8, 0, (1 << 63) - 1) == 0
    assert fits(1 << 62, 2, 4, 1, 8, 0, (1 << 63) - 1) == 0
    # nonsense
    assert fits(0, 3, 1, 1, 4, 0, 100) == 0 and fits(3, 3, -1, 3, 4, 0, 100) == 0 and fits(3, 3, 1, 3, 0, 0, 100) == 0
    assert fits(3, 3, 1, 3, 4, -4, 100) == 0

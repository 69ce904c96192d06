"""Masked coordinate descent on the device (smallk_amd.nmf_masked, SparseMatrix.masked_residual; smallk_amd/csrc/masked_cd.hip,
masked_cd.cpp) against the numpy restatement tests/masked_reference.py in numpy.longdouble.  That the cases hold these
bars by themselves -- no zero pattern, no iteration count hangs on a rounding -- is checked on the CPU by tests/test_masked_cpu.py.

Bars.  One H sweep and the W sweep after it, entry by entry: within 8 x the recorded float64-against-longdouble deviation of the
case (masked_cases.SWEEP_DEVIATION) of the factor's largest entry, never below 64 k 2^-53; equal zero patterns.  A fit: the same
n_iter and converged, factors within 1e-12 of the largest factor entry, equal zero patterns, violation_init, violation and error
within 1e-12 relative, the same bits on a second run.  The residual: within 1e-12 of the sum of the sizes of its terms.  The file
passes with SMK_POISON=1 as well."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import masked_cases as MC
import masked_reference as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the longdouble fit of the case, with the factors after the first H sweep and the W sweep that follows it"""
    c = MC.case(name)
    first = {}
    ref = R.fit(c["csc"], c["W0"], c["H0"], order="pair", dtype=np.longdouble,
                after_first=lambda Wt, H: first.update(W=np.array(Wt.T, dtype=np.float64), H=np.array(H, dtype=np.float64)), **c["kw"])
    return dict(ref, first=first)


def _matrix(gpu, name, which="csc"):
    data, rows, indptr, shape = MC.case(name)[which]
    return gpu.SparseMatrix(data, rows, indptr, shape)


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


# ---- one sweep, entry by entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_one_sweep_of_each_side(gpu, name):
    c, first = MC.case(name), _reference(name)["first"]
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_masked(mat, c["W0"], c["H0"], **dict(c["kw"], max_iter=1))
    finally:
        mat.close()
    eh = np.abs(r.H - first["H"]).max() / first["H"].max()
    ew = np.abs(r.W - first["W"]).max() / first["W"].max()
    print(f"one sweep {name}: H {eh:.2e} (bar {MC.sweep_bar(name, 0):.2e}), W {ew:.2e} (bar {MC.sweep_bar(name, 1):.2e})")
    assert r.n_iter == 1
    assert eh <= MC.sweep_bar(name, 0) and ew <= MC.sweep_bar(name, 1)
    assert np.array_equal(r.H == 0, first["H"] == 0) and np.array_equal(r.W == 0, first["W"] == 0)


# ---- fits --------------------------------------------------------------------------------------------------------------------
def _compare(r, ref, tag):
    top = max(ref["W"].max(), ref["H"].max())
    ew, eh = np.abs(r.W - ref["W"]).max() / top, np.abs(r.H - ref["H"]).max() / top
    ev0, ev, ee = _rel(r.violation_init, ref["violation_init"]), _rel(r.violation, ref["violation"]), _rel(r.error, ref["error"])
    print(f"fit {tag}: n_iter {r.n_iter} (restatement {ref['n_iter']}), W {ew:.2e} H {eh:.2e}, violation_init {ev0:.2e} violation {ev:.2e} "
          f"error {ee:.2e} (bar {MC.FIT_BAR:.0e})")
    assert r.n_iter == ref["n_iter"] and r.converged == ref["converged"]
    assert ew <= MC.FIT_BAR and eh <= MC.FIT_BAR
    assert np.array_equal(r.W == 0, ref["W"] == 0) and np.array_equal(r.H == 0, ref["H"] == 0)
    assert ev0 <= MC.FIT_BAR and ev <= MC.FIT_BAR and ee <= MC.FIT_BAR


@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_fit(gpu, name):
    c, ref = MC.case(name), _reference(name)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_masked(mat, c["W0"], c["H0"], **c["kw"])
        r2 = gpu.nmf_masked(mat, c["W0"], c["H0"], **c["kw"])
    finally:
        mat.close()
    _compare(r, ref, name)
    assert np.array_equal(r.W, r2.W) and np.array_equal(r.H, r2.H)
    assert (r.n_iter, r.converged, r.violation_init, r.violation, r.error) == (r2.n_iter, r2.converged, r2.violation_init, r2.violation, r2.error)


def test_full_mask_is_nmf_cd(gpu):
    """every entry stored: the same problem as nmf_cd on the same SparseMatrix"""
    c = MC.case(MC.FULL_MASK)
    mat = _matrix(gpu, MC.FULL_MASK)
    try:
        r = gpu.nmf_masked(mat, c["W0"], c["H0"], **c["kw"])
        cd = gpu.nmf_cd(mat, c["W0"], c["H0"], **c["kw"])
    finally:
        mat.close()
    top = max(cd.W.max(), cd.H.max())
    ew, eh = np.abs(r.W - cd.W).max() / top, np.abs(r.H - cd.H).max() / top
    print(f"full mask: n_iter {r.n_iter} (nmf_cd {cd.n_iter}), W {ew:.2e} H {eh:.2e} (bar {MC.FIT_BAR:.0e})")
    assert r.n_iter == cd.n_iter and r.converged and cd.converged
    assert ew <= MC.FIT_BAR and eh <= MC.FIT_BAR


def test_planted_holdout(gpu):
    """the gap the feature closes: fitted to the observed 40 %, the held-out 60 % are recovered; the zero-filled fit misses them"""
    c, ref = MC.case(MC.PLANTED), _reference(MC.PLANTED)
    rr, ra = R.masked_residual(c["test_csc"], ref["W"], ref["H"])[:2]
    ref_rel = math.sqrt(rr / ra)
    train, test = _matrix(gpu, MC.PLANTED), _matrix(gpu, MC.PLANTED, "test_csc")
    try:
        r = gpu.nmf_masked(train, c["W0"], c["H0"], **c["kw"])
        held = test.masked_residual(r.W, r.H)
        zf = gpu.nmf_cd(train, c["W0"], c["H0"], **c["kw"])
        held_zf = test.masked_residual(zf.W, zf.H)
    finally:
        train.close()
        test.close()
    print(f"planted: held-out relative error {held.relative:.6e} (restatement {ref_rel:.6e}), rmse {held.rmse:.3e}; zero-filled nmf_cd {held_zf.relative:.3f}")
    assert held.count == c["test_csc"][0].size
    assert _rel(held.relative, ref_rel) <= 1e-9
    assert held.relative <= 1e-3
    assert held_zf.relative >= 0.3


# ---- the residual ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_masked_residual(gpu, name):
    c, ref = MC.case(name), _reference(name)
    which = "test_csc" if name == MC.PLANTED else "csc"
    rr, ra, cnt, col_r, col_a, terms, col_terms = R.masked_residual(c[which], ref["W"], ref["H"])
    mat = _matrix(gpu, name, which)
    try:
        got = mat.masked_residual(ref["W"], ref["H"], per_column=True)
        plain = mat.masked_residual(ref["W"], ref["H"])
    finally:
        mat.close()
    er, ea = abs(got.resid_sq - rr) / terms, abs(got.norm_sq - ra) / terms
    ec = np.max(np.abs(got.col_resid_sq - col_r) / np.where(col_terms > 0, col_terms, 1.0))
    eca = np.max(np.abs(got.col_norm_sq - col_a) / np.where(col_terms > 0, col_terms, 1.0))
    print(f"residual {name}: total {er:.2e} / {ea:.2e}, per column {ec:.2e} / {eca:.2e} of the sum of |terms| (bar 1e-12)")
    assert got.count == cnt == c[which][0].size
    assert er <= 1e-12 and ea <= 1e-12 and ec <= 1e-12 and eca <= 1e-12
    empty = np.diff(c[which][2]) == 0
    assert (got.col_resid_sq[empty] == 0).all() and (got.col_norm_sq[empty] == 0).all()
    assert (plain.resid_sq, plain.norm_sq, plain.count) == (got.resid_sq, got.norm_sq, got.count) and plain.col_resid_sq is None
    assert got.rmse == math.sqrt(got.resid_sq / got.count) and got.relative == math.sqrt(got.resid_sq / got.norm_sq)


# ---- fold-in -----------------------------------------------------------------------------------------------------------------
def test_update_w_false(gpu):
    """W's bits are untouched, H is the restatement's, one sweep over the entries per iteration (two for a fit)"""
    import torch
    from smallk_amd.solver import masked_last_profile
    name = MC.FOLD_IN_CASE
    c, fitted = MC.case(name), _reference(name)
    W = fitted["W"]
    kw = dict(c["kw"], tol=1e-3, max_iter=25)
    ref = R.fit(c["csc"], W, c["H0"], update_W=False, order="pair", dtype=np.longdouble, **kw)
    dev = torch.device("cuda", 0)
    Wt, Ht = torch.from_numpy(W).to(dev), torch.from_numpy(c["H0"]).to(dev)
    mat = _matrix(gpu, name)
    try:
        r = gpu.nmf_masked(mat, Wt, Ht, update_W=False, inplace=True, **kw)
        fold = masked_last_profile()
        full = gpu.nmf_masked(mat, c["W0"], c["H0"], **c["kw"])
        fit = masked_last_profile()
    finally:
        mat.close()
    assert r.W is Wt and np.array_equal(Wt.cpu().numpy(), W)
    got = gpu.MaskedResult(W, Ht.cpu().numpy(), r.n_iter, r.converged, r.violation_init, r.violation, r.error)
    _compare(got, dict(ref, W=W), name + " update_W=False")
    assert r.n_iter > 1 and fold == (r.n_iter, 1) and fit == (2 * full.n_iter, 1)


# ---- views -------------------------------------------------------------------------------------------------------------------
def test_fp32_and_strided_views(gpu):
    """fp32 factor views, W the transpose of a k x m tensor, H every second column of a wider tensor, updated in place: the
    contiguous fp64 results rounded to fp32, bit for bit (the start is exact in fp32, the iteration runs in fp64 as ever)"""
    import torch
    name = MC.FP32_VIEW_CASE
    c = MC.case(name)
    dev = torch.device("cuda", 0)
    m, n, k = c["W0"].shape[0], c["H0"].shape[1], c["k"]
    mat = _matrix(gpu, name)
    try:
        W64, H64 = torch.from_numpy(c["W0"]).to(dev), torch.from_numpy(c["H0"]).to(dev)
        r64 = gpu.nmf_masked(mat, W64, H64, inplace=True, **c["kw"])
        W32 = torch.from_numpy(c["W0"]).to(dev, torch.float32).t().contiguous().t()
        wide = torch.full((k, 2 * n), -7.0, dtype=torch.float32, device=dev)
        wide[:, ::2] = torch.from_numpy(c["H0"]).to(dev, torch.float32)
        H32 = wide[:, ::2]
        assert W32.stride() == (1, m) and H32.stride() == (2 * n, 2)
        r32 = gpu.nmf_masked(mat, W32, H32, inplace=True, **c["kw"])
        assert r32.W is W32 and r32.H is H32
        assert torch.equal(W32, W64.float()) and torch.equal(H32, H64.float()) and bool((wide[:, 1::2] == -7.0).all())
        assert (r64.n_iter, r64.converged, r64.violation_init, r64.violation, r64.error) == (r32.n_iter, r32.converged, r32.violation_init, r32.violation, r32.error)
        # the residual of the rounded factors: fp32 strided views against the same values as contiguous fp64
        a = mat.masked_residual(W32, H32, per_column=True)
        b = mat.masked_residual(W32.double().contiguous(), H32.double().contiguous(), per_column=True)
        assert (a.resid_sq, a.norm_sq, a.count) == (b.resid_sq, b.norm_sq, b.count) and a.resid_sq > 0
        assert torch.equal(a.col_resid_sq, b.col_resid_sq) and torch.equal(a.col_norm_sq, b.col_norm_sq)
    finally:
        mat.close()


# ---- the rejection rows of tests/test_gpu_view_entries.py, for the two new entries ---------------------------------------------
M, N, K = 5, 7, 3
BAD_PARAM = -3
F64, F32, BF16, UNKNOWN = 0, 1, 2, 9
ENTRIES = {
    "nmf_masked": dict(prefix="smk_nmf_masked_device", output=True, options=True),
    "masked_residual": dict(prefix="smk_matrix_masked_residual_device", output=False, options=False),
}
OPTION_ROWS = [(dict(alpha_w=-1.0), ": alpha_w and alpha_h must be >= 0"), (dict(alpha_h=-1.0), ": alpha_w and alpha_h must be >= 0"),
               (dict(alpha_w=math.nan), ": alpha_w and alpha_h must be >= 0"), (dict(l1_ratio=1.5), ": l1_ratio must lie in [0, 1]"),
               (dict(l1_ratio=-0.5), ": l1_ratio must lie in [0, 1]"), (dict(tol=-1.0), ": tol must be >= 0"), (dict(max_iter=0), ": max_iter < 1")]


def _rows():
    out = []
    for name, e in ENTRIES.items():
        for i, vname in enumerate(("W", "H")):
            what = f"{e['prefix']}({vname})"
            out.append((f"{name}-{vname}-null", name, ("view", i, "null"), e["prefix"] + ": null argument"))
            out.append((f"{name}-{vname}-bf16", name, ("view", i, "bf16"), e["prefix"] + ": W and H are fp64 or fp32"))
            out.append((f"{name}-{vname}-unknown-dtype", name, ("view", i, "unknown"), e["prefix"] + ": W and H are fp64 or fp32"))
            out.append((f"{name}-{vname}-negative-stride", name, ("view", i, "negative"), what + ": negative stride"))
            if e["output"]:
                out.append((f"{name}-{vname}-zero-stride", name, ("view", i, "zero"), what + ": the elements of an output overlap"))
                out.append((f"{name}-{vname}-equal-strides", name, ("view", i, "equal"), what + ": the elements of an output overlap"))
            out.append((f"{name}-{vname}-host-pointer", name, ("view", i, "host"), what + ": not a pointer to memory of the current device"))
            out.append((f"{name}-{vname}-past-allocation", name, ("view", i, "past"), what + ": the strided extent leaves the allocation"))
        out.append((f"{name}-k0", name, ("k", 0), e["prefix"] + ": k < 1"))
        out.append((f"{name}-k-above-min", name, ("k", min(M, N) + 1), e["prefix"] + ": k exceeds min(m, n)"))
        if e["options"]:
            for j, (change, text) in enumerate(OPTION_ROWS):
                out.append((f"{name}-option-{j}-{next(iter(change))}", name, ("option", change), e["prefix"] + text))
    out.append(("masked_residual-one-column-output", "masked_residual", ("cols", None), "smk_matrix_masked_residual_device: both per-column outputs or neither"))
    return out


ROWS = _rows()


@pytest.fixture(scope="module")
def table(gpu):
    import torch

    class B:
        pass

    b = B()
    b.L, b.lib = gpu._lib, gpu._lib.lib()
    rng = np.random.default_rng(5)
    mask = rng.random((M, N)) < 0.4
    mask[np.arange(M), np.arange(M) % N] = True
    b.sparse = gpu.SparseMatrix.from_observed(rng.random((M, N)), mask)
    b.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.empty_cache()
    b.own = torch.zeros(20 * 2 ** 20 // 8, dtype=torch.float64, device="cuda")        # an allocation of its own: it ends where the tensor ends
    b.host = np.zeros(64)
    b.good = {(r, c): torch.rand((r, c), dtype=torch.float64, device="cuda") + 0.1 for r, c in ((M, K), (K, N))}
    b.col = torch.zeros(N, dtype=torch.float64, device="cuda")
    yield b
    b.sparse.close()


def _view(t):
    return [C.c_void_p(t.data_ptr()), {"torch.float64": F64, "torch.float32": F32}[str(t.dtype)], int(t.stride(0)), int(t.stride(1))]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_rejection_table(table, row):
    _, name, change, text = row
    b, e = table, ENTRIES[name]
    views = [_view(b.good[(M, K)]), _view(b.good[(K, N)])]
    before = [b.good[(M, K)].clone(), b.good[(K, N)].clone()]
    k = K
    o = dict(alpha_w=0.01, alpha_h=0.02, l1_ratio=0.5, tol=0.0, max_iter=3, update_w=1)
    cols = [C.c_void_p(b.col.data_ptr()), C.c_void_p(b.col.data_ptr())]
    if change[0] == "view":
        _, i, how = change
        rows_, cols_ = ((M, K), (K, N))[i]
        v = views[i]
        if how == "null":
            v[0] = None
        elif how == "bf16":
            v[1] = BF16
        elif how == "unknown":
            v[1] = UNKNOWN
        elif how == "negative":
            v[2] = -v[2]
        elif how == "zero":
            v[2] = 0
        elif how == "equal":
            v[2] = v[3] = 1
        elif how == "host":
            v[0] = C.c_void_p(b.host.ctypes.data)
        elif how == "past":
            v[0] = C.c_void_p(b.own.data_ptr() + (b.own.numel() - rows_ * cols_) * 8)
            v[2], v[3] = 1, rows_ + 1
    elif change[0] == "k":
        k = change[1]
    elif change[0] == "option":
        o.update(change[1])
    else:
        cols[1] = None
    if name == "nmf_masked":
        opt = b.L.CdOptions(o["alpha_w"], o["alpha_h"], o["l1_ratio"], o["tol"], o["max_iter"], o["update_w"])
        rc = b.lib.smk_nmf_masked_device(b.sparse._h, k, C.byref(opt), *views[0], *views[1], b.stream, C.byref(b.L.MaskedStats()))
    else:
        rc = b.lib.smk_matrix_masked_residual_device(b.sparse._h, k, *views[0], *views[1], cols[0], cols[1], b.stream, (C.c_double * 3)())
    got = b.lib.smk_last_error().decode()
    print(f"{row[0]}: rc {rc}, {got!r}")
    assert rc == BAD_PARAM
    assert got == text
    assert bool((b.good[(M, K)] == before[0]).all()) and bool((b.good[(K, N)] == before[1]).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_factors_untouched(gpu):
    import torch
    from smallk_amd import _lib as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    A = rng.integers(0, 8, (140, 130)).astype(np.float64)
    mask = rng.random(A.shape) < 0.3

    def attempt(mat, k, code, **kw):
        W = torch.from_numpy(rng.random((mat.height, k))).to(dev)
        H = torch.from_numpy(rng.random((k, mat.ncols))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(L.SmallkError) as e:
            gpu.nmf_masked(mat, W, H, inplace=True, **kw)
        assert e.value.code == code, (kw, e.value)
        assert bool((W == W0).all()) and bool((H == H0).all())
        return str(e.value)

    sparse = gpu.SparseMatrix.from_observed(A, mask)
    data, rows, indptr, shape = MC.csc_of(A, mask)
    j = int(np.argmax(np.diff(indptr) > 0))                    # the first entry of column j, stored twice
    p = int(indptr[j])
    twice = gpu.SparseMatrix(np.insert(data, p, data[p]), np.insert(rows, p, rows[p]), indptr + (np.arange(indptr.size) > j), shape)
    narrow = gpu.SparseMatrix.from_observed(A[:, :6], mask[:, :6])
    dense = gpu.DenseMatrix.from_host(A)
    try:
        assert "k > 128" in attempt(sparse, 129, L.UNSUPPORTED)
        assert "twice" in attempt(twice, 4, L.UNSUPPORTED)
        assert "exceeds min" in attempt(narrow, 7, L.BAD_PARAM)
        attempt(sparse, 4, L.BAD_PARAM, l1_ratio=1.5)
        attempt(sparse, 4, L.BAD_PARAM, alpha_W=-1e-3)
        attempt(sparse, 4, L.BAD_PARAM, alpha_W=0.0, alpha_H=-1e-3)
        attempt(sparse, 4, L.BAD_PARAM, max_iter=0)
        attempt(sparse, 4, L.BAD_PARAM, tol=-1.0)
        # a dense matrix: the wrapper refuses it by type, the library by SMK_UNSUPPORTED
        W, H = torch.from_numpy(rng.random((140, 4))).to(dev), torch.from_numpy(rng.random((4, 130))).to(dev)
        W0, H0 = W.clone(), H.clone()
        with pytest.raises(ValueError):
            gpu.nmf_masked(dense, W, H, inplace=True)
        o, st = L.CdOptions(0.0, 0.0, 0.0, 1e-4, 5, 1), L.MaskedStats()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.lib().smk_nmf_masked_device(dense._h, 4, C.byref(o), C.c_void_p(W.data_ptr()), F64, 4, 1, C.c_void_p(H.data_ptr()), F64, 130, 1, stream, C.byref(st))
        assert rc == L.UNSUPPORTED and "dense" in L.lib().smk_last_error().decode()
        rc = L.lib().smk_matrix_masked_residual_device(dense._h, 4, C.c_void_p(W.data_ptr()), F64, 4, 1, C.c_void_p(H.data_ptr()), F64, 130, 1, None, None, stream,
                                                       (C.c_double * 3)())
        assert rc == L.UNSUPPORTED
        assert bool((W == W0).all()) and bool((H == H0).all())
        with pytest.raises(L.SmallkError) as e:
            twice.masked_residual(W, H)
        assert e.value.code == L.UNSUPPORTED
        # negative stored values are served, as by nmf_cd
        neg = gpu.SparseMatrix.from_observed(A - 3.0, mask)
        try:
            r = gpu.nmf_masked(neg, W0, H0, max_iter=3)
            assert r.n_iter == 3 and np.isfinite(r.error) and bool((r.W >= 0).all()) and bool((r.H >= 0).all())
        finally:
            neg.close()
    finally:
        for mat in (sparse, twice, narrow, dense):
            mat.close()


# ---- the segment length (read once per process: fresh child processes) ---------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import smallk_amd
from smallk_amd import _lib as L
import masked_cases as MC
smallk_amd.initialize(0)
c = MC.case("k5")
mat = smallk_amd.SparseMatrix(*c["csc"])
try:
    r = smallk_amd.nmf_masked(mat, c["W0"], c["H0"], **c["kw"])
    np.savez(sys.argv[3], W=r.W, H=r.H, n_iter=r.n_iter)
    print("FIT", r.n_iter)
except L.SmallkError as e:
    print("REFUSED", e.code, e)
"""


def test_segment_lengths_above_64_are_refused_and_shorter_ones_served(gpu, tmp_path):
    """SMK_SPMM_SEG_LEN = 128: SMK_UNSUPPORTED with a text that names the switch; 32: more columns take the long path, the same fit"""
    import os
    import subprocess
    import sys
    from smallk_amd import _lib as L
    here = os.path.dirname(os.path.abspath(__file__))
    procs = {}
    for seg in (128, 32):
        env = dict(os.environ, SMK_SPMM_SEG_LEN=str(seg))
        procs[seg] = subprocess.Popen([sys.executable, "-c", _CHILD, os.path.dirname(here), here, str(tmp_path / f"seg{seg}.npz")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {seg: p.communicate(timeout=120)[0] for seg, p in procs.items()}
    assert all(p.returncode == 0 for p in procs.values()), out
    assert f"REFUSED {L.UNSUPPORTED}" in out[128] and "segments of at most 64 entries (SMK_SPMM_SEG_LEN)" in out[128], out[128]
    ref = _reference("k5")
    got = np.load(tmp_path / "seg32.npz")
    top = max(ref["W"].max(), ref["H"].max())
    assert int(got["n_iter"]) == ref["n_iter"]
    assert np.abs(got["W"] - ref["W"]).max() <= MC.FIT_BAR * top and np.abs(got["H"] - ref["H"]).max() <= MC.FIT_BAR * top


# ---- the example ---------------------------------------------------------------------------------------------------------------
def test_example_finds_the_planted_rank(gpu, capsys):
    """examples/choose_rank_by_holdout.py: the held-out error has its minimum at the planted rank (its own assertion), the training
    error keeps falling, and the zero-filled nmf_cd score stays far above"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "choose_rank_by_holdout.py")
    spec = importlib.util.spec_from_file_location("choose_rank_by_holdout", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    scores = ex.main()
    print(capsys.readouterr().out)
    assert min(scores, key=scores.get) == ex.RANK and scores[ex.RANK] < 1.2 * ex.NOISE and scores[ex.RANK - 1] > 1.5 * scores[ex.RANK]

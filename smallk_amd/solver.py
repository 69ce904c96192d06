"""Object wrappers over the C ABI: device-resident A and the NmfSolve<> solver.

Host-side mirror of the reference's inner seam (common/include/nmf.hpp:77-81,
common/include/nmf_solve_generic.hpp:34-140).  Numpy in/out, fp64, column-major.
All compute happens in libsmallk_amd.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L

ALGORITHMS = {"MU": L.ALG_MU, "HALS": L.ALG_HALS, "RANK2": L.ALG_RANK2, "BPP": L.ALG_BPP}
STORAGE = {"f32": L.STORE_F32, "fp32": L.STORE_F32, "bf16": L.STORE_BF16}


def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _tensor_view(t, what, *, ndim=2, kinds="float"):
    """(data_ptr, SMK_DT_* / SMK_IDX_* code, strides in elements) of a torch tensor in GPU memory.  Raises TypeError / ValueError
    before the library is called: not a tensor, a wrong rank, an element type the entry does not take, a CPU tensor, a tensor on
    another device than the library's.  torch is imported here, not with the package."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    codes = {"float": {torch.float64: L.DT_F64, torch.float32: L.DT_F32, torch.bfloat16: L.DT_BF16, torch.float16: L.DT_F16},
             "factor": {torch.float64: L.DT_F64, torch.float32: L.DT_F32},
             "index": {torch.int32: L.IDX_I32, torch.int64: L.IDX_I64}}[kinds]
    if t.layout != torch.strided:
        raise TypeError(f"{what}: expected a strided tensor, got layout {t.layout}")
    if t.dtype not in codes:
        raise TypeError(f"{what}: dtype {t.dtype} is not one of {sorted(str(d) for d in codes)}")
    if t.dim() != ndim:
        raise ValueError(f"{what}: expected {ndim} dimensions, got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{what}: empty tensor")
    if not t.is_cuda:
        raise ValueError(f"{what}: the tensor is on {t.device}; it must be in GPU memory")
    dev = L.lib().smk_current_device()
    if t.device.index != dev:
        raise ValueError(f"{what}: the tensor is on {t.device}, the library works on device {dev}")
    return C.c_void_p(t.data_ptr()), codes[t.dtype], tuple(int(x) for x in t.stride())


def _stream_of(t):
    """the stream torch is issuing work on for t's device: where t was produced / where a result will be consumed"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _is_tensor(x) -> bool:
    """a torch tensor, told without importing torch (a process that never made one has none to pass)"""
    return type(x).__module__.split(".")[0] == "torch"


@dataclass
class Residual:
    """||A - W H||_F^2 and ||A||_F^2 of a factorisation (stored values of A, fp64), and the former per column when asked for
    (a numpy array, or a torch tensor on the GPU when the factors were tensors)."""
    resid_sq: float
    a_sq: float
    col_resid_sq: object = None

    @property
    def norm(self) -> float:
        """||A - W H||_F"""
        return math.sqrt(self.resid_sq)

    @property
    def relative(self) -> float:
        """||A - W H||_F / ||A||_F; nan for an all-zero A"""
        return math.sqrt(self.resid_sq / self.a_sq) if self.a_sq > 0 else math.nan


@dataclass
class KlDivergence:
    """D(A || W H) of ``SparseMatrix.kl_divergence`` / ``DenseMatrix.kl_divergence`` and its two large terms: sum a log(a / w_i . h_j)
    over the stored entries and sum WH (D = a_log_ratio - sum a + sum_wh)."""
    divergence: float
    a_log_ratio: float
    sum_wh: float

    @property
    def error(self) -> float:
        """sqrt(2 max(D, 0)): scikit-learn's ``reconstruction_err_`` for this loss"""
        return math.sqrt(2.0 * max(self.divergence, 0.0))


@dataclass
class BetaDivergence:
    """D_beta(A || W H) of ``DenseMatrix.beta_divergence`` and the sums it is formed from.  beta = 0: (sum a / d, sum log(a / d),
    m n) with D = sums[0] - sums[2] - sums[1]; beta = 1: (sum a log(a / d), sum WH, 0); any other beta: (sum a^beta,
    sum a d^(beta - 1), sum d^beta) with D = (sums[0] - beta sums[1] + (beta - 1) sums[2]) / (beta (beta - 1))."""
    beta: float
    divergence: float
    sums: tuple

    @property
    def error(self) -> float:
        """sqrt(2 max(D, 0)): scikit-learn's ``reconstruction_err_`` for this loss"""
        return math.sqrt(2.0 * max(self.divergence, 0.0))


@dataclass
class MaskedResidual:
    """What ``SparseMatrix.masked_residual`` returns: the sum over the stored entries of (a - w_i . h_j)^2, of a^2, and their number;
    with ``per_column`` the first two per column (numpy arrays, or torch tensors on the GPU when the factors were tensors)."""
    resid_sq: float
    norm_sq: float
    count: int
    col_resid_sq: object = None
    col_norm_sq: object = None

    @property
    def rmse(self) -> float:
        """the root of the mean squared error over the stored entries; nan for a matrix without any"""
        return math.sqrt(self.resid_sq / self.count) if self.count > 0 else math.nan

    @property
    def relative(self) -> float:
        """sqrt(resid_sq / norm_sq); nan when every stored value is zero"""
        return math.sqrt(self.resid_sq / self.norm_sq) if self.norm_sq > 0 else math.nan


def _residual_factors(W, H, height, ncols, what):
    """The checks of ``DenseMatrix.residual`` made before the library is called: both factors on the host (array-likes of
    numbers) or both torch tensors, 2-D, W (height, k) and H (k, ncols) with k >= 1.  Returns (on_device, k)."""
    tw, th = _is_tensor(W), _is_tensor(H)
    if tw != th:
        raise TypeError(f"{what}: W and H must both be host arrays or both be torch tensors in GPU memory")
    if tw:
        for x, name in ((W, "W"), (H, "H")):
            if str(x.dtype) not in ("torch.float64", "torch.float32"):
                raise TypeError(f"{what}: {name} has dtype {x.dtype}; the factors are float64 or float32")
    else:
        for x, name in ((W, "W"), (H, "H")):
            kind = np.asarray(x).dtype.kind
            if kind not in "fiu":
                raise TypeError(f"{what}: {name} has dtype {np.asarray(x).dtype}; expected real numbers")
    ws, hs = tuple(W.shape) if hasattr(W, "shape") else np.shape(W), tuple(H.shape) if hasattr(H, "shape") else np.shape(H)
    if len(ws) != 2 or len(hs) != 2:
        raise ValueError(f"{what}: W and H must be 2-D, got shapes {ws} and {hs}")
    k = int(ws[1])
    if k < 1 or ws[0] != height or hs != (k, ncols):
        raise ValueError(f"{what}: W {ws} / H {hs} do not match ({height}, k) / (k, {ncols})")
    return tw, k


NNDSVD_VARIANTS = {"nndsvd": L.NNDSVD, "nndsvda": L.NNDSVDA}


def _svd_options(what, k, height, ncols, oversample, power_iters, seed, omega):
    """The checks of ``DenseMatrix.svd`` / ``nndsvd`` made before the library is called, and the ``smk_svd_options`` they fill.
    Integers are integers (TypeError otherwise) and non-negative (ValueError); ``omega`` is None or a 2-D float64 / float32 torch
    tensor in GPU memory (``_tensor_view``).  Its shape must be (ncols, min(k + oversample, height, ncols)): another shape is the
    library's SMK_BAD_PARAM, raised here because the C entry sees only a pointer and strides.  Returns (options, keep-alive)."""
    for name, v in (("k", k), ("oversample", oversample), ("power_iters", power_iters), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{what}: {name} must be an integer, got {type(v).__name__}")
    if oversample < 0 or power_iters < 0 or seed < 0:
        raise ValueError(f"{what}: oversample, power_iters and seed must be >= 0")
    o = L.SvdOptions(int(k), int(oversample), int(power_iters), int(seed), None, L.DT_F64, 0, 0)
    if omega is not None:
        ptr, dt, (rs, cs) = _tensor_view(omega, f"{what}(omega)", kinds="factor")
        l = min(int(k) + int(oversample), height, ncols)
        if 1 <= k <= min(height, ncols) and tuple(omega.shape) != (ncols, l):
            raise L.SmallkError(L.BAD_PARAM, what, f"omega has shape {tuple(omega.shape)}, expected ({ncols}, {l})")
        o.omega, o.omega_dtype, o.omega_rs, o.omega_cs = ptr, dt, rs, cs
    return o, omega


def _nndsvd_variant(what, variant):
    if variant not in NNDSVD_VARIANTS:
        raise ValueError(f"{what}: variant must be one of {sorted(NNDSVD_VARIANTS)}, got {variant!r}")
    return NNDSVD_VARIANTS[variant]


def _factor_tensor(t, what):
    """``_tensor_view(t, what, kinds="factor")`` for the labelling entries: a 2-D float64 / float32 torch tensor in GPU memory.
    Everything else -- not a tensor, another element type, another rank, an empty or a CPU tensor -- is a ValueError, raised
    before the library is loaded."""
    if not _is_tensor(t):
        raise ValueError(f"{what}: expected a torch tensor in GPU memory, got {type(t).__name__}")
    if str(t.dtype) not in ("torch.float64", "torch.float32"):
        raise ValueError(f"{what}: dtype {t.dtype}; the factors are float64 or float32")
    if t.dim() != 2:
        raise ValueError(f"{what}: expected 2 dimensions, got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{what}: empty tensor")
    if not t.is_cuda:
        raise ValueError(f"{what}: the tensor is on {t.device}; it must be in GPU memory")
    return _tensor_view(t, what, kinds="factor")


def _maxterms(maxterms, what):
    if isinstance(maxterms, bool) or not isinstance(maxterms, (int, np.integer)) or maxterms < 1:
        raise ValueError(f"{what}: maxterms must be an integer >= 1, got {maxterms!r}")
    return int(maxterms)


def labels_device(H, *, memberships=False):
    """Cluster labels of the columns of H (k, n), a float64 / float32 torch tensor in GPU memory (any strides): an int32 tensor
    (n,), label = row of the largest entry, the first one on ties -- ``flatclust.compute_assignments`` without the download and
    without its k <= n rule.  With ``memberships`` also P (k, n) float32, column c = column c of H scaled to sum 1, bit-equal to
    ``compute_fuzzy_assignments`` (NaN for an all-zero column); its memory is document-major as the host function's."""
    import torch
    hp, ht, (rs, cs) = _factor_tensor(H, "labels_device(H)")
    k, n = int(H.shape[0]), int(H.shape[1])
    labels = torch.empty(n, dtype=torch.int32, device=H.device)
    P = torch.empty((n, k), dtype=torch.float32, device=H.device) if memberships else None
    L.check(L.lib().smk_labels_device(hp, ht, rs, cs, k, n, _stream_of(H), C.c_void_p(labels.data_ptr()),
                                      C.c_void_p(P.data_ptr()) if memberships else None), "smk_labels_device")
    return (labels, P.t()) if memberships else labels


def top_terms_device(W, maxterms):
    """The indices of the ``maxterms`` largest entries of every column of W (m, k), a float64 / float32 torch tensor in GPU
    memory: an int32 tensor (k, maxterms), row j for topic j, largest first, equal entries by increasing index --
    ``flatclust.top_terms`` without the download.  Slots past min(maxterms, m) read -1."""
    import torch
    maxterms = _maxterms(maxterms, "top_terms_device")
    wp, wt, (rs, cs) = _factor_tensor(W, "top_terms_device(W)")
    m, k = int(W.shape[0]), int(W.shape[1])
    out = torch.full((k, maxterms), -1, dtype=torch.int32, device=W.device)
    L.check(L.lib().smk_top_terms_device(wp, wt, rs, cs, m, k, maxterms, _stream_of(W), C.c_void_p(out.data_ptr())),
            "smk_top_terms_device")
    return out


def initialize(device: int = -1):
    """NmfInitialize (nmf.hpp:71): select the GPU, create the stream.  Raises without a GPU."""
    L.check(L.lib().smk_initialize(device), "smk_initialize")


def is_initialized() -> bool:
    return L.lib().smk_is_initialized() == L.INITIALIZED


def finalize():
    L.lib().smk_finalize()


def thread_context_begin(device: int = -1):
    """this host thread gets a device context of its own (stream, handles) until thread_context_end()"""
    L.check(L.lib().smk_thread_context_begin(device), "smk_thread_context_begin")


def thread_context_end():
    L.lib().smk_thread_context_end()


def trim_device_cache() -> int:
    """Return the library's cached (freed) device workspaces of the current device to the HIP runtime; bytes that were cached."""
    return int(L.lib().smk_device_trim())


def set_stream(stream_ptr: int):
    L.check(L.lib().smk_set_stream(C.c_void_p(stream_ptr)), "smk_set_stream")


def uniform_host(rows, cols, seed, *, quant=0, r0=0, c0=0, gheight=None) -> np.ndarray:
    """Counter-based uniform [0,1) matrix on the host (RandomMatrix stand-in)."""
    out = np.empty((rows, cols), order="F")
    L.lib().smk_uniform_fill_host(_p(out), rows, rows, cols, r0, c0, rows if gheight is None else gheight, seed, quant)
    return out


def make_options(m, n, k, algorithm, *, min_iter=5, max_iter=5000, tol=0.005, tolcount=1,
                 prog_est=None, normalize=True, max_threads=1, verbose=False) -> L.Options:
    alg = ALGORITHMS[algorithm] if isinstance(algorithm, str) else int(algorithm)
    if prog_est is None:   # smallk::Nmf's rule (smallk/src/smallk.cpp:581-584)
        prog_est = L.PROG_DELTA_FNORM if alg == L.ALG_MU else L.PROG_PG_RATIO
    return L.Options(tol, alg, prog_est, m, n, k, min_iter, max_iter, tolcount, max_threads,
                     int(verbose), int(normalize))


class DenseMatrix:
    """A (or the column shard [col0, col0+ncols) of it) resident in HBM with its transpose."""

    def __init__(self, height, width_global, *, col0=0, ncols=None, storage="f32", single_copy=False):
        """single_copy: no stored transpose (bf16 or fp32 storage; serves MU, HALS and BPP with the 16-bit product forms; RANK2 and the
        accurate form build the transpose on demand -- smk_matrix_create_single_copy)"""
        self.height = int(height)
        self.width_global = int(width_global)
        self.col0 = int(col0)
        self.ncols = int(width_global - col0 if ncols is None else ncols)
        self.storage = STORAGE[storage] if isinstance(storage, str) else int(storage)
        self._h = C.c_void_p()
        create = L.lib().smk_matrix_create_single_copy if single_copy else L.lib().smk_matrix_create
        L.check(create(C.byref(self._h), self.height, self.width_global, self.col0, self.ncols, self.storage),
                "smk_matrix_create_single_copy" if single_copy else "smk_matrix_create")

    @property
    def single_copy(self) -> bool:
        return bool(L.lib().smk_matrix_is_single_copy(self._h))

    @property
    def device_bytes(self) -> int:
        return int(L.lib().smk_matrix_device_bytes(self._h))

    @classmethod
    def from_host(cls, A, *, storage="f32", single_copy=False):
        A = _f(A)
        mat = cls(A.shape[0], A.shape[1], storage=storage, single_copy=single_copy)
        mat.upload(A)
        return mat

    @classmethod
    def from_device(cls, t, *, storage="f32", single_copy=False):
        """The resident matrix of a 2-D torch tensor that is already in GPU memory (float64 / float32 / bfloat16 / float16, any
        strides): converted and transposed on the device, nothing crosses PCIe.  Same stored values as ``from_host`` of
        ``t.cpu().double()``.  Ordered after the work queued on torch's current stream; returns when the copy is done."""
        _tensor_view(t, "DenseMatrix.from_device")
        mat = cls(t.shape[0], t.shape[1], storage=storage, single_copy=single_copy)
        mat.adopt(t)
        return mat

    def adopt(self, t):
        """new contents from a torch tensor in GPU memory (the device twin of ``upload``)"""
        ptr, dt, (rs, cs) = _tensor_view(t, "DenseMatrix.adopt")
        if tuple(t.shape) != (self.height, self.ncols):
            raise ValueError(f"DenseMatrix.adopt: shape {tuple(t.shape)} does not match the matrix ({self.height}, {self.ncols})")
        L.check(L.lib().smk_matrix_adopt_device(self._h, ptr, dt, rs, cs, _stream_of(t)), "smk_matrix_adopt_device")

    def to_device(self, dtype=None, *, out=None):
        """the stored values as a torch tensor on the GPU (``dtype`` default torch.float32), or written into ``out`` (any strides)"""
        import torch
        if out is None:
            out = torch.empty((self.height, self.ncols), dtype=dtype or torch.float32,
                              device=torch.device("cuda", L.lib().smk_current_device()))
        ptr, dt, (rs, cs) = _tensor_view(out, "DenseMatrix.to_device")
        if tuple(out.shape) != (self.height, self.ncols):
            raise ValueError(f"DenseMatrix.to_device: out has shape {tuple(out.shape)}, the matrix ({self.height}, {self.ncols})")
        L.check(L.lib().smk_matrix_copy_to_device(self._h, ptr, dt, rs, cs, _stream_of(out)), "smk_matrix_copy_to_device")
        return out

    def upload(self, A_local):
        A_local = _f(A_local)
        assert A_local.shape == (self.height, self.ncols)
        L.check(L.lib().smk_matrix_upload_f64(self._h, _p(A_local), A_local.shape[0]), "smk_matrix_upload_f64")

    def fill_uniform(self, seed):
        L.check(L.lib().smk_matrix_fill_uniform(self._h, seed), "smk_matrix_fill_uniform")

    def fill_planted(self, seed, kstar, threshold=0.7, noise=0.05):
        """A = Ws Hs + noise U with sparse planted factors (entries <= threshold dropped), SURVEY 8(d)."""
        L.check(L.lib().smk_matrix_fill_planted(self._h, seed, kstar, threshold, noise), "smk_matrix_fill_planted")

    def download(self) -> np.ndarray:
        out = np.empty((self.height, self.ncols), order="F")
        L.check(L.lib().smk_matrix_download_f64(self._h, _p(out), self.height), "smk_matrix_download_f64")
        return out

    def residual(self, W, H, *, per_column=False) -> Residual:
        """||A - W H||_F^2 and ||A||_F^2 of the local columns, computed on the device in fp64 against the stored values of A
        (dense: one streaming read of A; sparse: over the stored entries; no m x n temporary either way).  W (height, k) and
        H (k, ncols): both numpy arrays, or both torch tensors in GPU memory (float64 or float32, any strides); with tensors
        the per-column values come back as a tensor on the GPU."""
        on_device, k = _residual_factors(W, H, self.height, self.ncols, "residual")
        r, a = C.c_double(0), C.c_double(0)
        if on_device:
            import torch
            wp, wt, (wrs, wcs) = _tensor_view(W, "residual(W)", kinds="factor")
            hp, ht, (hrs, hcs) = _tensor_view(H, "residual(H)", kinds="factor")
            col = torch.empty(self.ncols, dtype=torch.float64, device=W.device) if per_column else None
            L.check(L.lib().smk_matrix_residual_device(self._h, k, wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W), C.byref(r), C.byref(a),
                                                       C.c_void_p(col.data_ptr()) if per_column else None), "smk_matrix_residual_device")
        else:
            W, H = _f(W), _f(H)
            col = np.empty(self.ncols) if per_column else None
            L.check(L.lib().smk_matrix_residual(self._h, k, _p(W), W.shape[0], _p(H), H.shape[0], C.byref(r), C.byref(a),
                                                _p(col) if per_column else None), "smk_matrix_residual")
        return Residual(r.value, a.value, col)

    def kl_divergence(self, W, H) -> KlDivergence:
        """The generalised Kullback-Leibler divergence D(A || W H) = sum a log(a / w_i . h_j) - sum a + sum WH over every entry
        of the stored A (the terms of a = 0 are sum WH's alone), computed on the device in fp64 in one streaming read of A (dot
        products below 2^-23 count as 2^-23, as in scikit-learn).  W (height, k) and H (k, ncols): both numpy arrays, or both
        float64 / float32 torch tensors in GPU memory (any strides).  A single-copy matrix is served."""
        return self._kl_divergence("smk_matrix_kl_divergence_dense_device", W, H)

    def beta_divergence(self, W, H, beta_loss) -> "BetaDivergence":
        """The beta-divergence D_beta(A || W H) of ``nmf_beta_dense`` (``beta_loss`` as there) over the entries of the stored A with
        a > 2^-23, computed on the device in fp64 in one streaming read of A, with the three sums it is formed from.  W and H as in
        ``kl_divergence``.  A single-copy matrix is served."""
        beta = _beta_of("beta_divergence", beta_loss)
        if isinstance(self, SparseMatrix):
            raise ValueError("beta_divergence: takes a resident DenseMatrix (SparseMatrix has kl_divergence)")
        on_device, k = _residual_factors(W, H, self.height, self.ncols, "beta_divergence")
        if not on_device:
            import torch
            dev = torch.device("cuda", L.lib().smk_current_device())
            W = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(dev)
            H = torch.from_numpy(np.ascontiguousarray(H, dtype=np.float64)).to(dev)
        wp, wt, (wrs, wcs) = _tensor_view(W, "beta_divergence(W)", kinds="factor")
        hp, ht, (hrs, hcs) = _tensor_view(H, "beta_divergence(H)", kinds="factor")
        out = (C.c_double * 4)()
        entry = "smk_matrix_beta_divergence_dense_device"
        L.check(getattr(L.lib(), entry)(self._h, k, C.c_double(beta), wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W), out), entry)
        return BetaDivergence(beta, out[0], (out[1], out[2], out[3]))

    def _kl_divergence(self, entry, W, H) -> KlDivergence:
        on_device, k = _residual_factors(W, H, self.height, self.ncols, "kl_divergence")
        if not on_device:
            import torch
            dev = torch.device("cuda", L.lib().smk_current_device())
            W = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(dev)
            H = torch.from_numpy(np.ascontiguousarray(H, dtype=np.float64)).to(dev)
        wp, wt, (wrs, wcs) = _tensor_view(W, "kl_divergence(W)", kinds="factor")
        hp, ht, (hrs, hcs) = _tensor_view(H, "kl_divergence(H)", kinds="factor")
        out = (C.c_double * 3)()
        L.check(getattr(L.lib(), entry)(self._h, k, wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W), out), entry)
        return KlDivergence(out[0], out[1], out[2])

    def svd(self, k, *, oversample=8, power_iters=2, seed=0, omega=None):
        """The k leading singular triplets of the stored A, computed on the device in fp64 (randomised range finder with
        ``power_iters`` power iterations on min(k + oversample, m, n) columns; k + oversample <= 128): ``(U, S, V)`` with U (m, k)
        and V (n, k) float64 torch tensors on the GPU and S a numpy array, largest first.  The same bits on every call; no sign
        convention.  Triplets past the numerical rank of A come back as S = 0 with zero vectors.  ``omega``: the caller's test
        matrix (n, l), a float64 / float32 tensor in GPU memory, instead of the one drawn from ``seed``."""
        import torch
        o, keep = _svd_options("svd", k, self.height, self.ncols, oversample, power_iters, seed, omega)
        dev = torch.device("cuda", L.lib().smk_current_device())
        kk = max(int(k), 1)
        U = torch.empty((self.height, kk), dtype=torch.float64, device=dev)
        V = torch.empty((self.ncols, kk), dtype=torch.float64, device=dev)
        S = np.zeros(kk)
        L.check(L.lib().smk_matrix_svd_device(self._h, C.byref(o), C.c_void_p(U.data_ptr()), L.DT_F64, U.stride(0), U.stride(1), _p(S),
                                              C.c_void_p(V.data_ptr()), L.DT_F64, V.stride(0), V.stride(1), _stream_of(U)),
                "smk_matrix_svd_device")
        return U, S, V

    def nndsvd(self, k, *, variant="nndsvd", oversample=8, power_iters=2, seed=0, omega=None):
        """The NNDSVD start (Boutsidis & Gallopoulos 2008) of a rank-k factorisation from ``svd`` with the same arguments:
        ``(W0, H0)``, float64 torch tensors on the GPU, W0 (m, k) and H0 (k, n).  ``variant``: "nndsvd" keeps the zeros,
        "nndsvda" replaces them by mean(A).  Deterministic: no seed files, the same start on every run."""
        import torch
        v = _nndsvd_variant("nndsvd", variant)
        o, keep = _svd_options("nndsvd", k, self.height, self.ncols, oversample, power_iters, seed, omega)
        dev = torch.device("cuda", L.lib().smk_current_device())
        kk = max(int(k), 1)
        W = torch.empty((self.height, kk), dtype=torch.float64, device=dev)
        H = torch.empty((kk, self.ncols), dtype=torch.float64, device=dev)
        L.check(L.lib().smk_matrix_nndsvd_device(self._h, C.byref(o), v, C.c_void_p(W.data_ptr()), L.DT_F64, W.stride(0), W.stride(1),
                                                 C.c_void_p(H.data_ptr()), L.DT_F64, H.stride(0), H.stride(1), _stream_of(W)),
                "smk_matrix_nndsvd_device")
        return W, H

    def close(self):
        if self._h:
            L.lib().smk_matrix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SparseMatrix(DenseMatrix):
    """Sparse A in CSC (scipy.sparse.csc_matrix or (data, indices, indptr, shape)), resident in HBM with
    its transpose.  Shares the NmfSolver interface with DenseMatrix."""

    def __init__(self, data, indices, indptr, shape, *, col0=0, width_global=None):
        self.height = int(shape[0])
        self.ncols = int(shape[1])
        self.width_global = int(width_global if width_global is not None else shape[1])
        self.col0 = int(col0)
        self.storage = L.STORE_F32
        d = np.ascontiguousarray(data, dtype=np.float64)
        ri = np.ascontiguousarray(indices, dtype=np.uint32)
        co = np.ascontiguousarray(indptr, dtype=np.uint32)
        self.nnz = int(co[-1] - co[0])
        self._h = C.c_void_p()
        L.check(L.lib().smk_matrix_create_sparse(C.byref(self._h), self.height, self.width_global, self.col0,
                                                 self.ncols, self.nnz, co.ctypes.data_as(C.POINTER(C.c_uint)),
                                                 ri.ctypes.data_as(C.POINTER(C.c_uint)), _p(d)),
                "smk_matrix_create_sparse")

    @classmethod
    def from_device(cls, ccol_indices, row_indices=None, values=None, shape=None):
        """CSC arrays that are already in GPU memory: 1-D torch tensors (int32 / int64 offsets and row indices, float values) and
        ``shape``, or one ``torch.sparse_csc_tensor``.  The index arrays are checked on the device before anything reads through
        them; bad arrays raise SmallkError(BAD_PARAM)."""
        import torch
        if isinstance(ccol_indices, torch.Tensor) and ccol_indices.layout == torch.sparse_csc:
            t = ccol_indices
            if t.dim() != 2:
                raise ValueError(f"SparseMatrix.from_device: expected a 2-D sparse tensor, got shape {tuple(t.shape)}")
            ccol_indices, row_indices, values, shape = t.ccol_indices(), t.row_indices(), t.values(), tuple(t.shape)
        if row_indices is None or values is None or shape is None:
            raise TypeError("SparseMatrix.from_device: ccol_indices, row_indices, values and shape, or a sparse CSC tensor")
        views = []
        for t, what, kinds in ((ccol_indices, "ccol_indices", "index"), (row_indices, "row_indices", "index"), (values, "values", "float")):
            _tensor_view(t, f"SparseMatrix.from_device({what})", ndim=1, kinds=kinds)
            t = t.contiguous()
            views.append((t,) + _tensor_view(t, f"SparseMatrix.from_device({what})", ndim=1, kinds=kinds))
        (co, co_p, co_t, _), (ri, ri_p, ri_t, _), (va, va_p, va_t, _) = views
        self = cls.__new__(cls)
        self.height, self.ncols = int(shape[0]), int(shape[1])
        self.width_global, self.col0, self.storage = self.ncols, 0, L.STORE_F32
        if co.numel() != self.ncols + 1 or ri.numel() != va.numel():
            raise ValueError("SparseMatrix.from_device: ccol_indices needs shape[1] + 1 entries, row_indices as many as values")
        self.nnz = int(va.numel())
        self._h = C.c_void_p()
        L.check(L.lib().smk_matrix_create_sparse_device(C.byref(self._h), self.height, self.ncols, self.nnz, co_p, co_t, ri_p, ri_t,
                                                        va_p, va_t, _stream_of(va)), "smk_matrix_create_sparse_device")
        return self

    @classmethod
    def from_scipy(cls, A):
        A = A.tocsc()
        return cls(A.data, A.indices, A.indptr, A.shape)

    @classmethod
    def from_observed(cls, X, mask):
        """The matrix whose stored entries are the entries of the dense array ``X`` where the boolean array ``mask`` is true -- the
        observed ones, for ``nmf_masked``.  An observed 0 is stored as a zero: it is a measurement, not a gap."""
        X = np.asarray(X, dtype=np.float64)
        mask = np.asarray(mask)
        if X.ndim != 2 or mask.shape != X.shape or mask.dtype != np.bool_:
            raise ValueError(f"SparseMatrix.from_observed: X {X.shape} must be 2-D and mask {mask.shape} a boolean array of its shape")
        cols, rows = np.nonzero(mask.T)                  # column by column, rows ascending
        indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=0))])
        return cls(X[rows, cols], rows, indptr, X.shape)

    def masked_residual(self, W, H, *, per_column=False) -> MaskedResidual:
        """The squared error of W H over the STORED entries of this matrix only, stored zeros included, computed on the device in
        fp64: the held-out score of ``nmf_masked`` when this matrix holds the entries withheld from the fit.  W (height, k) and
        H (k, ncols): both numpy arrays, or both float64 / float32 torch tensors in GPU memory (any strides).  The matrix must
        store no entry twice."""
        import torch
        what = "masked_residual"
        on_device, k = _residual_factors(W, H, self.height, self.ncols, what)
        dev = torch.device("cuda", L.lib().smk_current_device())
        if not on_device:
            W = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(dev)
            H = torch.from_numpy(np.ascontiguousarray(H, dtype=np.float64)).to(dev)
        wp, wt, (wrs, wcs) = _tensor_view(W, f"{what}(W)", kinds="factor")
        hp, ht, (hrs, hcs) = _tensor_view(H, f"{what}(H)", kinds="factor")
        cr = torch.empty(self.ncols, dtype=torch.float64, device=W.device) if per_column else None
        ca = torch.empty(self.ncols, dtype=torch.float64, device=W.device) if per_column else None
        out = (C.c_double * 3)()
        entry = "smk_matrix_masked_residual_device"
        L.check(getattr(L.lib(), entry)(self._h, k, wp, wt, wrs, wcs, hp, ht, hrs, hcs, C.c_void_p(cr.data_ptr()) if per_column else None,
                                        C.c_void_p(ca.data_ptr()) if per_column else None, _stream_of(W), out), entry)
        if per_column and not on_device:
            cr, ca = cr.cpu().numpy(), ca.cpu().numpy()
        return MaskedResidual(out[0], out[1], int(out[2]), cr, ca)

    def product(self, X, *, transposed=False, reps=0):
        """The sparse Gemm by itself: X (k x height) * A, or with ``transposed`` X (k x width) * A'; returns the k x ncols
        result and, for reps > 0, the average launch time in ms (smk_matrix_sparse_product)."""
        X = _f(X)
        k = X.shape[0]
        assert X.shape[1] == (self.ncols if transposed else self.height)
        out = np.zeros((k, self.height if transposed else self.ncols), order="F")
        ms = C.c_double(0)
        L.check(L.lib().smk_matrix_sparse_product(self._h, int(transposed), k, _p(X), k, _p(out), k, int(reps),
                                                  C.byref(ms) if reps > 0 else None), "smk_matrix_sparse_product")
        return (out, ms.value) if reps > 0 else out

    def kl_divergence(self, W, H) -> KlDivergence:
        """The generalised Kullback-Leibler divergence D(A || W H) = sum a log(a / w_i . h_j) - sum a + sum WH over the stored
        entries of A, computed on the device in fp64 (dot products below 2^-23 count as 2^-23, as in scikit-learn).  W (height, k)
        and H (k, ncols): both numpy arrays, or both float64 / float32 torch tensors in GPU memory (any strides)."""
        return self._kl_divergence("smk_matrix_kl_divergence_device", W, H)


def load_matrix_market(path):
    """MatrixMarket coordinate file -> (data, indices, indptr, (height, width)) in CSC."""
    h, w, nz = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    p = str(path).encode()
    if L.lib().smk_load_matrix_market(p, C.byref(h), C.byref(w), C.byref(nz), None, None, None) != 1:
        raise RuntimeError(f"could not load MatrixMarket file {path}")
    indptr = np.zeros(w.value + 1, dtype=np.uint32)
    indices = np.zeros(nz.value, dtype=np.uint32)
    data = np.zeros(nz.value, dtype=np.float64)
    L.lib().smk_load_matrix_market(p, C.byref(h), C.byref(w), C.byref(nz), indptr.ctypes.data_as(C.POINTER(C.c_uint)),
                                   indices.ctypes.data_as(C.POINTER(C.c_uint)), _p(data))
    return data, indices, indptr, (h.value, w.value)


def nmf_sparse(A, W0, H0, algorithm, **kw):
    """One-shot sparse NMF = ``NmfSparse(...)`` (common/src/nmf.cpp:232-300); A is a scipy sparse matrix."""
    A = A.tocsc()
    W = _f(W0).copy(order="F")
    H = _f(H0).copy(order="F")
    m, n = A.shape
    k = W.shape[1]
    o = make_options(m, n, k, algorithm, **kw)
    st = L.Stats()
    d = np.ascontiguousarray(A.data, dtype=np.float64)
    ri = np.ascontiguousarray(A.indices, dtype=np.uint32)
    co = np.ascontiguousarray(A.indptr, dtype=np.uint32)
    rc = L.lib().smk_nmf_sparse(C.byref(o), m, n, d.size, co.ctypes.data_as(C.POINTER(C.c_uint)),
                                ri.ctypes.data_as(C.POINTER(C.c_uint)), _p(d), _p(W), m, _p(H), k, C.byref(st))
    if rc not in (L.OK, L.FAILURE, L.BAD_PARAM, L.NOTINITIALIZED, L.SIZE_TOO_LARGE):
        L.check(rc, "smk_nmf_sparse")
    return NmfResult(rc, W, H, st.iteration_count, st.elapsed_us)


@dataclass
class NmfResult:
    result: int
    W: np.ndarray
    H: np.ndarray
    iteration_count: int
    elapsed_us: int


class NmfSolver:
    """One NmfSolve<> instance bound to a DenseMatrix."""

    def __init__(self, A: DenseMatrix, options: L.Options):
        self.A = A
        self.options = options
        self.k = options.k
        self._h = C.c_void_p()
        self._cb = None
        L.check(L.lib().smk_solver_create(C.byref(self._h), C.byref(options), A._h), "smk_solver_create")

    def set_factors(self, W0, H0_local):
        W0, H0 = _f(W0), _f(H0_local)
        assert W0.shape == (self.A.height, self.k) and H0.shape == (self.k, self.A.ncols)
        L.check(L.lib().smk_solver_set_factors(self._h, _p(W0), W0.shape[0], _p(H0), H0.shape[0]),
                "smk_solver_set_factors")

    def set_factors_device(self, W0, H0_local):
        """``set_factors`` from torch tensors in GPU memory (float64 or float32, any strides): W0 (m, k), H0 (k, ncols)"""
        wp, wt, (wrs, wcs) = _tensor_view(W0, "set_factors_device(W0)", kinds="factor")
        hp, ht, (hrs, hcs) = _tensor_view(H0_local, "set_factors_device(H0)", kinds="factor")
        if tuple(W0.shape) != (self.A.height, self.k) or tuple(H0_local.shape) != (self.k, self.A.ncols):
            raise ValueError(f"set_factors_device: W0 {tuple(W0.shape)} / H0 {tuple(H0_local.shape)} do not match "
                             f"({self.A.height}, {self.k}) / ({self.k}, {self.A.ncols})")
        L.check(L.lib().smk_solver_set_factors_device(self._h, wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W0)),
                "smk_solver_set_factors_device")

    def set_factors_nndsvd(self, variant="nndsvd", *, oversample=8, power_iters=2, seed=0, omega=None):
        """The NNDSVD start of ``A.nndsvd(k, ...)`` as the initial factors, built and handed over on the device: the solver is
        left exactly as ``set_factors_device(*A.nndsvd(k, ...))`` leaves it."""
        v = _nndsvd_variant("set_factors_nndsvd", variant)
        o, keep = _svd_options("set_factors_nndsvd", self.k, self.A.height, self.A.ncols, oversample, power_iters, seed, omega)
        L.check(L.lib().smk_solver_set_factors_nndsvd(self._h, C.byref(o), v), "smk_solver_set_factors_nndsvd")

    def factors_device(self, normalize=False, dtype=None):
        """``factors`` as torch tensors on the GPU: W (m, k) and H (k, ncols), float64 (default) or float32 = the fp64 factor
        rounded to nearest even.  They never visit the host."""
        import torch
        dev = torch.device("cuda", L.lib().smk_current_device())
        W = torch.empty((self.A.height, self.k), dtype=dtype or torch.float64, device=dev)
        H = torch.empty((self.k, self.A.ncols), dtype=dtype or torch.float64, device=dev)
        wp, wt, (wrs, wcs) = _tensor_view(W, "factors_device", kinds="factor")
        hp, ht, (hrs, hcs) = _tensor_view(H, "factors_device", kinds="factor")
        rc = L.lib().smk_solver_get_factors_device(self._h, int(normalize), wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W))
        if rc not in (L.OK, L.FAILURE):
            L.check(rc, "smk_solver_get_factors_device")
        return W, H

    def set_factors_uniform(self, seed_w, seed_h):
        """W0 / H0 = uniform_host(m, k, seed_w) / uniform_host(k, n, seed_h), generated on the device"""
        L.check(L.lib().smk_solver_set_factors_uniform(self._h, seed_w, seed_h), "smk_solver_set_factors_uniform")

    def run(self):
        st = L.Stats()
        rc = L.lib().smk_solver_run(self._h, C.byref(st))
        return rc, st.iteration_count, st.elapsed_us

    def iterate(self, iters):
        L.check(L.lib().smk_solver_iterate(self._h, iters), "smk_solver_iterate")

    def iterate_checked(self, iters) -> float:
        """`iters` iterations with the stopping rule's metric formed and read back after each (never stopping); returns the last metric"""
        v = C.c_double(0)
        L.check(L.lib().smk_solver_iterate_checked(self._h, iters, C.byref(v)), "smk_solver_iterate_checked")
        return v.value

    def sync(self):
        return L.lib().smk_solver_sync(self._h)

    def progress(self) -> float:
        v = C.c_double(0)
        L.check(L.lib().smk_solver_progress(self._h, C.byref(v)), "smk_solver_progress")
        return v.value

    def progress_sums(self):
        """The scalars of the stopping-rule check evaluated last and the estimator's first norm: (projected-gradient sum of W,
        of H, ||W - Wprev||^2, ||W||^2, pg0); the pair the rule does not use reads 0.  Host state only.  Raises
        SmallkError(BAD_PARAM) before any check, SmallkError(UNSUPPORTED) after a run the resident RANK2 kernel finished."""
        out = (C.c_double * 5)()
        L.check(L.lib().smk_solver_progress_sums(self._h, out), "smk_solver_progress_sums")
        return tuple(out)

    def factors(self, normalize=False):
        W = np.empty((self.A.height, self.k), order="F")
        H = np.empty((self.k, self.A.ncols), order="F")
        rc = L.lib().smk_solver_get_factors(self._h, int(normalize), _p(W), W.shape[0], _p(H), H.shape[0])
        if rc not in (L.OK, L.FAILURE):
            L.check(rc, "smk_solver_get_factors")
        return W, H

    def labels_device(self, normalize=True, memberships=False):
        """``labels_device`` of the solver's resident H (the local columns), no copy of it; ``normalize`` as in ``factors`` (the
        clustering flows label from normalised factors)."""
        import torch
        dev = torch.device("cuda", L.lib().smk_current_device())
        n = self.A.ncols
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        P = torch.empty((n, self.k), dtype=torch.float32, device=dev) if memberships else None
        L.check(L.lib().smk_solver_labels(self._h, int(normalize), _stream_of(labels), C.c_void_p(labels.data_ptr()),
                                          C.c_void_p(P.data_ptr()) if memberships else None), "smk_solver_labels")
        return (labels, P.t()) if memberships else labels

    def top_terms_device(self, maxterms, normalize=True):
        """``top_terms_device`` of the solver's resident W, no copy of it"""
        import torch
        maxterms = _maxterms(maxterms, "top_terms_device")
        out = torch.full((self.k, maxterms), -1, dtype=torch.int32, device=torch.device("cuda", L.lib().smk_current_device()))
        L.check(L.lib().smk_solver_top_terms(self._h, int(normalize), maxterms, _stream_of(out), C.c_void_p(out.data_ptr())),
                "smk_solver_top_terms")
        return out

    def project(self):
        """H := argmin_{H >= 0} ||A - W H||_F with the solver's W fixed (BPP solvers): one exact block-pivoting solve, warm
        start = the current H.  W and ``iteration_count`` stay.  Raises SmallkError(FAILURE) for a rank-deficient W."""
        L.check(L.lib().smk_solver_project_h(self._h), "smk_solver_project_h")

    @property
    def iteration_count(self) -> int:
        return int(L.lib().smk_solver_iteration_count(self._h))

    def residual(self, per_column=False) -> Residual:
        """``A.residual`` of the solver's current factors (not normalised), taken on the device; the solver is left exactly as
        it was.  Not for a solver with a communicator attached; a plain column shard returns its local sums."""
        r, a = C.c_double(0), C.c_double(0)
        col = np.empty(self.A.ncols) if per_column else None
        L.check(L.lib().smk_solver_residual(self._h, C.byref(r), C.byref(a), _p(col) if per_column else None), "smk_solver_residual")
        return Residual(r.value, a.value, col)

    def product_form(self):
        """(form, guard_checks, guard_fired, cond x delta of the last check); form: 3 bf16x3, 4 fp16 two-term, 8 accurate"""
        c, f, v = C.c_int(0), C.c_int(0), C.c_double(0)
        form = L.lib().smk_solver_product_form(self._h, C.byref(c), C.byref(f), C.byref(v))
        return form, c.value, f.value, v.value

    def enable_timing(self, on=True):
        L.check(L.lib().smk_solver_enable_timing(self._h, int(on)), "smk_solver_enable_timing")

    def kernel_time(self, which):
        ms, cnt = C.c_double(0), C.c_int(0)
        L.check(L.lib().smk_solver_kernel_time(self._h, which, C.byref(ms), C.byref(cnt)), "smk_solver_kernel_time")
        return ms.value, cnt.value

    def kernel_name(self, which) -> str:
        """the kernel pass `which` (0 = W'A, 1 = H*At) launches; which = 2: how the stopping-rule checks were formed so far (counts per route)"""
        buf = C.create_string_buffer(512)
        L.check(L.lib().smk_solver_kernel_name(self._h, which, buf, 512), "smk_solver_kernel_name")
        return buf.value.decode()

    def kernel_work(self, which):
        b, f = C.c_double(0), C.c_double(0)
        L.check(L.lib().smk_solver_kernel_work(self._h, which, C.byref(b), C.byref(f)), "smk_solver_kernel_work")
        return b.value, f.value

    def comm_workspace_bytes(self) -> int:
        n = C.c_size_t(0)
        L.check(L.lib().smk_solver_comm_workspace_bytes(self._h, C.byref(n)), "smk_solver_comm_workspace_bytes")
        return n.value

    def set_comm(self, rank, world, callback, workspace_ptr, workspace_bytes):
        """callback(ptr:int, count:int, dtype:int) -> 0 on success; kept alive by this object."""
        def _tramp(_user, ptr, count, dtype):
            try:
                return int(callback(ptr, count, dtype) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                print("all-reduce callback failed:", e, flush=True)
                return 1
        self._cb = L.ALLREDUCE_FN(_tramp)
        L.check(L.lib().smk_solver_set_comm(self._h, rank, world, self._cb, None, C.c_void_p(workspace_ptr),
                                            workspace_bytes), "smk_solver_set_comm")

    def attach_comm(self, comm):
        """Native collectives (RCCL / in-process stand-in); call before set_factors()."""
        L.check(L.lib().smk_solver_attach_comm(self._h, comm._h), "smk_solver_attach_comm")
        self._comm = comm          # keep alive

    def close(self):
        if self._h:
            L.lib().smk_solver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nmf(A, W0, H0, algorithm, *, storage="f32", **kw) -> NmfResult:
    """One-shot dense NMF = ``Nmf(NmfOptions, A, W, H, stats)`` (common/src/nmf.cpp:173-229)."""
    A = _f(A)
    W = _f(W0).copy(order="F")
    H = _f(H0).copy(order="F")
    m, n = A.shape
    k = W.shape[1]
    o = make_options(m, n, k, algorithm, **kw)
    st = L.Stats()
    stg = STORAGE[storage] if isinstance(storage, str) else int(storage)
    rc = L.lib().smk_nmf_dense(C.byref(o), _p(A), m, _p(W), m, _p(H), k, C.byref(st), stg)
    if rc not in (L.OK, L.FAILURE, L.BAD_PARAM, L.NOTINITIALIZED, L.SIZE_TOO_LARGE):
        L.check(rc, "smk_nmf_dense")
    return NmfResult(rc, W, H, st.iteration_count, st.elapsed_us)


def relative_error(A, W, H) -> float:
    """||A - W H||_F / ||A||_F of a resident matrix (DenseMatrix or SparseMatrix) and factors on the host or on the GPU: the
    short form of ``A.residual(W, H).relative``"""
    return A.residual(W, H).relative


def nmf_device(A, W0, H0, algorithm, *, storage="f32", **kw) -> NmfResult:
    """One-shot NMF of a torch tensor that is already in GPU memory: A dense (2-D, any float type, any strides) or a sparse CSC
    tensor, W0 (m, k) and H0 (k, n) float64 or float32 tensors.  The steps of ``nmf`` / ``nmf_sparse``; the factors come back as
    tensors of W0's dtype and never leave the device."""
    import torch
    sparse = isinstance(A, torch.Tensor) and A.layout == torch.sparse_csc
    if not sparse:
        _tensor_view(A, "nmf_device(A)")
    _tensor_view(W0, "nmf_device(W0)", kinds="factor")
    _tensor_view(H0, "nmf_device(H0)", kinds="factor")
    mat = SparseMatrix.from_device(A) if sparse else DenseMatrix.from_device(A, storage=storage)
    solver = None
    try:
        o = make_options(mat.height, mat.ncols, int(W0.shape[1]), algorithm, **kw)
        if not L.lib().smk_is_valid(C.byref(o), 1):
            return NmfResult(L.BAD_PARAM, W0, H0, 0, 0)
        solver = NmfSolver(mat, o)
        solver.set_factors_device(W0, H0)
        rc, iters, us = solver.run()
        if rc not in (L.OK, L.FAILURE):
            L.check(rc, "smk_solver_run")
        W, H = solver.factors_device(dtype=W0.dtype)     # like the reference, the last iterate even when the solver reports failure
        return NmfResult(rc, W, H, iters, us)
    finally:
        if solver is not None:
            solver.close()
        mat.close()


def transform(A, W, *, H0=None):
    """Fold new documents into a trained model: H = argmin_{H >= 0} ||A - W H||_F for the columns of A, a resident
    ``DenseMatrix`` / ``SparseMatrix``, and W (m, k) a torch tensor in GPU memory or a numpy array.  Returns H (k, ncols) as a
    float64 tensor on the GPU.  H0 (k, ncols, tensor or array; default zeros) is only the warm start of the block-pivoting
    solve.  A BPP solver is built for the call, so its rule k <= ncols applies."""
    if not isinstance(A, DenseMatrix):
        raise ValueError(f"transform: A must be a resident DenseMatrix / SparseMatrix, got {type(A).__name__}")

    def check(X, name, shape):
        if _is_tensor(X):
            _factor_tensor(X, f"transform({name})")
        else:
            X = np.asarray(X)
            if X.dtype.kind not in "fiu":
                raise ValueError(f"transform({name}): dtype {X.dtype}; expected real numbers")
            X = np.ascontiguousarray(X, dtype=np.float64)
        if len(X.shape) != 2 or (shape[0] is not None and X.shape[0] != shape[0]) or (shape[1] is not None and X.shape[1] != shape[1]):
            raise ValueError(f"transform({name}): shape {tuple(X.shape)} does not match {shape}")
        return X

    W = check(W, "W", (A.height, None))
    k = int(W.shape[1])
    if k < 1:
        raise ValueError("transform(W): k < 1")
    if H0 is not None:
        H0 = check(H0, "H0", (k, A.ncols))
    import torch
    dev = torch.device("cuda", L.lib().smk_current_device())
    Wt = W if _is_tensor(W) else torch.from_numpy(W).to(dev)
    if H0 is None:
        H0t = torch.zeros((k, A.ncols), dtype=torch.float64, device=dev)
    else:
        H0t = H0 if _is_tensor(H0) else torch.from_numpy(H0).to(dev)
    solver = NmfSolver(A, make_options(A.height, A.width_global, k, "BPP"))
    try:
        solver.set_factors_device(Wt, H0t)
        solver.project()
        return solver.factors_device()[1]
    finally:
        solver.close()


def _penalised_fit(what, kind, entry, stats_type, last_two, result_type, A, W0, H0, *, alpha_W, alpha_H, l1_ratio, tol, max_iter, update_W, inplace,
                   before_options=()):
    """What ``nmf_cd`` and ``nmf_kl`` share: the checks made before the library is called, the start as tensors on the GPU, the options,
    the C entry ``entry`` with its statistics struct and the result as ``result_type(W, H, n_iter, converged, *last_two(stats))``.
    ``before_options``: what the entry takes between k and the options (``nmf_beta_dense``: beta)."""
    if not isinstance(A, DenseMatrix):
        raise ValueError(f"{what}: A must be a resident {kind}, got {type(A).__name__}")
    on_device, k = _residual_factors(W0, H0, A.height, A.ncols, what)
    if inplace and not on_device:
        raise ValueError(f"{what}: inplace needs torch tensors")
    import torch
    if alpha_H == "same":
        alpha_H = alpha_W
    o = L.PenaltyOptions(float(alpha_W), float(alpha_H), float(l1_ratio), float(tol), int(max_iter), int(bool(update_W)))
    if on_device:
        W, H = (W0, H0) if inplace else (W0.clone(), H0.clone())
    else:
        dev = torch.device("cuda", L.lib().smk_current_device())
        W = torch.from_numpy(np.ascontiguousarray(W0, dtype=np.float64)).to(dev)
        H = torch.from_numpy(np.ascontiguousarray(H0, dtype=np.float64)).to(dev)
    wp, wt, (wrs, wcs) = _tensor_view(W, f"{what}(W0)", kinds="factor")
    hp, ht, (hrs, hcs) = _tensor_view(H, f"{what}(H0)", kinds="factor")
    st = stats_type()
    L.check(getattr(L.lib(), entry)(A._h, k, *before_options, C.byref(o), wp, wt, wrs, wcs, hp, ht, hrs, hcs, _stream_of(W), C.byref(st)), entry)
    if not on_device:
        W, H = W.cpu().numpy(), H.cpu().numpy()
    return result_type(W, H, st.iterations, bool(st.converged), *last_two(st))


def _last_profile(entry):
    """the two counters ``entry`` (smk_cd_last_profile / smk_kl_last_profile / smk_kl_dense_last_profile) reports for this thread's last run"""
    p, s = C.c_int(0), C.c_int(0)
    L.check(getattr(L.lib(), entry)(C.byref(p), C.byref(s)), entry)
    return p.value, s.value


@dataclass
class CdResult:
    """What ``nmf_cd`` returns: the factors (numpy arrays, or torch tensors on the GPU when the start was tensors), the iterations
    run (sklearn's ``n_iter_``), whether the stopping rule ended them, and the violation of iteration 1 and of the last one."""
    W: object
    H: object
    n_iter: int
    converged: bool
    violation_init: float
    violation: float


def nmf_cd(A, W0, H0, *, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, inplace=False) -> CdResult:
    """Regularised NMF by cyclic coordinate descent -- scikit-learn's ``solver="cd"`` with ``shuffle=False`` -- on a resident
    ``DenseMatrix`` / ``SparseMatrix`` A (m, n), from the start W0 (m, k), H0 (k, n): both numpy arrays, or both float64 / float32
    torch tensors in GPU memory (any strides).  Minimises

        1/2 ||A - W H||_F^2 + n alpha_W l1_ratio ||W||_1 + m alpha_H l1_ratio ||H||_1
                            + 1/2 n alpha_W (1 - l1_ratio) ||W||_F^2 + 1/2 m alpha_H (1 - l1_ratio) ||H||_F^2

    which is ``sklearn.decomposition.NMF`` on X = A' with sklearn's ``alpha_W`` = this ``alpha_H`` and its ``alpha_H`` = this
    ``alpha_W``, W_sklearn = H' and ``components_`` = W'.  ``alpha_H="same"`` takes ``alpha_W``.  ``update_W=False``: W stays, only H is
    fitted (fold-in).  The start is not modified unless ``inplace`` (tensors only): then W0 / H0 receive the result."""
    return _penalised_fit("nmf_cd", "DenseMatrix / SparseMatrix", "smk_nmf_cd_device", L.CdStats, lambda st: (st.violation_init, st.violation), CdResult,
                          A, W0, H0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, tol=tol, max_iter=max_iter, update_W=update_W, inplace=inplace)


def cd_last_profile():
    """(passes over A, sweeps launched) of this thread's last ``nmf_cd``"""
    return _last_profile("smk_cd_last_profile")


@dataclass
class KlResult:
    """What ``nmf_kl`` returns: the factors (numpy arrays, or torch tensors on the GPU when the start was tensors), the iterations
    run (sklearn's ``n_iter_``), whether the stopping rule ended them, and sqrt(2 D(A || W H)) of the start and of the result
    (the latter is sklearn's ``reconstruction_err_``)."""
    W: object
    H: object
    n_iter: int
    converged: bool
    error_init: float
    error: float


def nmf_kl(A, W0, H0, *, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, inplace=False) -> KlResult:
    """NMF under the generalised Kullback-Leibler divergence by multiplicative updates -- scikit-learn's ``solver="mu"`` with
    ``beta_loss="kullback-leibler"`` -- on a resident ``SparseMatrix`` A (m, n), from the start W0 (m, k), H0 (k, n): both numpy
    arrays, or both float64 / float32 torch tensors in GPU memory (any strides).  Minimises

        D(A || W H) + n alpha_W l1_ratio ||W||_1 + m alpha_H l1_ratio ||H||_1
                    + 1/2 n alpha_W (1 - l1_ratio) ||W||_F^2 + 1/2 m alpha_H (1 - l1_ratio) ||H||_F^2

    which is ``sklearn.decomposition.NMF`` on X = A' with sklearn's ``alpha_W`` = this ``alpha_H`` and its ``alpha_H`` = this
    ``alpha_W``, W_sklearn = H' and ``components_`` = W'; the stopping rule is sklearn's, looked at every tenth iteration.
    ``alpha_H="same"`` takes ``alpha_W``.  ``update_W=False``: W stays, only H is fitted (fold-in).  The start is not modified unless
    ``inplace`` (tensors only): then W0 / H0 receive the result.  A must store no entry twice and no negative value."""
    return _penalised_fit("nmf_kl", "SparseMatrix", "smk_nmf_kl_device", L.KlStats, lambda st: (st.error_init, st.error), KlResult,
                          A, W0, H0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, tol=tol, max_iter=max_iter, update_W=update_W, inplace=inplace)


def kl_last_profile():
    """(sweeps over the stored entries that updated a factor, sweeps that formed the divergence) of this thread's last ``nmf_kl``"""
    return _last_profile("smk_kl_last_profile")


@dataclass
class MaskedResult:
    """What ``nmf_masked`` returns: the factors (numpy arrays, or torch tensors on the GPU when the start was tensors), the iterations
    run, whether the stopping rule ended them, the violation of iteration 1 and of the last one, and the root of the summed squared
    error over the stored entries."""
    W: object
    H: object
    n_iter: int
    converged: bool
    violation_init: float
    violation: float
    error: float


def nmf_masked(A, W0, H0, *, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, inplace=False) -> MaskedResult:
    """NMF fitted to the STORED entries of a resident ``SparseMatrix`` A (m, n) only, by cyclic coordinate descent: an entry that A
    does not store is "not measured" -- a missing rating, an empty well, an entry held out on purpose (``holdout_split``) -- where
    every other solver here reads it as 0.  Stored zeros are measurements (``SparseMatrix.from_observed``).  Minimises

        1/2 sum over the stored (i, j, a) of (a - w_i . h_j)^2 + the penalty terms of ``nmf_cd``

    with ``nmf_cd``'s arguments, orientation and stopping rule; when every entry is stored it is ``nmf_cd``'s iteration up to
    rounding.  ``update_W=False``: W stays, only H is fitted (fold-in of new columns against fixed rows).  A must store no entry
    twice.  ``SparseMatrix.masked_residual`` of the held-out entries scores the fit."""
    if not isinstance(A, SparseMatrix):
        raise ValueError(f"nmf_masked: A must be a resident SparseMatrix, got {type(A).__name__}")
    return _penalised_fit("nmf_masked", "SparseMatrix", "smk_nmf_masked_device", L.MaskedStats,
                          lambda st: (st.violation_init, st.violation, st.error), MaskedResult,
                          A, W0, H0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, tol=tol, max_iter=max_iter, update_W=update_W, inplace=inplace)


def masked_last_profile():
    """(sweeps over the stored entries that updated a factor, sweeps that formed the residual) of this thread's last ``nmf_masked``"""
    return _last_profile("smk_masked_last_profile")


def holdout_split(A, fraction, seed):
    """Split the stored entries of A -- a scipy sparse matrix or a CSC triple (data, indices, indptr, shape) -- at random into two
    CSC triples of the same shape: ``(train, test)``, ``test`` holding round(fraction * nnz) of them.  Host code, numpy only.  A
    stored zero stays a stored entry of its part (the triples are built by index: scipy arithmetic would drop it).  The same
    split for the same seed."""
    if hasattr(A, "tocsc"):
        A = A.tocsc()
        data, indices, indptr, shape = A.data, A.indices, A.indptr, A.shape
    else:
        data, indices, indptr, shape = A
    data, indices, indptr = np.asarray(data, dtype=np.float64), np.asarray(indices), np.asarray(indptr).astype(np.int64)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"holdout_split: fraction {fraction} must lie in [0, 1]")
    nnz, ncols = data.shape[0], int(shape[1])
    if indptr.shape[0] != ncols + 1 or indptr[0] != 0 or indptr[-1] != nnz or indices.shape[0] != nnz:
        raise ValueError("holdout_split: not a CSC triple of that shape")
    held = np.zeros(nnz, dtype=bool)
    held[np.random.default_rng(seed).permutation(nnz)[:int(round(fraction * nnz))]] = True
    col = np.repeat(np.arange(ncols), np.diff(indptr))

    def part(keep):
        ptr = np.concatenate([[0], np.cumsum(np.bincount(col[keep], minlength=ncols))]).astype(np.int64)
        return data[keep].copy(), indices[keep].astype(np.uint32), ptr, (int(shape[0]), ncols)

    return part(~held), part(held)


def nmf_kl_dense(A, W0, H0, *, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, inplace=False) -> KlResult:
    """``nmf_kl`` on a resident ``DenseMatrix`` A (m, n) -- counts or intensities without many zeros: a spectrogram, an image, word
    counts over a small vocabulary.  The same objective, arguments, stopping rule and result as ``nmf_kl``; the sums run over every
    entry of the stored A (bf16 or fp32 storage, widened exactly), so on the same data the two agree up to summation order.  Each
    half-iteration is one streaming read of one stored copy (A for H, the stored transpose for W), hence a ``single_copy`` matrix
    serves ``update_W=False`` only.  A must store no negative value.  (The estimator ``NMF`` takes sparse X for this loss.)"""
    return _penalised_fit("nmf_kl_dense", "DenseMatrix", "smk_nmf_kl_dense_device", L.KlStats, lambda st: (st.error_init, st.error), KlResult,
                          A, W0, H0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, tol=tol, max_iter=max_iter, update_W=update_W, inplace=inplace)


def kl_dense_last_profile():
    """(streaming passes over A or A' that updated a factor, passes that formed the divergence) of this thread's last ``nmf_kl_dense``"""
    return _last_profile("smk_kl_dense_last_profile")


def _beta_of(what, beta_loss):
    """``beta_loss`` as a number: scikit-learn's names "itakura-saito" (0) and "kullback-leibler" (1), or a finite number >= 0 other
    than 2 (the Frobenius norm has solvers of its own).  Raised here, before any library call."""
    names = {"itakura-saito": 0.0, "kullback-leibler": 1.0}
    if isinstance(beta_loss, str):
        if beta_loss == "frobenius":
            raise ValueError(f"{what}: beta_loss='frobenius' (beta = 2) is what nmf_cd and NmfSolver minimise")
        if beta_loss not in names:
            raise ValueError(f"{what}: beta_loss must be one of {sorted(names)} or a number, got {beta_loss!r}")
        return names[beta_loss]
    if isinstance(beta_loss, bool) or not isinstance(beta_loss, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: beta_loss must be one of {sorted(names)} or a number, got {beta_loss!r}")
    beta = float(beta_loss)
    if not math.isfinite(beta) or beta < 0.0:
        raise ValueError(f"{what}: beta_loss must be finite and >= 0, got {beta_loss!r}")
    if beta == 2.0:
        raise ValueError(f"{what}: beta_loss=2 is the Frobenius norm, which nmf_cd and NmfSolver minimise")
    return beta


def nmf_beta_dense(A, W0, H0, *, beta_loss, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, inplace=False) -> KlResult:
    """``nmf_kl_dense`` under another beta-divergence -- scikit-learn's ``solver="mu"`` with ``beta_loss`` = "itakura-saito" (beta = 0,
    the scale-invariant loss a power spectrogram is fitted under), "kullback-leibler" (beta = 1: ``nmf_kl_dense`` itself, the same
    bits) or any number >= 0 other than 2 -- on a resident ``DenseMatrix`` A (m, n).  Arguments, orientation, penalties, stopping rule
    and result are ``nmf_kl``'s; ``error`` is sqrt(2 D_beta(A || W H)).  Each half-iteration is one streaming read of one stored
    copy, hence a ``single_copy`` matrix serves ``update_W=False`` only.  A must store no negative value and, for beta <= 0, no zero
    (add a small value first).  beta = 0 costs divisions only; any other beta pays a double-precision power per entry and
    half-iteration (DESIGN.md 21 has the measured cost)."""
    beta = _beta_of("nmf_beta_dense", beta_loss)
    if isinstance(A, SparseMatrix):
        raise ValueError(f"nmf_beta_dense: A must be a resident DenseMatrix, got {type(A).__name__}")
    return _penalised_fit("nmf_beta_dense", "DenseMatrix", "smk_nmf_beta_dense_device", L.KlStats, lambda st: (st.error_init, st.error), KlResult,
                          A, W0, H0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, tol=tol, max_iter=max_iter, update_W=update_W, inplace=inplace,
                          before_options=(C.c_double(beta),))


def beta_dense_last_profile():
    """(streaming passes over A or A' that updated a factor, passes that formed the divergence) of this thread's last ``nmf_beta_dense``
    (beta != 1)"""
    return _last_profile("smk_beta_dense_last_profile")


def cd_sweep(G, R, X, l1=0.0, l2=0.0):
    """One coordinate-descent sweep on the device, by itself (``smk_cd_sweep``): G (k, k), R (k, ncols), X (k, ncols) numpy
    arrays.  For every column x and t = 0 .. k-1 in order, with G' = G + l2 I and R' = R - l1: grad = G'[t] . x - R'[t],
    the violation grows by |min(0, grad)| where x[t] == 0 and by |grad| elsewhere, x[t] = max(x[t] - grad / G'[t, t], 0) unless
    G'[t, t] == 0.  Returns (X_new, violation); X is not modified."""
    G, R = _f(G), _f(R)
    X = _f(X).copy(order="F")
    k, ncols = R.shape
    if G.shape != (k, k) or X.shape != (k, ncols):
        raise ValueError(f"cd_sweep: G {G.shape} / R {R.shape} / X {X.shape} do not match (k, k) / (k, ncols) / (k, ncols)")
    v = C.c_double(0)
    L.check(L.lib().smk_cd_sweep(k, ncols, _p(G), k, _p(R), k, _p(X), k, float(l1), float(l2), C.byref(v)), "smk_cd_sweep")
    return X, v.value


def nnls_blockpivot(LHS, RHS, Xinit):
    """``NnlsBlockpivot`` (common/include/nnls.hpp:144-244) on the device, by itself.

    LHS k x k SPD, RHS k x ncols, Xinit the warm start (passive set = Xinit > 0).
    Returns (ok, X, Y) with Y = LHS X - RHS; ok False = the reference's ``false``."""
    G = _f(LHS)
    B = _f(RHS)
    X = _f(Xinit).copy(order="F")
    k, ncols = B.shape
    Y = np.zeros((k, ncols), order="F")
    rc = L.lib().smk_nnls_blockpivot(k, ncols, _p(G), k, _p(B), k, _p(X), k, _p(Y), k)
    if rc not in (L.OK, L.FAILURE):
        L.check(rc, "smk_nnls_blockpivot")
    return rc == L.OK, X, Y


class Comm:
    """A communicator of the column-sharded solver (include/smallk_amd.h, multi-GPU section): RCCL, or the
    in-process stand-in for several shards on one device."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def unique_id(cls) -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.lib().smk_comm_unique_id(buf), "smk_comm_unique_id")
        return buf.raw

    @classmethod
    def init_rank(cls, uid: bytes, rank: int, world: int):
        h = C.c_void_p()
        L.check(L.lib().smk_comm_init_rank(C.byref(h), C.create_string_buffer(uid, 128), rank, world), "smk_comm_init_rank")
        return cls(h)

    @classmethod
    def init_all(cls, ndev: int, devices=None):
        hs = (C.c_void_p * ndev)()
        dv = (C.c_int * ndev)(*devices) if devices is not None else None
        L.check(L.lib().smk_comm_init_all(hs, ndev, dv), "smk_comm_init_all")
        return [cls(C.c_void_p(h)) for h in hs]

    @classmethod
    def init_local(cls, nranks: int):
        hs = (C.c_void_p * nranks)()
        L.check(L.lib().smk_comm_init_local(hs, nranks), "smk_comm_init_local")
        return [cls(C.c_void_p(h)) for h in hs]

    def selftest(self):
        """known values through one all-reduce and one all-gather; every rank calls it; raises on a wrong answer"""
        L.check(L.lib().smk_comm_selftest(self._h), "smk_comm_selftest")

    @property
    def rank(self):
        return L.lib().smk_comm_rank(self._h)

    @property
    def world(self):
        return L.lib().smk_comm_world(self._h)

    def close(self):
        if self._h:
            L.lib().smk_comm_destroy(self._h)
            self._h = None


def nmf_sharded(A, W0, H0, algorithm, nshards, *, storage="f32", devices=None, local_stub=False, **kw) -> NmfResult:
    """``Nmf(...)`` on ``nshards`` column shards, one host thread and one device per shard (RCCL), or all shards on
    the current device through the in-process stand-in (``local_stub=True``)."""
    A = _f(A)
    W = _f(W0).copy(order="F")
    H = _f(H0).copy(order="F")
    m, n = A.shape
    k = W.shape[1]
    o = make_options(m, n, k, algorithm, **kw)
    st = L.Stats()
    stg = STORAGE[storage] if isinstance(storage, str) else int(storage)
    dv = (C.c_int * nshards)(*devices) if devices is not None else None
    rc = L.lib().smk_nmf_dense_sharded(C.byref(o), _p(A), m, _p(W), m, _p(H), k, C.byref(st), stg, nshards, dv,
                                       1 if local_stub else 0)
    if rc not in (L.OK, L.FAILURE, L.BAD_PARAM, L.NOTINITIALIZED, L.SIZE_TOO_LARGE):
        L.check(rc, "smk_nmf_dense_sharded")
    return NmfResult(rc, W, H, st.iteration_count, st.elapsed_us)

"""smallk_amd -- MI355X-native dense NMF (MU / HALS / BPP) behind the libsmallk API.

The numeric path is hand-written HIP for gfx950 in ``smallk_amd/csrc`` behind the C ABI
``include/smallk_amd.h``; this package is the host-side mirror of the reference's Python
surface (pysmallk ``SmallkAPI``) plus thin object wrappers.  No CPU fallback exists.
"""
from . import _lib
from .solver import (DenseMatrix, SparseMatrix, NmfSolver, NmfResult, nmf, nmf_sparse, nmf_device, load_matrix_market,
                     initialize, finalize, is_initialized, make_options, uniform_host, set_stream,
                     nnls_blockpivot, nmf_sharded, Comm, thread_context_begin, thread_context_end, trim_device_cache,
                     Residual, relative_error, labels_device, top_terms_device, transform, NNDSVD_VARIANTS, nmf_cd, cd_sweep, CdResult,
                     nmf_kl, nmf_kl_dense, kl_dense_last_profile, KlResult, KlDivergence,
                     nmf_beta_dense, beta_dense_last_profile, BetaDivergence,
                     nmf_masked, masked_last_profile, MaskedResult, MaskedResidual, holdout_split)
from .estimator import NMF
from .api import SmallkAPI
from . import hierclust
from . import flatclust
from .hierclust import hier_nmf2, TreeResults, TreeRouter

__all__ = ["DenseMatrix", "SparseMatrix", "nmf_sparse", "load_matrix_market", "NmfSolver", "NmfResult", "nmf", "nmf_device", "initialize", "finalize", "is_initialized",
           "make_options", "uniform_host", "nnls_blockpivot", "nmf_sharded", "Comm", "set_stream", "thread_context_begin", "thread_context_end", "trim_device_cache", "SmallkAPI", "hierclust", "flatclust", "hier_nmf2", "TreeResults", "TreeRouter", "Residual", "relative_error", "labels_device", "top_terms_device", "transform", "NNDSVD_VARIANTS", "nmf_cd", "cd_sweep", "CdResult", "nmf_kl", "nmf_kl_dense", "kl_dense_last_profile", "KlResult", "KlDivergence", "nmf_beta_dense", "beta_dense_last_profile", "BetaDivergence", "nmf_masked", "masked_last_profile", "MaskedResult", "MaskedResidual", "holdout_split", "NMF", "Vocabulary", "_lib"]


def __getattr__(name):
    """``smallk_amd.Hierclust`` / ``smallk_amd.Flatclust`` / ``smallk_amd.pyclust`` (pysmallk's clustering classes,
    pysmallk/interface/smallk_lib.pyx:924-1420) and ``smallk_amd.Preprocessor`` (:1643-1815) with ``smallk_amd.Vocabulary``, loaded on first use."""
    if name in ("Preprocessor", "preprocess", "Vocabulary"):
        import importlib
        mod = importlib.import_module(".preprocess", __name__)
        return mod if name == "preprocess" else getattr(mod, name)
    if name in ("Hierclust", "Flatclust", "pyclust"):
        import importlib
        mod = importlib.import_module(".pyclust", __name__)
        return mod if name == "pyclust" else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

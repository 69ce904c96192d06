"""``smallk_amd.NMF``: the scikit-learn-style estimator over ``nmf_cd`` (coordinate descent with L1 / L2 penalties, on the GPU)
and, for ``solver="mu"`` with ``beta_loss="kullback-leibler"``, over ``nmf_kl`` (multiplicative updates of the generalised
Kullback-Leibler divergence on a sparse X).

X is in scikit-learn's orientation, samples x features; the library factors A = X' (features x samples), which costs nothing:
a scipy CSR X hands its three arrays over as the CSC of A, a C-contiguous dense X is the column-major A, a torch tensor is
adopted through its transposed view.  ``fit_transform`` returns W_sklearn = H', ``components_`` is W'.
"""
from __future__ import annotations

import math

import numpy as np

from . import solver as S

INITS = (None, "nndsvd", "nndsvda", "random", "custom")
KL_LOSSES = ("kullback-leibler", 1, 1.0)


def _is_sparse(X) -> bool:
    return type(X).__module__.split(".")[0] == "scipy" and hasattr(X, "tocsr")


class NMF:
    """``sklearn.decomposition.NMF`` with ``solver="cd"``, ``beta_loss="frobenius"``, ``shuffle=False``: the constructor arguments
    that apply, ``fit`` / ``fit_transform`` / ``transform`` / ``inverse_transform``, ``components_``, ``n_iter_``,
    ``reconstruction_err_``, ``n_components_``.  With ``init="custom"`` and the same start it runs sklearn's iteration: the same
    ``n_iter_``, factors equal to rounding.

    ``init=None`` is "nndsvda" (``DenseMatrix.nndsvd``, a randomised SVD: a start of sklearn's kind, not sklearn's numbers) while
    n_components + 8 <= 128 and "random" above that.  "random" is sqrt(mean(X) / k) |N(0, 1)| drawn from
    ``numpy.random.default_rng(random_state)``, H first, then W: not sklearn's random stream.  ``n_components=None`` is the
    number of features.  X: a numpy array, a scipy sparse matrix, or a torch tensor in GPU memory (results then stay tensors).
    The library's rules apply: n_components <= min(samples, features) and <= 128, also for the samples given to ``transform``.

    ``solver="mu"`` together with ``beta_loss="kullback-leibler"`` (or 1) is sklearn's multiplicative-update iteration for the
    generalised Kullback-Leibler divergence (``nmf_kl``): X is a scipy sparse matrix, ``reconstruction_err_`` is
    sqrt(2 D(X || W H)) as sklearn's, the stopping rule is sklearn's (every tenth iteration).  Either half alone is refused:
    ``solver="mu"`` with the Frobenius loss is not sklearn's iteration here, and ``solver="cd"`` has no KL form."""

    def __init__(self, n_components=None, *, init=None, solver="cd", beta_loss="frobenius", tol=1e-4, max_iter=200,
                 random_state=None, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, shuffle=False):
        kl = solver == "mu" and not isinstance(beta_loss, bool) and beta_loss in KL_LOSSES
        if solver != "cd" and not kl:
            raise ValueError(f"NMF: solver must be 'cd', or 'mu' together with beta_loss='kullback-leibler'; got {solver!r} with {beta_loss!r}")
        if not kl and beta_loss not in ("frobenius", 2, 2.0):
            raise ValueError(f"NMF: beta_loss must be 'frobenius', or 'kullback-leibler' together with solver='mu'; got {beta_loss!r}")
        if shuffle:
            raise ValueError("NMF: shuffle=True is not available; the coordinates are swept in order")
        if init not in INITS:
            raise ValueError(f"NMF: init must be one of {INITS}, got {init!r}")
        if n_components is not None and (isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1):
            raise ValueError(f"NMF: n_components must be a positive integer or None, got {n_components!r}")
        if alpha_H != "same" and (isinstance(alpha_H, str) or not float(alpha_H) >= 0):
            raise ValueError(f"NMF: alpha_H must be 'same' or a number >= 0, got {alpha_H!r}")
        if not float(alpha_W) >= 0:
            raise ValueError(f"NMF: alpha_W must be >= 0, got {alpha_W!r}")
        if not 0 <= float(l1_ratio) <= 1:
            raise ValueError(f"NMF: l1_ratio must lie in [0, 1], got {l1_ratio!r}")
        if not float(tol) >= 0:
            raise ValueError(f"NMF: tol must be >= 0, got {tol!r}")
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
            raise ValueError(f"NMF: max_iter must be an integer >= 1, got {max_iter!r}")
        self.n_components, self.init, self.solver, self.beta_loss = n_components, init, solver, beta_loss
        self.tol, self.max_iter, self.random_state = tol, max_iter, random_state
        self.alpha_W, self.alpha_H, self.l1_ratio, self.shuffle = alpha_W, alpha_H, l1_ratio, shuffle

    @property
    def _kl(self):
        return self.solver == "mu"

    def _fit_factors(self, A, W0, H0, **kw):
        return (S.nmf_kl if self._kl else S.nmf_cd)(A, W0, H0, **kw, **self._penalties())

    # ---- X -> the resident A = X', the mean of X, whether results go back as tensors
    def _resident(self, X):
        if self._kl and not _is_sparse(X):
            raise ValueError("NMF: the Kullback-Leibler path takes sparse input (a scipy sparse matrix); a dense X is not supported with this loss")
        if _is_sparse(X):
            X = X.tocsr()
            ns, nf = X.shape
            return S.SparseMatrix(X.data, X.indices, X.indptr, (nf, ns)), float(X.sum()) / (ns * nf), False
        if S._is_tensor(X):
            if X.dim() != 2:
                raise ValueError(f"NMF: X must be 2-D, got shape {tuple(X.shape)}")
            return S.DenseMatrix.from_device(X.t()), float(X.double().mean()), True
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError(f"NMF: X must be 2-D, got shape {X.shape}")
        return S.DenseMatrix.from_host(X.T), float(X.mean()), False

    def _penalties(self):
        """sklearn's alpha_W weighs W_sklearn = H', its alpha_H weighs components_ = W'"""
        a_w = float(self.alpha_W)
        a_h = a_w if self.alpha_H == "same" else float(self.alpha_H)
        return {"alpha_W": a_h, "alpha_H": a_w, "l1_ratio": float(self.l1_ratio), "tol": float(self.tol), "max_iter": int(self.max_iter)}

    @staticmethod
    def _to_device(x):
        import torch
        if S._is_tensor(x):
            return x
        dev = torch.device("cuda", S.L.lib().smk_current_device())
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)

    def _start(self, A, k, mean, W, H):
        import torch
        m, n = A.height, A.ncols                    # features, samples
        init = self.init
        if init == "custom":
            if W is None or H is None:
                raise ValueError("NMF: init='custom' needs W (samples, k) and H (k, features)")
            if tuple(W.shape) != (n, k) or tuple(H.shape) != (k, m):
                raise ValueError(f"NMF: W {tuple(W.shape)} / H {tuple(H.shape)} do not match ({n}, {k}) / ({k}, {m})")
            return self._to_device(H).t(), self._to_device(W).t()
        if init is None:
            init = "nndsvda" if k + 8 <= 128 else "random"
        if init == "random":
            rng = np.random.default_rng(self.random_state)
            avg = math.sqrt(mean / k)
            Hs = avg * np.abs(rng.standard_normal((k, m)))
            Ws = avg * np.abs(rng.standard_normal((n, k)))
            return self._to_device(Hs).t(), self._to_device(Ws).t()
        seed = 0 if self.random_state is None else int(self.random_state)
        return A.nndsvd(k, variant=init, oversample=min(8, 128 - k), seed=seed)

    def fit_transform(self, X, y=None, W=None, H=None):
        A, mean, as_tensor = self._resident(X)
        try:
            k = int(self.n_components) if self.n_components is not None else A.height
            W0, H0 = self._start(A, k, mean, W, H)
            r = self._fit_factors(A, W0, H0)
            self._W, self._H = r.W, r.H             # (features, k) and (k, samples), float64 tensors on the GPU
            self.n_iter_ = r.n_iter
            self.n_components_ = k
            self.n_features_in_ = A.height
            self.reconstruction_err_ = r.error if self._kl else math.sqrt(A.residual(r.W, r.H).resid_sq)
            self._as_tensor = as_tensor
        finally:
            A.close()
        return self._out(self._H.t(), as_tensor)

    def fit(self, X, y=None, **params):
        self.fit_transform(X, **params)
        return self

    @staticmethod
    def _out(t, as_tensor):
        return t if as_tensor else t.cpu().numpy()

    @property
    def components_(self):
        """(n_components, features): W'"""
        if not hasattr(self, "_W"):
            raise AttributeError("NMF: not fitted")
        return self._out(self._W.t(), self._as_tensor)

    def transform(self, X):
        """W_sklearn of new samples against the fitted ``components_``: only H moves, from the constant sqrt(mean(X) / k)"""
        import torch
        if not hasattr(self, "_W"):
            raise AttributeError("NMF: not fitted")
        A, mean, as_tensor = self._resident(X)
        try:
            if A.height != self.n_features_in_:
                raise ValueError(f"NMF.transform: X has {A.height} features, the model {self.n_features_in_}")
            k = self.n_components_
            H0 = torch.full((k, A.ncols), math.sqrt(mean / k), dtype=torch.float64, device=self._W.device)
            r = self._fit_factors(A, self._W, H0, update_W=False)
        finally:
            A.close()
        return self._out(r.H.t(), as_tensor)

    def inverse_transform(self, W):
        """W (samples, n_components) -> W @ components_"""
        if S._is_tensor(W):
            return W.to(self._W.dtype) @ self._W.t()
        return np.asarray(W, dtype=np.float64) @ self._W.t().cpu().numpy()

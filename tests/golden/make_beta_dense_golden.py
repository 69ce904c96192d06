"""Records tests/golden/beta_dense_sklearn.npz: scikit-learn's own result on the golden cases of tests/beta_dense_cases.py (k <= 33, see there).

sklearn.decomposition.NMF(solver="mu", beta_loss=the case's beta, init="custom") is run on the dense X of each case from the
case's start.  Stored per case, in this project's orientation (float64): W (m x k) = components_', H (k x n) = W_sklearn', n_iter_
and reconstruction_err_; the inputs are not stored, tests/beta_dense_cases.py rebuilds them from the seed (a checksum of X
and of the start is stored instead).

    python tests/golden/make_beta_dense_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import beta_dense_cases as C  # noqa: E402


def main():
    import sklearn
    from sklearn.decomposition import NMF
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in C.GOLDEN_CASES:
        c = C.case(name)
        X = c["X"]
        model = NMF(n_components=c["k"], init="custom", solver="mu", **c["sk"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # a case that runs to max_iter warns about it
            Wsk = model.fit_transform(X, W=c["Wsk0"].copy(), H=c["Hsk0"].copy())
        out[f"{name}/checksum"] = np.array([c["X"].sum(), c["W0"].sum(), c["H0"].sum()])
        out[f"{name}/W"] = np.ascontiguousarray(model.components_.T)
        out[f"{name}/H"] = np.ascontiguousarray(Wsk.T)
        out[f"{name}/n_iter"] = np.array(model.n_iter_)
        out[f"{name}/reconstruction_err"] = np.array(model.reconstruction_err_)
        print(name, "n_iter", model.n_iter_, "reconstruction_err", model.reconstruction_err_)
    path = os.path.join(HERE, "beta_dense_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

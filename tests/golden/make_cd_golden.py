"""Records tests/golden/cd_sklearn.npz: scikit-learn's own result on the golden cases of tests/cd_reference.py.

sklearn.decomposition.NMF(solver="cd", init="custom", shuffle=False) is run on X = A' of each case, from the case's start, with
alpha_W / alpha_H exchanged (sklearn's W is this project's H').  Stored per case: A and the start (float32, they are exact in
it), sklearn's factors in this project's orientation (W m x k, H k x n, float64), n_iter_ and reconstruction_err_.

    python tests/golden/make_cd_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cd_reference as R  # noqa: E402


def main():
    import sklearn
    from sklearn.decomposition import NMF
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in R.GOLDEN_CASES:
        A, _, W0, H0, kw = R.fit_case(name)
        model = NMF(n_components=W0.shape[1], init="custom", solver="cd", beta_loss="frobenius", tol=kw["tol"], max_iter=kw["max_iter"],
                    alpha_W=kw["alpha_H"], alpha_H=kw["alpha_W"], l1_ratio=kw["l1_ratio"], shuffle=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # the case that runs to max_iter warns about it
            Wsk = model.fit_transform(np.ascontiguousarray(A.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
        for key, v in (("A", A), ("W0", W0), ("H0", H0)):
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
            out[f"{name}/{key}"] = v.astype(np.float32)
        out[f"{name}/W"] = np.ascontiguousarray(model.components_.T)
        out[f"{name}/H"] = np.ascontiguousarray(Wsk.T)
        out[f"{name}/n_iter"] = np.array(model.n_iter_)
        out[f"{name}/reconstruction_err"] = np.array(model.reconstruction_err_)
        print(name, "n_iter", model.n_iter_, "reconstruction_err", model.reconstruction_err_)
    path = os.path.join(HERE, "cd_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

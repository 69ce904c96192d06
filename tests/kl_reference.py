"""The numpy restatement of KL-divergence NMF by multiplicative updates (include/smallk_amd.h: smk_nmf_kl_device):
scikit-learn 1.7's _fit_multiplicative_update with beta_loss = 1 on X = A', in the library's orientation (A m x n sparse, W m x k,
H k x n; W_sklearn = H', components_ = W', sklearn's alpha_W = our alpha_H and the other way round).

Only the stored entries (i, j, a) of A enter: d = w_i . h_j clamped at EPS from below, q = a / d.
  H step: H[t, j] *= (sum over column j of q W[i, t]) / den,  den = sum_i W[i, t] (+ l1_H if > 0) (+ l2_H H[t, j] if > 0), 0 -> EPS
  W step: the same over the rows of A with the new H; sum_j H[t, j] == 0 is replaced by 1.0 first; W < 2^-52 becomes 0 afterwards
  error = sqrt(2 max(D, 0)),  D = sum a log(a / d) - sum a + (sum_i w_i) . (sum_j h_j), taken before iteration 1 and, when
  tol > 0, at n_iter = 10, 20, ...: stop when (previous_error - error) / error_init < tol.
Two summation orders of the dot product ("pair": numpy's sum over the products, as sklearn forms it; "seq": t = 0 .. k-1 one
after the other) and any float type (numpy.longdouble) are available, so that the tests can tell what hangs on rounding.  A third
order, "gemm", forms the dot products and the sums as dense matrix products (float64): the quick one, for the GPU tests' fits.
"""
import numpy as np

EPS = 2.0 ** -23            # sklearn's EPSILON: float32's
EPS64 = 2.0 ** -52
U53 = 2.0 ** -53
FIT_BAR = 1e-12             # factors of a whole fit, relative to the largest factor entry (DESIGN 17's bar for cd fits)


class Entries:
    """the stored entries of A in CSC order (column by column) and the permutation into row order (CSC of A')"""

    def __init__(self, A):
        A = np.asarray(A)
        self.m, self.n = A.shape
        jj, ii = np.nonzero(A.T)                  # column-major order
        self.i, self.j, self.a = ii, jj, np.asarray(A[ii, jj], dtype=np.float64)
        self.by_row = np.lexsort((jj, ii))        # row by row, columns ascending
        self.col_count = np.bincount(jj, minlength=self.n)
        self.row_count = np.bincount(ii, minlength=self.m)

    def scatter(self, q):
        """the m x n array that holds q at the stored entries"""
        Q = np.zeros((self.m, self.n), dtype=q.dtype)
        Q[self.i, self.j] = q
        return Q


def _dots(E, W, H, order):
    if order == "gemm":
        return (W @ H)[E.i, E.j]
    d = np.empty(len(E.a), dtype=W.dtype)
    if order == "pair":
        HT = H.T
        for s in range(0, len(d), 2048):          # (in chunks that stay in the cache; the sum of a row does not depend on the chunk)
            c = slice(s, s + 2048)
            d[c] = np.multiply(W[E.i[c]], HT[E.j[c]]).sum(axis=1)
        return d
    d[:] = 0
    WT = np.ascontiguousarray(W.T)
    for t in range(W.shape[1]):
        d += WT[t][E.i] * H[t][E.j]
    return d


def _quotients(E, W, H, order):
    d = _dots(E, W, H, order)
    d[d < EPS] = EPS
    return E.a.astype(W.dtype) / d


def _grouped_sum(q, rows, count):
    """sum of q[e] rows[e] group by group, the groups consecutive with `count` entries each, in entry order"""
    if rows.dtype == np.float64:                  # the same sums in the same order, by scipy's CSR product where there is one
        try:
            import scipy.sparse as sp
            ptr = np.concatenate([[0], np.cumsum(count)])
            return sp.csr_matrix((q, np.arange(len(q)), ptr), shape=(len(count), len(q))) @ (rows if rows.flags.c_contiguous else np.ascontiguousarray(rows))
        except ImportError:
            pass
    prod = q[:, None] * rows
    out = np.zeros((len(count), prod.shape[1]), dtype=prod.dtype)
    live = count > 0
    starts = (np.cumsum(count) - count)[live]
    if len(starts):
        out[live] = np.add.reduceat(prod, starts, axis=0)
    return out


def _denominator(s, l1, l2, X):
    """X: N x k"""
    den = np.broadcast_to(s[None, :], X.shape).copy()
    if l1 > 0:
        den += X.dtype.type(l1)
    if l2 > 0:
        den = den + X.dtype.type(l2) * X
    den[den == 0] = EPS
    return den


def step_h(E, W, H, l1, l2, order="pair", wsum=None):
    """in place on H (k x n)"""
    q = _quotients(E, W, H, order)
    if order == "gemm":
        num = E.scatter(q).T @ W
    else:
        num = _grouped_sum(q, W[E.i], E.col_count)                # storage order inside a column
    s = W.sum(axis=0) if wsum is None else wsum
    H *= (num / _denominator(s, l1, l2, H.T)).T
    return H


def step_w(E, W, H, l1, l2, order="pair"):
    """in place on W (m x k), with the flush"""
    q = _quotients(E, W, H, order)
    o = E.by_row
    if order == "gemm":
        num = E.scatter(q) @ H.T
    else:
        num = _grouped_sum(q[o], H.T[E.j[o]], E.row_count)
    s = H.sum(axis=1)
    s[s == 0] = 1.0
    W *= num / _denominator(s, l1, l2, W)
    W[W < EPS64] = 0.0
    return W


def divergence(E, W, H, order="pair"):
    """(D, sum a log(a / d), sum WH, sum |a log(a / d)|, sum a) -- D not clamped"""
    d = _dots(E, W, H, order)
    a = E.a.astype(W.dtype)
    keep = a > EPS
    d, a = d[keep], a[keep]
    d[d < EPS] = EPS
    terms = a * np.log(a / d)
    alog, swh, sa = terms.sum(), W.sum(axis=0) @ H.sum(axis=1), a.sum()
    return alog + (swh - sa), alog, swh, np.abs(terms).sum(), sa


def error_of(E, W, H, order="pair"):
    D = divergence(E, W, H, order)[0]
    return np.sqrt(2 * max(D, 0))


def fit(A, W0, H0, *, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, tol=1e-3, max_iter=200, update_W=True, order="pair", dtype=np.float64):
    """the loop of smk_nmf_kl_device; returns a dict: W, H, n_iter, converged, error_init, error, margins (per check: the stop
    quantity minus tol, relative to tol)"""
    dt = np.dtype(dtype)
    E = A if isinstance(A, Entries) else Entries(A)
    W = np.array(W0, dtype=dt, order="C")
    H = np.array(H0, dtype=dt, order="C")
    m, n = E.m, E.n
    l1h, l2h = m * alpha_H * l1_ratio, m * alpha_H * (1.0 - l1_ratio)
    l1w, l2w = n * alpha_W * l1_ratio, n * alpha_W * (1.0 - l1_ratio)
    error_init = error_of(E, W, H, order)
    previous, error, checked = error_init, error_init, 0
    margins, converged, it = [], False, 0
    wsum = None if update_W else W.sum(axis=0)
    for it in range(1, max_iter + 1):
        step_h(E, W, H, l1h, l2h, order, wsum)
        if update_W:
            step_w(E, W, H, l1w, l2w, order)
        if tol > 0 and it % 10 == 0:
            error, checked = error_of(E, W, H, order), it
            stop = (previous - error) / error_init
            margins.append(float(abs(stop - tol) / tol))
            if stop < tol:
                converged = True
                break
            previous = error
    if checked != it:
        error = error_of(E, W, H, order)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return {"W": f64(W), "H": f64(H), "n_iter": it, "converged": converged, "error_init": float(error_init), "error": float(error),
            "margins": margins}


def step_bar(k, L):
    """one step by itself against the longdouble restatement, relative, entry by entry: k products and L quotient terms, all
    non-negative"""
    return 4 * (k + L) * U53

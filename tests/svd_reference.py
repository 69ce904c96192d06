"""numpy fp64 restatement of the truncated SVD and NNDSVD of smallk_amd/csrc/svd.cpp, and the case generators of
tests/test_svd_cpu.py and tests/test_gpu_svd.py.  The host step is numpy.linalg.eigh where the library runs cyclic Jacobi; the
thresholds (2^-40) are the library's."""
import numpy as np

U53 = 2.0 ** -53
RANK_TOL = 2.0 ** -40


def eig_desc(G):
    lam, E = np.linalg.eigh(0.5 * (G + G.T))
    return lam[::-1].copy(), E[:, ::-1].copy()


def orth(Y):
    """eigen-orthonormalisation, two rounds: Y <- Y E Lambda^(-1/2) over the eigenvalues above 2^-40 lambda_max, zero columns else"""
    for _ in range(2):
        lam, E = eig_desc(Y.T @ Y)
        M = np.zeros_like(E)
        keep = (lam > RANK_TOL * lam[0]) & (lam > 0)
        M[:, keep] = E[:, keep] / np.sqrt(lam[keep])
        Y = Y @ M
    return Y


def svd_restated(A, k, *, oversample=8, power_iters=2, omega=None, rng=None):
    m, n = A.shape
    l = min(k + oversample, m, n)
    if omega is None:
        omega = (rng or np.random.default_rng(0)).random((n, l)) - 0.5
    assert omega.shape == (n, l)
    Q = orth(A @ omega)
    for _ in range(power_iters):
        Z = orth(A.T @ Q)
        Q = orth(A @ Z)
    Bt = A.T @ Q
    lam, E = eig_desc(Bt.T @ Bt)
    S = np.zeros(k)
    U, V = np.zeros((m, k)), np.zeros((n, k))
    for j in range(k):
        if lam[j] > 0 and lam[j] > RANK_TOL * lam[0]:
            S[j] = np.sqrt(lam[j])
            U[:, j] = Q @ E[:, j]
            V[:, j] = Bt @ E[:, j] / S[j]
    return U, S, polish(V)


def polish(V):
    """V <- V (V'V)^(-1/2), the symmetric (nearest) orthonormalisation: V = B' E / S keeps V'V = I only to u (sigma_1 / sigma_k)^2"""
    lam, E = eig_desc(V.T @ V)
    keep = (lam > RANK_TOL * lam[0]) & (lam > 0)
    return V @ ((E[:, keep] / np.sqrt(lam[keep])) @ E[:, keep].T)


def nndsvd_from_svd(U, S, V, *, variant="nndsvd", mean=0.0, info=None):
    """Boutsidis & Gallopoulos; info (a dict) receives the tie margins and the distance of the entries from the zero threshold"""
    m, k = U.shape
    n = V.shape[0]
    W, H = np.zeros((m, k)), np.zeros((k, n))
    margins, near = [], []

    def cut(part, scale):
        top = part.max() if part.size else 0.0
        out = np.where(part < RANK_TOL * top, 0.0, part * scale)
        nz = part[part > 0]
        if nz.size and top > 0:
            near.append(np.min(np.abs(np.log2(nz / (RANK_TOL * top)))))
        return out

    for j in range(k):
        if not S[j] > 0:
            continue
        u, v = U[:, j], V[:, j]
        if j == 0:
            W[:, 0] = cut(np.abs(u), np.sqrt(S[0]))
            H[0] = cut(np.abs(v), np.sqrt(S[0]))
            continue
        up, un, vp, vn = np.maximum(u, 0), np.maximum(-u, 0), np.maximum(v, 0), np.maximum(-v, 0)
        nup, nun, nvp, nvn = (np.sqrt(np.sum(x * x)) for x in (up, un, vp, vn))
        mp, mn = nup * nvp, nun * nvn
        margins.append(abs(mp - mn) / max(mp, mn) if max(mp, mn) > 0 else 0.0)
        pos = mp >= mn
        mm = mp if pos else mn
        if not mm > 0:
            continue
        f = np.sqrt(S[j] * mm)
        W[:, j] = cut(up if pos else un, f / (nup if pos else nun))
        H[j] = cut(vp if pos else vn, f / (nvp if pos else nvn))
    if variant == "nndsvda":
        W[W == 0] = mean
        H[H == 0] = mean
    if info is not None:
        info["tie_margin"] = min(margins) if margins else np.inf
        info["threshold_distance_log2"] = min(near) if near else np.inf
    return W, H


def align(X, Xref):
    """flip the sign of every column of X to agree with Xref"""
    s = np.sign(np.sum(X * Xref, axis=0))
    s[s == 0] = 1.0
    return X * s


def numpy_svd(A, k):
    U, S, Vt = np.linalg.svd(A, full_matrices=False)
    return U[:, :k], S, Vt[:k].T          # S in full: the gap below sigma_k needs sigma_{k+1}


def relative_gap(S, k):
    """g = min over j <= k of (sigma_j - sigma_{j+1}) / sigma_j (sigma_{k+1} = 0 past the end)"""
    s = np.concatenate([S, [0.0]])
    return min((s[j] - s[j + 1]) / s[j] for j in range(k))


def bars(S, k):
    """(relative bar on S, absolute bar on the sign-aligned vectors): 64 u (sigma_1 / sigma_k)^2 and that over g"""
    b = 64 * U53 * (S[0] / S[k - 1]) ** 2
    return b, b / relative_gap(S, k)


# ---- cases -----------------------------------------------------------------------------------------------------------------
# (m, n, r, k): A = W* H* with integer entries in {0, 1, 2}: exact in fp32 and, the entries being integers <= 256, in bf16
EXACT_CASES = [(1, 1, 1, 1), (65, 63, 4, 4), (63, 65, 4, 3), (129, 257, 8, 8), (257, 131, 16, 12), (257, 131, 64, 56), (200, 300, 70, 66)]
EXACT_SEEDS = {c: 1 for c in EXACT_CASES}
EXACT_SEEDS[(200, 300, 70, 66)] = 2          # seed 1 leaves an entry 2^17.8 from the zero threshold
LOW_RANK_CASE = (65, 63, 4, 6)
REPLAY_CASES = [(129, 257, 8), (257, 131, 16), (63, 65, 4)]
SPARSE_CASES = [(65, 63, 4, 4), (257, 131, 16, 12), (1000, 900, 20, 16)]
SPARSE_SEEDS = {c: 1 for c in SPARSE_CASES}


def exact_rank(m, n, r, seed):
    rng = np.random.default_rng(1000 * seed + m + 7 * n + 13 * r)
    if (m, n) == (1, 1):
        return np.array([[2.0]])
    return rng.integers(0, 3, (m, r)).astype(np.float64) @ rng.integers(0, 3, (r, n)).astype(np.float64)


def replay_values(rows, cols, seed):
    """random values in [0, 3) rounded to fp32, with a tenth of zeros"""
    rng = np.random.default_rng(seed)
    v = rng.random(rows * cols) * 3.0
    v[rng.random(rows * cols) < 0.1] = 0.0
    return v.reshape(rows, cols).astype(np.float32).astype(np.float64)


def sparse_exact_rank(m, n, r, seed):
    """A = W* H* with sparse integer factors (about 30 % non-zero), one empty column, one empty row, and one stored entry given
    twice (the halves add up).  Returns (scipy CSC built from triplets so that the duplicate survives, the dense equivalent)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(2000 * seed + m + 7 * n + 13 * r)
    Ws = rng.integers(1, 3, (m, r)) * (rng.random((m, r)) < 0.3)
    Hs = rng.integers(1, 3, (r, n)) * (rng.random((r, n)) < 0.3)
    Ws[m // 3] = 0                       # an empty row
    Hs[:, n // 2] = 0                    # an empty column
    D = (Ws @ Hs).astype(np.float64)
    rows, cols = np.nonzero(D.T)[1], np.nonzero(D.T)[0]          # column-major order of the stored entries
    vals = D[rows, cols]
    # the first stored entry with an even value is stored as two halves
    i = int(np.flatnonzero(vals % 2 == 0)[0])
    rows = np.concatenate([rows[:i + 1], rows[i:]])
    cols = np.concatenate([cols[:i + 1], cols[i:]])
    vals = np.concatenate([vals[:i], [vals[i] / 2, vals[i] / 2], vals[i + 1:]])
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))])
    return (vals, rows.astype(np.uint32), indptr.astype(np.uint32), (m, n)), D

"""The cases tests/test_masked_cpu.py and tests/test_gpu_masked.py share (masked coordinate descent), and what the CPU
test records about them for the GPU test's bars.

The pattern cases sit on the edges of the kernel: segments of 64 entries, lane groups of 16 with four entries a lane, KP steps
8 / 16 / 32 / 64 / 128.  Each has an empty row and an empty column; a row and a column of exactly 1, 16, 17, 63, 64, 65 and 129 stored
entries; a row and a column of 220 (four pieces); at least 5 % of the stored values exactly 0.0; data and starts rounded to fp32.  The
special rows and columns do not meet each other, so the counts are exact.  The full-mask and planted cases are what their names say.
"""
import functools

import numpy as np

U53 = 2.0 ** -53
FIT_BAR = 1e-12               # of the largest factor entry; also the relative bar of violation_init, violation and error
SWEEP_MARGIN = 8              # the device's reduction tree is another fixed order than either of the restatement's
EDGE_COUNTS = [0, 1, 16, 17, 63, 64, 65, 129, 220]
MARGIN = 3e-3                 # the stop quantity stays this far (relative to tol) from tol at every check

# name: (m, n, k, alpha_W, alpha_H, l1_ratio, seed, tol, max_iter, start)
PATTERN_CASES = {
    "k2": (300, 260, 2, 0.0, 0.0, 0.0, 1, 2e-2, 40, "plain"),
    "k5": (290, 262, 5, 0.0, 0.0, 0.0, 1, 3e-2, 40, "plain"),
    "k16": (310, 258, 16, 0.0, 0.0, 0.0, 1, 4e-2, 40, "plain"),
    "k17": (300, 270, 17, 0.0, 0.0, 0.0, 2, 1e-3, 40, "plain"),          # runs to max_iter
    "k33": (320, 264, 33, 0.0, 0.0, 0.0, 1, 1e-3, 12, "away"),
    "k64": (300, 280, 64, 0.0, 0.0, 0.0, 3, 1e-3, 6, "away"),
    "k128": (330, 290, 128, 0.0, 0.0, 0.0, 4, 1e-3, 3, "away"),
    "k5_l1": (290, 262, 5, 2e-4, 3e-4, 1.0, 1, 4e-2, 40, "plain"),
    "k17_elastic": (300, 270, 17, 2e-4, 3e-4, 0.5, 1, 4e-2, 40, "plain"),
    "k5_degenerate": (290, 262, 5, 0.0, 0.0, 0.0, 3, 3e-2, 40, "degenerate"),
}
DENSITY = {"k33": 0.17, "k64": 0.35, "k128": 0.6}
FULL_MASK = "full_mask"       # 150 x 30, k = 5, every entry stored: long on the H side (150 entries a column), short on the W side
PLANTED = "planted"           # 200 x 150, rank 4, 40 % observed; the other 60 % is the test matrix
ALL_CASES = list(PATTERN_CASES) + [FULL_MASK, PLANTED]
FP32_VIEW_CASE = "k17_elastic"
FOLD_IN_CASE = "k5"
DEGENERATE_ZERO_COLUMN = 2    # the column of W0 that is zero in the degenerate start

# The largest deviation of the float64 orders ("seq", "pair") from the longdouble restatement after ONE H sweep and after the W sweep
# that follows it, relative to the largest entry of the swept factor -- written down from tests/test_masked_cpu.py, which checks that
# they still bound what it computes.  The GPU bar of the single sweeps is SWEEP_MARGIN times these, and never below 64 k 2^-53.
SWEEP_DEVIATION = {            # (H sweep, W sweep); the floor 64 k 2^-53 is 1.4e-14 at k = 2 and 9.1e-13 at k = 128
    "k2": (3.1e-16, 3.5e-16),
    "k5": (3.6e-16, 4.0e-16),
    "k16": (5.9e-16, 1.7e-15),
    "k17": (2.1e-16, 1.2e-15),
    "k33": (4.7e-16, 1.6e-15),
    "k64": (6.7e-16, 4.3e-14),
    "k128": (2.0e-15, 5.1e-15),
    "k5_l1": (3.0e-16, 6.1e-16),
    "k17_elastic": (3.1e-16, 9.3e-16),
    "k5_degenerate": (1.5e-16, 4.0e-16),
    "full_mask": (7.1e-16, 1.0e-15),
    "planted": (6.5e-16, 6.9e-16),
}


def sweep_bar(name, side):
    """the GPU bar of one sweep; side 0: the H sweep, 1: the W sweep"""
    k = case(name)["k"]
    return max(SWEEP_MARGIN * SWEEP_DEVIATION[name][side], 64 * k * U53)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def pattern(m, n, seed, density=0.06):
    """the boolean m x n pattern of a pattern case, and its special rows and columns in the order of EDGE_COUNTS"""
    rng = np.random.default_rng(9000 + seed + 7 * m + 13 * n)
    srows = rng.choice(m, len(EDGE_COUNTS), replace=False)
    scols = rng.choice(n, len(EDGE_COUNTS), replace=False)
    body_r = np.setdiff1d(np.arange(m), srows)
    body_c = np.setdiff1d(np.arange(n), scols)
    mask = np.zeros((m, n), dtype=bool)
    mask[np.ix_(body_r, body_c)] = rng.random((body_r.size, body_c.size)) < density
    for r, c, cnt in zip(srows, scols, EDGE_COUNTS):
        mask[r, rng.choice(body_c, cnt, replace=False)] = True
        mask[rng.choice(body_r, cnt, replace=False), c] = True
    return mask, srows, scols


def csc_of(X, mask):
    """the CSC triple of the entries of X where mask is true, zeros included"""
    cols, rows = np.nonzero(mask.T)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int64)
    return X[rows, cols].astype(np.float64), rows.astype(np.uint32), indptr, (int(X.shape[0]), int(X.shape[1]))


def start(m, n, k, mean, seed, kind="plain", mask=None):
    """|N(0, 1)| sqrt(mean / k), rounded to fp32.  kind "away": uniform on [0.5, 1.5) sqrt(mean / k) instead -- where a column stores
    fewer entries than k, its first coordinates fit them exactly and the later ones divide what rounding left of the residual by
    W[i, t]: a start that comes arbitrarily close to zero makes that quotient as large as it likes"""
    rng = np.random.default_rng(500 * seed + m + 3 * n + 7 * k)
    s = np.sqrt(mean / k)
    if kind == "away":
        return f32((0.5 + rng.random((m, k))) * s), f32((0.5 + rng.random((k, n))) * s)
    W0, H0 = f32(np.abs(rng.standard_normal((m, k))) * s), f32(np.abs(rng.standard_normal((k, n))) * s)
    if kind == "degenerate":
        # Zeros only where a row / column stores at least 2 k entries.  With fewer entries than k the first coordinates fit them
        # exactly, and whether a later coordinate that starts at zero stays there hangs on the sign of what rounding left.
        many_r, many_c = mask.sum(axis=1) >= 2 * k, mask.sum(axis=0) >= 2 * k
        W0[many_r, DEGENERATE_ZERO_COLUMN] = 0.0           # hess == 0 on the H side (l2 = 0) wherever a column meets such rows only
        H0[(rng.random((k, n)) < 0.2) & many_c[None, :]] = 0.0      # the projected-gradient rule
    return W0, H0


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: csc (data, indices, indptr, shape), W0, H0, k, kw (the keyword arguments of the fit), and for the planted case test_csc;
    dense: the full matrix where every entry is stored"""
    if name == FULL_MASK:
        m, n, k, seed = 150, 30, 5, 1
        rng = np.random.default_rng(77)
        Ws = rng.integers(0, 4, (m, k)) * (rng.random((m, k)) < 0.5)
        Hs = rng.integers(0, 4, (k, n)) * (rng.random((k, n)) < 0.5)
        A = (Ws @ Hs * 4 + rng.integers(0, 8, (m, n))).astype(np.float64) / 8          # exact in fp32; has zeros
        W0, H0 = start(m, n, k, A.mean(), seed)
        kw = {"alpha_W": 0.0, "alpha_H": 0.0, "l1_ratio": 0.0, "tol": 1e-4, "max_iter": 200}
        return {"csc": csc_of(A, np.ones((m, n), dtype=bool)), "dense": A, "W0": W0, "H0": H0, "k": k, "kw": kw}
    if name == PLANTED:
        # seed 6: the first at which no row of the planted W and no column of the planted H is all zero.  Such a row or column of A
        # is all zero, its exact fit lies on the boundary, and whether a coordinate ends at 0 or at 1e-17 hangs on a rounding.
        m, n, k, seed = 200, 150, 4, 6
        rng = np.random.default_rng(4242 + seed)
        Ws = rng.random((m, k)) * (rng.random((m, k)) < 0.7)
        Hs = rng.random((k, n)) * (rng.random((k, n)) < 0.7)
        A = f32(Ws @ Hs)
        seen = rng.random((m, n)) < 0.4
        W0, H0 = start(m, n, k, A[seen].mean(), seed)
        kw = {"alpha_W": 0.0, "alpha_H": 0.0, "l1_ratio": 0.0, "tol": 1e-5, "max_iter": 300}
        return {"csc": csc_of(A, seen), "test_csc": csc_of(A, ~seen), "dense": A, "seen": seen, "W0": W0, "H0": H0, "k": k, "kw": kw}
    m, n, k, aw, ah, rho, seed, tol, max_iter, kind = PATTERN_CASES[name]
    mask, srows, scols = pattern(m, n, seed, DENSITY.get(name, 0.06))
    rng = np.random.default_rng(100 * seed + m + 3 * n + 7 * k)
    rank = min(k, 6)
    Ws = rng.random((m, rank)) * (rng.random((m, rank)) < 0.7)
    Hs = rng.random((rank, n)) * (rng.random((rank, n)) < 0.7)
    A = f32(Ws @ Hs + 0.05 * rng.random((m, n)))
    # measured zeros, off the special rows and columns: where a column stores fewer entries than k and one of them is 0, the exact
    # fit lies ON the boundary x = 0 and whether the last coordinate ends at 0 or at 1e-16 hangs on a rounding
    zero = rng.random((m, n)) < 0.09
    zero[srows, :] = False
    zero[:, scols] = False
    A[zero] = 0.0
    W0, H0 = start(m, n, k, A[mask].mean(), seed, kind, mask)
    kw = {"alpha_W": aw, "alpha_H": ah, "l1_ratio": rho, "tol": tol, "max_iter": max_iter}
    return {"csc": csc_of(A, mask), "mask": mask, "dense": A, "srows": srows, "scols": scols, "W0": W0, "H0": H0, "k": k, "kw": kw}

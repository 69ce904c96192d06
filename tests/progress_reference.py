"""The stopping rule's sums restated on the host -- TEST INFRASTRUCTURE ONLY.

For every algorithm the scalars the rule is formed from are a pure function of A and the iteration's final factors
(projected_gradient.hpp:125-171, progress_estimator_generic.hpp:30-109; oracle/nmf_oracle.c: pg_sum and the ends of mu_iter,
hals_iter, bpp_iter and rank2_iter):

    gradW = W HH' - A H'        gradH = W'W H - W'A        S_X = sum g^2 over the entries with g < 0 or x > 0
    DELTA_FNORM: ||W - Wprev||^2 and ||W||^2, Wprev = W at the previous evaluation (W0 before the first)

Plain numpy, evaluated twice: in np.longdouble (the reference value) and in float64 (whose distance from the former, e_ref, is
the rounding error of an fp64 evaluation of the same sums and sets the bar for the device's).  A is taken as the device holds
it: a dense array of the stored values, or the CSC arrays of a sparse matrix.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble


def kp_of(k: int) -> int:
    """the padded rank of the column-tile kernels (smallk_amd/csrc/common.h: kp_of)"""
    for kp in (8, 16, 32, 64, 128):
        if k <= kp:
            return kp
    return (k + 63) // 64 * 64


def tile_columns(algorithm: str, k: int) -> int:
    """Columns of a factor per workgroup of the kernels that form the projected sums: 256 threads at KP / 4 lanes per column in
    the column-tile kernels (kernels.hip: grad_pg_body), one column per thread in rank2_progress_kernel, 4 columns per workgroup
    in the wide kernels (k > 128)."""
    if algorithm == "RANK2":
        return 256
    if k > 128:
        return 4
    return 1024 // kp_of(k)


def _csc(A):
    """(data, indices, indptr, shape) of a scipy sparse matrix or of such a tuple; None for a dense array"""
    if isinstance(A, tuple):
        return A
    if hasattr(A, "tocsc"):
        A = A.tocsc()
        return A.data, A.indices, A.indptr, A.shape
    return None


def products(A, W, H, dtype):
    """(A H', W'A) in `dtype`: m x k and k x n"""
    W = np.asarray(W, dtype=dtype)
    H = np.asarray(H, dtype=dtype)
    sp = _csc(A)
    if sp is None:
        A = np.asarray(A, dtype=dtype)
        return A @ H.T, W.T @ A
    data, indices, indptr, (m, n) = sp
    rows = np.asarray(indices, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(indptr, dtype=np.int64)))
    v = np.asarray(data, dtype=dtype)[:, None]
    AHt = np.zeros((m, W.shape[1]), dtype=dtype)
    WtAt = np.zeros((n, W.shape[1]), dtype=dtype)
    np.add.at(AHt, rows, v * H.T[cols])          # stored entries in storage order, duplicates add up
    np.add.at(WtAt, cols, v * W[rows])
    return AHt, WtAt.T


def _side(G, X):
    """per column of the k-major side (a row of W / a column of H): the projected sum and the whole sum of g^2"""
    g2 = G * G
    return np.where((G < 0) | (X > 0), g2, 0).sum(axis=0), g2.sum(axis=0)


def _tile_shares(contrib, tile):
    total = contrib.sum()
    nt = (len(contrib) + tile - 1) // tile
    if not total > 0:
        return np.zeros(nt)
    return np.array([float(contrib[t * tile:(t + 1) * tile].sum() / total) for t in range(nt)])


@dataclass
class ProjectedSums:
    sw: LD                      # the projected sum of the W side / the H side, long double
    sh: LD
    sw64: float                 # the same evaluated in float64
    sh64: float
    e_ref_w: float              # |s64 - s_ld| / s_ld per side (0 for an all-zero side)
    e_ref_h: float
    excluded_w: float           # the share of sum g^2 the projection leaves out, per side
    excluded_h: float
    tile_share_w: np.ndarray    # every kernel column tile's share of its side's projected sum
    tile_share_h: np.ndarray
    col_w: np.ndarray = None    # the projected sum per row of W / per column of H (long double)
    col_h: np.ndarray = None

    def shard_tile_shares_h(self, col0, ncols, tile):
        """the shares (of the whole H side's sum) of the column tiles of a rank that holds columns [col0, col0 + ncols) and tiles
        them from its own first column"""
        c = self.col_h[col0:col0 + ncols]
        return np.array([float(c[t:t + tile].sum() / self.sh) for t in range(0, ncols, tile)])

    @property
    def pg(self) -> LD:
        return np.sqrt(self.sw + self.sh)


def _projected(A, W, H, dtype):
    W = np.asarray(W, dtype=dtype)
    H = np.asarray(H, dtype=dtype)
    AHt, WtA = products(A, W, H, dtype)
    gradW = W @ (H @ H.T) - AHt
    gradH = (W.T @ W) @ H - WtA
    return _side(gradW.T, W.T), _side(gradH, H)


def projected_sums(A, W, H, tile) -> ProjectedSums:
    """The two projected-gradient sums of (A, W, H), separately, with each kernel tile's share (tile = tile_columns(...))"""
    (cw, aw), (ch, ah) = _projected(A, W, H, LD)
    (cw64, _), (ch64, _) = _projected(A, W, H, np.float64)
    sw, sh = cw.sum(), ch.sum()
    sw64, sh64 = float(cw64.sum()), float(ch64.sum())
    rel = lambda s64, s: float(abs(LD(s64) - s) / s) if s > 0 else 0.0
    exc = lambda s, a: float(1 - s / a) if a > 0 else 0.0
    return ProjectedSums(sw, sh, sw64, sh64, rel(sw64, sw), rel(sh64, sh), exc(sw, aw.sum()), exc(sh, ah.sum()),
                         _tile_shares(cw, tile), _tile_shares(ch, tile), cw, ch)


@dataclass
class DeltaSums:
    num: LD                     # ||W - Wprev||_F^2 and ||W||_F^2, long double / float64
    den: LD
    num64: float
    den64: float
    e_ref_num: float
    e_ref_den: float

    @property
    def metric(self) -> LD:
        return np.sqrt(self.num) / np.sqrt(self.den)


def delta_fnorm_sums(W, Wprev) -> DeltaSums:
    """DELTA_FNORM's two sums from (W, Wprev)"""
    out = []
    for dt in (LD, np.float64):
        w, p = np.asarray(W, dtype=dt), np.asarray(Wprev, dtype=dt)
        d = p - w
        out.append(((d * d).sum(), (w * w).sum()))
    (num, den), (num64, den64) = out
    rel = lambda s64, s: float(abs(LD(s64) - s) / s) if s > 0 else 0.0
    return DeltaSums(num, den, float(num64), float(den64), rel(num64, num), rel(den64, den))


def bar(s_ld, e_ref, total, floor=1e-12, multiple=64.0) -> float:
    """How far a device sum may lie from the long-double sum s_ld of its side: max(multiple * e_ref, floor) * s_ld, and for a side
    that is pure rounding (s_ld < floor * total, total = both sides together) floor * total on top"""
    b = max(multiple * e_ref, floor) * float(s_ld)
    if float(s_ld) < floor * float(total):
        b += floor * float(total)
    return b

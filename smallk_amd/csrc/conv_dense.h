// smallk_amd/csrc/conv_dense.h -- what conv_dense.hip offers conv_dense.cpp: convolutive NMF on a dense stored matrix,
//     Lambda[i, j] = sum_{t < T} sum_{r < k} W_t[i, r] H[r, j - t]                       (terms with j - t < 0 are absent),
// under the Kullback-Leibler (beta = 1) and Itakura-Saito (beta = 0) divergences.  The resident factors: Wc is m x (T KP4), row i
// holding the T slices one after the other, entry (t, r) at i T KP4 + t KP4 + r; Hc is KP4 x n with pitch KP4, entry (r, j) at
// j KP4 + r; KP4 = conv_kp4(k), and every pad entry (r >= k) is zero and stays zero.  T KP4 <= 128.
#pragma once
#include "common.h"

namespace smk {

inline int conv_kp4(int k) { return (k + 3) / 4 * 4; }

// doubles of scratch every launch below is content with, for a matrix of m x n and its transpose
size_t conv_dense_scratch_elems(i64 m, i64 n, int k, int T, int num_cus);
// one half-iteration.  w_side = 0: H in place from A (m x n as stored, ld elements per column) and Wc; w_side = 1: Wc in place from
// the stored transpose At (n x m) and Hc.  beta 0 or 1; l1, l2, flush: beta_update's (kl_dev.h); gamma is 1 at beta = 1, 1/2 at 0
int launch_conv_dense_step(const void* A, int storage, i64 ld, i64 m, i64 n, int w_side, double* Wc, double* Hc, int k, int T, int beta, double l1,
                           double l2, int flush, double* scratch, int num_cus, hipStream_t st);
// out4 (device; and host_out when not null, pinned) = D and the sums it is formed from, over A (m x n as stored).  beta = 0:
// {D, sum a / d, sum log(a / d), m n}; beta = 1: {D, sum a log(a / d), sum Lambda, 0}; the entries with a > EPS, d clamped at EPS
int launch_conv_dense_divergence(const void* A, int storage, i64 ld, i64 m, i64 n, const double* Wc, const double* Hc, int k, int T, int beta,
                                 double* scratch, double* out4, double* host_out, int num_cus, hipStream_t st);

}  // namespace smk

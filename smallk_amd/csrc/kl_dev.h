// smallk_amd/csrc/kl_dev.h -- what the kernels of the two KL-divergence paths share (kl.hip: sparse; kl_dense.hip:
// dense) and the other beta-divergences (beta_dense.hip): scikit-learn's two epsilons and the
// multiplicative update of one factor entry.  Device code only.
#pragma once
#include "devutil.h"

namespace smk {

static constexpr double KL_EPS = 1.1920928955078125e-07;       // 2^-23: sklearn's EPSILON (float32's)
static constexpr double KL_EPS64 = 2.220446049250313e-16;      // 2^-52

// the multiplicative update of one entry; base: the sum of row t of the other factor (unit: a zero sum counts as 1.0)
__device__ __forceinline__ double kl_update(double x, double num, double base, int unit, double l1, double l2, int flush)
{
    double den = (unit && base == 0.0) ? 1.0 : base;
    if (l1 > 0.0) den = den + l1;
    if (l2 > 0.0) den = den + __dmul_rn(l2, x);
    if (den == 0.0) den = KL_EPS;
    double xn = __dmul_rn(x, num / den);
    if (flush && xn < KL_EPS64) xn = 0.0;
    return xn;
}

// the same for another beta-divergence (beta_dense.hip): the denominator is a sum of its own, there is no unit rule,
// and the quotient is raised to gamma -- gmode 0: gamma = 1, 1: gamma = 1/2 (a square root, not a power), 2: pow
__device__ __forceinline__ double beta_update(double x, double num, double den, double l1, double l2, int gmode, double gamma, int flush)
{
    if (l1 > 0.0) den = den + l1;
    if (l2 > 0.0) den = den + __dmul_rn(l2, x);
    if (den == 0.0) den = KL_EPS;
    double q = num / den;
    if (gmode == 1) q = __dsqrt_rn(q);
    else if (gmode == 2) q = pow(q, gamma);
    double xn = __dmul_rn(x, q);
    if (flush && xn < KL_EPS64) xn = 0.0;
    return xn;
}

}  // namespace smk

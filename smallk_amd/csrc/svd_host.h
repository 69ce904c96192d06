// smallk_amd/csrc/svd_host.h -- the host steps of the truncated SVD (svd.cpp): the symmetric eigendecomposition of
// an l x l Gram matrix (l <= 128) by cyclic Jacobi rotations in a fixed sweep order, and the matrix M = E Lambda^(-1/2) that
// orthonormalises the factor the Gram matrix came from.  Plain C++ without a HIP header: tests/svd_host/jacobi_check.cpp
// includes this file by itself.  Sequential fp64 arithmetic throughout: the same input gives the same bits on every run.
#pragma once
#include <cmath>
#include <cstddef>
#include <numeric>
#include <algorithm>
#include <vector>

namespace smk {
namespace svdh {

// eigenvalues at or below this fraction of the largest one count as zero (rank deficient factors are ordinary inputs)
constexpr double RANK_TOL = 0x1.0p-40;
constexpr int JACOBI_MAX_SWEEPS = 60;

// jacobi_eigh's time follows where the linker happens to start it within a 64-byte line of code (12 decompositions at l = 24: 0.70 ms
// from 32 or 48 bytes into a line, 0.79 ms from its start; profiles/view_entries_ab.txt): pinned at 32, by 32 bytes of no-ops.
#if defined(__clang__) && defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define SVDH_PLACED __attribute__((aligned(64), patchable_function_entry(32)))
#else
#define SVDH_PLACED
#endif

// G: l x l symmetric with leading dimension ldg (only read).  lambda: l eigenvalues, largest first (equal ones by the
// order Jacobi left them in); E: l x l row-major, column j the unit eigenvector of lambda[j].  Returns the sweeps taken.
SVDH_PLACED inline int jacobi_eigh(const double* G, int ldg, int l, std::vector<double>& lambda, std::vector<double>& E)
{
    std::vector<double> a((size_t)l * l), v((size_t)l * l, 0.0);
    double gmax = 0.0;
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
            // the two triangles of a Gram matrix formed in a fixed order agree; averaging makes the copy symmetric whatever came in
            const double x = 0.5 * (G[(size_t)i * ldg + j] + G[(size_t)j * ldg + i]);
            a[(size_t)i * l + j] = x;
            if (std::fabs(x) > gmax) gmax = std::fabs(x);
        }
    for (int i = 0; i < l; ++i) v[(size_t)i * l + i] = 1.0;
    const double u = 0x1.0p-53;
    const double floor_abs = gmax * u * u;          // below u^2 ||G||: nothing a rotation could improve
    int sweeps = 0;
    for (; sweeps < JACOBI_MAX_SWEEPS; ++sweeps) {
        int rotations = 0;
        for (int p = 0; p < l - 1; ++p)
            for (int q = p + 1; q < l; ++q) {
                const double apq = a[(size_t)p * l + q];
                const double app = a[(size_t)p * l + p], aqq = a[(size_t)q * l + q];
                if (apq == 0.0 || std::fabs(apq) <= floor_abs) continue;
                if (std::fabs(apq) <= 2.0 * u * std::sqrt(std::fabs(app) * std::fabs(aqq))) continue;   // relative: small eigenvalues keep their digits
                ++rotations;
                const double theta = (aqq - app) / (2.0 * apq);
                double t;
                if (std::fabs(theta) > 1.0e150) t = 0.5 / theta;
                else t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < l; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[(size_t)k * l + p], akq = a[(size_t)k * l + q];
                    const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                    a[(size_t)k * l + p] = a[(size_t)p * l + k] = np_;
                    a[(size_t)k * l + q] = a[(size_t)q * l + k] = nq_;
                }
                a[(size_t)p * l + p] = app - t * apq;
                a[(size_t)q * l + q] = aqq + t * apq;
                a[(size_t)p * l + q] = a[(size_t)q * l + p] = 0.0;
                for (int k = 0; k < l; ++k) {
                    const double vkp = v[(size_t)k * l + p], vkq = v[(size_t)k * l + q];
                    v[(size_t)k * l + p] = c * vkp - s * vkq;
                    v[(size_t)k * l + q] = s * vkp + c * vkq;
                }
            }
        if (rotations == 0) break;
    }
    std::vector<int> order((size_t)l);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * l + x] > a[(size_t)y * l + y]; });
    lambda.assign((size_t)l, 0.0);
    E.assign((size_t)l * l, 0.0);
    for (int j = 0; j < l; ++j) {
        lambda[(size_t)j] = a[(size_t)order[(size_t)j] * l + order[(size_t)j]];
        for (int i = 0; i < l; ++i) E[(size_t)i * l + j] = v[(size_t)i * l + order[(size_t)j]];
    }
    return sweeps;
}

// how many eigenvalues (largest first) exceed RANK_TOL times the largest; 0 for a zero or negative spectrum
inline int numerical_rank(const std::vector<double>& lambda)
{
    const double top = lambda.empty() ? 0.0 : lambda[0];
    int r = 0;
    while (r < (int)lambda.size() && lambda[(size_t)r] > RANK_TOL * top && lambda[(size_t)r] > 0.0) ++r;
    return r;
}

// M (l x l row-major) = E Lambda^(-1/2) for the eigenvalues above the rank threshold, zero columns for the rest: Y M has
// orthonormal columns where Y'Y = G has rank, and exact zeros where it has none.  Returns the rank.
inline int orth_matrix(const std::vector<double>& lambda, const std::vector<double>& E, int l, std::vector<double>& M)
{
    const int r = numerical_rank(lambda);
    M.assign((size_t)l * l, 0.0);
    for (int j = 0; j < r; ++j) {
        const double d = 1.0 / std::sqrt(lambda[(size_t)j]);
        for (int i = 0; i < l; ++i) M[(size_t)i * l + j] = E[(size_t)i * l + j] * d;
    }
    return r;
}

// M (l x l row-major) = E Lambda^(-1/2) E' over the eigenvalues above the rank threshold: X M = X (X'X)^(-1/2) is the orthonormal
// matrix nearest to X, column by column the same vectors (no rotation among them); zero columns of X stay zero
inline void polish_matrix(const std::vector<double>& lambda, const std::vector<double>& E, int l, std::vector<double>& M)
{
    const int r = numerical_rank(lambda);
    M.assign((size_t)l * l, 0.0);
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
            double s = 0.0;
            for (int p = 0; p < r; ++p) s += E[(size_t)i * l + p] * E[(size_t)j * l + p] / std::sqrt(lambda[(size_t)p]);
            M[(size_t)i * l + j] = s;
        }
}

}  // namespace svdh
}  // namespace smk

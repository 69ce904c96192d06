// tests/svd_host/jacobi_check.cpp -- stand-alone check of smallk_amd/csrc/svd_host.h (the host steps of the truncated SVD):
// built with -fsanitize=address,undefined by tests/test_svd_host.py and run as a program.  For every matrix:
//   max |G E - E Lambda| <= 64 l 2^-53 max|G|,  max |E'E - I| <= 64 l 2^-53,
//   M = E Lambda^(-1/2) has zero columns exactly where lambda <= 2^-40 lambda_max,  two runs give identical bits.
// Prints one line per matrix; exit status 0 only when every check holds.
#include "../../smallk_amd/csrc/svd_host.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace smk::svdh;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double rnd()          // xorshift64*, uniform in [-1, 1)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// G = Q diag(d) Q' with Q the orthogonal factor of a random matrix (modified Gram-Schmidt, twice)
static std::vector<double> with_spectrum(const std::vector<double>& d)
{
    const int l = (int)d.size();
    std::vector<double> Q((size_t)l * l);
    for (double& x : Q) x = rnd();
    for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < l; ++j) {
            for (int p = 0; p < j; ++p) {
                double dot = 0.0;
                for (int i = 0; i < l; ++i) dot += Q[(size_t)i * l + j] * Q[(size_t)i * l + p];
                for (int i = 0; i < l; ++i) Q[(size_t)i * l + j] -= dot * Q[(size_t)i * l + p];
            }
            double nn = 0.0;
            for (int i = 0; i < l; ++i) nn += Q[(size_t)i * l + j] * Q[(size_t)i * l + j];
            nn = std::sqrt(nn);
            for (int i = 0; i < l; ++i) Q[(size_t)i * l + j] /= nn;
        }
    std::vector<double> G((size_t)l * l, 0.0);
    for (int i = 0; i < l; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int p = 0; p < l; ++p) s += Q[(size_t)i * l + p] * d[(size_t)p] * Q[(size_t)j * l + p];
            G[(size_t)i * l + j] = G[(size_t)j * l + i] = s;
        }
    return G;
}

// G = Y Y' for a random l x r matrix Y: exact rank r
static std::vector<double> gram_of_rank(int l, int r)
{
    std::vector<double> Y((size_t)l * r);
    for (double& x : Y) x = rnd();
    std::vector<double> G((size_t)l * l, 0.0);
    for (int i = 0; i < l; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int p = 0; p < r; ++p) s += Y[(size_t)i * r + p] * Y[(size_t)j * r + p];
            G[(size_t)i * l + j] = G[(size_t)j * l + i] = s;
        }
    return G;
}

static bool check(const std::string& name, const std::vector<double>& G, int l)
{
    std::vector<double> lam, E, M, lam2, E2, M2;
    const int sweeps = jacobi_eigh(G.data(), l, l, lam, E);
    const int rank = orth_matrix(lam, E, l, M);
    jacobi_eigh(G.data(), l, l, lam2, E2);
    orth_matrix(lam2, E2, l, M2);
    bool ok = true;
    const bool same = !std::memcmp(lam.data(), lam2.data(), lam.size() * sizeof(double)) &&
                      !std::memcmp(E.data(), E2.data(), E.size() * sizeof(double)) && !std::memcmp(M.data(), M2.data(), M.size() * sizeof(double));
    if (!same) ok = false;
    double gmax = 0.0;
    for (double x : G) gmax = std::fabs(x) > gmax ? std::fabs(x) : gmax;
    double res = 0.0, orth = 0.0;
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
            double ge = 0.0, ee = 0.0;
            for (int p = 0; p < l; ++p) { ge += G[(size_t)i * l + p] * E[(size_t)p * l + j]; ee += E[(size_t)p * l + i] * E[(size_t)p * l + j]; }
            res = std::fmax(res, std::fabs(ge - E[(size_t)i * l + j] * lam[(size_t)j]));
            orth = std::fmax(orth, std::fabs(ee - (i == j ? 1.0 : 0.0)));
        }
    const double bar = 64.0 * l * 0x1.0p-53;
    if (!(res <= bar * gmax)) ok = false;
    if (!(orth <= bar)) ok = false;
    for (int j = 1; j < l; ++j)
        if (lam[(size_t)j] > lam[(size_t)j - 1]) ok = false;            // largest first
    // zero columns of M exactly where lambda <= 2^-40 lambda_max
    bool cols_ok = true;
    for (int j = 0; j < l; ++j) {
        const bool expect_zero = !(lam[(size_t)j] > RANK_TOL * lam[0]) || !(lam[0] > 0.0);
        bool is_zero = true;
        for (int i = 0; i < l; ++i) {
            const double x = M[(size_t)i * l + j];
            if (x != 0.0) is_zero = false;
            if (!std::isfinite(x)) cols_ok = false;
        }
        if (is_zero != expect_zero) cols_ok = false;
    }
    if (!cols_ok) ok = false;
    std::printf("%-22s l=%3d sweeps=%2d rank=%3d resid=%.3e (bar %.3e) orth=%.3e (bar %.3e) same_bits=%d zero_cols=%d %s\n", name.c_str(), l, sweeps,
                rank, res, bar * gmax, orth, bar, (int)same, (int)cols_ok, ok ? "ok" : "FAILED");
    return ok;
}

int main()
{
    bool ok = true;
    ok &= check("l=1", std::vector<double>{3.5}, 1);
    {
        std::vector<double> d(128);
        for (int i = 0; i < 128; ++i) d[(size_t)i] = 1.0 + 0.37 * i;
        ok &= check("l=128", with_spectrum(d), 128);
    }
    ok &= check("zero", std::vector<double>(12 * 12, 0.0), 12);
    ok &= check("repeated", with_spectrum({4.0, 4.0, 4.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.5}), 10);
    ok &= check("identity", with_spectrum(std::vector<double>(9, 1.0)), 9);
    ok &= check("gram rank 3, l=20", gram_of_rank(20, 3), 20);
    {
        std::vector<double> d(16);
        for (int i = 0; i < 16; ++i) d[(size_t)i] = std::ldexp(1.0, -4 * i);        // 1 .. 2^-60
        ok &= check("2^-60 .. 1", with_spectrum(d), 16);
    }
    std::printf(ok ? "jacobi_check: all ok\n" : "jacobi_check: FAILED\n");
    return ok ? 0 : 1;
}

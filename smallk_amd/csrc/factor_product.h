// smallk_amd/csrc/factor_product.h -- the product of a resident matrix with a tall-skinny fp64 factor, outside the solver: what
// svd.cpp and cd.cpp run for every pass over A.  Dense A takes the accurate-form streaming product (launch_bigprod on an NSPLIT_F64
// plan) and the reduction of its partial products, sparse A the fp64 gather product (launch_spmm_seg / launch_spmm_gather).
// Factors are KP x N with pitch KP = kp_of(l), l <= 128 live rows.  Host code: include after state.h.
#pragma once
#include "state.h"

#include <string>

namespace smk {

struct FactorProduct {
    const smk_matrix* a = nullptr;
    int l = 0, KP = 0;
    hipStream_t st = nullptr;
    double *P = nullptr, *pieces[2] = {nullptr, nullptr};
    BigProdPlan over_m[2], over_n[2];             // dense: the contraction runs over the rows of A (B = A) / over its columns (B = A')
    int ng = 0;
};

// the product's matrix, rank, pitch and stream, its plans and workspaces (blocks of `own`).  who: the prefix of the error texts.
static inline int factor_product_alloc(FactorProduct& f, const smk_matrix* a, int l, int KP, hipStream_t st, Owned& own, const char* who)
{
    f.a = a; f.l = l; f.KP = KP; f.st = st;
    const std::string w(who);
    if (!a->sparse) {
        // one P layout for both directions and all groups: KP doubles per column, so the summed product IS a factor
        f.ng = plan_bigprod_groups(a->storage, f.l, a->m, a->n, NSPLIT_F64, ctx().cus, f.over_m);
        const int ng2 = plan_bigprod_groups(a->storage, f.l, a->n, a->m, NSPLIT_F64, ctx().cus, f.over_n);
        if (ng2 != f.ng || f.ng < 1 || f.ng > 2) { set_error(w + ": unexpected product plan"); return SMK_FAILURE; }
        size_t pe = 0;
        for (BigProdPlan* pl : {f.over_m, f.over_n})
            for (int g = 0; g < f.ng; ++g) {
                pl[g].ldx = f.KP;
                pl[g].pstride = f.KP;
                pl[g].p_elems = (size_t)pl[0].S * pl[0].ncols_pad * f.KP;
                if (pl[g].p_elems > pe) pe = pl[g].p_elems;
            }
        if (own.dev(&f.P, pe)) { set_error(w + ": no memory for the partial products"); return SMK_DEVICE_ERROR; }
        SMK_HIP(hipMemsetAsync(f.P, 0, pe * sizeof(double), f.st));      // rows of P no group writes (l <= 96 in a 128-row column) stay zero
    } else {
        ensure_seg_plans(a);             // read-only use, as the residual
        const SegPlan* sp[2] = {&a->segA, &a->segAt};
        for (int i = 0; i < 2; ++i)
            if (sp[i]->rowflag && sp[i]->npieces > 0 && own.dev(&f.pieces[i], (size_t)sp[i]->npieces * 128)) {
                set_error(w + ": no memory for the long-column partial sums");
                return SMK_DEVICE_ERROR;
            }
    }
    return 0;
}

// dense A only: the streaming launches without the reduction; *pv views the partial products in f.P (valid until the next product)
static inline int factor_product_partials(FactorProduct& f, bool over_rows, const double* X, PartialView* pv)
{
    const smk_matrix* a = f.a;
    const BigProdPlan* pl = over_rows ? f.over_m : f.over_n;
    for (int g = 0; g < f.ng; ++g) {
        const int rc = over_rows ? launch_bigprod(pl[g], a->A, a->ldA, X + pl[g].k0, f.P + pl[g].k0, f.st)
                                 : launch_bigprod(pl[g], a->At, a->ldAt, X + pl[g].k0, f.P + pl[g].k0, f.st);
        if (rc < 0) return rc;
    }
    *pv = PartialView{f.P, pl[0].S, (i64)pl[0].ncols_pad * f.KP, f.KP, 1};
    return 0;
}

// over_rows: out (KP x n) = (A' X')' for X = KP x m, the contraction over the rows of A; else out (KP x m) = (A X')' for X = KP x n
static inline int factor_product(FactorProduct& f, bool over_rows, const double* X, double* out)
{
    const smk_matrix* a = f.a;
    const i64 N = over_rows ? a->n : a->m;
    if (!a->sparse) {
        PartialView pv;
        const int rc = factor_product_partials(f, over_rows, X, &pv);
        if (rc) return rc;
        return launch_reduce_partials(pv, f.l, 0, N, out, 1, f.st);
    }
    // sparse: column j of the output gathers the rows of X named by column j of CSC(A) (over_rows) or of CSC(A')
    const i64* colptr = over_rows ? a->colptr : a->colptr_t;
    const unsigned* rowidx = over_rows ? a->rowidx : a->rowidx_t;
    const double* val = over_rows ? a->val : a->val_t;
    const SegPlan& seg = over_rows ? a->segA : a->segAt;
    int rc;
    if (f.l > 2 && seg.rowflag && seg.ncols == N && !seg.uniform)
        rc = launch_spmm_seg(seg, colptr, val, X, f.l, out, f.KP, f.st, f.pieces[over_rows ? 0 : 1]);
    else {
        if (f.l <= 2) SMK_HIP(hipMemsetAsync(out, 0, (size_t)f.KP * N * sizeof(double), f.st));    // the rank-2 gather writes two rows
        rc = launch_spmm_gather(colptr, rowidx, val, N, a->nnz, X, f.KP, f.l, out, f.KP, f.st);
    }
    return rc < 0 ? rc : 0;
}

}  // namespace smk

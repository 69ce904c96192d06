// Prints what smallk_amd/csrc/bigprod_plan.h states and decides, one record per line, for tests/test_bigprod_plan_cpu.py to compare
// with restatements that do not come from the header.  Includes nothing of the library but that header.
#include "../../smallk_amd/csrc/bigprod_plan.h"
#include <cstdio>
#include <vector>

using namespace smk;

int main()
{
    // ---- the tables and the fit functions ----
    for (int i = 0; i < kNumVariants; ++i) {
        const BPRow& r = kVariants[i];
        printf("bp %d %d %d %d %d %d\n", i, r.mb, r.nstage, r.cw, r.wk, r.nwl);
        for (int ebytes : {2, 4})
            for (int kt : {1, 2})
                for (int nsplit : {1, 2, 3, 4}) printf("bpfits %d %d %d %d %d\n", i, ebytes, kt, nsplit, (int)bp_fits(ebytes, kt, nsplit, r));
    }
    for (int i = 0; i < kNumF3; ++i) {
        const F3Row& r = kF3Variants[i];
        printf("f3 %d %s %d %d %d %d %d %d %d %d\n", 100 + i, r.kernel == F3P ? "f3p" : "f3", r.mb, r.nstage, r.nwl, r.fold, r.arg, (int)r.bf, (int)r.f16,
               (int)r.tail);
        for (int kt : {1, 2})
            for (int form : {2, 3, 4}) printf("f3fits %d %d %d %d\n", 100 + i, kt, form, (int)f3_fits(r, kt, pack_terms(form)));
    }

    // ---- the variant a plan settles on ----
    std::vector<Want> wants = {{false, 0}, {true, -1}};
    for (int v = 0; v <= 30; ++v) wants.push_back({true, v});
    wants.push_back({true, 99});
    for (int v = 100; v <= 131; ++v) wants.push_back({true, v});
    wants.push_back({true, 200});
    printf("wants");
    for (const Want& w : wants) w.set ? printf(" %d", w.v) : printf(" unset");
    printf("\n");
    const long lens[] = {1, 4095, 4096, 16383, 16384, 65535, 65536};
    for (int storage : {STORE_F32, STORE_BF16})
        for (int k : {1, 16, 17, 32, 33, 64})
            for (long len : lens) {
                for (int form : {1, 2, 3, 4, 8}) {
                    printf("variant %d %d %ld %d", storage, k, len, form);
                    for (const Want& w : wants)
                        for (const Want& w64 : wants) printf(" %d", choose_variant(storage, kt_of(k), form, len, w, w64));
                    printf("\n");
                }
                printf("variant_tr %d %d %ld %d\n", storage, k, len, choose_variant(storage, kt_of(k), storage == STORE_F32 ? 4 : 3, len, {}, {}, true));
            }

    // ---- chain lengths, riders ----
    std::vector<int> variants;
    for (int v = 0; v < kNumVariants; ++v) variants.push_back(v);
    for (int v = 100; v < 100 + kNumF3; ++v) variants.push_back(v);
    variants.push_back(ACCURATE_VARIANT);
    for (int storage : {STORE_F32, STORE_BF16})
        for (int v : variants)
            for (int tr : {0, 1}) printf("chain %d %d %d %d\n", storage, v, tr, chain_rows(storage, v, tr != 0));
    for (int v : {-1, 24, 99, 130, 199}) printf("chain_unknown %d %d %d\n", v, chain_rows(STORE_F32, v, false), chain_rows(STORE_BF16, v, false));
    variants.insert(variants.end(), {24, 99, 130, 131});
    for (int storage : {STORE_F32, STORE_BF16})
        for (int nsplit : {1, 2, 3, 4, 8})
            for (int v : variants) {
                for (int tr : {0, 1}) printf("ride %d %d %d %d %d\n", storage, nsplit, v, tr, (int)variant_rides(storage, nsplit, v, tr != 0));
                for (int kt : {1, 2}) printf("tail %d %d %d %d %d\n", storage, nsplit, kt, v, (int)variant_tails(storage, nsplit, kt, v));
            }

    // ---- the product form ----
    const Want nsplits[] = {{false, 0}, {true, -1}, {true, 0}, {true, 1}, {true, 2}, {true, 3}, {true, 4}, {true, 5}, {true, 8}, {true, 9}};
    for (int alg : {ALG_MU, ALG_HALS, ALG_RANK2, ALG_BPP})
        for (int k : {2, 16, 32, 33, 64, 65, 200})
            for (int storage : {STORE_F32, STORE_BF16})
                for (int sparse : {0, 1})
                    for (long entries : {1L << 24, (1L << 24) + 1})
                        for (int spread : {-1, 0, 28, 29})
                            for (int small : {0, 1})
                                for (const Want& ns : nsplits) {
                                    printf("form %d %d %d %d %ld %d %d ", alg, k, storage, sparse, entries, spread, small);
                                    ns.set ? printf("%d", ns.v) : printf("unset");
                                    printf(" %d %d\n", default_product_form(alg, k, storage, sparse != 0, entries, spread, small != 0, ns.set),
                                           resolve_product_form(alg, k, storage, sparse != 0, entries, spread, small != 0, ns));
                                }
    printf("plan_dump: done\n");
    return 0;
}

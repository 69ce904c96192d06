// smallk_amd/csrc/tree_route.cpp -- new documents down a fitted HierNMF2 tree, on the device (include/smallk_amd.h: smk_tree_router_*,
// smk_tree_route_device).  A router is built once from a tree's links and topic vectors -- the arrays themselves
// (smk_tree_router_create: a saved tree) or a live smk_tree through its public accessors (smk_tree_router_from_tree); nothing here
// reads hierclust.cpp's types.  The structure check is host code of its own (tree_route_check.h).  Per pair of siblings the router
// keeps the two topic vectors interleaved (16 bytes per term), their Gram triple and its prepared rank-2 solve; routing is one launch
// of tree_route.hip over the columns of a resident sparse matrix.  The entry is synchronous; its stream wait and the timing
// events belong to the smk::Entry local (entry.h); the outputs are written by that one launch and by nothing before it.
#include "entry.h"
#include "tree_route.h"
#include "tree_route_check.h"

#include <string>
#include <vector>

struct smk_tree_router {
    i64 m = 0;
    int node_count = 0;
    RoutePlan plan;
    // what create took, for smk_tree_router_download (a saved router is rebuilt from them)
    std::vector<unsigned> left, right;
    std::vector<int> valid;
    std::vector<double> topics;              // m x node_count, column-major, ld m
    // the device tables: T[p][row] = (w_l[row], w_r[row]); gram[3 p ..] = (w_l.w_l, w_l.w_r, w_r.w_r); solve[p] = its r2_prepare;
    // child_pair per node, pair_nodes per pair
    double *T = nullptr, *gram = nullptr;
    void* solve = nullptr;
    int *child_pair = nullptr, *pair_nodes = nullptr;
    smk::Owned own;
    i64 table_bytes() const { return (i64)plan.pairs * m * 16; }
};

namespace smk {

// the last smk_tree_route_device call of the calling thread (smk_tree_route_last_profile)
static thread_local int g_route_launches = 0;
static thread_local i64 g_route_entries = 0;

static int route_plan_or_error(const std::string& w, int node_count, const unsigned* left, const unsigned* right, const int* valid, RoutePlan* plan)
{
    std::string err;
    if (tree_route_plan(node_count, left, right, valid, plan, &err)) { set_error(w + ": " + err); return SMK_BAD_PARAM; }
    return SMK_OK;
}

// the device tables of a router whose host arrays and plan are in place
static int router_pack(smk_tree_router* r, const std::string& w)
{
    const hipStream_t st = ctx().stream;
    const i64 m = r->m;
    const int pairs = r->plan.pairs;
    char* solve = nullptr;
    int* bad = nullptr;
    if (r->own.dev(&r->T, (size_t)pairs * (size_t)m * 2) || r->own.dev(&r->gram, (size_t)pairs * 3) ||
        r->own.dev(&solve, (size_t)pairs * tree_route_solve_bytes()) || r->own.dev(&r->child_pair, (size_t)r->node_count) ||
        r->own.dev(&r->pair_nodes, (size_t)pairs * 2) || r->own.dev(&bad, (size_t)pairs)) {
        set_error(w + ": no device memory for the tables (" + std::to_string(r->table_bytes()) + " bytes of topic vectors)");
        return SMK_DEVICE_ERROR;
    }
    r->solve = solve;
    std::vector<double> g((size_t)pairs * 3), stage((size_t)m * 2);
    for (int p = 0; p < pairs; ++p) {
        const double* wl = r->topics.data() + (size_t)r->plan.pair_nodes[2 * p] * m;
        const double* wr = r->topics.data() + (size_t)r->plan.pair_nodes[2 * p + 1] * m;
        double a00 = 0.0, a01 = 0.0, a11 = 0.0;              // row order: the same sums on every build
        for (i64 i = 0; i < m; ++i) {
            a00 += wl[i] * wl[i];
            a01 += wl[i] * wr[i];
            a11 += wr[i] * wr[i];
            stage[2 * i] = wl[i];
            stage[2 * i + 1] = wr[i];
        }
        g[3 * (size_t)p] = a00; g[3 * (size_t)p + 1] = a01; g[3 * (size_t)p + 2] = a11;
        SMK_HIP(hipMemcpyAsync(r->T + (size_t)p * m * 2, stage.data(), (size_t)m * 2 * sizeof(double), hipMemcpyHostToDevice, st));
        SMK_HIP(hipStreamSynchronize(st));                    // (the staging row is written again)
    }
    SMK_HIP(hipMemcpyAsync(r->gram, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, st));
    SMK_HIP(hipMemcpyAsync(r->child_pair, r->plan.child_pair.data(), (size_t)r->node_count * sizeof(int), hipMemcpyHostToDevice, st));
    SMK_HIP(hipMemcpyAsync(r->pair_nodes, r->plan.pair_nodes.data(), (size_t)pairs * 2 * sizeof(int), hipMemcpyHostToDevice, st));
    if (int rc = launch_tree_route_prepare(r->gram, pairs, r->solve, bad, st)) return rc;
    std::vector<int> hbad((size_t)pairs);
    SMK_HIP(hipMemcpyAsync(hbad.data(), bad, (size_t)pairs * sizeof(int), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    r->own.drop(&bad);
    for (int p = 0; p < pairs; ++p)
        if (hbad[(size_t)p]) {
            set_error(w + ": the topic vectors of nodes " + std::to_string(r->plan.pair_nodes[2 * p]) + " and " +
                      std::to_string(r->plan.pair_nodes[2 * p + 1]) + " (pair " + std::to_string(p) + ") have a singular Gram matrix");
            return SMK_FAILURE;
        }
    return SMK_OK;
}

static int route_args(const std::string& w, const smk_tree_router* r, const smk_matrix* a)
{
    if (int rc = require_init()) return rc;
    if (!r || !a) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (!a->sparse) { set_error(w + ": sparse input only (dense new documents are not routed)"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (a->m != r->m) { set_error(w + ": the matrix has " + std::to_string(a->m) + " rows, the tree " + std::to_string(r->m) + " terms"); return SMK_BAD_PARAM; }
    return SMK_OK;
}

static int route_launch(const smk_tree_router* r, const smk_matrix* a, int* leaf, int* depth, double* h, hipStream_t st)
{
    return launch_tree_route(a->colptr, a->rowidx, a->val, a->n, r->m, r->T, r->solve, r->child_pair, r->pair_nodes, r->plan.pairs,
                             r->plan.max_depth, leaf, depth, h, st);
}

}  // namespace smk

extern "C" {

int smk_tree_router_check(int node_count, const unsigned* left, const unsigned* right, const int* valid, int* pairs, int* max_depth)
{
    RoutePlan plan;
    if (int rc = route_plan_or_error("smk_tree_router_check", node_count, left, right, valid, &plan)) return rc;
    if (pairs) *pairs = plan.pairs;
    if (max_depth) *max_depth = plan.max_depth;
    return SMK_OK;
}

int smk_tree_router_create(int64_t m, int node_count, const unsigned* left, const unsigned* right, const int* valid, const double* topics_host,
                           int64_t ld, smk_tree_router** router)
{
    const std::string w("smk_tree_router_create");
    if (!router) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    *router = nullptr;
    if (!left || !right || !topics_host) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (m < 1 || m > 0xFFFFFFFFll || ld < m) { set_error(w + ": m < 1, m beyond 32-bit row indices, or ld < m"); return SMK_BAD_PARAM; }
    RoutePlan plan;
    if (int rc = route_plan_or_error(w, node_count, left, right, valid, &plan)) return rc;
    if (int rc = require_init()) return rc;
    smk_tree_router* r = new smk_tree_router;
    r->m = m;
    r->node_count = node_count;
    r->plan = std::move(plan);
    r->left.assign(left, left + node_count);
    r->right.assign(right, right + node_count);
    r->valid.assign((size_t)node_count, 1);
    if (valid) r->valid.assign(valid, valid + node_count);
    r->topics.resize((size_t)m * node_count);
    for (int q = 0; q < node_count; ++q) std::copy(topics_host + (size_t)q * ld, topics_host + (size_t)q * ld + m, r->topics.begin() + (size_t)q * m);
    const int rc = router_pack(r, w);
    if (rc) { delete r; return rc; }
    *router = r;
    return SMK_OK;
}

int smk_tree_router_from_tree(const smk_tree* t, smk_tree_router** router)
{
    const std::string w("smk_tree_router_from_tree");
    if (!router) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    *router = nullptr;
    if (!t) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    const int nc = smk_tree_node_count(t);
    const i64 m = smk_tree_term_count(t);
    if (nc < 2 || m < 1) { set_error(w + ": the tree has no nodes"); return SMK_BAD_PARAM; }
    std::vector<unsigned> left((size_t)nc), right((size_t)nc);
    std::vector<int> valid((size_t)nc);
    std::vector<double> topics((size_t)m * nc);
    for (int q = 0; q < nc; ++q) {
        smk_tree_node nd;
        int rc = smk_tree_get_node(t, q, &nd);
        if (!rc) rc = smk_tree_node_topic(t, q, topics.data() + (size_t)q * m);
        if (rc) { set_error(w + ": node " + std::to_string(q) + " cannot be read"); return rc; }
        left[(size_t)q] = nd.left_child;
        right[(size_t)q] = nd.right_child;
        valid[(size_t)q] = nd.is_valid;
    }
    return smk_tree_router_create(m, nc, left.data(), right.data(), valid.data(), topics.data(), m, router);
}

void smk_tree_router_destroy(smk_tree_router* r) { delete r; }

int smk_tree_router_sizes(const smk_tree_router* r, int64_t* m, int* node_count, int* pairs, int* max_depth, int64_t* table_bytes)
{
    if (!r) return SMK_BAD_PARAM;
    if (m) *m = r->m;
    if (node_count) *node_count = r->node_count;
    if (pairs) *pairs = r->plan.pairs;
    if (max_depth) *max_depth = r->plan.max_depth;
    if (table_bytes) *table_bytes = r->table_bytes();
    return SMK_OK;
}

int smk_tree_router_download(const smk_tree_router* r, unsigned* left, unsigned* right, int* valid, double* topics_host, int64_t ld)
{
    if (!r || (topics_host && ld < r->m)) return SMK_BAD_PARAM;
    if (left) std::copy(r->left.begin(), r->left.end(), left);
    if (right) std::copy(r->right.begin(), r->right.end(), right);
    if (valid) std::copy(r->valid.begin(), r->valid.end(), valid);
    if (topics_host)
        for (int q = 0; q < r->node_count; ++q)
            std::copy(r->topics.begin() + (size_t)q * r->m, r->topics.begin() + (size_t)(q + 1) * r->m, topics_host + (size_t)q * ld);
    return SMK_OK;
}

int smk_tree_route_device(const smk_tree_router* r, const smk_matrix* a, void* stream, void* leaf, void* depth, void* h)
{
    const std::string w("smk_tree_route_device");
    int rc = route_args(w, r, a);
    if (rc) return rc;
    if (!leaf) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    // (leaves and depths are 32-bit integers: the extent of as many 4-byte elements)
    rc = check_device_view(leaf, DT_F32, a->n, 1, 1, a->n, true, (w + "(leaf)").c_str());
    if (!rc && depth) rc = check_device_view(depth, DT_F32, a->n, 1, 1, a->n, true, (w + "(depth)").c_str());
    if (!rc && h) rc = check_device_view(h, DT_F64, 2, a->n, 1, 2, true, (w + "(h)").c_str());
    if (rc) return rc;
    Entry e(matrix_stream(a));
    rc = e.join(stream);
    if (!rc) rc = route_launch(r, a, (int*)leaf, (int*)depth, (double*)h, e.st);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    g_route_launches = 1;
    g_route_entries = a->nnz;
    return SMK_OK;
}

int smk_tree_route_last_profile(int* launches, int64_t* entries)
{
    if (launches) *launches = g_route_launches;
    if (entries) *entries = g_route_entries;
    return SMK_OK;
}

int smk_tree_route_time(const smk_tree_router* r, const smk_matrix* a, int reps, double* ms)
{
    const std::string w("smk_tree_route_time");
    int rc = route_args(w, r, a);
    if (rc) return rc;
    if (!ms || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    Entry e(matrix_stream(a));
    int *leaf = nullptr, *depth = nullptr;
    double* h = nullptr;
    if (e.own.dev(&leaf, (size_t)a->n) || e.own.dev(&depth, (size_t)a->n) || e.own.dev(&h, (size_t)a->n * 2)) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    return e.synced(time_launches(w, e.own, e.st, reps, [&]() -> int { return route_launch(r, a, leaf, depth, h, e.st); }, ms));
}

}  // extern "C"

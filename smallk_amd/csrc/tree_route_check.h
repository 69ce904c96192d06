// smallk_amd/csrc/tree_route_check.h -- the structure check of a tree router (tree_route.cpp): is (left, right,
// valid) the forest HierNMF2 leaves behind -- roots 0 and 1, every reachable node a leaf or a split with two valid children,
// every node reached once -- and, if so, its pairs and its longest descent.  Host code without HIP and without the library's
// state: tests/tree_route/check_sim.cpp compiles it by itself under the sanitizers.
#pragma once
#include <string>
#include <vector>

namespace smk {

constexpr unsigned ROUTE_NONE = 0xFFFFFFFFu;      // SMK_TREE_NONE

// What the descent reads.  Pair 0 is the root pair (0, 1); every split adds the pair of its children, numbered in the order in
// which a breadth-first walk from the roots meets the splits.
struct RoutePlan {
    int pairs = 0, max_depth = 0;            // splits + the root pair; decisions on the longest descent
    std::vector<int> pair_nodes;             // [2 p], [2 p + 1]: the left and the right node of pair p
    std::vector<int> child_pair;             // per node: the pair of its children, -1 for a leaf (and for a node never reached)
};

// 0, or -1 with *err naming the node.  valid may be null: every node counts as valid.  Nodes that are invalid or cannot be
// reached from the roots are ignored, whatever their links hold.
inline int tree_route_plan(int node_count, const unsigned* left, const unsigned* right, const int* valid, RoutePlan* out, std::string* err)
{
    auto fail = [&](const std::string& what, long long q) { *err = what + " (node " + std::to_string(q) + ")"; return -1; };
    if (node_count < 2) { *err = "a tree has at least the two root nodes"; return -1; }
    if (!left || !right) { *err = "null argument"; return -1; }
    auto is_valid = [&](unsigned q) { return !valid || valid[q] != 0; };
    for (unsigned q = 0; q < 2; ++q)
        if (!is_valid(q)) return fail("a root is missing", q);
    RoutePlan p;
    p.child_pair.assign((size_t)node_count, -1);
    p.pair_nodes = {0, 1};
    p.pairs = 1;
    std::vector<int> depth((size_t)node_count, 0);       // decisions taken on arrival; 0 = not reached
    std::vector<unsigned> queue = {0u, 1u};
    depth[0] = depth[1] = 1;
    for (size_t at = 0; at < queue.size(); ++at) {
        const unsigned q = queue[at];
        if (depth[q] > p.max_depth) p.max_depth = depth[q];
        const unsigned l = left[q], r = right[q];
        if (l == ROUTE_NONE && r == ROUTE_NONE) continue;      // a leaf
        if (l == ROUTE_NONE || r == ROUTE_NONE) return fail("a node has one child", q);
        if (l >= (unsigned)node_count || r >= (unsigned)node_count) return fail("a child index is not below node_count", q);
        if (!is_valid(l) || !is_valid(r)) return fail("a child is not a valid node", q);
        if (l == r) return fail("both children of a node are the same node", q);
        for (unsigned c : {l, r}) {
            if (depth[c]) return fail("a node is reached twice (two parents, or a cycle)", c);
            depth[c] = depth[q] + 1;
            queue.push_back(c);
        }
        p.child_pair[q] = p.pairs++;
        p.pair_nodes.push_back((int)l);
        p.pair_nodes.push_back((int)r);
    }
    *out = std::move(p);
    return 0;
}

}  // namespace smk

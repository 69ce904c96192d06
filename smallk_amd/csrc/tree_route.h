// smallk_amd/csrc/tree_route.h -- the launchers of tree_route.hip: documents down a HierNMF2 tree.  All asynchronous
// on `st`.  T: per pair p and term the two sibling topic vectors interleaved (T[(p m + row) 2 ..]); gram: 3 doubles per pair; solve:
// tree_route_solve_bytes() per pair, written by launch_tree_route_prepare (r2_prepare of the Gram triple, side 0) together with
// bad[p], its "singular matrix" flag.  launch_tree_route: per column j of the CSC (m rows, n columns) leaf[j] = the node it ends at,
// depth[j] = decisions taken (<= max_depth), h[2 j ..] = (h0, h1) of the last one; depth and h may be null.  child_pair: per node the
// pair of its children or -1; pair_nodes: 2 nodes per pair.
#pragma once
#include "common.h"

namespace smk {

size_t tree_route_solve_bytes();
int launch_tree_route_prepare(const double* gram, int pairs, void* solve, int* bad, hipStream_t st);
int launch_tree_route(const i64* colptr, const unsigned* rowidx, const double* val, i64 n, i64 m, const double* T, const void* solve,
                      const int* child_pair, const int* pair_nodes, int pairs, int max_depth, int* leaf, int* depth, double* h, hipStream_t st);

}  // namespace smk

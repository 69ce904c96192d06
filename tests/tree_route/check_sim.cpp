// tests/tree_route/check_sim.cpp -- the tree router's structure check (smallk_amd/csrc/tree_route_check.h) by itself: the header
// compiles without HIP and without the library, so test_tree_route_cpu.py builds this program with AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it directly.  Input, one structure per line: node_count, then left right valid per node
// (4294967295 = none).  Output per line: "ok <pairs> <max_depth> <pair_nodes ...> | <child_pair ...>" or "bad <message>".
#include "../../smallk_amd/csrc/tree_route_check.h"

#include <cstdio>
#include <iostream>
#include <sstream>

int main()
{
    std::string line;
    int done = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int count = 0;
        in >> count;
        std::vector<unsigned> left, right;
        std::vector<int> valid;
        for (int q = 0; q < count; ++q) {
            unsigned l = 0, r = 0;
            int v = 0;
            in >> l >> r >> v;
            left.push_back(l); right.push_back(r); valid.push_back(v);
        }
        if (!in) { std::printf("check_sim: cannot read line %d\n", done + 1); return 2; }
        smk::RoutePlan plan;
        std::string err;
        if (smk::tree_route_plan(count, left.data(), right.data(), valid.data(), &plan, &err)) {
            std::printf("bad %s\n", err.c_str());
        } else {
            std::printf("ok %d %d", plan.pairs, plan.max_depth);
            for (int v : plan.pair_nodes) std::printf(" %d", v);
            std::printf(" |");
            for (int v : plan.child_pair) std::printf(" %d", v);
            std::printf("\n");
        }
        ++done;
    }
    std::printf("check_sim: done %d\n", done);
    return 0;
}

// tests/check_ring/ring_sim.cpp -- drives the schedule of the stopping-rule check (smallk_amd/csrc/check_ring.h, included by itself)
// with scripted metrics and scripted failures and prints one line per operation.  tests/test_check_ring_cpu.py builds it with
// AddressSanitizer + UndefinedBehaviorSanitizer, feeds it the cases and checks the lines.
//
// One case per input line:  depth sync every base min_iter max_iter tolcount tol fail_at fail_code n m_0 ... m_{n-1}
// (m_i: the metric of iteration i, "nan" allowed; fail_at: the iteration whose `end` returns fail_code, -1 = none).
// Output per case: "case", then "step i snap" / "begin i slot snapshot" / "end i slot" / "restore i slot" / "say <text>" in
// the order the driver issued them, then "result code iterations".
#include "../../smallk_amd/csrc/check_ring.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main()
{
    std::string text;
    long cases = 0;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        smk::check_ring::Params p;
        int fail_at = -1, fail_code = 0, n = 0;
        in >> p.depth >> p.sync >> p.every >> p.base >> p.min_iter >> p.max_iter >> p.tolcount >> p.tol >> fail_at >> fail_code >> n;
        std::vector<double> metric((size_t)n);
        for (double& m : metric) {
            std::string word;
            in >> word;
            m = word == "nan" ? std::nan("") : std::atof(word.c_str());
        }
        if (!in) { fprintf(stderr, "ring_sim: bad case line: %s\n", text.c_str()); return 2; }
        p.verbose = true;
        printf("case\n");
        const smk::check_ring::Result r = smk::check_ring::drive(p,
            [](int i, int snap) { printf("step %d %d\n", i, snap); return 0; },
            [](int i, int slot, bool snapshot) { printf("begin %d %d %d\n", i, slot, snapshot ? 1 : 0); return 0; },
            [&](int i, int slot, double* m) {
                printf("end %d %d\n", i, slot);
                if (i - p.base == fail_at) return fail_code;
                *m = metric.at((size_t)(i - p.base));
                return 0;
            },
            [](int i, int slot) { printf("restore %d %d\n", i, slot); return 0; },
            [](const char* line) {
                std::string esc;
                for (const char* c = line; *c; ++c) esc += *c == '\n' ? "\\n" : *c == '\t' ? "\\t" : std::string(1, *c);
                printf("say %s\n", esc.c_str());
            });
        printf("result %d %d\n", r.code, r.iterations);
        ++cases;
    }
    printf("ring_sim: done %ld\n", cases);
    return 0;
}

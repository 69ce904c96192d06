"""The environment switches of the library (smallk_amd/csrc/switches.h): one table, read through one place.

Two checks, both on the CPU.

Hygiene: no getenv under smallk_amd/csrc outside the table (OMP_NUM_THREADS in preprocess.cpp is not a project switch); every
name of the table is documented in tools/README.md; every SMK_* / SMALLK_* name a test sets exists in the table -- a typo in a
test would otherwise silently test the default path.

Parse parity: a few lines of C++ print every accessor of the table, compiled with the host compiler of tests/asan (no
sanitizers), run with each variable unset and set to a handful of texts.  EXPECTED below was written from the expressions
that stood at the read sites before the table existed (the parent of the commit that added switches.h), not from the table: it is the
check that no switch changed its parse, its default or the time it is read.  Thresholds that sit at the sites -- the guard
runs for SMK_GUARD_EVERY > 0, the priority laps print for SMK_CLUST_TIMING > 1 -- stay there; the accessor hands out the number."""
import ast
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallk_amd", "csrc")

# the texts every variable is set to; None: unset
TEXTS = (None, "", "0", "1", "2", "-1", "multi", "h")
U64_MAX = 18446744073709551615

# what the seven conventions of the old read sites give for TEXTS
ON_UNLESS_0 = (1, 1, 0, 1, 1, 1, 1, 1)              # !(e && e[0] == '0')
ON_IF_NONZERO = (0, 0, 0, 1, 1, 1, 0, 0)            # e && atoi(e) != 0
FIRST_IS_1 = (0, 0, 0, 1, 0, 0, 0, 0)               # e && e[0] == '1'
FIRST_IS_M = (0, 0, 0, 0, 0, 0, 1, 0)               # e && e[0] == 'm'
FIRST_IS_H = (0, 0, 0, 0, 0, 0, 0, 1)               # e && e[0] == 'h'
INT_IF_SET = ("unset", 0, 0, 1, 2, -1, 0, 0)        # if (e) x = atoi(e), or a test of e itself
U64_IF_SET = ("unset", 0, 0, 1, 2, U64_MAX, 0, 0)   # if (e) x = strtoull(e, nullptr, 10)


def NUM(unset):                                     # e ? atoi(e) / atoll(e) / atof(e) : unset
    return (unset, 0, 0, 1, 2, -1, 0, 0)


ONCE, LIVE = "ONCE", "LIVE"     # static const ... = [] {...}() at the old site / a plain read on every call

# environment name -> [(accessor, read time, values for TEXTS)]
EXPECTED = {
    "SMK_NSPLIT": [("nsplit", LIVE, INT_IF_SET)],
    "SMK_BPP_SMALL_ACCURATE": [("bpp_small_accurate", LIVE, ON_UNLESS_0)],
    "SMK_BP_VARIANT": [("bp_variant", LIVE, INT_IF_SET)],
    "SMK_BP_VARIANT_K64": [("bp_variant_k64", LIVE, INT_IF_SET)],
    "SMK_BP_SPLITS": [("bp_splits", LIVE, NUM(0))],                  # envS && atoi(envS) > 0
    "SMK_BP_TR_VARIANT": [("bp_tr_variant", ONCE, NUM(-1))],
    "SMK_BP_TEMPORAL": [("bp_temporal", ONCE, NUM(-1))],
    "SMK_LD_SKEW": [("ld_skew", ONCE, INT_IF_SET)],                  # e ? atoll(e) / ROW_PAD * ROW_PAD : ROW_PAD
    "SMK_SINGLE_COPY": [("single_copy", LIVE, FIRST_IS_1)],
    "SMK_GUARD_EVERY": [("guard_every", ONCE, NUM(0))],              # -1: no guard at either site (> 0, <= 0)
    "SMK_GUARD_TAU": [("guard_tau", ONCE, NUM(1e-4))],
    "SMK_GUARD_VERBOSE": [("guard_verbose", ONCE, ON_IF_NONZERO)],
    "SMK_FUSED_GRAM": [("fused_gram", ONCE, ON_UNLESS_0)],
    "SMK_REDUCE_PACK": [("reduce_pack", ONCE, ON_UNLESS_0)],
    "SMK_NNLS_GRAM": [("nnls_gram", ONCE, ON_UNLESS_0)],
    "SMK_NNLS_PACK": [("nnls_pack", LIVE, ON_UNLESS_0)],
    "SMK_GRAM_RIDE": [("gram_ride", ONCE, ON_UNLESS_0)],
    "SMK_INV_RIDE": [("inv_ride", ONCE, ON_UNLESS_0)],
    "SMK_INV_STREAM": [("inv_stream", ONCE, NUM(-1))],
    "SMK_NNLS_INV": [("nnls_inv", ONCE, NUM(1))],
    "SMK_NNLS_INV32": [("nnls_inv32", ONCE, ON_UNLESS_0)],
    "SMK_NNLS_ROUNDS": [("nnls_rounds", ONCE, NUM(0))],
    "SMK_NNLS_G16": [("nnls_g16", ONCE, NUM(1))],
    "SMK_WIDE_NW": [("wide_nw", ONCE, NUM(0))],
    "SMK_NNLS_STATS": [("nnls_stats", ONCE, ON_IF_NONZERO)],
    "SMK_BPP_GRADW": [("bpp_gradw", ONCE, FIRST_IS_1)],              # true = the W-side gradient is formed; "2": not formed
    "SMK_HALS_EPILOGUE": [("hals_epilogue", ONCE, ON_UNLESS_0)],
    "SMK_HALS_W_BLOCKED": [("hals_w_blocked", ONCE, ON_UNLESS_0)],
    "SMK_HALS_W": [("hals_w_multi", ONCE, FIRST_IS_M)],
    "SMK_HALS_SPIN": [("hals_spin", ONCE, NUM(0))],                  # honoured when atoi > 0
    "SMK_HALS_NT": [("hals_nt", ONCE, NUM(256))],
    "SMK_SYNC_PROGRESS": [("sync_progress", ONCE, ON_IF_NONZERO)],
    "SMK_PROGRESS_FUSED": [("progress_fused", ONCE, ON_UNLESS_0)],
    "SMK_PROGRESS_DEFER": [("progress_defer", ONCE, ON_UNLESS_0)],
    "SMK_PROGRESS_TAIL": [("progress_tail", ONCE, ON_UNLESS_0)],
    "SMK_PROGRESS_POLL": [("progress_poll", ONCE, ON_UNLESS_0)],
    "SMK_PROGRESS_DEPTH": [("progress_depth", ONCE, NUM(0))],
    "SMK_TIMING_STRIDE": [("timing_stride", LIVE, INT_IF_SET)],
    "SMK_SPMM_SEG": [("spmm_seg", ONCE, ON_UNLESS_0)],
    "SMK_SPMM_SEG_LEN": [("spmm_seg_len", ONCE, NUM(64))],           # clamped to 8 .. 4096 by spmm_seg_len()
    "SMK_SPMM_SEG_U": [("spmm_seg_u", ONCE, NUM(0))],
    "SMK_SPMM2_LPC": [("spmm2_lpc", ONCE, NUM(0))],
    "SMK_SPMM_BLOCKS": [("spmm_blocks", ONCE, NUM(0))],
    "SMK_SPMM_BLOCKED_LPC": [("spmm_blocked_lpc", ONCE, NUM(0))],
    "SMK_SPMM_UNROLL": [("spmm_unroll", ONCE, NUM(1))],
    "SMK_TRANSPOSE": [("transpose_host", ONCE, FIRST_IS_H)],
    "SMK_SPARSE_SUBSET": [("sparse_subset_host", ONCE, FIRST_IS_H)],
    "SMK_R2_PERSIST": [("r2_persist", ONCE, NUM(1))],
    "SMK_R2_PERSIST_NNZ": [("r2_persist_nnz", ONCE, NUM(1 << 40))],
    "SMK_R2P_WGS": [("r2p_wgs", ONCE, NUM(0))],
    "SMK_R2P_LDS": [("r2p_lds", ONCE, NUM(1))],                      # e && atoi(e) == 0: the small layout ("" too)
    "SMK_R2P_PROFILE": [("r2p_profile", ONCE, ON_IF_NONZERO)],
    "SMK_NUM_GPUS": [("num_gpus", LIVE, NUM(0))],                    # !e || atoi(e) <= 1: one device
    "SMK_SHARDS_ON_ONE_GPU": [("shards_on_one_gpu", LIVE, ON_IF_NONZERO)],
    "SMK_COMM_FORCE": [("comm_force", LIVE, ON_IF_NONZERO)],
    "SMK_COMM_CHUNKS": [("comm_chunks", LIVE, INT_IF_SET)],
    "SMK_COMM_F64": [("comm_f64", LIVE, NUM(1))],                    # !(e && atoi(e) == 0): "" is fp32 on the wire
    "SMK_COMM_EMULATE_WORLD": [("comm_emulate_world", LIVE, NUM(0))],    # honoured for 2 .. 64
    "SMK_CLUST_DEVICES": [("clust_devices", LIVE, NUM(0))],          # !e || atoi(e) < 2: one device
    "SMK_CLUST_SERIALIZE": [("clust_serialize", ONCE, ON_IF_NONZERO)],
    "SMK_CLUST_TIMING": [("clust_timing", ONCE, NUM(0)), ("clust_timing_live", LIVE, NUM(0))],
    "SMK_PRIORITY_HOST": [("priority_host", ONCE, ON_IF_NONZERO)],
    "SMK_POISON": [("poison", ONCE, ON_IF_NONZERO)],
    "SMK_DEVMEM_CACHE": [("devmem_cache", ONCE, NUM(1))],            # !(e && atoi(e) == 0)
    "SMK_DEVMEM_CACHE_MB": [("devmem_cache_mb", ONCE, NUM(4096))],   # e ? atoll(e) << 20 : 4 << 30
    "SMALLK_SEED": [("seed", LIVE, U64_IF_SET)],
    "SMK_NNLS_PACK_TEST_ANORM": [("nnls_pack_test_anorm", LIVE, NUM(1.0))],      # if (e) anorm *= atof(e)
    "SMK_R2P_TEST_ABORT": [("r2p_test_abort", LIVE, ON_IF_NONZERO)],
}

# SMK_* names that only Python reads (bench.py, tools/, tests/ref_results.py): not switches of the library
PYTHON_ONLY = {
    "SMK_BENCH_BACKEND", "SMK_BENCH_DUMP_W", "SMK_BENCH_HEARTBEAT", "SMK_BENCH_NO_RANK_WATCHDOG", "SMK_BENCH_RCCL_LOG_GLOB",
    "SMK_BENCH_RCCL_TUNING", "SMK_BENCH_SHARE_GPU", "SMK_BENCH_TEST_HANG", "SMK_BENCH_VERBOSE", "SMK_FUZZ_ONLY", "SMK_LEG",
    "SMK_LEG_BPP_ONLY", "SMK_LIB_PATH", "SMK_LONG_AT", "SMK_LONG_CASE", "SMK_REF_RECORD", "SMK_TOOL_ALG",
}


def table_rows():
    """(accessor, environment name, read time) of every row of switches.h"""
    text = open(os.path.join(CSRC, "switches.h")).read()
    return [(m.group(2), m.group(3), m.group(1)) for m in re.finditer(r'^SMK_SW_(ONCE|LIVE)\((\w+),\s*"(\w+)",', text, re.M)]


def names_set_by_tests():
    """SMK_* / SMALLK_* names that tests/*.py put into an environment: keyword arguments (dict(os.environ, SMK_X="1")),
    keys of dict literals, and the name given to setenv / delenv / setdefault / pop / get"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.basename(path) == os.path.basename(__file__):
            continue
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = []
            if isinstance(node, ast.Call):
                names += [kw.arg for kw in node.keywords if kw.arg]
                if isinstance(node.func, ast.Attribute) and node.func.attr in ("setenv", "delenv", "setdefault", "pop", "get") and node.args:
                    names += [node.args[0].value] if isinstance(node.args[0], ast.Constant) else []
            elif isinstance(node, ast.Dict):
                names += [k.value for k in node.keys if isinstance(k, ast.Constant)]
            elif isinstance(node, ast.Subscript) and isinstance(node.slice, ast.Constant):
                names += [node.slice.value]
            for n in names:
                if isinstance(n, str) and re.fullmatch(r"(SMK|SMALLK)_[A-Z0-9_]+", n):
                    found.setdefault(n, os.path.basename(path))
    return found


def test_switches_are_read_through_the_table_and_documented():
    rows = table_rows()
    assert sorted(set(r[1] for r in rows)) == sorted(EXPECTED)
    # 1. no getenv outside the table
    stray = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) == "switches.h" or not os.path.isfile(path):
            continue
        for i, line in enumerate(open(path, errors="replace"), 1):
            if "getenv(" in line and not (os.path.basename(path) == "preprocess.cpp" and '"OMP_NUM_THREADS"' in line):
                stray.append("%s:%d" % (os.path.basename(path), i))
    assert not stray, stray
    omp = [l for l in open(os.path.join(CSRC, "preprocess.cpp")) if "getenv(" in l]
    assert len(omp) == 1, omp
    # one accessor per name; SMK_CLUST_TIMING is the one variable read both ways
    accessors = [r[0] for r in rows]
    assert len(set(accessors)) == len(accessors)
    envs = [r[1] for r in rows]
    assert sorted(e for e in set(envs) if envs.count(e) > 1) == ["SMK_CLUST_TIMING"]
    # 2. every name is documented
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    missing = [e for e in sorted(set(envs)) if not re.search(r"\b%s\b" % e, readme)]
    assert not missing, missing
    # 3. every name a test sets exists
    used = names_set_by_tests()
    assert len(used) >= 40, sorted(used)           # the scan itself works
    unknown = {n: f for n, f in used.items() if n not in set(envs) and n not in PYTHON_ONLY}
    assert not unknown, unknown


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    """a program that prints every accessor twice: as the environment stands, and after the environment was cleared"""
    d = tmp_path_factory.mktemp("switches")
    lines = ['    std::cout << tag << " %s " << smk::sw::%s() << "\\n";' % (fn, fn) for fn, _, _ in table_rows()]
    src = ('#include "switches.h"\n#include <iostream>\n'
           "namespace smk { namespace sw {\n"
           "template <typename T> std::ostream& operator<<(std::ostream& o, const Maybe<T>& m) { return m.set ? o << m.v : o << \"unset\"; }\n"
           "}}\n"
           "static void dump(const char* tag)\n{\n    std::cout.precision(17);\n" + "\n".join(lines) + "\n}\n"
           'int main() { dump("first"); clearenv(); dump("second"); return 0; }\n')
    (d / "dump_switches.cpp").write_text(src)
    mk = open(os.path.join(ROOT, "tests", "asan", "Makefile")).read()
    cxx = os.environ.get("CXX") or re.search(r"^CXX\s*\?=\s*(\S+)", mk, re.M).group(1)
    exe = str(d / "dump_switches")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(d / "dump_switches.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_dumper(exe, env):
    base = {k: v for k, v in os.environ.items() if not re.match(r"(SMK|SMALLK)_", k)}
    r = subprocess.run([exe], env=dict(base, **env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {"first": {}, "second": {}}
    for line in r.stdout.splitlines():
        tag, fn, val = line.split()
        out[tag][fn] = val if val == "unset" else float(val) if re.search(r"[.e]", val) else int(val)
    return out["first"], out["second"]


def test_every_switch_parses_as_its_old_read_site_did(dumper):
    rows = table_rows()
    assert sorted((fn, env, rd) for fn, env, rd in rows) == sorted((fn, env, rd) for env, accs in EXPECTED.items() for fn, rd, _ in accs)
    unset = {fn: vals[0] for accs in EXPECTED.values() for fn, _, vals in accs}
    read = {fn: rd for accs in EXPECTED.values() for fn, rd, _ in accs}
    first, second = run_dumper(dumper, {})
    assert first == unset and second == unset
    bad = []
    for env, accs in EXPECTED.items():
        for i, text in enumerate(TEXTS):
            if text is None:
                continue
            first, second = run_dumper(dumper, {env: text})
            want = dict(unset, **{fn: vals[i] for fn, _, vals in accs})
            # a latched switch keeps its value when the environment changes under it, a live one follows
            want_after = {fn: (want[fn] if read[fn] == ONCE else unset[fn]) for fn in want}
            for fn in want:
                if first[fn] != want[fn]:
                    bad.append("%s=%r: %s() gives %r, the old site gave %r" % (env, text, fn, first[fn], want[fn]))
                if second[fn] != want_after[fn]:
                    bad.append("%s=%r then cleared: %s() (%s) gives %r, expected %r" % (env, text, fn, read[fn], second[fn], want_after[fn]))
    assert not bad, "\n".join(bad[:40])

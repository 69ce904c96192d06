"""The planning facts of the streaming products (smallk_amd/csrc/bigprod_plan.h: the variant tables, the fit rule, the variant a plan
settles on, the launches that carry the riders, the product form of a solver) against restatements that do not come from the header:
tests/entrywise.py, the number lists that stood in bigprod.hip before the tables existed, and the form rule written out below.
tests/bigprod_plan/plan_dump.cpp includes the header by itself and prints every record; it is built with AddressSanitizer +
UndefinedBehaviorSanitizer and run directly."""
import itertools
import os
import subprocess

import pytest

import entrywise as ew

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
STORAGE = {0: "f32", 1: "bf16"}
WANTS = [None, -1] + list(range(31)) + [99] + list(range(100, 132)) + [200]

# the fp32-storage rows: variant -> (kernel, wps / pin, bf16 forms, fp16 form, tail), copied from the table of the issue that asked
# for the header
F3_COLUMNS = {100: ("f3", 2, 1, 0, 0), 101: ("f3", 2, 1, 0, 0), 102: ("f3", 2, 1, 0, 0), 103: ("f3", 2, 1, 0, 0), 104: ("f3", 3, 1, 0, 0),
              105: ("f3", 2, 1, 0, 0), 106: ("f3", 2, 1, 0, 0), 107: ("f3", 2, 1, 0, 0), 108: ("f3", 2, 1, 1, 1), 109: ("f3", 2, 1, 0, 0),
              110: ("f3p", 1, 1, 1, 0), 111: ("f3p", 1, 1, 1, 0), 112: ("f3p", 1, 1, 0, 0), 113: ("f3p", 1, 1, 0, 0), 114: ("f3p", 1, 1, 0, 0),
              115: ("f3p", 1, 1, 1, 0), 116: ("f3p", 1, 1, 0, 0), 117: ("f3p", 0, 1, 0, 0), 118: ("f3p", 2, 1, 0, 0), 119: ("f3p", 4, 1, 0, 0),
              120: ("f3p", 6, 1, 0, 0), 121: ("f3p", 9, 1, 0, 0), 122: ("f3p", 8, 1, 0, 0), 123: ("f3p", 16, 1, 0, 0), 124: ("f3p", 22, 1, 0, 0),
              125: ("f3", 2, 1, 1, 1), 126: ("f3", 2, 1, 1, 0), 127: ("f3", 2, 1, 1, 0), 128: ("f3", 2, 0, 1, 1), 129: ("f3", 2, 0, 1, 1)}


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """the program's lines, grouped by their first word"""
    exe = tmp_path_factory.mktemp("bigprod_plan") / "plan_dump"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "bigprod_plan", "plan_dump.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    text = r.stdout[-2000:] + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert r.returncode == 0 and r.stdout.endswith("plan_dump: done\n"), text[-3000:]
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        word, _, rest = line.partition(" ")
        out.setdefault(word, []).append(rest.split())
    return out


def ints(fields):
    return [int(f) for f in fields]


def test_tables(records):
    assert [tuple(ints(r)) for r in records["bp"]] == [(i,) + row for i, row in enumerate(ew.KVARIANTS)]
    rows = records["f3"]
    assert [int(r[0]) for r in rows] == list(range(100, 100 + len(ew.F3VARIANTS))) == sorted(F3_COLUMNS)
    for v, kernel, mb, nstage, nwl, fold, arg, bf, f16, tail in rows:
        assert (int(mb), int(nstage), int(nwl), int(fold)) == ew.F3VARIANTS[int(v) - 100], v
        assert (kernel, int(arg), int(bf), int(f16), int(tail)) == F3_COLUMNS[int(v)], v
    assert tuple(v for v in sorted(F3_COLUMNS) if F3_COLUMNS[v][3]) == ew.F16_VARIANTS


def test_fit_functions(records):
    assert len(records["bpfits"]) == len(ew.KVARIANTS) * 2 * 2 * 4 and len(records["f3fits"]) == len(ew.F3VARIANTS) * 2 * 3
    for i, ebytes, kt, nsplit, fits in map(ints, records["bpfits"]):
        assert bool(fits) == ew.bp_fits(ebytes, kt, nsplit, *ew.KVARIANTS[i]), (i, ebytes, kt, nsplit)
    for v, kt, form, fits in map(ints, records["f3fits"]):
        assert bool(fits) == ew.f3_fits(v, kt, form), (v, kt, form)
    assert any(int(r[-1]) for r in records["f3fits"]) and not all(int(r[-1]) for r in records["f3fits"])


def test_choose_variant(records):
    assert [None if w == "unset" else int(w) for w in records["wants"][0]] == WANTS
    grid = set()
    for rec in records["variant"]:
        storage, k, length, form = ints(rec[:4])
        got = ints(rec[4:])
        want = [ew.planned_variant(STORAGE[storage], k, length, form, w, w64) for w in WANTS for w64 in WANTS]
        if got != want:
            bad = next(i for i in range(len(want)) if got[i] != want[i])
            pytest.fail("storage %s k %d len %d form %d want %s want_k64 %s: %d, restated %d"
                        % (STORAGE[storage], k, length, form, WANTS[bad // len(WANTS)], WANTS[bad % len(WANTS)], got[bad], want[bad]))
        grid.add((storage, k, length, form))
    lens = (1, 4095, 4096, 16383, 16384, 65535, 65536)
    assert grid == set(itertools.product((0, 1), (1, 16, 17, 32, 33, 64), lens, (1, 2, 3, 4, 8)))
    assert len(records["variant_tr"]) == 2 * 6 * len(lens)
    for storage, k, length, v in map(ints, records["variant_tr"]):
        assert v == ew.planned_variant_transposed(STORAGE[storage], k, length), (storage, k, length)


def test_chain_length(records):
    assert len(records["chain"]) == 2 * (len(ew.KVARIANTS) + len(ew.F3VARIANTS) + 1) * 2
    for storage, v, tr, rows in map(ints, records["chain"]):
        assert rows == ew.chain_rows(STORAGE[storage], None, v, transposed=bool(tr)), (storage, v, tr)
    assert [ints(r) for r in records["chain_unknown"]] == [[v, 0, 0] for v in (-1, 24, 99, 130, 199)]      # no kernel, no chain


def test_riders(records):
    """the number lists of bigprod_supports_ride / bigprod_supports_tail as they stood before the tables"""
    def rides(storage, nsplit, v, tr):
        if nsplit == 8:
            return not tr
        if tr:
            return False
        if STORAGE[storage] == "bf16" or v < 100:
            return True
        i = v - 100
        if nsplit == 4:
            return i == 8 or 25 <= i <= 29
        return nsplit in (2, 3) and (0 <= i <= 9 or 25 <= i <= 27)

    assert len(records["ride"]) == len(records["tail"]) == 2 * 5 * (len(ew.KVARIANTS) + len(ew.F3VARIANTS) + 5) * 2
    for storage, nsplit, v, tr, got in map(ints, records["ride"]):
        assert bool(got) == rides(storage, nsplit, v, tr), (storage, nsplit, v, tr)
    for storage, nsplit, kt, v, got in map(ints, records["tail"]):
        assert bool(got) == (nsplit == 4 and STORAGE[storage] == "f32" and kt == 1 and v in (108, 125, 128, 129)), (storage, nsplit, kt, v)


MU, HALS, RANK2, BPP = 0, 1, 2, 3           # SMK_ALG_* of include/smallk_amd.h


def default_form(alg, k, storage, sparse, entries, spread, small_accurate, nsplit):
    form = 4 if storage == "f32" and alg != HALS and k <= 64 else 3
    if alg == HALS and not sparse and k > 64:
        form = 8
    if alg == BPP and not sparse and k > 64:
        form = 8
    if alg == BPP and not sparse and k > 32 and entries <= 2 ** 24 and small_accurate:
        form = 8
    if alg == RANK2 and not sparse:
        form = 8
    if spread > 28 and nsplit is None and not sparse and alg != RANK2:
        form = 8
    return form


def resolved_form(alg, k, storage, sparse, entries, spread, small_accurate, nsplit):
    default = default_form(alg, k, storage, sparse, entries, spread, small_accurate, nsplit)
    form = default if nsplit is None else nsplit
    if form != 8 and not 1 <= form <= 4:
        form = default
    if form == 8 and sparse:
        form = 3
    if form == 4 and not (storage == "f32" and not sparse and alg != RANK2):
        form = 3
    return form


def test_product_form(records):
    grid = set()
    for rec in records["form"]:
        alg, k, storage, sparse, entries, spread, small = ints(rec[:7])
        nsplit = None if rec[7] == "unset" else int(rec[7])
        args = (alg, k, STORAGE[storage], bool(sparse), entries, spread, bool(small), nsplit)
        assert int(rec[8]) == default_form(*args), args
        assert int(rec[9]) == resolved_form(*args), args
        if alg == MU and not sparse and spread <= 28 and nsplit in (None, 1, 2, 3, 4, 8):
            assert int(rec[9]) == ew.expected_form(STORAGE[storage], k, nsplit), args
        grid.add(args)
    assert grid == set(itertools.product((MU, HALS, RANK2, BPP), (2, 16, 32, 33, 64, 65, 200), ("f32", "bf16"), (False, True), (2 ** 24, 2 ** 24 + 1),
                                         (-1, 0, 28, 29), (False, True), (None, -1, 0, 1, 2, 3, 4, 5, 8, 9)))

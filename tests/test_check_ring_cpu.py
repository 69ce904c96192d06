"""The schedule of the stopping-rule check (smallk_amd/csrc/check_ring.h: which iteration is checked in which slot, when a check is
read, when a snapshot is promised, what is restored) against the plain check-every-iteration loop of the reference's NmfSolve<>
(common/include/nmf_solve_generic.hpp:67-139), restated below and not derived from the header.  tests/check_ring/ring_sim.cpp
includes the header by itself and prints one line per operation; it is built with AddressSanitizer + UndefinedBehaviorSanitizer
and run directly."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
TOL, HIT, MISS, FAIL = 0.5, 0.1, 1.0, 7
BASE = 5                        # the iterate_checked form: iterations already done on the handle


def plain_loop(min_iter, max_iter, tolcount, metrics, fail_at, reset_on_miss=True):
    """((code, iteration count), verbose lines) of the loop that reads every check before it goes on"""
    said, count = [], 0
    for i in range(max_iter):
        if i == 0 or i >= min_iter:                  # iteration 0 initialises the estimator
            if i == fail_at:
                return (FAIL, i), said
        if i < min_iter:
            said.append("%d:\\tprogress metric: \\t(min_iter)\\n" % (i + 1))
            continue
        if i + 1 < 10 or (i + 1) % 10 == 0:
            said.append("%d:\\tprogress metric:\\t%g\\n" % (i + 1, metrics[i]))
        if metrics[i] <= TOL:
            count += 1
            if count >= tolcount:
                said.append("\\nSolution converged after %d iterations.\\n\\n" % (i + 1))
                return (0, i), said
        elif reset_on_miss:
            count = 0
    return (0, max_iter), said


def scripts(max_iter, tolcount):
    """(family, metrics, fail_at): the rule never fires; hits from q on; hits, one miss, hits again; a failure or a NaN at p"""
    n = max_iter
    yield "never", [MISS] * n, -1
    for q in range(n):
        yield "from", [MISS] * q + [HIT] * (n - q), -1
        yield "reset", ([MISS] * q + [HIT] * max(tolcount - 1, 1) + [MISS] + [HIT] * n)[:n], -1
        yield "alternate", ([MISS] * q + [HIT, MISS] * n)[:n], -1
        yield "fail", [MISS] * n, q
        yield "fail_then_hits", [MISS] * q + [HIT] * (n - q), q
        yield "hits_then_fail", [HIT] * n, q
        yield "nan", ([MISS] * q + [float("nan")] + [HIT] * n)[:n], -1
        yield "hit_nan_hit", ([HIT] * q + [float("nan")] + [HIT] * n)[:n], -1


def case_line(depth, sync, every, base, min_iter, max_iter, tolcount, metrics, fail_at):
    words = [depth, int(sync), int(every), base, min_iter, max_iter, tolcount, TOL, fail_at, FAIL, len(metrics)]
    return " ".join(str(w) for w in words + ["nan" if m != m else repr(m) for m in metrics])


def all_cases():
    """(key, input line): the runs of smk_solver_run, then those of smk_solver_iterate_checked"""
    out = []
    for depth, sync, min_iter, max_iter, tolcount in itertools.product((1, 2, 3), (False, True), (1, 2, 5), range(1, 13), (1, 2, 3)):
        for j, (family, metrics, fail_at) in enumerate(scripts(max_iter, tolcount)):
            key = dict(depth=depth, sync=sync, every=False, base=0, min_iter=min_iter, max_iter=max_iter, tolcount=tolcount,
                       family=family, script=j, metrics=metrics, fail_at=fail_at)
            out.append((key, case_line(depth, sync, False, 0, min_iter, max_iter, tolcount, metrics, fail_at)))
    for depth, n in itertools.product((1, 2, 3), range(1, 10)):
        for fail_at in [-1] + list(range(n)):
            key = dict(depth=depth, sync=False, every=True, base=BASE, min_iter=0, max_iter=n, tolcount=1, family="every", script=fail_at,
                       metrics=[HIT] * n, fail_at=fail_at)
            out.append((key, case_line(depth, False, True, BASE, 0, n, 1, [HIT] * n, fail_at)))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """[(key, operations)]: what the program printed for every case"""
    exe = tmp_path_factory.mktemp("check_ring") / "ring_sim"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "check_ring", "ring_sim.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    cases = all_cases()
    r = subprocess.run([str(exe)], input="".join(line + "\n" for _, line in cases), capture_output=True, text=True, timeout=300, env=ENV)
    text = r.stdout[-2000:] + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert r.returncode == 0 and r.stdout.endswith("ring_sim: done %d\n" % len(cases)), text[-3000:]
    blocks = r.stdout.split("case\n")[1:]
    assert len(blocks) == len(cases)
    blocks[-1] = blocks[-1][:blocks[-1].rindex("ring_sim: done")]
    out = []
    for (key, _), block in zip(cases, blocks):
        ops = []
        for line in block.splitlines():
            word, _, rest = line.partition(" ")
            ops.append((word, rest) if word == "say" else (word,) + tuple(int(f) for f in rest.split()))
        assert ops and ops[-1][0] == "result" and all(o[0] in ("step", "begin", "end", "restore", "say") for o in ops[:-1]), (key, ops)
        out.append((key, ops))
    return out


def expected(key):
    if key["every"]:
        return ((FAIL, key["fail_at"]) if key["fail_at"] >= 0 else (0, key["max_iter"])), []
    return plain_loop(key["min_iter"], key["max_iter"], key["tolcount"], key["metrics"], key["fail_at"])


def test_the_enumeration_is_the_one_asked_for(runs):
    keys = [k for k, _ in runs]
    grid = set((k["depth"], k["sync"], k["min_iter"], k["max_iter"], k["tolcount"]) for k in keys if not k["every"])
    assert grid == set(itertools.product((1, 2, 3), (False, True), (1, 2, 5), range(1, 13), (1, 2, 3)))
    assert set(k["family"] for k in keys) >= {"never", "from", "reset", "fail", "nan", "every"}
    assert set((k["depth"], k["max_iter"]) for k in keys if k["every"]) == set(itertools.product((1, 2, 3), range(1, 10)))
    # the families do what their names say: some run converges at every iteration from min_iter on, and some run loses a count
    for min_iter, max_iter in itertools.product((1, 2, 5), range(1, 13)):
        fired = set(expected(k)[0][1] for k in keys if k["family"] == "from" and (k["min_iter"], k["max_iter"], k["tolcount"]) == (min_iter, max_iter, 1))
        assert fired >= set(range(min_iter, max_iter)), (min_iter, max_iter, fired)
    for tolcount in (2, 3):
        assert any(expected(k)[0] != plain_loop(k["min_iter"], k["max_iter"], tolcount, k["metrics"], -1, reset_on_miss=False)[0]
                   for k in keys if k["family"] == "reset" and k["tolcount"] == tolcount), "no script depends on the count being reset"


def test_result_is_that_of_the_plain_loop(runs):
    """(a): code and iteration count, in every mode and at every depth"""
    for key, ops in runs:
        assert ops[-1][1:] == expected(key)[0], key


def test_restore_exactly_when_something_ran_after_the_converged_iteration(runs):
    """(b), and the snapshot that is restored was asked for and is read right behind the check that fired"""
    seen = 0
    for key, ops in runs:
        (code, count), _ = expected(key)
        steps = [o[1] for o in ops if o[0] == "step"]
        restores = [o for o in ops if o[0] == "restore"]
        converged = code == 0 and count < key["max_iter"]             # the plain loop ended before its iterations were used up
        if converged and steps[-1] > count:
            slot = next(o[2] for o in ops if o[0] == "begin" and o[1] == count)
            assert restores == [("restore", count, slot)], key
            assert ("begin", count, slot, 1) in ops, key
            plain = [o for o in ops if o[0] != "say"]
            assert plain[plain.index(restores[0]) - 1] == ("end", count, slot), key
            seen += 1
        else:
            assert restores == [], key
        if key["sync"]:
            assert restores == [], key
    assert seen > 1000


def test_slots(runs):
    """(c): checks begun and not ended, and the slot handed to the step in progress, never share a slot; all below depth + 1;
    depth 1 is the `iter & 1` of the first rounds"""
    for key, ops in runs:
        depth, base = key["depth"], key["base"]
        flying, handed = {}, None           # iteration -> slot of the checks in flight; (iteration, slot) handed to the current step
        for o in ops[:-1]:
            if o[0] == "step":
                handed = (o[1], o[2]) if o[2] >= 0 else None
                assert o[2] < depth + 1 and o[2] not in flying.values(), (key, o)
                assert len(flying) <= (0 if key["sync"] else depth), (key, o)      # at most `depth` checks behind an iteration
                if o[2] >= 0 and depth == 1:
                    assert o[2] == (o[1] - base) & 1, (key, o)
            elif o[0] == "begin":
                assert 0 <= o[2] < depth + 1 and o[2] not in flying.values(), (key, o)
                assert handed is None or handed == (o[1], o[2]), (key, o)      # the slot the step wrote is the slot of its check
                assert o[1] not in flying, (key, o)
                if depth == 1:
                    assert o[2] == (o[1] - base) & 1, (key, o)
                flying[o[1]] = o[2]
                handed = None
            elif o[0] == "end":
                assert flying.pop(o[1], None) == o[2], (key, o)


def test_snapshots(runs):
    """(d): asked for exactly for the checked iterations from min_iter on in speculative mode, never in synchronous mode, for
    every iteration in the iterate_checked form -- from the step (which may write it) and from the check alike"""
    for key, ops in runs:
        base, min_iter = key["base"], key["min_iter"]
        begun = {}
        for o in ops[:-1]:
            want = key["every"] or (not key["sync"] and o[1] - base >= min_iter) if o[0] in ("step", "begin") else None
            if o[0] == "step":
                assert (o[2] >= 0) == want, (key, o)
            elif o[0] == "begin":
                assert bool(o[3]) == want, (key, o)
                begun[o[1]] = True
        # which iterations are checked: 0 and everything from min_iter on (all of them in the iterate_checked form)
        for i in (o[1] for o in ops if o[0] == "step"):
            assert (i in begun) == (key["every"] or i - base == 0 or i - base >= min_iter), (key, i)


def test_order(runs):
    """(e): checks end in iteration order, each at most once and only after it began; nothing is started after a failure; at
    most `depth` iterations follow the one that converged (none in synchronous mode); steps come in order, one each"""
    for key, ops in runs:
        code, count = ops[-1][1:]
        ends = [o[1] for o in ops if o[0] == "end"]
        assert ends == sorted(set(ends)), key
        for o in ops:
            if o[0] == "end":
                assert any(b[0] == "begin" and b[1] == o[1] for b in ops[:ops.index(o)]), (key, o)
        steps = [o[1] for o in ops if o[0] == "step"]
        assert steps == list(range(key["base"], key["base"] + len(steps))) and len(steps) <= key["max_iter"], key
        # ... and no sooner than the ring allows: a check is read once `depth` iterations have been enqueued behind it (none in
        # synchronous mode), unless an unchecked iteration or the end of the iterations flushes the ring
        for j, o in enumerate(ops):
            if o[0] == "end":
                last = max(s[1] for s in ops[:j] if s[0] == "step") - key["base"]
                behind = last - (o[1] - key["base"])
                assert behind == (0 if key["sync"] else key["depth"]) or last == key["max_iter"] - 1 or 0 < last < key["min_iter"], (key, o)
        if code:
            assert ops[-2][0] == "end" and ops[-2][1] - key["base"] == count == key["fail_at"], key
        elif count < key["max_iter"]:
            assert steps[-1] - count <= (0 if key["sync"] else key["depth"]), key
        else:
            assert len(steps) == key["max_iter"] and not any(o[0] == "begin" and o[1] not in ends for o in ops), key


def test_verbose_lines(runs):
    """(f): the same lines, in the same order, in speculative and in synchronous mode -- those of the plain loop.  (A run whose
    check fails is left out: the speculative loop has said "(min_iter)" for an iteration the synchronous one never reached.)"""
    by_script = {}
    for key, ops in runs:
        if key["every"]:
            assert not [o for o in ops if o[0] == "say"], key
            continue
        if ops[-1][1] != 0:
            continue
        said = [o[1] for o in ops if o[0] == "say"]
        assert said == expected(key)[1], key
        by_script.setdefault((key["min_iter"], key["max_iter"], key["tolcount"], key["script"]), []).append(said)
    assert all(len(v) == 6 and all(s == v[0] for s in v) for v in by_script.values())

"""The stopping rule's sums on every route against the device's OWN factors (smk_solver_progress_sums, progress.cpp): the four
scalars of a check are a function of A and the iteration's final factors, so the parent takes the factors back, restates the sums
on the host in long double (tests/progress_reference.py) and holds each side of each route to rounding error.

Dense cases run under the accurate product form (SMK_NSPLIT=8: the right-hand sides the kernels read are fp64 products of the
stored A); sparse products are fp64 gathers anyway.  The progress switches are read once per process: each switch set gets one
fresh child (tests/progress_cases.py) that runs the whole case list and compares nothing; the children run one after another.
The cases have teeth by tests/test_progress_sums_cpu.py (every kernel tile holds >= 1e-8 of its side's sum: a dropped tile is
1e4 bars).

Bar, per side (progress_reference.bar): |S_dev - S_ld| <= max(64 e_ref, 1e-12) S_ld, plus 1e-12 (S_W + S_H) for a side that is
pure rounding; e_ref = the float64 restatement's relative distance from the long-double one; the metric gets twice the relative
bar.  The floor and the multiple of e_ref are test_gpu_entrywise.py's Tier C; 64 allows for the device's other summation order in
the sums and in the right-hand-side products.

The pass-tail route of the totals (bigprod.hip: check_totals_tail) exists only where the NNLS launch packs its factor, which needs
the fp16 two-term product form (solver.cpp: pack_in_solve): it cannot be reached under SMK_NSPLIT=8, and under the fp16 form the
right-hand sides are not fp64 products of A, so no case here takes it.  test_gpu_round6.py::test_check_totals_ride_in_the_pass_tail
holds that route to the totals launch at 8192 x 4096, k = 16: same stopping iteration, bit-identical factors and bit-identical
progress_sums() -- both add up the same partial sums of the riders -- and the totals launch is held to the factors here.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import progress_cases as pc          # noqa: E402
import progress_reference as pr      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = pc.ROOT
BASE_ENV = {"SMK_NSPLIT": "8", "SMK_R2_PERSIST": "0"}       # SMK_R2_PERSIST=0: leg c's sparse RANK2 runs the launch-per-kernel loop
SWITCH_SETS = [{}, {"SMK_PROGRESS_FUSED": "0"}, {"SMK_PROGRESS_DEFER": "0"}, {"SMK_PROGRESS_TAIL": "0"}, {"SMK_PROGRESS_POLL": "0"},
               {"SMK_PROGRESS_DEPTH": "3"}, {"SMK_BPP_GRADW": "1"}]
ROUTE_TEXT = {1: "launches of its own behind the iteration", 2: "totals as one launch", 3: "tail of the pass"}

_children = {}          # switch set -> (records by case id, arrays)
_host = {}              # (case id, sha(W), sha(H)) -> ProjectedSums
_worst = {}             # (leg, route label) -> (error / bar, case id)


@pytest.fixture(scope="module", autouse=True)
def _worst_error_table():
    """after the last test of the file: the table of profiles/progress_sums.txt, the worst error / bar per leg and route of the
    tests that ran (visible with -s)"""
    yield
    print("\nleg  route                                                                worst error/bar  case")
    for (leg, label), (ratio, cid) in sorted(_worst.items()):
        print(f"{leg:4s} {label:68s} {ratio:15.3g}  {cid}")


def _name(env):
    return ",".join(f"{k}={v}" for k, v in sorted(env.items())) or "default"


def _child(env, legs, tmp_path_factory):
    """the records and factors of one child process per switch set (legs a, b and c share the default one)"""
    key = (_name(env), legs)
    if key not in _children:
        out = str(tmp_path_factory.mktemp("progress_sums") / "factors.npz")
        full = dict(os.environ, **BASE_ENV, **env)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "progress_cases.py"), out] + list(legs), capture_output=True,
                           text=True, cwd=ROOT, timeout=600, env=full)
        recs = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
        want = sum(len(pc.CASES[leg]) for leg in legs)
        assert r.returncode == 0 and len(recs) == want and "DONE" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        _children[key] = ({(x["leg"], x["id"]): x for x in recs}, dict(np.load(out)))
    return _children[key]


def _routes(text):
    """{route number: count} of smk_solver_kernel_name(s, 2)"""
    if text == "none formed yet":
        return {}
    out = {}
    for part in text.split("; "):
        m = re.fullmatch(r"(\d+) x (.*)", part)
        hit = [r for r, t in ROUTE_TEXT.items() if t in m.group(2)]
        assert len(hit) == 1, text
        out[hit[0]] = int(m.group(1))
    return out


def _rides(case, env):
    """progress.cpp: check_rides_in_nnls"""
    return (case["alg"] == "BPP" and case["k"] <= 16 and case["rule"] == "PG_RATIO"
            and not any(k in env for k in ("SMK_PROGRESS_FUSED", "SMK_PROGRESS_DEFER", "SMK_BPP_GRADW", "SMK_SYNC_PROGRESS")))


def _direct_label(case, env, leg):
    """the kernels that form a check by launches of their own (progress.cpp: progress_begin / enqueue_progress_kernels)"""
    if case["rule"] == "DELTA_FNORM":
        return "launch_delta_fnorm"
    if case["k"] > 128:
        return "grad_pg_apply_wide_kernel + sum_partials"
    if leg == "a":
        return "grad_pg_kernel pair + sum_partials"
    if case["alg"] == "RANK2":
        return "rank2_progress_kernel, partials added on the host"
    if "SMK_PROGRESS_FUSED" in env:
        return "grad_pg2_kernel + sum_partials2_kernel"
    return "grad_pg2_snap_kernel + sum_partials2_host_kernel"


RIDER_LABEL = "NNLS riders (pg_part) + pg_defer_sum_kernel"


def _note(leg, label, ratio, cid):
    if ratio > _worst.get((leg, label), (-1.0, ""))[0]:
        _worst[(leg, label)] = (ratio, cid)


def _matrix(case, rec):
    A = pc.problem(case)[0]
    if case["data"] == "dense":
        assert rec["stored"] == pc.sha(np.asfortranarray(A)), (case["id"], "the device stores other values than oracle.quantize")
    return A


def _host_sums(case, A, arrays, key, tile):
    W, H = arrays[key + "_W"], arrays[key + "_H"]
    ck = (case["id"], tile, pc.sha(W), pc.sha(H))
    if ck not in _host:
        _host[ck] = pr.projected_sums(A, W, H, tile)
    return _host[ck]


def _rel_bar(*e_refs):
    return max(64.0 * max(e_refs), 1e-12)


def _check_sides(leg, label, cid, dev, hs, bpp_zero=None):
    """both projected sums of one check against the host's, each side by itself"""
    total = hs.sw + hs.sh
    for side, got, want, e_ref in (("W", dev[0], hs.sw, hs.e_ref_w), ("H", dev[1], hs.sh, hs.e_ref_h)):
        b = pr.bar(want, e_ref, total)
        err = abs(float(np.longdouble(got) - want))
        print(f"  {cid} {label} S_{side} device {got:.17g} host {float(want):.17g} error/bar {err / b:.3g}")
        _note(leg, label, err / b, cid)
        assert err <= b, (cid, label, side, got, float(want), err, b)
    if bpp_zero is True:
        assert dev[0] == 0.0, (cid, label, "block pivoting's W-side sum is the dual's: exactly 0", dev[0])
    elif bpp_zero is False:          # a real gradient: rounding only
        assert dev[0] <= 1e-12 * float(total), (cid, label, dev[0], float(total))


def _check_ratio(leg, label, cid, got, num, den, rel, what="metric"):
    """a metric (or pg0 with den = 1) against the host's value, twice the relative bar of the sums (a square root halves it)"""
    want = float(num / den)
    err = abs(got - want)
    b = 2.0 * rel * want
    print(f"  {cid} {label} {what} device {got:.17g} host {want:.17g} error/bar {err / b:.3g}")
    _note(leg, label + " (metric, pg0)", err / b, cid)
    assert err <= b, (cid, label, what, got, want, err, b)


def _check_ab(leg, env, case, rec, arrays):
    """legs a and b: the sums after iteration 1 and after iteration 4 against the factors read at those points, the second metric
    against the host's ratio"""
    cid = case["id"]
    label = _direct_label(case, env, leg)
    if case["data"] == "dense":
        assert rec["form"] == 8, (cid, rec["form"])
    A = _matrix(case, rec)
    if case["rule"] == "DELTA_FNORM":
        W0 = pc.problem(case)[1]
        prev4 = arrays[cid + "_1_W"] if leg == "a" else arrays[cid + "_3_W"]       # Wprev = W at the previous evaluation
        reads = [("sums1", "metric1", arrays[cid + "_1_W"], W0), ("sums4", "metric4", arrays[cid + "_4_W"], prev4)]
        if leg == "b":
            reads.append(("once_sums4", "once_metric4", arrays[cid + "_once4_W"], prev4))
        for skey, mkey, W, Wprev in reads:
            d = pr.delta_fnorm_sums(W, Wprev)
            for what, got, want, e_ref in (("num", rec[skey][2], d.num, d.e_ref_num), ("den", rec[skey][3], d.den, d.e_ref_den)):
                b = pr.bar(want, e_ref, want)
                err = abs(float(np.longdouble(got) - want))
                print(f"  {cid} {label} {what} device {got:.17g} host {float(want):.17g} error/bar {err / b:.3g}")
                _note(leg, label, err / b, cid)
                assert err <= b, (cid, what, got, float(want))
            assert rec[skey][0] == 0.0 and rec[skey][1] == 0.0
            _check_ratio(leg, label, cid, rec[mkey], d.metric, 1.0, _rel_bar(d.e_ref_num, d.e_ref_den))
        return
    tile = pc.tiles(case, leg)
    h1 = _host_sums(case, A, arrays, cid + "_1", tile)
    h4 = _host_sums(case, A, arrays, cid + "_4", tile)
    rel = _rel_bar(h1.e_ref_h, h4.e_ref_h, *((h1.e_ref_w, h4.e_ref_w) if case["alg"] in ("MU", "HALS") else ()))
    # block pivoting's W side: a real gradient on the generic route and under SMK_BPP_GRADW, the dual's exact zero otherwise
    zero = None if case["alg"] != "BPP" else (leg == "b" and "SMK_BPP_GRADW" not in env)
    _check_sides(leg, label, cid, rec["sums1"], h1, zero)
    _check_sides(leg, label, cid, rec["sums4"], h4, zero)
    assert rec["metric1"] == 1.0
    _check_ratio(leg, label, cid, rec["sums1"][4], h1.pg, 1.0, rel, "pg0")           # pg0
    _check_ratio(leg, label, cid, rec["sums4"][4], h1.pg, 1.0, rel, "pg0")
    _check_ratio(leg, label, cid, rec["metric4"], h4.pg, h1.pg, rel)
    if leg == "a":
        assert rec["route"] == "none formed yet", (cid, rec["route"])
        return
    # the first handle: iterate_checked(1) forms its only check directly, iterate_checked(3) the last of its three; a check that is
    # followed by an iteration of the same call rides in that iteration's H-side NNLS launch where block pivoting allows it
    rides = _rides(case, env)
    assert _routes(rec["route"]) == ({1: 2, 2: 2} if rides else {1: 4}), (cid, env, rec["route"])
    # the second handle, iterate_checked(4) in one call: pg0 comes from a check formed inside the loop
    assert _routes(rec["once_route"]) == ({1: 1, 2: 3} if rides else {1: 4}), (cid, env, rec["once_route"])
    assert np.array_equal(arrays[cid + "_once4_W"], arrays[cid + "_4_W"]) and np.array_equal(arrays[cid + "_once4_H"], arrays[cid + "_4_H"])
    inner = RIDER_LABEL if rides else label
    _check_sides(leg, label, cid, rec["once_sums4"], h4, zero)
    _check_ratio(leg, inner, cid, rec["once_sums4"][4], h1.pg, 1.0, rel, "pg0")
    _check_ratio(leg, inner, cid, rec["once_metric4"], h4.pg, h1.pg, rel)


def test_progress_after_iterate_on_the_generic_route(tmp_path_factory):
    """a. smk_solver_progress -- what examples/resident_nmf.c calls -- after iterate(1) and again after iterate(3): the pair of
    grad_pg_kernel launches with sum_partials (MU with PG_RATIO, HALS, BPP, RANK2 on dense A, HALS and RANK2 on a sparse matrix), the
    wide kernels at k = 130 and 200, launch_delta_fnorm for MU's default rule (Wprev = W at the previous call, W0 before the first).
    progress_sums() must be the host's sums of factors(normalize=False) taken at that point, the second metric the host's ratio; for
    block pivoting the W-side sum is a real gradient here: at most 1e-12 of the total.  No check of the ring is formed."""
    recs, arrays = _child({}, "abc", tmp_path_factory)
    for case in pc.CASES["a"]:
        _check_ab("a", {}, case, recs[("a", case["id"])], arrays)


@pytest.mark.parametrize("env", SWITCH_SETS, ids=_name)
def test_iterate_checked_on_every_switch_set(env, tmp_path_factory):
    """b. iterate_checked(1) then iterate_checked(3) on one handle, on every switch set of the check: after each call the sums of the
    check evaluated last against the factors then held, the last metric against the host's ratio.  Block pivoting at k = 8 and 16
    (n ragged in the H-side NNLS launch's 256 / KP columns per workgroup) and on a sparse matrix takes the riders, k = 24 and 128 the
    fused launch, MU / HALS the fused launch, the wide kernels (k = 130) or launch_delta_fnorm.  The last check of a call is always
    formed by launches of its own, so a second handle runs iterate_checked(4) at once: its pg0 is the first check's norm, formed
    inside the loop (by the riders where they apply), and with the last metric it is held to the host's values too.  Without
    SMK_BPP_GRADW block pivoting's W-side sum is exactly 0.0.  The route string is asserted per case."""
    recs, arrays = _child(env, "abc" if not env else "b", tmp_path_factory)
    for case in pc.CASES["b"]:
        _check_ab("b", env, case, recs[("b", case["id"])], arrays)


@pytest.mark.parametrize("env", [{}, {"SMK_SYNC_PROGRESS": "1"}], ids=_name)
def test_tolerance_stopped_run_reports_the_sums_of_the_returned_factors(env, tmp_path_factory):
    """c. run() stopped by its tolerance (min_iter 2; the tolerances come from the CPU oracle and fire after 7 or 8 iterations), one
    check in flight with snapshot and restore, and SMK_SYNC_PROGRESS=1: progress_sums() must be the host's sums of the RETURNED
    factors -- block pivoting at k = 8 and 16 forms them in the NNLS launch of the speculated next iteration, which is then undone -- pg0
    the host's norm of a second handle's factors after iterate(1), the host's metric of the returned factors <= tol and that of a
    handle after one iteration less > tol.  This holds the ring, the snapshot and the restore to the factors themselves."""
    recs, arrays = _child(env, "abc" if not env else "c", tmp_path_factory)
    for case in pc.CASES["c"]:
        cid, rec, tol = case["id"], recs[("c", case["id"])], case["tol"]
        rides = _rides(case, env)
        label = RIDER_LABEL if rides else _direct_label(case, env, "c")
        A = _matrix(case, rec)
        if case["data"] == "dense":
            assert rec["form"] == 8, (cid, rec["form"])
        assert "rank2_persist" not in rec["pass0"], rec["pass0"]
        # a converged run reports the index of the iteration the rule fired at (nmf_solve_generic.hpp:98-121)
        assert rec["rc"] == 0 and rec["done"] == rec["iters"] + 1 == case["stop"], (cid, rec)
        routes = _routes(rec["route"])
        assert set(routes) == ({2} if rides else {1}) and sum(routes.values()) >= case["stop"] - pc.MIN_ITER + 1, (cid, env, rec["route"])
        if case["rule"] == "DELTA_FNORM":
            dT = pr.delta_fnorm_sums(arrays[cid + "_T_W"], arrays[cid + "_Tm1_W"])
            dP = pr.delta_fnorm_sums(arrays[cid + "_Tm1_W"], arrays[cid + "_Tm2_W"])
            for what, got, want, e_ref in (("num", rec["sums"][2], dT.num, dT.e_ref_num), ("den", rec["sums"][3], dT.den, dT.e_ref_den)):
                b = pr.bar(want, e_ref, want)
                err = abs(float(np.longdouble(got) - want))
                print(f"  {cid} {label} {what} device {got:.17g} host {float(want):.17g} error/bar {err / b:.3g}")
                _note("c", label, err / b, cid)
                assert err <= b, (cid, what, got, float(want))
            assert dT.metric <= tol < dP.metric, (cid, float(dT.metric), tol, float(dP.metric))
            continue
        tile = pc.tiles(case, "c")
        hT = _host_sums(case, A, arrays, cid + "_T", tile)
        hP = _host_sums(case, A, arrays, cid + "_Tm1", tile)
        h1 = _host_sums(case, A, arrays, cid + "_1", tile)
        rel = _rel_bar(hT.e_ref_h, h1.e_ref_h, *((hT.e_ref_w, h1.e_ref_w) if case["alg"] in ("MU", "HALS") else ()))
        _check_sides("c", label, cid, rec["sums"], hT, True if case["alg"] == "BPP" else None)
        _check_ratio("c", label, cid, rec["sums"][4], h1.pg, 1.0, rel, "pg0")          # pg0
        assert hT.pg / h1.pg <= tol < hP.pg / h1.pg, (cid, float(hT.pg / h1.pg), tol, float(hP.pg / h1.pg))


def test_sharded_run_reports_the_whole_matrix_on_every_rank(gpu):
    """d. Two ranks column-shard a sparse matrix in one process (the in-process communicator), HALS at k = 16: after
    iterate_checked(1) and iterate_checked(3) every rank's progress_sums() must be the host's sums over the WHOLE matrix (the H-side
    sums of the shards joined by dist_agree), the same on both ranks, and the last metric the host's ratio."""
    import threading
    from smallk_amd import Comm, NmfSolver, SparseMatrix, make_options, thread_context_begin, thread_context_end
    from smallk_amd import dist as sdist
    case, world = pc.SHARDED, 2
    m, n, k = case["m"], case["n"], case["k"]
    A, W0, H0 = pc.problem(case)
    comms = Comm.init_local(world)
    out, errors = [None] * world, []

    def run(rank):
        try:
            thread_context_begin(0)
            c0, nc = sdist.shard_columns(n, world, rank)
            sub = A[:, c0:c0 + nc].tocsc()
            S = SparseMatrix(sub.data, sub.indices, sub.indptr, (m, nc), col0=c0, width_global=n)
            sv = NmfSolver(S, make_options(m, n, k, case["alg"], min_iter=1, max_iter=100, normalize=False))
            sv.attach_comm(comms[rank])
            sv.set_factors(W0, H0[:, c0:c0 + nc])
            got = []
            for iters in (1, 3):
                metric = sv.iterate_checked(iters)
                sums = sv.progress_sums()
                rc = sv.sync()
                got.append((rc, metric, sums) + sv.factors(normalize=False))
            out[rank] = (got, sv.kernel_name(2))
            sv.close()
            S.close()
        except Exception as e:          # pragma: no cover
            errors.append((rank, repr(e)))
        finally:
            thread_context_end()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    for c in comms:
        c.close()
    assert not errors, errors
    assert all(o is not None for o in out)
    label, hs = "grad_pg_kernel pair + dist_agree", []
    for step in range(2):
        assert all(o[0][step][0] == 0 for o in out)
        assert np.array_equal(out[0][0][step][3], out[1][0][step][3])              # W is replicated
        assert out[0][0][step][1:3] == out[1][0][step][1:3], (out[0][0][step][1:3], out[1][0][step][1:3])      # metric and sums agree
        H = np.concatenate([o[0][step][4] for o in out], axis=1)
        hs.append(pr.projected_sums(A, out[0][0][step][3], H, pc.tiles(case, "d")))
        _check_sides("d", label, case["id"], out[0][0][step][2], hs[-1])
    rel = _rel_bar(hs[0].e_ref_w, hs[0].e_ref_h, hs[1].e_ref_w, hs[1].e_ref_h)
    assert out[0][0][0][1] == 1.0
    _check_ratio("d", label, case["id"], out[0][0][1][2][4], hs[0].pg, 1.0, rel, "pg0")
    _check_ratio("d", label, case["id"], out[0][0][1][1], hs[1].pg, hs[0].pg, rel)
    assert all(_routes(o[1]) == {1: 4} for o in out), [o[1] for o in out]


def test_accessor_says_when_it_has_nothing(gpu):
    """smk_solver_progress_sums: SMK_BAD_PARAM before any check has been evaluated (and again after set_factors), SMK_UNSUPPORTED
    after a run that the resident RANK2 kernel finished -- that launch returns pg0 and the metric only."""
    from smallk_amd import _lib as L
    case = [c for c in pc.CASES["c"] if c["id"] == "c-rank2sp"][0]
    A, W0, H0 = pc.problem(case)
    S = gpu.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    s = gpu.NmfSolver(S, gpu.make_options(case["m"], case["n"], 2, "RANK2", min_iter=pc.MIN_ITER, max_iter=pc.MAX_ITER, tol=case["tol"]))
    s.set_factors(W0, H0)
    with pytest.raises(L.SmallkError) as e:
        s.progress_sums()
    assert e.value.code == L.BAD_PARAM
    rc, iters, _ = s.run()
    assert rc == 0 and iters + 1 == case["stop"] and s.kernel_name(0) == "smk::rank2_persist_kernel"
    with pytest.raises(L.SmallkError) as e:
        s.progress_sums()
    assert e.value.code == L.UNSUPPORTED
    s.set_factors(W0, H0)
    s.iterate(1)
    assert s.progress() == 1.0 and s.progress_sums()[4] > 0.0
    s.set_factors(W0, H0)
    with pytest.raises(L.SmallkError) as e:
        s.progress_sums()
    assert e.value.code == L.BAD_PARAM
    s.close()
    S.close()

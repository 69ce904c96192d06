"""The stopping rule's sums restated on the host (tests/progress_reference.py) against the CPU oracle, and the conditions under which
the GPU cases of tests/test_gpu_progress_sums.py have teeth -- all on the reference alone, no GPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import progress_cases as pc          # noqa: E402
import progress_reference as pr      # noqa: E402


@functools.lru_cache(maxsize=None)
def _oracle_run(cid, iters, min_iter=1, tol=1e-300):
    import oracle
    case = CASES_BY_ID[cid]
    A, W0, H0 = pc.problem(case)
    rule = oracle.DELTA_FNORM if case["rule"] == "DELTA_FNORM" else oracle.PG_RATIO
    run = oracle.nmf_sparse if case["data"] == "sparse" else oracle.nmf
    r = run(A, W0, H0, case["alg"], min_iter=min_iter, max_iter=iters, tol=tol, prog_est=rule, normalize=False)
    assert r.result == 0
    return A, r


# the restatement's own cases: every algorithm on a dense and on a sparse matrix
RESTATED = [pc._c("r-hals", "HALS", 257, 131, 12), pc._c("r-bpp", "BPP", 300, 203, 16), pc._c("r-bpp5", "BPP", 257, 131, 5),
            pc._c("r-rank2", "RANK2", 257, 131, 2), pc._c("r-hals-sp", "HALS", 300, 203, 12, data="sparse"),
            pc._c("r-bpp-sp", "BPP", 300, 203, 16, data="sparse"), pc._c("r-rank2-sp", "RANK2", 300, 203, 2, data="sparse"),
            pc._c("r-mu", "MU", 257, 131, 8), pc._c("r-mu-sp", "MU", 300, 203, 8, data="sparse"),
            pc._c("r-mu-pg", "MU", 200, 150, 33, rule="PG_RATIO"), pc._c("r-hals33", "HALS", 200, 150, 33)]
GPU_CASES = [(leg, c) for leg in "abc" for c in pc.CASES[leg]] + [("d", pc.SHARDED)]
CASES_BY_ID = {c["id"]: c for c in RESTATED + [c for _, c in GPU_CASES]}


@pytest.mark.parametrize("case", RESTATED, ids=lambda c: c["id"])
def test_restatement_reproduces_the_oracles_metric(case):
    """The rule's scalars are a function of (A, W, H) alone: recomputed in long double from the factors oracle.nmf / nmf_sparse
    return after i iterations (and after 1, and for DELTA_FNORM after i - 1), their ratio is the metric the oracle's driver formed
    inside iteration i from its own gradients -- to 1e-12 relative (measured: 2.7e-15 at most)."""
    for i in (4, 7):
        A, ri = _oracle_run(case["id"], i)
        assert ri.iteration_count == i
        want = float(ri.metrics[i - 1])
        if case["rule"] == "DELTA_FNORM":
            _, prev = _oracle_run(case["id"], i - 1)
            got = pr.delta_fnorm_sums(ri.W, prev.W).metric
        else:
            _, r1 = _oracle_run(case["id"], 1)
            tile = pr.tile_columns(case["alg"], case["k"])
            got = pr.projected_sums(A, ri.W, ri.H, tile).pg / pr.projected_sums(A, r1.W, r1.H, tile).pg
        err = float(abs(got - want) / want)
        print(case["id"], i, "restated / oracle - 1 =", err)
        assert np.isfinite(want) and err <= 1e-12, (case["id"], i, float(got), want)


def _reads(leg, case):
    """the iterations whose factors the GPU test compares sums at"""
    return pc.READS[leg] if leg in pc.READS else (1, 4) if leg == "d" else (1, case["stop"])


@pytest.mark.parametrize("leg,case", GPU_CASES, ids=lambda x: x if isinstance(x, str) else x["id"])
def test_every_gpu_case_has_teeth(leg, case):
    """On the oracle's factors at the iterations the GPU case reads:
    1. every column tile of the kernel that forms the sums (1024 / KP columns, 256 for RANK2's own kernel, 4 for k > 128) holds
       at least 1e-8 of its side's sum -- a dropped tile is then 1e4 bars of 1e-12;
    2. HALS and BPP: the projection excludes at least 1 % of sum g^2 on the H side (HALS: on the W side too) at the later
       iteration -- a kernel that forgot the projection is far outside the bar;
    3. the float64 restatement is within 1e-13 of the long-double one per side (a side that is pure rounding -- below 1e-12 of both
       sides together: block pivoting's and RANK2's W side -- has no relative error to speak of)."""
    reads = _reads(leg, case)
    for it in reads:
        A, r = _oracle_run(case["id"], it)
        if case["rule"] == "DELTA_FNORM":
            _, prev = _oracle_run(case["id"], it - 1) if it > 1 else (None, None)
            Wprev = prev.W if prev is not None else pc.problem(case)[1]
            d = pr.delta_fnorm_sums(r.W, Wprev)
            print(case["id"], it, "e_ref", d.e_ref_num, d.e_ref_den)
            assert d.num > 0 and d.den > 0 and d.e_ref_num <= 1e-13 and d.e_ref_den <= 1e-13
            continue
        s = pr.projected_sums(A, r.W, r.H, pc.tiles(case, leg))
        total = s.sw + s.sh
        print(case["id"], it, "S_W %.4g S_H %.4g e_ref %.2g %.2g excluded %.3f %.3f smallest tile %.2g %.2g"
              % (s.sw, s.sh, s.e_ref_w, s.e_ref_h, s.excluded_w, s.excluded_h, s.tile_share_w.min(), s.tile_share_h.min()))
        shares_h = s.tile_share_h
        if leg == "d":          # every rank tiles its own shard of H from its first column (W is replicated: tiled whole)
            from smallk_amd.dist import shard_columns
            shares_h = np.concatenate([s.shard_tile_shares_h(*shard_columns(case["n"], 2, rank), pc.tiles(case, leg)) for rank in range(2)])
            assert abs(shares_h.sum() - 1.0) < 1e-12 and len(shares_h) == 4
        for side, ssum, shares, e_ref in (("W", s.sw, s.tile_share_w, s.e_ref_w), ("H", s.sh, shares_h, s.e_ref_h)):
            if ssum < 1e-12 * total:
                assert side == "W" and case["alg"] in ("BPP", "RANK2"), (case["id"], it, side)
                continue
            assert shares.min() >= 1e-8, (case["id"], it, side, shares.min())
            assert e_ref <= 1e-13, (case["id"], it, side, e_ref)
        if it == reads[-1] and case["alg"] in ("HALS", "BPP"):
            assert s.excluded_h >= 0.01, (case["id"], it, s.excluded_h)
            if case["alg"] == "HALS":
                assert s.excluded_w >= 0.01, (case["id"], it, s.excluded_w)


@pytest.mark.parametrize("case", pc.CASES["c"], ids=lambda c: c["id"])
def test_tolerances_of_the_stopped_runs(case):
    """leg c's tolerances: the oracle's driver (min_iter 2) stops after the recorded number of iterations, not before iteration 6,
    and the tolerance lies 2 % clear of the metrics on both sides of the stop, so the device's 1e-12-class distance cannot move it.
    (The count NmfSolve<> reports for a converged run is the index of the iteration the rule fired at: one less.)"""
    _, r = _oracle_run(case["id"], pc.MAX_ITER, pc.MIN_ITER, case["tol"])
    T = case["stop"]
    assert r.iteration_count == T - 1 and 6 <= T < pc.MAX_ITER
    assert r.metrics[T - 1] <= 0.98 * case["tol"]
    assert all(r.metrics[i] >= 1.02 * case["tol"] for i in range(pc.MIN_ITER, T - 1))

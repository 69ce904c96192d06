"""The entry-by-entry checker itself (tests/entrywise.py), with the oracle as the stand-in device: the two inversions of one MU
iteration return the products, a single changed entry of A is named exactly, the oracle passes Tier C's bound, and every
Tier A / Tier B case meets the preconditions its bound rests on."""
import numpy as np
import pytest

import entrywise as ew
import oracle

SHAPES = [(65, 129, 17), (257, 383, 33), (321, 257, 130)]


def oracle_mu(A, W0, H0):
    """W1 from the oracle; H1 from the same arithmetic (the oracle returns only the final pair, and H1 is final too)"""
    r = oracle.nmf(A, W0, H0, "MU", min_iter=1, max_iter=1, normalize=False)
    assert r.result == 0 and r.iteration_count == 1
    return r.W, r.H


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_both_inversions_return_the_products(m, n, k):
    A, W0, H0 = ew.integer_inputs(m, n, k)
    W1, H1 = oracle_mu(A, W0, H0)
    bad1, r1 = ew.check_p1(A, W0, H0, H1)
    bad2, r2 = ew.check_p2(A, W0, H1, W1, ew.EXACT_RTOL)
    print(f"{m}x{n} k={k}: P1 error/bound {r1:.3f}, P2 error/bound {r2:.3f}")
    assert len(bad1) == 0 and len(bad2) == 0, (r1, r2)


@pytest.mark.parametrize("where", ["last_row", "last_column", "interior"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_one_changed_entry_is_named(m, n, k, where):
    """the checker is handed an A that differs from the one the stand-in device saw in ONE entry, by 1: exactly the k entries
    of W0'A in that column and the k entries of A H1' in that row are outside the bound"""
    A, W0, H0 = ew.integer_inputs(m, n, k)
    W1, H1 = oracle_mu(A, W0, H0)
    i, j = {"last_row": (m - 1, n // 3), "last_column": (m // 3, n - 1), "interior": (m // 2, n // 2)}[where]
    A2 = A.copy()
    A2[i, j] += 1.0
    bad1, _ = ew.check_p1(A2, W0, H0, H1)
    bad2, _ = ew.check_p2(A2, W0, H1, W1, ew.EXACT_RTOL)
    assert sorted(map(tuple, bad1)) == [(c, j) for c in range(k)]
    assert sorted(map(tuple, bad2)) == [(i, c) for c in range(k)]


@pytest.mark.parametrize("m,n,k", [(257, 131, 5), (257, 131, 17), (300, 263, 33), (600, 523, 65)])
def test_oracle_passes_the_hals_bound(m, n, k):
    """Tier C's bound is 256 x the distance between make_golden.hals in fp64 and in long double: the oracle, a third
    implementation in fp64, must be inside it"""
    A, W0, H0 = ew.tier_c_inputs(m, n, k, 0)
    Wl, Hl, e_ref, bound = ew.hals_reference(m, n, k, 0)
    r = oracle.nmf(A, W0, H0, "HALS", min_iter=1, max_iter=1, normalize=False)
    e = ew.scaled_distance(r.W, r.H, Wl, Hl)
    print(f"{m}x{n} k={k}: e_ref {e_ref:.2e} oracle {e:.2e} bound {bound:.2e}")
    assert (np.asarray(Wl) > 0).mean() > 0.5                     # a regular update, not the all-zero-column guard
    assert e <= bound


ALL_CASES = ew.form_cases() + ew.split_cases() + ew.single_copy_cases() + ew.variant_cases()[0]


def test_preconditions_of_every_case():
    """Conditions, not measurements: fp32 partial sums of the W'A pass stay exact integers (105 len < 2^24), and where the H*A'
    pass is judged, its bound is at least four times below the smallest term of any entry, from the actual inputs."""
    assert len({c.id() for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        assert 105 * c.m < 2 ** 24, c.id()
        A, W0, H0 = c.inputs()
        assert A.min() >= 1 and A.max() <= 15 and W0.min() >= 1 and W0.max() <= 7 and H0.min() >= 1 and H0.max() <= 7
        if c.tau is not None:
            assert 4.0 * c.tau <= ew.term_share(c.m, c.n, c.k, c.range), (c.id(), c.tau, ew.term_share(c.m, c.n, c.k, c.range))
            assert c.tau <= 2.0 ** -14


def test_variant_list_holds_what_the_planner_honours():
    honoured, refused = ew.variant_cases()
    assert honoured and all(c.v1 == c.v2 == (c.variant if c.variant is not None else c.variant_k64) for c in honoured)
    asked = set(ew.OLD_SCREEN + ew.EXTRA_VARIANTS)
    kept = {(c.variant if c.variant is not None else c.variant_k64, c.storage, c.nsplit) for c in honoured}
    # each runs as itself at one k at least, but variant 13 under bf16x3 on bf16 storage (no k fits: EXTRA_VARIANTS covers it)
    assert asked - kept == {(13, "bf16", None)} and kept <= asked

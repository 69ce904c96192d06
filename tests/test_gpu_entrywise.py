"""Dense products and single factor updates, entry by entry at tile edges (helpers, bounds and case lists: tests/entrywise.py).

Tier A: one MU iteration on small integers; W0'A recovered from H1 must be the exact integer product within 1e-14 per entry, in
every product form, storage, forced variant and row split -- which also judges both Gram routes, since the host uses its own.
Tier B: A H1' recovered from W1 of the same run against the fp64 product with the H1 the device returned, inside a bound derived
from the form's operand width and the kernel's fp32 chain length (accurate form: an fp64 dot product).  bf16 storage with ONE
bf16 term of the factor (SMK_NSPLIT=1, 8-bit operands) is judged in Tier A only: no shape keeps its bound four times below a
dropped term.
Tier C: one HALS / BPP iteration under the accurate form against make_golden.hals in long double / the oracle.
Every case asserts the product form and the kernel names the solver reports, so no case tests something other than its name."""
import numpy as np
import pytest

import entrywise as ew
import oracle

pytestmark = pytest.mark.gpu

WORST = {}          # largest error / bound per (tier, storage, form), printed by the last test (python -m pytest -s)


def note(tier, c, ratio):
    key = (tier, c.storage, c.form)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def one_iteration(gpu, monkeypatch, env, A, W0, H0, alg, storage):
    for name, v in env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    m, n = A.shape
    k = W0.shape[1]
    D = gpu.DenseMatrix.from_host(A, storage=storage)
    s = gpu.NmfSolver(D, gpu.make_options(m, n, k, alg, min_iter=1, max_iter=1, normalize=False))
    s.set_factors(W0, H0)
    s.iterate(1)
    rc = s.sync()
    W, H = s.factors()
    info = (s.product_form()[0], s.kernel_name(0), s.kernel_name(1), D.single_copy)
    s.close()
    D.close()
    assert rc == 0
    return W, H, info


def run_case(gpu, monkeypatch, c):
    A, W0, H0 = c.inputs()
    W1, H1, (form, name1, name2, single) = one_iteration(gpu, monkeypatch, c.env(), A, W0, H0, "MU", c.storage)
    assert form == c.form, (form, c.form)
    assert name1 == f"{c.kernel()} variant {c.v1}", name1
    assert name2 == f"{c.kernel()} variant {c.v2}" + (" (transposed source)" if c.single_copy else ""), name2
    assert single == c.single_copy
    bad1, r1 = ew.check_p1(A, W0, H0, H1)
    print(f"{c.id()}: form {form} | {name1} | {name2} | P1 error/1e-14 {r1:.3f}", end="")
    note("A", c, r1)
    assert len(bad1) == 0, (r1, bad1[:8])
    if c.tau is not None:
        bad2, r2 = ew.check_p2(A, W0, H1, W1, c.tau)
        print(f" | tau {c.tau:.3e} (chain {c.chain}) P2 error/tau {r2:.3f}", end="")
        note("B", c, r2)
        assert len(bad2) == 0, (r2, c.tau, bad2[:8])
    print()


@pytest.mark.parametrize("c", ew.form_cases(), ids=ew.Case.id)
def test_product_forms_at_tile_edges(gpu, monkeypatch, c):
    run_case(gpu, monkeypatch, c)


@pytest.mark.parametrize("c", ew.split_cases(), ids=ew.Case.id)
def test_row_splits(gpu, monkeypatch, c):
    run_case(gpu, monkeypatch, c)


@pytest.mark.parametrize("c", ew.single_copy_cases(), ids=ew.Case.id)
def test_transposed_source(gpu, monkeypatch, c):
    run_case(gpu, monkeypatch, c)


@pytest.mark.parametrize("c", ew.variant_cases()[0], ids=ew.Case.id)
def test_forced_variants_run_as_themselves(gpu, monkeypatch, c):
    run_case(gpu, monkeypatch, c)


TIER_C = [(m, n, k, st, q) for (m, n, k) in ew.HALS_SHAPES for (st, q) in (("f32", 0), ("bf16", 1))]
ACCURATE = {"SMK_NSPLIT": "8"}


@pytest.mark.parametrize("m,n,k,storage,quant", TIER_C)
def test_hals_one_iteration(gpu, monkeypatch, m, n, k, storage, quant):
    """every entry of W against its row's maximum, of H against its column's, reference make_golden.hals in long double;
    e_dev <= max(256 e_ref, 1e-12), e_ref = the same distance for make_golden.hals in fp64"""
    A, W0, H0 = ew.tier_c_inputs(m, n, k, quant)
    Wl, Hl, e_ref, bound = ew.hals_reference(m, n, k, quant)
    assert (np.asarray(Wl) > 0).mean() > 0.5                     # the regular update
    W, H, (form, _, _, _) = one_iteration(gpu, monkeypatch, ACCURATE, A, W0, H0, "HALS", storage)
    e_dev = ew.scaled_distance(W, H, Wl, Hl)
    print(f"HALS {m}x{n} k={k} {storage}: e_ref {e_ref:.2e} e_dev {e_dev:.2e} bound {bound:.2e}")
    assert form == 8
    assert e_dev <= bound, (e_dev, bound)


def test_hals_from_the_unscaled_start(gpu, monkeypatch):
    """the first W sweep clamps every entry to zero and takes the all-zero-column guard: deterministic, same bound"""
    m, n, k = 257, 131, 16
    A, W0, H0 = ew.tier_c_inputs(m, n, k, 0, matched=False)
    Wl, Hl, e_ref, bound = ew.hals_reference(m, n, k, 0, False)
    guard = np.all(np.abs(np.asarray(Wl, dtype=np.float64) - 1.0 / np.sqrt(m)) < 1e-12, axis=0)
    assert guard.any()                                           # columns of eps, normalised to 1 / sqrt(m): the guard path
    W, H, _ = one_iteration(gpu, monkeypatch, ACCURATE, A, W0, H0, "HALS", "f32")
    e_dev = ew.scaled_distance(W, H, Wl, Hl)
    print(f"HALS unscaled start {m}x{n} k={k}: e_ref {e_ref:.2e} e_dev {e_dev:.2e} bound {bound:.2e}")
    assert e_dev <= bound, (e_dev, bound)


@pytest.mark.parametrize("m,n,k,storage,quant", TIER_C)
def test_bpp_one_iteration(gpu, monkeypatch, m, n, k, storage, quant):
    """same passive sets as the oracle, every entry within 1e-9 of its column's (H) or row's (W) maximum (the bar of an isolated
    solve, tests/test_gpu_nnls.py::compare)"""
    A, W0, H0 = ew.tier_c_inputs(m, n, k, quant)
    ref = oracle.nmf(A, W0, H0, "BPP", min_iter=1, max_iter=1, normalize=False)
    W, H, (form, _, _, _) = one_iteration(gpu, monkeypatch, ACCURATE, A, W0, H0, "BPP", storage)
    e_dev = ew.scaled_distance(W, H, ref.W, ref.H)
    print(f"BPP {m}x{n} k={k} {storage}: e_dev {e_dev:.2e}")
    assert form == 8 and ref.result == 0
    assert np.array_equal(W > 0, ref.W > 0) and np.array_equal(H > 0, ref.H > 0)
    assert e_dev <= 1e-9, e_dev


def test_print_largest_error_over_bound():
    """prints the largest error / bound per tier, storage and form of the cases that ran before it (profiles/entrywise_checks.txt)"""
    for (tier, st, form), r in sorted(WORST.items()):
        print(f"tier {tier} {st} form {form}: largest error/bound {r:.3f}")

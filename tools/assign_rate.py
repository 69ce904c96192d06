#!/usr/bin/env python3
"""What labels, memberships and top terms cost on the device, and what the route without them costs (profiles/assign_rate.txt).

One solver at the sizes the README quotes -- 10^6 documents, 2^20 terms, k = 64 -- on a sparse matrix with eight stored entries
per document, its factors set to random values on the device (the labelling does not care where the factors came from).
  (d) the device entries on the resident factors: ``solver.labels_device(normalize=False)``, the same with memberships,
      ``solver.top_terms_device(5 / 50, normalize=False)``: host clock around the call, which ends in a stream synchronise.
      Warm, then windows of several calls; minimum, average and maximum window.
  (k) their kernels alone (launch_labels / launch_top_terms on tensors in the resident layout, device events around `reps`
      launches), with the bytes the algorithm has to move over that time, as a share of the 6.29 TB/s copy rate.
  (h) the route that exists without them: ``solver.factors()`` (both factors to the host), then
      ``flatclust.compute_assignments`` / ``compute_fuzzy_assignments`` / ``top_terms`` on one core.
  (x) the results of (d) and (h) compared: equal integers, equal membership bits.
Needs a GPU; nothing here falls back to the CPU.

    python tools/assign_rate.py [--small] [--out profiles/assign_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd
from smallk_amd import _lib as L
from smallk_amd import flatclust

LAUNCH_LABELS = "_ZN3smk13launch_labelsEPKvililPjPfP12ihipStream_t"
LAUNCH_TERMS = "_ZN3smk16launch_top_termsEPKvilliiPvPiiP12ihipStream_t"
SCRATCH_TERMS = "_ZN3smk22topterms_scratch_bytesEliii"
COPY_RATE = 6.29e12               # MI355X, measured float4 copy
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def windows(fn, calls, nwin):
    fn()
    fn()
    out = []
    for _ in range(nwin):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls)
    return min(out), sum(out) / len(out), max(out)


def event_windows(fn, reps, nwin):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / reps)
    return min(out), sum(out) / len(out), max(out)


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms (avg {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def rate(nbytes, t):
    return f"{nbytes / 1e9:.2f} GB -> {nbytes / t[0] / 1e12:.2f} TB/s = {100 * nbytes / t[0] / COPY_RATE:.0f} % of the copy rate"


def once(label, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    say(f"      {label}: {dt * 1e3:10.1f} ms")
    return out, dt


def kernels_alone(m, n, k, KP, cus):
    lib = L.lib()
    labels_fn, terms_fn, scratch_fn = getattr(lib, LAUNCH_LABELS), getattr(lib, LAUNCH_TERMS), getattr(lib, SCRATCH_TERMS)
    labels_fn.restype, terms_fn.restype, scratch_fn.restype = C.c_int, C.c_int, C.c_size_t
    i64, vp = C.c_int64, C.c_void_p
    g = torch.Generator(device="cuda").manual_seed(3)
    H = torch.rand((n, KP), generator=g, dtype=torch.float64, device="cuda")       # column c at c * KP: the resident layout
    Wt = torch.rand((m, KP), generator=g, dtype=torch.float64, device="cuda")      # row i at i * KP
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    P = torch.empty((n, k), dtype=torch.float32, device="cuda")
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def lab(memb):
        rc = labels_fn(vp(H.data_ptr()), L.DT_F64, i64(KP), k, i64(n), vp(labels.data_ptr()), vp(P.data_ptr()) if memb else None, stream)
        assert rc == 0, rc
    t = event_windows(lambda: lab(False), 10, 5)
    say(f"  (k) launch_labels, labels only:        {ms(t)}; H read once, {rate(8.0 * k * n + 4.0 * n, t)}")
    t = event_windows(lambda: lab(True), 10, 5)
    say(f"  (k) launch_labels, with memberships:   {ms(t)}; H read twice (k > 16), P written, {rate(16.0 * k * n + 4.0 * k * n + 4.0 * n, t)}")
    for maxterms in (5, 50, 256):
        nb = scratch_fn(i64(m), k, maxterms, cus)
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        out = torch.empty((k, maxterms), dtype=torch.int32, device="cuda")

        def top():
            rc = terms_fn(vp(Wt.data_ptr()), L.DT_F64, i64(KP), i64(m), k, maxterms, vp(scratch.data_ptr()), vp(out.data_ptr()), cus, stream)
            assert rc == 0, rc
        t = event_windows(top, 10, 5)
        # (the workspace holds two sets of candidates for the merge levels; stage one writes one set and the first level reads it)
        say(f"  (k) launch_top_terms, maxterms = {maxterms:3d}:  {ms(t)}; W read once + {nb / 2e6:.1f} MB of candidates written and read, "
            f"{rate(8.0 * k * m + 1.0 * nb, t)}")
    del H, Wt, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a sixteenth of the documents and terms")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    k = 64
    n, m = (10 ** 6, 2 ** 20) if not args.small else (62500, 2 ** 16)
    say(f"device: {torch.cuda.get_device_name(0)}; k = {k}, n = {n} documents, m = {m} terms; times are the minimum window unless noted")
    rng = np.random.default_rng(1)
    per = 8
    S = smallk_amd.SparseMatrix(rng.random(n * per) + 0.1, rng.integers(0, m, n * per), np.arange(n + 1, dtype=np.uint32) * per, (m, n))
    s = smallk_amd.NmfSolver(S, smallk_amd.make_options(m, n, k, "BPP"))
    g = torch.Generator(device="cuda").manual_seed(2)
    s.set_factors_device(torch.rand((m, k), generator=g, dtype=torch.float64, device="cuda"),
                         torch.rand((k, n), generator=g, dtype=torch.float64, device="cuda"))
    torch.cuda.empty_cache()

    say("(d) the device entries on the solver's resident factors, whole call")
    d_lab = windows(lambda: s.labels_device(normalize=False), 5, 5)
    say(f"  (d) labels_device:                       {ms(d_lab)}")
    d_mem = windows(lambda: s.labels_device(normalize=False, memberships=True), 5, 5)
    say(f"  (d) labels_device(memberships=True):     {ms(d_mem)}")
    d_top = {}
    for maxterms in (5, 50):
        d_top[maxterms] = windows(lambda: s.top_terms_device(maxterms, normalize=False), 5, 5)
        say(f"  (d) top_terms_device({maxterms:2d}):                {ms(d_top[maxterms])}")
    t257 = windows(lambda: s.top_terms_device(257, normalize=False), 1, 2)
    say(f"  (d) top_terms_device(257), the radix sort route ({k} sorts of {m} keys): {ms(t257)}")

    say("(k) the kernels alone, device events around 10 launches")
    kernels_alone(m, n, k, 64, L.lib().smk_device_cu_count())

    say("(h) the route without them, once (one host core)")
    (W, H), t_dl = once(f"factors(): W and H to the host, {8.0 * k * (m + n) / 1e9:.2f} GB", lambda: s.factors(normalize=False))
    h_lab, t_a = once("compute_assignments(H)", lambda: flatclust.compute_assignments(H))
    h_mem, t_f = once("compute_fuzzy_assignments(H)", lambda: flatclust.compute_fuzzy_assignments(H))
    h_top, t_t = {}, {}
    for maxterms in (5, 50):
        h_top[maxterms], t_t[maxterms] = once(f"top_terms(W, {maxterms})", lambda: flatclust.top_terms(W, maxterms))
    say(f"  (h) labels + memberships + top terms(5):  {(t_dl + t_a + t_f + t_t[5]) * 1e3:10.1f} ms; "
        f"(d) the same three: {(d_mem[0] + d_top[5][0]) * 1e3:.3f} ms")
    say(f"  (h) labels + memberships + top terms(50): {(t_dl + t_a + t_f + t_t[50]) * 1e3:10.1f} ms; "
        f"(d) the same three: {(d_mem[0] + d_top[50][0]) * 1e3:.3f} ms")

    say("(x) the two routes agree")
    labels, P = s.labels_device(normalize=False, memberships=True)
    ok_l = np.array_equal(labels.cpu().numpy().astype(np.int64), h_lab.astype(np.int64))
    ok_p = np.array_equal(P.t().contiguous().cpu().numpy().view(np.uint32), np.ascontiguousarray(h_mem.T).view(np.uint32))
    say(f"  labels equal: {ok_l}; membership bits equal: {ok_p}")
    for maxterms in (5, 50):
        got = s.top_terms_device(maxterms, normalize=False).cpu().numpy()
        say(f"  top terms({maxterms}) equal: {np.array_equal(got, h_top[maxterms].reshape(k, maxterms))}")
    s.close()
    S.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

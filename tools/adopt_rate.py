#!/usr/bin/env python3
"""What DenseMatrix.from_device costs, and what it replaces (profiles/adopt_rate.txt).

For a torch tensor in GPU memory, at C3's shape (65536 x 16384) and C2's (8192 x 4096), sources fp32 row-major, fp32
column-major and fp64 column-major, storages bf16 and f32:
  (a) DenseMatrix.from_device (creation + the fused convert-and-transpose) and adopt() into an existing matrix: host clock
      around the call, which ends in a stream synchronise;
  (b) the only route without the feature: t.cpu().double().numpy(), a Fortran-order copy, DenseMatrix.from_host;
  (c) the kernel by itself (launch_adopt_dense on the caller's stream, device events around `reps` launches): minimum bytes
      = the source once + each stored copy once, over its time, as a share of the chip's measured copy rate (6.29 TB/s);
  (d) the two-pass form it stands beside, launch_convert_f64 + launch_transpose_store, timed the same way on the same
      buffers (fp64 column-major source only: that is all the pair takes).
(c) and (d) call the library's launch functions through their C++ symbol names; when a build does not export them the two
rows say so.  Needs a GPU; nothing here falls back to the CPU.

    python tools/adopt_rate.py [--small] [--out profiles/adopt_rate.txt]
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

COPY_RATE = 6.29e12       # float4 copy kernel on this chip, bytes per second read + written
LAUNCHERS = {"adopt": "_ZN3smk18launch_adopt_denseEPKvillPvlS2_lillP12ihipStream_t",
             "convert": "_ZN3smk18launch_convert_f64EPKdlPvilllP12ihipStream_t",
             "transpose": "_ZN3smk22launch_transpose_storeEPKvlPvlillP12ihipStream_t"}
DT = {torch.float64: (L.DT_F64, 8), torch.float32: (L.DT_F32, 4)}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def round_up(x, m):
    return (x + m - 1) // m * m


def source(m, n, dtype, layout):
    g = torch.Generator(device="cuda").manual_seed(1)
    if layout == "row-major":
        return torch.rand((m, n), generator=g, device="cuda", dtype=dtype)
    return torch.rand((n, m), generator=g, device="cuda", dtype=dtype).t()


def host_timed(fn, reps):
    fn()                                  # warm-up: code objects, the allocator's blocks
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sum(ts) / len(ts), max(ts)


def event_timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def launcher(lib, name):
    try:
        fn = getattr(lib, LAUNCHERS[name])
    except AttributeError:
        return None
    fn.restype = C.c_int
    return fn


def kernel_rows(lib, t, storage, reps):
    """(c) and (d) on buffers laid out as smk_matrix_create lays them out"""
    m, n = t.shape
    es = 2 if storage == "bf16" else 4
    st_code = L.STORE_BF16 if storage == "bf16" else L.STORE_F32
    ldA, ldAt = round_up(m, 256), round_up(n, 128)
    A = torch.zeros(ldA * round_up(n, 256) * es, dtype=torch.uint8, device="cuda")
    At = torch.zeros(ldAt * round_up(m, 256) * es, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp, i64 = C.c_void_p, C.c_int64
    dt, ses = DT[t.dtype]
    rs, cs = t.stride()
    min_bytes = m * n * (ses + 2 * es)
    out = {}
    adopt = launcher(lib, "adopt")
    if adopt:
        def fused():
            rc = adopt(vp(t.data_ptr()), dt, i64(rs), i64(cs), vp(A.data_ptr()), i64(ldA), vp(At.data_ptr()), i64(ldAt), st_code,
                       i64(m), i64(n), stream)
            assert rc == 0, rc
        sec = event_timed(fused, reps)
        out["c"] = (sec, min_bytes)
    conv, tr = launcher(lib, "convert"), launcher(lib, "transpose")
    if conv and tr and t.dtype == torch.float64 and rs == 1:
        def two_pass():
            rc = conv(vp(t.data_ptr()), i64(cs), vp(A.data_ptr()), st_code, i64(ldA), i64(m), i64(n), stream)
            rc |= tr(vp(A.data_ptr()), i64(ldA), vp(At.data_ptr()), i64(ldAt), st_code, i64(m), i64(n), stream)
            assert rc == 0, rc
        out["d"] = (event_timed(two_pass, reps), min_bytes)
    del A, At
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="C2's shape only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-reps", type=int, default=2, help="timed repetitions of the host route (b)")
    args = ap.parse_args()
    smallk_amd.initialize(0)
    lib = L.lib()
    say(f"device: {torch.cuda.get_device_name(0)}; copy rate taken as {COPY_RATE / 1e12:.2f} TB/s; times are the minimum over the repetitions unless noted")
    shapes = [("C2", 8192, 4096)] + ([] if args.small else [("C3", 65536, 16384)])
    for name, m, n in shapes:
        for dtype, layout in ((torch.float32, "row-major"), (torch.float32, "column-major"), (torch.float64, "column-major")):
            t = source(m, n, dtype, layout)
            for storage in ("bf16", "f32"):
                say(f"{name} {m} x {n}, source {str(dtype).split('.')[1]} {layout}, storage {storage}:")
                mats = []

                def from_device():
                    for d in mats:
                        d.close()
                    mats[:] = [smallk_amd.DenseMatrix.from_device(t, storage=storage)]
                a_min, a_avg, a_max = host_timed(from_device, 5)
                D = mats[0]
                ad_min, ad_avg, ad_max = host_timed(lambda: D.adopt(t), 10)
                say(f"  (a) from_device {a_min * 1e3:9.3f} ms (avg {a_avg * 1e3:.3f}, max {a_max * 1e3:.3f}); adopt() into an existing matrix "
                    f"{ad_min * 1e3:9.3f} ms (avg {ad_avg * 1e3:.3f}, max {ad_max * 1e3:.3f})")
                D.close()
                mats.clear()
                # (b) is host work in the main: at C3's shape only for the first storage of each source, one timed repetition
                if name == "C2" or storage == "bf16":
                    def host_route():
                        h = np.asfortranarray(t.cpu().double().numpy())
                        smallk_amd.DenseMatrix.from_host(h, storage=storage).close()
                    b_min, b_avg, b_max = host_timed(host_route, args.host_reps if name == "C2" else 1)
                    say(f"  (b) .cpu().double().numpy() + Fortran copy + from_host {b_min * 1e3:9.1f} ms (avg {b_avg * 1e3:.1f}, max {b_max * 1e3:.1f}): "
                        f"{b_min / a_min:.0f} x from_device")
                rows = kernel_rows(lib, t, storage, 20)
                for key, label in (("c", "(c) launch_adopt_dense, one launch"), ("d", "(d) launch_convert_f64 + launch_transpose_store")):
                    if key not in rows:
                        if key == "c" or (dtype == torch.float64):
                            say(f"  {label}: not measured (launch function not exported by this build)")
                        continue
                    sec, nbytes = rows[key]
                    say(f"  {label}: {sec * 1e3:8.3f} ms; minimum bytes {nbytes / 1e9:.3f} GB -> {nbytes / sec / 1e12:.2f} TB/s = "
                        f"{100 * nbytes / sec / COPY_RATE:.0f} % of the copy rate")
            del t
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

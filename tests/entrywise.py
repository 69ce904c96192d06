"""Host side of the entry-by-entry checks of the dense products and single factor updates (no GPU import).

One MU iteration with normalize=False can be undone entry by entry (tests/golden/make_golden.py::mu, eps = 1e-13):

    H1 = H0 * (W0'A) / (W0'W0 H0 + eps)   =>   P1 := W0'A  = H1 * (G_W H0 + eps) / H0
    W1 = W0 * (A H1') / (W0 H1H1' + eps)  =>   P2 := A H1' = W1 * (W0 G_H + eps) / W0

G_W = W0'W0 and G_H = H1 H1' are formed HERE in fp64, G_H from the H1 the device returned, so that a fault of the first pass is
not charged to the second one and a wrong Gram matrix on the device shows like a wrong product.  This file holds the inputs, the
two inversions, the bounds (derived from the number formats and from the kernels' structure, never from their output), a
restatement of the planner's variant choice (so that the test lists hold only combinations the planner honours and the GPU tests
can assert the name of the kernel that ran) and the case lists that the CPU and the GPU tests share.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402

EPS = 1e-13
EXACT_RTOL = 1e-14          # Tier A: three roundings of the device update + the host inversion, ten times over (<= 9e-16)

# ---- the planner, restated (smallk_amd/csrc/bigprod_plan.h: kVariants, kF3Variants, bp_fits, f3_fits, choose_variant) ----
# (rows per stage, ring depth, 128-column tiles per workgroup, k-tile waves, loader waves)
KVARIANTS = [(64, 3, 1, 1, 0), (64, 4, 1, 1, 0), (64, 5, 1, 1, 0), (128, 2, 1, 1, 0), (128, 3, 1, 1, 0), (64, 3, 2, 1, 0),
             (64, 2, 1, 1, 0), (32, 2, 1, 1, 0), (32, 3, 1, 1, 0), (32, 4, 1, 1, 0), (64, 2, 1, 2, 0), (64, 3, 1, 2, 0),
             (64, 4, 1, 2, 0), (32, 4, 1, 2, 0), (64, 2, 2, 2, 0), (64, 3, 1, 1, 4), (64, 4, 1, 1, 4), (64, 5, 1, 1, 4),
             (64, 3, 1, 2, 4), (64, 4, 1, 2, 4), (32, 4, 1, 1, 2), (32, 4, 1, 2, 4), (32, 5, 1, 2, 4), (64, 2, 1, 1, 4)]
# 100 + index: (rows per stage, ring depth, loader waves, stages between two folds into fp64)
F3VARIANTS = [(32, 2, 0, 2), (32, 3, 0, 2), (32, 4, 4, 2), (32, 5, 4, 2), (32, 2, 2, 2), (64, 2, 0, 1), (64, 2, 4, 1), (32, 4, 4, 4),
              (32, 2, 0, 4), (32, 4, 2, 2), (32, 4, 4, 4), (32, 5, 4, 4), (32, 5, 4, 2), (32, 4, 2, 4), (32, 5, 2, 4), (32, 3, 2, 4),
              (32, 5, 4, 8)] + [(32, 5, 4, 4)] * 8 + [(32, 2, 0, 8), (32, 3, 0, 4), (32, 2, 0, 16), (32, 2, 0, 2), (32, 2, 0, 1)]
F16_VARIANTS = (108, 110, 111, 115, 125, 126, 127, 128, 129)
ACCURATE = 200              # the variant number the accurate form reports


def kt_of(k):
    return (k + 31) // 32


def bp_fits(ebytes, kt, nsplit, mb, nstage, cw, wk, nwl):
    if kt % wk:
        return False
    cpc = mb // (16 // ebytes)
    qs = mb // 16 if (ebytes == 2 or nsplit == 3) else cpc // 2
    if qs < 1:
        return False
    stage = 128 * cw * mb * ebytes + qs * nsplit * kt * 1024
    ti, nw = stage // 1024, (nwl if nwl > 0 else 4 * wk)
    return ti % nw == 0 and (ti // nw) * (nstage - 1) <= 63 and stage * nstage <= 160 * 1024


def f3_fits(v, kt, form):
    if v < 100 or v >= 100 + len(F3VARIANTS):
        return False
    mb, nstage, nwl, _ = F3VARIANTS[v - 100]
    stage = 128 * mb * 4 + (mb // 16) * (2 if form == 4 else form) * kt * 1024
    ti, nld = stage // 1024, (nwl if nwl > 0 else 4)
    return ti % nld == 0 and (ti // nld) * (nstage - 1) <= 63 and stage * nstage <= 160 * 1024


def f16_variant_by_length(length):
    return 125 if length >= 65536 else 108 if length >= 16384 else 128 if length >= 4096 else 129


def planned_variant(storage, k, length, form, want=None, want_k64=None):
    """The variant plan_bigprod settles on for the first group of 64 factor rows: `form` is the solver's product form, `want` /
    `want_k64` what SMK_BP_VARIANT / SMK_BP_VARIANT_K64 ask for."""
    kt = kt_of(min(k, 64))
    bf16 = storage == "bf16"
    ns = form if bf16 else (form if form >= 2 else 1)
    if form == 8:
        return ACCURATE
    v = 6 if bf16 else 7
    if kt == 2:
        v = 18 if bf16 else 21
    if not bf16 and ns >= 2:
        v = 108 if kt == 2 else 115
    if not bf16 and ns == 4:
        v = f16_variant_by_length(length)
    if want is not None:
        v = want
    if want_k64 is not None and kt == 2:
        v = want_k64
    if not bf16 and ns == 2 and v < 100:
        v = 108 if kt == 2 else 115
    if ns != 4 and v in (128, 129):
        v = 108
    if ns == 4 and v not in F16_VARIANTS:
        v = 125
    if v >= 100 and not bf16 and ns >= 2:
        if not f3_fits(v, kt, ns):
            v = 125 if ns == 4 else 108
        if not f3_fits(v, kt, ns):
            v = 115
        if not f3_fits(v, kt, ns):
            v = 110
        return v
    if v < 0 or v >= len(KVARIANTS):
        v = 6
    fits = lambda vv: bp_fits(2 if bf16 else 4, kt, ns, *KVARIANTS[vv])
    if not fits(v):
        v = 11 if kt == 2 else 0
    if not fits(v) and kt == 2:
        v = 13
    if not fits(v):
        v = 0
    if not fits(v):
        v = 7
    return v


def planned_variant_transposed(storage, k, length):
    """plan_bigprod_groups_tr: the H*A' pass of a single-copy matrix reads A itself"""
    if storage == "bf16":
        return 18 if kt_of(min(k, 64)) == 2 else 6
    return f16_variant_by_length(length)


def chain_rows(storage, form, variant, transposed=False):
    """Longest fp32 accumulation chain between two folds into fp64, in rows of the contraction, read from the kernels:
    bigprod_kernel (bf16 storage; fp32 storage natively or in its first bf16x3 form) flushes its fp32 sums after every stage;
    bigprod_f3_kernel / bigprod_f3p_kernel fold every `fold` stages of 32 or 64 rows; the transposed source of bf16 storage always
    takes 64-column stages (launch_bigprod_tr_v), whatever variant the plan names."""
    if variant == ACCURATE:
        return 0
    if transposed and storage == "bf16":
        return 64
    if variant >= 100:
        mb, _, _, fold = F3VARIANTS[variant - 100]
        return mb * fold
    return KVARIANTS[variant][0]


def expected_form(storage, k, nsplit_env):
    """smk_solver_create for dense MU on integer data (no column spread): SMK_NSPLIT, else fp16 two-term up to k = 64 on fp32
    storage and bf16x3 otherwise; the fp16 form exists on fp32 storage only."""
    form = nsplit_env if nsplit_env is not None else (4 if storage == "f32" and k <= 64 else 3)
    return 3 if form == 4 and storage != "f32" else form


# operand width the project documents per form; bf16 storage with ONE bf16 term of the factor keeps 8 bits and
# is checked in the exact tier only
OPERAND_BITS = {("f32", 1): 24, ("f32", 2): 16, ("f32", 3): 24, ("f32", 4): 22, ("bf16", 2): 16, ("bf16", 3): 24}


def tau_accurate(length, k):
    return (length + k + 8) * 2.0 ** -52


def tau_reduced(bits, chain):
    return 2.0 * 2.0 ** -bits + chain * 2.0 ** -24


# ---- inputs -------------------------------------------------------------------------------------------------------------------
# value ranges (A lo, A hi, W0 lo, W0 hi, H0 lo, H0 hi), widest first: all exact in bf16, fp16 and fp32
RANGES = ((1, 15, 1, 7, 1, 7), (8, 15, 1, 7, 4, 7), (12, 15, 4, 7, 6, 7))


@functools.lru_cache(maxsize=8)
def integer_inputs(m, n, k, seed=0, rng_index=0):
    """A in 1 .. 15 (a subset of Tier A's 0 .. 15: no term of either pass vanishes, so every dropped term shows), W0 and H0 in
    1 .. 7, or one of the narrower ranges.  Read-only: the tests share them."""
    a0, a1, w0, w1, h0, h1 = RANGES[rng_index]
    rng = np.random.default_rng(seed + 1000003 * (m * 131 + n) + k)
    A = np.asfortranarray(rng.integers(a0, a1 + 1, (m, n)).astype(np.float64))
    W0 = np.asfortranarray(rng.integers(w0, w1 + 1, (m, k)).astype(np.float64))
    H0 = np.asfortranarray(rng.integers(h0, h1 + 1, (k, n)).astype(np.float64))
    for x in (A, W0, H0):
        x.setflags(write=False)
    return A, W0, H0


def mu_step(A, W0, H0):
    """one iteration of make_golden.mu, keeping H1: (W1, H1)"""
    H1 = H0 * ((W0.T @ A) / ((W0.T @ W0) @ H0 + EPS))
    W1 = W0 * ((A @ H1.T) / (W0 @ (H1 @ H1.T) + EPS))
    return W1, H1


def smallest_term_share(A, H1):
    """min over the entries (i, c) of A H1' of (smallest term A_ij H1_cj) / entry: what ONE dropped term moves an entry by, at least"""
    P2 = A @ H1.T
    worst = np.inf
    for c in range(H1.shape[0]):
        worst = min(worst, float(((A * H1[c]).min(axis=1) / P2[:, c]).min()))
    return worst


@functools.lru_cache(maxsize=None)
def term_share(m, n, k, rng_index):
    A, W0, H0 = integer_inputs(m, n, k, 0, rng_index)
    return smallest_term_share(A, mu_step(A, W0, H0)[1])


def range_for(m, n, k, tau):
    """first (widest) value range whose smallest dropped term is at least four times tau; the narrowest if none is (the CPU test
    of the preconditions then fails: no case is left out to satisfy them)"""
    if tau is None:
        return 0
    for r in range(len(RANGES)):
        if 4.0 * tau <= term_share(m, n, k, r):
            return r
    return len(RANGES) - 1


# ---- the two inversions and their checks ---------------------------------------------------------------------------------------
def recover_p1(W0, H0, H1):
    return H1 * ((W0.T @ W0) @ H0 + EPS) / H0


def recover_p2(W0, H1, W1):
    return W1 * (W0 @ (H1 @ H1.T) + EPS) / W0


def check_p1(A, W0, H0, H1, rtol=EXACT_RTOL):
    """(indices of the entries of W0'A outside rtol, largest error / bound)"""
    ref = W0.T @ A                                              # exact: integers below 2^53
    err = np.abs(recover_p1(W0, H0, H1) - ref)
    return np.argwhere(err > rtol * ref), float((err / (rtol * ref)).max())


def check_p2(A, W0, H1, W1, tau):
    """the same for A H1' with the H1 that was returned"""
    ref = A @ H1.T
    err = np.abs(recover_p2(W0, H1, W1) - ref)
    return np.argwhere(err > tau * ref), float((err / (tau * ref)).max())


# ---- Tier C -----------------------------------------------------------------------------------------------------------------------
def scaled_distance(W, H, Wref, Href):
    """largest |W - Wref| against its row's maximum and |H - Href| against its column's maximum"""
    Wref, Href = np.asarray(Wref), np.asarray(Href)
    dw = np.abs(W - Wref) / np.maximum(np.abs(Wref).max(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    dh = np.abs(H - Href) / np.maximum(np.abs(Href).max(axis=0, keepdims=True), np.finfo(np.float64).tiny)
    return float(max(dw.max(), dh.max()))


def tier_c_inputs(m, n, k, quant, matched=True):
    import oracle
    A = mg.make_A(m, n, k, True, quant)
    W0 = oracle.fill_uniform(m, k, 43)
    H0 = oracle.fill_uniform(k, n, 44) * ((2.0 / k) if matched else 1.0)
    return A, W0, H0


@functools.lru_cache(maxsize=None)
def hals_reference(m, n, k, quant, matched=True):
    """(W, H of make_golden.hals in long double, e_ref = its scaled distance from the same code in fp64, bound on the device)"""
    A, W0, H0 = tier_c_inputs(m, n, k, quant, matched)
    ld = np.longdouble
    Wl, Hl = mg.hals(A.astype(ld), W0.astype(ld), H0.astype(ld), 1)
    Wd, Hd = mg.hals(A, W0, H0, 1)
    e_ref = scaled_distance(Wd, Hd, Wl, Hl)
    return Wl, Hl, e_ref, max(256.0 * e_ref, 1e-12)


HALS_SHAPES = [(257, 131, 1), (257, 131, 5), (257, 131, 16), (257, 131, 17), (257, 131, 32), (300, 263, 33), (520, 261, 64),
               (600, 523, 65), (600, 523, 100), (600, 523, 130), (4099, 37, 9)]

# ---- the case lists ---------------------------------------------------------------------------------------------------------------
K_EDGES = (1, 2, 15, 16, 17, 32, 33, 64, 65, 128, 129)
BASE_SHAPES = ((65, 129), (129, 65), (191, 257), (257, 383), (64, 128), (1, 130), (130, 1))
SHAPES = BASE_SHAPES + ((257, 191), (383, 257), (128, 64))                 # m and n exchanged: the other pass ragged
FORMS = (("f32", None), ("f32", 1), ("f32", 2), ("f32", 3), ("f32", 4), ("f32", 8), ("bf16", None), ("bf16", 1), ("bf16", 2), ("bf16", 8))
TALL = (70001, 129)
# what tests/test_gpu_variants.py screens: (variant, storage, SMK_NSPLIT)
OLD_SCREEN = [(v, "bf16" if v < 100 else "f32", None) for v in (0, 1, 5, 6, 7, 9, 11, 13, 14, 15, 18, 20, 21, 108, 110, 111, 115, 125, 126)] + \
             [(v, "f32", 3) for v in (7, 21, 100, 102, 106, 108, 111, 115, 117)]
# variant 13 (32-row stages, two k-tile waves) fits neither bf16x3 form the old screen ran it under; it does fit two bf16 terms on
# bf16 storage and the native fp32 form at k in (32, 64], so it is run there
EXTRA_VARIANTS = [(13, "bf16", 2), (13, "f32", 1)]


def ks_for(m, n):
    return tuple(k for k in K_EDGES if k <= min(m, n) and (k < 65 or (m, n) in ((257, 383), (383, 257))))


class Case:
    """one MU iteration: shape, storage, the switches, and what the planner must answer"""

    def __init__(self, m, n, k, storage, nsplit=None, variant=None, variant_k64=None, splits=None, single_copy=False):
        self.m, self.n, self.k, self.storage = m, n, k, storage
        self.nsplit, self.variant, self.variant_k64, self.splits, self.single_copy = nsplit, variant, variant_k64, splits, single_copy
        self.form = expected_form(storage, k, nsplit)
        self.v1 = planned_variant(storage, k, m, self.form, variant, variant_k64)
        self.v2 = planned_variant_transposed(storage, k, n) if single_copy else planned_variant(storage, k, n, self.form, variant, variant_k64)
        bits = OPERAND_BITS.get((storage, self.form))
        self.chain = chain_rows(storage, self.form, self.v2, single_copy)
        # bound of the H*A' pass (contraction over n); None: 8-bit operands, exact tier only
        self.tau = tau_accurate(n, k) if self.form == 8 else tau_reduced(bits, min(self.chain, -(-n // 32) * 32)) if bits else None
        self.range = range_for(m, n, k, self.tau)

    def env(self):
        e = {"SMK_NSPLIT": self.nsplit, "SMK_BP_VARIANT": self.variant, "SMK_BP_VARIANT_K64": self.variant_k64,
             "SMK_BP_SPLITS": self.splits, "SMK_SINGLE_COPY": 1 if self.single_copy else None}
        return {name: (None if v is None else str(v)) for name, v in e.items()}

    def inputs(self):
        return integer_inputs(self.m, self.n, self.k, 0, self.range)

    def kernel(self):
        if self.form == 8:
            return "smk::bigprod_f64_k2_kernel" if self.k <= 2 else "smk::bigprod_f64_kernel"
        return "smk::bigprod_f3_kernel" if self.storage == "f32" else "smk::bigprod_kernel"

    def id(self):
        s = f"{self.m}x{self.n}-k{self.k}-{self.storage}"
        for tag, v in (("form", self.nsplit), ("v", self.variant), ("v64_", self.variant_k64), ("splits", self.splits)):
            if v is not None:
                s += f"-{tag}{v}"
        return s + ("-single" if self.single_copy else "")


def form_cases():
    """every form at every k edge on two shapes, every shape at the default forms, the tall case for the Gram kernels' column
    partition in every form"""
    out = [Case(m, n, k, st, ns) for (m, n) in ((65, 129), (257, 383)) for k in ks_for(m, n) for (st, ns) in FORMS]
    out += [Case(m, n, k, st) for (m, n) in SHAPES if (m, n) not in ((65, 129), (257, 383)) for k in ks_for(m, n) for st in ("f32", "bf16")]
    out += [Case(TALL[0], TALL[1], k, st, ns) for k in (16, 33) for (st, ns) in FORMS]
    return out


def split_cases():
    """more row splits than stages (64 against 3 .. 6 stages) and a last split shorter than the others"""
    return [Case(m, n, k, st, splits=s) for (m, n) in ((65, 129), (191, 257)) for s in (1, 2, 8, 64) for k in (16, 33) for st in ("f32", "bf16")]


def single_copy_cases():
    """the H*A' pass from A itself, where the transposed-source kernels exist (single_copy_serves)"""
    return [Case(m, n, k, st, ns, single_copy=True) for (m, n) in ((65, 129), (129, 65), (191, 257), (257, 383), (383, 257))
            for k in ks_for(m, n) if k in (1, 16, 17, 33, 64, 65, 129) for (st, ns) in (("f32", None), ("f32", 3), ("bf16", None), ("bf16", 2))]


def variant_cases():
    """(honoured, refused): the old screen's (variant, storage, form) at k = 16 and 33 through SMK_BP_VARIANT and at k = 64 through
    SMK_BP_VARIANT_K64, split by whether plan_bigprod keeps the variant that was asked for"""
    honoured, refused = [], []
    for (v, st, ns) in OLD_SCREEN + EXTRA_VARIANTS:
        for k, k64 in ((16, False), (33, False), (64, True)):
            c = Case(191, 257, k, st, ns, variant_k64=v) if k64 else Case(191, 257, k, st, ns, variant=v)
            (honoured if c.v1 == v and c.v2 == v else refused).append(c)
    return honoured, refused


def old_screen_runs():
    """What the old screen's processes ran under SMK_BP_VARIANT = v: quick_parity.py's five shapes, HALS (bf16x3) and BPP (fp16
    two-term on fp32 storage, bf16x3 on bf16 storage), both passes.  One (v, SMK_NSPLIT, {(storage, k, form): variants that ran})
    per listed run."""
    shapes = ((300, 200, 33, "bf16"), (256, 192, 64, "f32"), (2048, 1024, 32, "bf16"), (1000, 3000, 20, "bf16"), (4096, 512, 16, "f32"))
    out = []
    for (v, _, ns) in OLD_SCREEN:
        ran = {}
        for (m, n, k, st) in shapes:
            for form in ((3,) if st == "bf16" or ns == 3 else (3, 4)):
                for length in (m, n):
                    ran.setdefault((st, k, form), set()).add(planned_variant(st, k, length, form, v))
        out.append((v, ns, ran))
    return out

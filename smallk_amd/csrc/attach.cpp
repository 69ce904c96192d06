// smallk_amd/csrc/attach.cpp -- giving a solver its communicator: the host-callback hook (smk_solver_set_comm) and the native
// communicator (smk_solver_attach_comm: the agreement on the product form, the chunk geometry, the workspace, the row-sharded W, the
// second stream and its events).  Its state is the solver's Exchange (state.h); the exchange itself runs on the per-iteration path
// (solver.cpp: prod1_sharded, prod2, the comm_fork / comm_join family).
#include "solver_internal.h"
#include "comm.h"

#include <algorithm>

namespace smk {

// workspace layout: [R2red: rows x kpp f32|f64][Gh: KP*KP f64][scal: 8 f64][Wt: KP x rows f64].  rows = the padded
// row count (callback hook: one all-reduce per buffer, any world) or world * nchunk * blk with a native communicator
// (equal blocks for the reduce-scatter / all-gather)
static inline i64 comm_rows(const smk_solver* s) { return s->ex.comm ? std::max<i64>(s->ex.rows_cap, s->pl2.ncols_pad) : s->pl2.ncols_pad; }
static size_t comm_bytes(const smk_solver* s)
{
    size_t b = (size_t)comm_rows(s) * s->kpp * (s->ex.red_f64 ? sizeof(double) : sizeof(float));
    b = (b + 255) / 256 * 256;
    b += (size_t)s->KP * s->KP * sizeof(double);
    b = (b + 255) / 256 * 256;
    b += 8 * sizeof(double);
    b = (b + 255) / 256 * 256;
    b += (size_t)s->KP * (size_t)comm_rows(s) * sizeof(double);
    return b;
}

static void carve_workspace(smk_solver* s, void* workspace)
{
    unsigned char* p = (unsigned char*)workspace;
    s->R2red = (float*)p;
    size_t b = (size_t)comm_rows(s) * s->kpp * (s->ex.red_f64 ? sizeof(double) : sizeof(float));      // same layout as comm_bytes()
    b = (b + 255) / 256 * 256;
    s->Gh = (double*)(p + b);
    b += (size_t)s->KP * s->KP * sizeof(double);
    b = (b + 255) / 256 * 256;
    s->scal = (double*)(p + b);
    b += 8 * sizeof(double);
    b = (b + 255) / 256 * 256;
    s->Wt = (double*)(p + b);
}

// this rank's blocks of the full W (every rank holds all of it after set_factors / a gather / the final scaling) -> Wown
int scatter_own(smk_solver* s)
{
    for (int j = 0; j < s->ex.nchunk; ++j) {
        i64 a, b;
        own_block(s, j, &a, &b);
        if (b > a)
            SMK_HIP(hipMemcpyAsync(s->ex.Wown + (i64)j * s->ex.blk * s->KP, s->Wt + a * s->KP, (size_t)(b - a) * s->KP * sizeof(double),
                                   hipMemcpyDeviceToDevice, s->st));
    }
    return 0;
}

}  // namespace smk

extern "C" {

int smk_solver_comm_workspace_bytes(const smk_solver* s, size_t* bytes)
{
    if (!s || !bytes) return SMK_BAD_PARAM;
    *bytes = comm_bytes(s);
    return SMK_OK;
}

int smk_solver_set_comm(smk_solver* s, int rank, int world, smk_allreduce_fn fn, void* user, void* workspace,
                        size_t workspace_bytes)
{
    if (!s || world < 1 || rank < 0 || rank >= world) return SMK_BAD_PARAM;
    if (world > 1 && !fn) return SMK_BAD_PARAM;
    Exchange& x = s->ex;
    if (x.comm) { set_error("a native communicator is attached"); return SMK_BAD_PARAM; }
    x.rank = rank; x.world = world;
    if (fn && (!workspace || workspace_bytes < comm_bytes(s))) return SMK_BAD_PARAM;
    if (fn) {
        if (!x.ar) { x.home[0] = s->Gh; x.home[1] = s->scal; x.home[2] = s->Wt; }      // still in the handle's own blocks: remember the way back
        carve_workspace(s, workspace);
    } else if (x.ar) {
        s->Gh = x.home[0]; s->scal = x.home[1]; s->Wt = x.home[2];
    }
    x.ar = fn; x.ar_user = user;
    return SMK_OK;
}

// Native path: every collective is issued from C on the solver's second stream (RCCL over xGMI, or the in-process
// stand-in).  Call before set_factors().  The communicator must outlive the solver.
int smk_solver_attach_comm(smk_solver* s, smk_comm* comm)
{
    if (!s || !comm) return SMK_BAD_PARAM;
    Exchange& x = s->ex;
    if (x.ar || x.comm) { set_error("solver already has a communicator"); return SMK_BAD_PARAM; }
    x.comm = comm;
    x.rank = comm->rank; x.world = comm->world;
    // MEASUREMENT HOOK (bench.py --emulate-world N, one GPU): the geometry of rank 0 of N ranks -- row blocks, chunk
    // sizes, per-rank NNLS / Gram / packing work -- while the collectives run through the real one-rank communicator.
    // Times a rank's work without the transfers; the blocks of the other ranks never arrive, so the factors mean nothing.
    if (const int emu = sw::comm_emulate_world(); comm->world == 1 && emu > 1 && emu <= 64) { x.world = emu; x.rank = 0; }
    // The ranks must run ONE exchange protocol.  The product form is chosen per solver, and one input of that choice -- the
    // spread of the column scales -- is measured on the rank's LOCAL column shard: a rank whose shard alone spans more than
    // 2^28 would take the accurate form (and with it other buffers and other collectives) while its peers do not.  So the
    // form is agreed here, first thing, over the communicator: any rank that wants the accurate form moves all of them.
    // Every rank of the communicator calls attach, so this is a collective like the ones that follow.
    if (comm->world > 1) {
        double want = s->nsplit == NSPLIT_F64 ? 1.0 : 0.0;
        SMK_HIP(hipMemcpy(s->scal, &want, sizeof(double), hipMemcpyHostToDevice));
        int arc = comm_allreduce(comm, s->scal, 1, 1, s->st);
        if (arc) { x.comm = nullptr; return arc; }
        SMK_HIP(hipStreamSynchronize(s->st));
        SMK_HIP(hipMemcpy(&want, s->scal, sizeof(double), hipMemcpyDeviceToHost));
        if (want > 0.0 && s->nsplit != NSPLIT_F64 && !s->a->sparse) {
            s->nsplit = NSPLIT_F64;
            arc = plan_products(s);
            if (!arc && alloc_product_buffers(s)) arc = SMK_DEVICE_ERROR;
            if (arc) { x.comm = nullptr; return arc; }
        }
    }
    // chunk geometry: blocks of >= 4096 rows, at most 4 chunks (SMK_COMM_CHUNKS overrides: 1 .. 8), block a multiple of
    // 256 rows (the column tile of the streaming kernels and a whole number of packed chunk pairs)
    {
        const i64 mpad = s->pl2.ncols_pad;
        i64 c = mpad / ((i64)x.world * 4096);
        c = std::max<i64>(1, std::min<i64>(c, 4));
        if (const auto ce = sw::comm_chunks(); ce.set) c = std::max(1, std::min(ce.v, MAX_CHUNKS));
        x.blk = round_up((mpad + (i64)x.world * c - 1) / ((i64)x.world * c), 256);
        x.nchunk = (int)((mpad + (i64)x.world * x.blk - 1) / ((i64)x.world * x.blk));      // chunks that hold rows
        x.rows_cap = (i64)x.nchunk * x.world * x.blk;
    }
    {
        // fp64 on the wire unless SMK_COMM_F64=0.  SURVEY 8e suggested fp32 (half the bytes); measured at the full C4 size on
        // the bench's noise-like data (tools/shard8_fullsize.py: 8 shards against one GPU): fp32 costs 1.1e-4 in W after ONE
        // iteration -- the sums over 65536 columns are ~500, their fp32 rounding 3e-5, and HH' of such data amplifies it a
        // thousand times -- against 6e-7 with fp64.  With the exchange pipelined behind the pass the extra bytes are hidden
        // except in the last chunk.
        x.red_f64 = sw::comm_f64() != 0;
    }
    // BPP and MU update the rows of W independently of each other: every rank takes its own blocks (HALS normalises column by
    // column over ALL rows inside its sweep and keeps the replicated update)
    // (also under the accurate product form: its W'A pass reads the fp64 factor itself, so the fp64 own blocks are gathered per
    // chunk in place of the packed operand -- prod1_sharded)
    x.w_sharded = (s->o.algorithm == SMK_ALG_BPP || s->o.algorithm == SMK_ALG_MU) && !s->a->sparse && (x.world > 1 || comm_forced());
    const size_t bytes = comm_bytes(s);
    if (s->own.dev((unsigned char**)&x.comm_ws, bytes)) { x.comm = nullptr; x.w_sharded = false; set_error("no memory for the communicator workspace"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemsetAsync(x.comm_ws, 0, bytes, s->st));
    carve_workspace(s, x.comm_ws);
    if (!s->a->sparse && s->pl2.S == 1 && x.red_f64) {
        // one row split and fp64 on the wire: the partial products ARE the send buffer.  They get room for the equal
        // blocks of the last chunk (rows past the padded row count are never written and stay zero).
        s->own.drop(&s->P2);
        const size_t pe = (size_t)comm_rows(s) * s->kpp;
        if (s->own.dev(&s->P2, pe)) return SMK_DEVICE_ERROR;
        SMK_HIP(hipMemsetAsync(s->P2, 0, pe * sizeof(double), s->st));
        s->R2red = (float*)s->P2;
        x.r2_alias = true;
    }
    if (x.w_sharded) {
        // the packed operand of W is gathered in equal blocks: room for rows_cap rows, groups laid out for that length
        s->own.drop(&s->packW);
        const size_t pb = packed_bytes(s->a->storage, s->k, x.rows_cap, s->nsplit);
        if (s->own.dev((unsigned char**)&s->packW, pb)) return SMK_DEVICE_ERROR;
        SMK_HIP(hipMemsetAsync(s->packW, 0, pb, s->st));
        size_t off = 0;
        for (int g = 0; g < s->ng; ++g) {
            s->pg1[g].pack_offset = off;
            off += packed_bytes(s->a->storage, s->pg1[g].kg, x.rows_cap, s->nsplit);
        }
        s->pl1.pack_offset = s->pg1[0].pack_offset;
        const size_t own_rows = (size_t)x.nchunk * x.blk;
        const size_t rb = x.red_f64 ? sizeof(double) : sizeof(float);
        if (s->own.dev(&x.Wown, own_rows * s->KP)) return SMK_DEVICE_ERROR;
        if (s->own.dev((unsigned char**)&x.R2own, own_rows * s->kpp * rb)) return SMK_DEVICE_ERROR;
        SMK_HIP(hipMemsetAsync(x.Wown, 0, own_rows * s->KP * sizeof(double), s->st));
        SMK_HIP(hipMemsetAsync(x.R2own, 0, own_rows * s->kpp * rb, s->st));
        x.n_own = 0;
        for (int j = 0; j < x.nchunk; ++j) {
            i64 a, b;
            own_block(s, j, &a, &b);
            if (b > a) x.n_own += b - a;
        }
    }
    int erc = s->own.stream(&x.st2, hipStreamNonBlocking);
    for (hipEvent_t* e : {&x.ev_gram, &x.ev_gh, &x.ev_x, &x.ev_y}) erc |= s->own.event(e, hipEventDisableTiming);
    for (int j = 0; j < MAX_CHUNKS; ++j)
        for (hipEvent_t* e : {&x.ev_c[j], &x.ev_r[j], &x.ev_a[j]}) erc |= s->own.event(e, hipEventDisableTiming);
    if (erc) return SMK_DEVICE_ERROR;
    // nothing is allocated once the collectives are in flight (several ranks may live in one process)
    return progress_prealloc(s);
}

}  // extern "C"

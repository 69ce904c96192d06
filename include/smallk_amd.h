/*
 * include/smallk_amd.h -- C ABI of the MI355X-native dense NMF solver.
 *
 * This is the drop-in boundary for the smallk hot path: plain
 * pointers and sizes, no C++ or torch types.  Every entry point names the
 * reference interface it stands in for (paths relative to /root/reference).
 * The C++ facade (include/smallk.hpp, include/nmf.hpp) and the Python mirror of
 * pysmallk (smallk_amd/api.py) are both thin layers over these symbols.
 *
 * Conventions (same as the reference's inner seam, common/include/nmf.hpp:77-81):
 *   - host matrices are fp64, column-major, leading dimension >= height;
 *   - W (m x k) and H (k x n) are in/out: initial guess in, factors out;
 *   - return values are `Result` codes (nmf.hpp:17-26) plus two negative
 *     extensions for device errors; smk_last_error() gives the text;
 *   - not thread safe (the reference is not either: smallk.cpp:46-67).
 */
#ifndef SMALLK_AMD_H
#define SMALLK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum Result, common/include/nmf.hpp:17-26 */
enum {
    SMK_OK = 0,
    SMK_NOTINITIALIZED = -1,
    SMK_INITIALIZED = -2,
    SMK_BAD_PARAM = -3,
    SMK_FAILURE = -4,
    SMK_SIZE_TOO_LARGE = -5,
    SMK_FLATCLUST_FAILURE = -6,
    /* extensions (never produced by the reference) */
    SMK_DEVICE_ERROR = -100, /* HIP runtime error, see smk_last_error() */
    SMK_UNSUPPORTED = -101   /* valid for the reference, not built here (k > 2048) */
};

/* enum NmfAlgorithm, common/include/nmf.hpp:28-34 (NOT smallk::Algorithm's order) */
enum { SMK_ALG_MU = 0, SMK_ALG_HALS = 1, SMK_ALG_RANK2 = 2, SMK_ALG_BPP = 3 };

/* enum NmfProgressAlgorithm, common/include/nmf.hpp:37-41 */
enum { SMK_PROG_PG_RATIO = 0, SMK_PROG_DELTA_FNORM = 1 };

/* how A is held in HBM (device-side option; the host API stays fp64) */
enum { SMK_STORE_F32 = 0, SMK_STORE_BF16 = 1 };

/* struct NmfOptions, common/include/nmf.hpp:55-69 (bool -> int) */
typedef struct smk_options {
    double tol;
    int algorithm;
    int prog_est_algorithm;
    int height;
    int width;
    int k;
    int min_iter;
    int max_iter;
    int tolcount;
    int max_threads; /* accepted, unused on the device path */
    int verbose;
    int normalize;
} smk_options;

/* struct NmfStats, common/include/nmf.hpp:43-53 */
typedef struct smk_stats {
    unsigned long long elapsed_us;
    int iteration_count;
} smk_stats;

typedef struct smk_matrix smk_matrix; /* A (and A') resident in HBM, possibly a column shard */
typedef struct smk_solver smk_solver; /* one NmfSolve<> instance */

/* ---- lifecycle: NmfInitialize / NmfIsInitialized / NmfFinalize, nmf.hpp:71-73 ------------ */
int smk_initialize(int device_ordinal); /* -1: keep the current HIP device */
int smk_is_initialized(void);           /* SMK_INITIALIZED or SMK_NOTINITIALIZED */
void smk_finalize(void);
const char* smk_last_error(void);
int smk_device_cu_count(void);

/* IsValid(const NmfOptions&, bool validate_matrix), common/src/nmf_options.cpp:23-112 */
int smk_is_valid(const smk_options* opts, int validate_matrix);

/* Use an existing HIP stream (e.g. torch's current stream) instead of the library's own. */
int smk_set_stream(void* hip_stream);

/* ---- one shot: Result Nmf(const NmfOptions&, double* A, int ldA, double* W, int ldW,
 *      double* H, int ldH, NmfStats&), common/include/nmf.hpp:77-81 / src/nmf.cpp:173-229.
 *      `storage` chooses how A sits in HBM (the reference has no such knob). */
int smk_nmf_dense(const smk_options* opts, const double* A, int64_t ldA, double* W, int64_t ldW,
                  double* H, int64_t ldH, smk_stats* stats, int storage);

/* ---- one shot, sparse: Result NmfSparse(const NmfOptions&, height, width, nz, col_offsets, row_indices,
 *      data, W, ldW, H, ldH, NmfStats&), common/include/nmf.hpp:83-92 / src/nmf.cpp:232-300 */
int smk_nmf_sparse(const smk_options* opts, unsigned height, unsigned width, unsigned nz,
                   const unsigned* col_offsets, const unsigned* row_indices, const double* data,
                   double* W, int64_t ldW, double* H, int64_t ldH, smk_stats* stats);

/* ---- device-resident A (replaces the DenseMatrix view of buf_a, nmf.cpp:224) ---------------
 * A matrix object holds the column shard [col0, col0 + ncols_local) of a height x width_global
 * matrix, plus its transpose (the reference's BPP solver keeps At too, nmf_solver_bpp.hpp:319). */
int smk_matrix_create(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0,
                      int64_t ncols_local, int storage);
/* The same without the stored transpose ("single copy"): the reference's MU and HALS call Gemm(NORMAL, TRANSPOSE)
 * on A itself (nmf_solver_mu.hpp:121-164, nmf_solver_hals.hpp:166-199) -- only its BPP keeps A' -- and so does this matrix: the
 * H*A' pass contracts down the strided direction of A (bf16: transposing LDS reads; fp32: strided 4-byte reads).  Half the footprint (twice the problem per GPU) and
 * no transpose pass at load time.  Solvers on it: MU, HALS and BPP with the 16-bit product forms read A only; the first solver that needs
 * the transpose (RANK2, the accurate form) makes the matrix allocate and fill it, after which it is an ordinary matrix
 * (smk_matrix_is_single_copy / smk_matrix_device_bytes tell).  SMK_SINGLE_COPY=1 makes smk_matrix_create do this for every dense matrix,
 * and smk_matrix_create does it by itself when A fits the device memory and A + A' do not. */
int smk_matrix_create_single_copy(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0,
                                  int64_t ncols_local, int storage);
int smk_matrix_is_single_copy(const smk_matrix* a);
/* bytes of HBM the resident matrix occupies (A, its transpose when stored, or the CSC arrays) */
int64_t smk_matrix_device_bytes(const smk_matrix* a);
/* copy a host fp64 column-major block (height x ncols_local, the shard) into HBM */
int smk_matrix_upload_f64(smk_matrix* a, const double* host, int64_t ld);
/* fill with the counter-based uniform [0,1) generator (matrixgen UNIFORM, matrixgen/src/main.cpp:64-72);
 * element (r, c) depends only on (seed, global index), so shards agree with the whole. */
int smk_matrix_fill_uniform(smk_matrix* a, uint64_t seed);
/* structured synthetic data (the planted-low-rank variant): A = Ws Hs + noise U, rounded to the storage type, with
 * Ws (height x kstar) / Hs (kstar x width_global) the uniform matrices of seed + 1 / seed + 2 with entries <= threshold set to
 * zero and U the uniform matrix of `seed`; keyed by the global element index like smk_matrix_fill_uniform, fp64 sums in
 * increasing j (oracle twin: orc_fill_planted, same bits) */
int smk_matrix_fill_planted(smk_matrix* a, uint64_t seed, int kstar, double threshold, double noise);
/* read the shard back as fp64 (tests) */
int smk_matrix_download_f64(const smk_matrix* a, double* host, int64_t ld);
void smk_matrix_destroy(smk_matrix* a);
/* a copy of a resident matrix in the calling thread's context (current device): device-to-device, also across devices */
int smk_matrix_clone(const smk_matrix* src, smk_matrix** out);
/* a host thread with a device context of its own (stream, handles) on `device_ordinal`, separate from the process-wide
 * one, until smk_thread_context_end(); smk_device_count / smk_current_device: the HIP runtime's answers */
int smk_thread_context_begin(int device_ordinal);
void smk_thread_context_end(void);
int smk_device_count(void);
int smk_current_device(void);
int smk_device_synchronize(void);   /* hipDeviceSynchronize on the calling thread's current device */
/* The library keeps freed device workspaces of up to 512 MB each (at most 4 GB per device, SMK_DEVMEM_CACHE_MB) for reuse; they are
 * invisible to other allocators in the process (torch, RCCL).  smk_device_trim returns those of the current device to the HIP
 * runtime (call it before creating communicators or large torch tensors); the return value is the number of bytes that were cached. */
size_t smk_device_trim(void);
/* sparse A in CSC (replaces SparseMatrix<double>, common/include/sparse_matrix_decl.hpp:21-132): the local
 * columns [col0, col0+ncols_local); 32-bit indices as in the reference, duplicates allowed (they add up).
 * The transpose is built here too (the reference does it in Solver_Generic_BPP::Init, nmf_solver_bpp.hpp:319). */
int smk_matrix_create_sparse(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0,
                             int64_t ncols_local, int64_t nnz_local, const unsigned* col_offsets,
                             const unsigned* row_indices, const double* data);
/* Host-side CSC bookkeeping behind the sparse matrix objects (no device needed).
 * smk_csc_transpose: Transpose(SparseMatrix), common/include/sparse_matrix_ops.hpp:36-127 (counting sort).
 * smk_csc_subset_cols_compact: SparseMatrix::SubMatrixColsCompact, common/include/sparse_matrix_impl.hpp:478-592;
 *   call with out_col_offsets == NULL for the sizes, then with arrays of *out_nnz / ncols+1 entries;
 *   old_to_new (height entries, 0xFFFFFFFF = dropped row) and new_to_old (*new_height entries) may be NULL.
 * smk_matrix_download_csc: the resident CSC (transposed != 0: the CSC of A') back on the host (tests). */
int smk_csc_transpose(int64_t height, int64_t width, const unsigned* col_offsets, const unsigned* row_indices,
                      const double* data, unsigned* out_col_offsets, unsigned* out_row_indices, double* out_data);
int smk_csc_subset_cols_compact(int64_t height, int64_t width, const unsigned* col_offsets, const unsigned* row_indices,
                                const double* data, const unsigned* cols, int64_t ncols, unsigned* out_col_offsets,
                                unsigned* out_row_indices, double* out_data, unsigned* old_to_new, unsigned* new_to_old,
                                int64_t* new_height, int64_t* out_nnz);
int smk_matrix_download_csc(const smk_matrix* a, int transposed, unsigned* col_offsets, unsigned* row_indices,
                            double* data);
/* The reference's sparse Gemm by itself (common/include/sparse_gemm_ab_impl.hpp:24-100, :480-582; sparse_gemm_ba_impl.hpp:25-99),
 * in the gather form the solver uses: out (k x ncols(B), ld ldo) = X (k x rows(B), ld ldx) * B, B = A (transposed == 0, i.e. W'A
 * from X = W') or B = A' (transposed != 0, i.e. (AH')' from X = H), on the kernel the solver takes at rank k.  reps > 0 and
 * avg_ms != NULL: that many more launches timed with HIP events. */
int smk_matrix_sparse_product(const smk_matrix* a, int transposed, int k, const double* X, int64_t ldx, double* out,
                              int64_t ldo, int reps, double* avg_ms);
int64_t smk_matrix_nnz(const smk_matrix* a);
int64_t smk_matrix_height(const smk_matrix* a);

/* ---- data that is already in device memory (a torch tensor: data_ptr(), stride(), the current stream) -------------------------
 * A view is a pointer, an element type and one stride per dimension IN ELEMENTS (>= 0; 0 only for inputs); any layout is taken,
 * row-major and column-major ones at copy rate.  `stream` is the HIP stream on which the caller produced the data or will consume
 * the result (0: the null stream): the entry records an event there, the library's stream waits for it, the work runs on the
 * library's stream, and the entry returns after that stream has been synchronised -- a source may be freed or overwritten, and an
 * output read from any stream, as soon as the call returns.  Checked before anything is launched (SMK_BAD_PARAM + smk_last_error):
 * null pointers, the element type, the strides, that the pointer is device memory of the current device, and that the strided
 * extent stays inside its allocation.
 * Rounding is that of smk_matrix_upload_f64 applied to the same values widened to fp64: to fp32 round-to-nearest-even, then (bf16
 * storage) to bf16 round-to-nearest-even; fp16 / bf16 sources widen exactly. */
enum { SMK_DT_F64 = 0, SMK_DT_F32 = 1, SMK_DT_BF16 = 2, SMK_DT_F16 = 3 };
enum { SMK_IDX_I32 = 0, SMK_IDX_I64 = 1 };
/* device twin of smk_matrix_upload_f64 (dense; `src` is the local height x ncols_local block): A and the stored transpose are
 * written from one read of the source */
int smk_matrix_adopt_device(smk_matrix* a, const void* src, int dtype, int64_t row_stride, int64_t col_stride, void* stream);
/* the stored values of a dense matrix into a strided device buffer (device twin of smk_matrix_download_f64) */
int smk_matrix_copy_to_device(const smk_matrix* a, void* dst, int dtype, int64_t row_stride, int64_t col_stride, void* stream);
/* CSC arrays in device memory: width + 1 offsets starting at 0, nnz row indices and values (fp64 / fp32 / bf16 / fp16).  A kernel
 * checks the index arrays (offsets monotone, spanning nnz and below 2^32; row indices < height) before anything consumes them; bad
 * arrays give SMK_BAD_PARAM.  The same matrix as smk_matrix_create_sparse on the same arrays. */
int smk_matrix_create_sparse_device(smk_matrix** out, int64_t height, int64_t width, int64_t nnz, const void* col_offsets, int idx_type,
                                    const void* row_indices, int row_idx_type, const void* values, int dtype, void* stream);
/* 1 when a rows x cols view with these strides, of elements of elem_size bytes, starting offset_bytes into an allocation of
 * alloc_bytes, stays inside it; 0 when it does not (or the arithmetic leaves 64 bits); the check behind the entries above */
int smk_strided_extent_fits(int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride, int64_t elem_size, int64_t offset_bytes,
                            int64_t alloc_bytes);

/* same generator on the host, for W0/H0 (RandomMatrix stand-in, smallk.cpp:533,554) */
void smk_uniform_fill_host(double* buf, int64_t ld, int64_t rows, int64_t cols, int64_t r0, int64_t c0,
                           int64_t global_height, uint64_t seed, int quant /* 0: 24 bit, 1: bf16 */);

/* ---- solver object = NmfSolve<> (common/include/nmf_solve_generic.hpp:34-140) ---------------- */
int smk_solver_create(smk_solver** out, const smk_options* opts, const smk_matrix* a);
void smk_solver_destroy(smk_solver* s);
/* W0 (m x k) and the local H0 shard (k x ncols_local); runs solver.Init + progress_est->Init (:62-63) */
int smk_solver_set_factors(smk_solver* s, const double* W0, int64_t ldW, const double* H0, int64_t ldH);
/* the same with W0 / H0 = the counter-based uniform matrices of smk_uniform_fill_host(seed_w) / (seed_h), generated on the device
 * (no host fill, no upload); unsharded solvers */
int smk_solver_set_factors_uniform(smk_solver* s, uint64_t seed_w, uint64_t seed_h);
/* the whole driver loop with stopping rule, final NormalizeAndScale, stats (:67-139) */
int smk_solver_run(smk_solver* s, smk_stats* stats);
/* enqueue `iters` solver iterations without convergence checks (the min_iter branch, :81-95);
 * asynchronous: returns before the GPU finishes. */
int smk_solver_iterate(smk_solver* s, int iters);
/* the same with the stopping rule's metric formed and read back after EVERY iteration, as NmfSolve<> does past min_iter
 * (common/include/nmf_solve_generic.hpp:98-121; gradients every iteration: nmf_solver_mu.hpp:151-164, nmf_solver_bpp.hpp:370-377),
 * never stopping: the per-iteration cost of the reference's default run.  MU / HALS / BPP.  last_metric may be NULL. */
int smk_solver_iterate_checked(smk_solver* s, int iters, double* last_metric);
int smk_solver_sync(smk_solver* s); /* wait + report solver failures (Result code) */
/* progress metric of the last iteration that computed one (PG ratio or delta-Fnorm) */
int smk_solver_progress(smk_solver* s, double* metric);
/* the four scalars of the check evaluated last, and pg0: the projected-gradient sums of W and of H (PG_RATIO), ||W - Wprev||^2 and
 * ||W||^2 (DELTA_FNORM; the pair the rule does not use reads 0), PG_RATIO's first norm.  Host state only: nothing is launched or
 * read.  SMK_BAD_PARAM before any check has been evaluated; SMK_UNSUPPORTED after a run the resident RANK2 kernel finished. */
int smk_solver_progress_sums(const smk_solver* s, double out5[5]);
/* optional final NormalizeAndScale (normalize.hpp:118-140), then copy factors to the host */
int smk_solver_get_factors(smk_solver* s, int normalize, double* W, int64_t ldW, double* H, int64_t ldH);
/* the same two with the factors in device memory (views as above; SMK_DT_F64 or SMK_DT_F32, fp32 output is the fp64 factor
 * rounded to nearest even): W is m x k, H is k x ncols_local */
int smk_solver_set_factors_device(smk_solver* s, const void* W0, int dtypeW, int64_t rsW, int64_t csW, const void* H0, int dtypeH,
                                  int64_t rsH, int64_t csH, void* stream);
int smk_solver_get_factors_device(smk_solver* s, int normalize, void* W, int dtypeW, int64_t rsW, int64_t csW, void* H, int dtypeH,
                                  int64_t rsH, int64_t csH, void* stream);
int smk_solver_iteration_count(const smk_solver* s);
/* the product form in use (SMK_NSPLIT numbering: 3 = bf16x3, 4 = fp16 two-term, 8 = the accurate fp64 form) and what the
 * opt-in run-time guard (BPP, SMK_GUARD_EVERY=n) has done so far: every n iterations it compares the fast form with the
 * accurate one on a column sample and changes to the accurate form when cond(Gram) x (product discrepancy) says one
 * iteration could move the factors by 1e-4 */
int smk_solver_product_form(const smk_solver* s, int* guard_checks, int* guard_fired, double* guard_last);

/* ---- the reconstruction error of a factorisation, on the device (the reference reports only its stopping-rule metric) --------
 * ||A - W H||_F^2 and ||A||_F^2 of the local columns of a resident matrix (dense or sparse), W m x k, H k x ncols_local;
 * col_resid_sq (ncols_local doubles, may be NULL): the same per column.  Stored values of A, fp64 throughout. */
int smk_matrix_residual(const smk_matrix* a, int k, const double* W, int64_t ldW, const double* H, int64_t ldH,
                        double* resid_sq, double* a_sq, double* col_resid_sq);
/* the same with the factors in device memory (views as for smk_solver_set_factors_device: SMK_DT_F64 / SMK_DT_F32, strides in
 * elements, the caller's stream); col_resid_sq: ncols_local contiguous fp64 in device memory, or NULL */
int smk_matrix_residual_device(const smk_matrix* a, int k, const void* W, int dtypeW, int64_t rsW, int64_t csW,
                               const void* H, int dtypeH, int64_t rsH, int64_t csH, void* stream,
                               double* resid_sq, double* a_sq, void* col_resid_sq);
/* of the solver's current factors on its matrix; the solver is left exactly as it was */
int smk_solver_residual(smk_solver* s, double* resid_sq, double* a_sq, double* col_resid_sq);

/* ---- truncated SVD and the NNDSVD start (Boutsidis & Gallopoulos 2008), on the device -------------------------------------------
 * A randomised range finder with power iterations (Halko, Martinsson, Tropp), fp64 against the stored values of A, the same bits
 * on every call.  l = min(k + oversample, m, n) columns are carried; k + oversample <= 128.
 * oversample / power_iters < 0: the defaults (8 / 2).  omega: NULL (the test matrix is drawn from `seed`), or the caller's test
 * matrix, an n x l view in device memory (SMK_DT_F64 / SMK_DT_F32, strides in elements).
 * SMK_BAD_PARAM: k < 1, k > min(m, n), a bad omega.  SMK_UNSUPPORTED: k + oversample > 128, a column shard, a single-copy dense
 * matrix (its transpose is NOT built behind the caller's back), a solver with a communicator. */
typedef struct smk_svd_options {
    int k, oversample, power_iters;
    uint64_t seed;
    const void* omega;
    int omega_dtype;
    int64_t omega_rs, omega_cs;
} smk_svd_options;
enum { SMK_NNDSVD = 0, SMK_NNDSVDA = 1 };       /* nndsvda: every zero of the start is replaced by mean(A) */
/* A ~ U diag(S) V': U m x k and V n x k views in device memory (SMK_DT_F64 / SMK_DT_F32, the caller's stream), S_host k doubles,
 * largest first.  A triplet past the numerical rank of A comes back as S = 0 with zero vectors.  No sign convention. */
int smk_matrix_svd_device(const smk_matrix* a, const smk_svd_options* opts, void* U, int dtypeU, int64_t rsU, int64_t csU,
                          double* S_host, void* V, int dtypeV, int64_t rsV, int64_t csV, void* stream);
/* the NNDSVD start built from that SVD: W m x k, H k x n */
int smk_matrix_nndsvd_device(const smk_matrix* a, const smk_svd_options* opts, int variant, void* W, int dtypeW, int64_t rsW,
                             int64_t csW, void* H, int dtypeH, int64_t rsH, int64_t csH, void* stream);
/* the same start as the solver's initial factors (opts->k is ignored: the solver's k); leaves the solver exactly as
 * smk_solver_set_factors_device would with those factors.  opts may be NULL (all defaults, seed 0). */
int smk_solver_set_factors_nndsvd(smk_solver* s, const smk_svd_options* opts, int variant);
/* diagnostics of the calling thread's last SVD / NNDSVD call: the Gram matrices that went to the host for their eigendecomposition
 * and the host time those decompositions took (tools/svd_rate.py) */
int smk_svd_last_profile(int* host_trips, double* host_ms);

/* ---- regularised NMF by cyclic coordinate descent: scikit-learn's solver="cd" without the shuffle, on the device -----------------
 * Minimises  1/2 ||A - W H||_F^2 + n alpha_w rho ||W||_1 + m alpha_h rho ||H||_1 + 1/2 n alpha_w (1 - rho) ||W||_F^2
 *            + 1/2 m alpha_h (1 - rho) ||H||_F^2                  (A m x n, W m x k, H k x n, rho = l1_ratio)
 * which is sklearn.decomposition.NMF on X = A' with alpha_W = alpha_h, alpha_H = alpha_w, W_sklearn = H', components_ = W'.
 * One iteration sweeps H (G = W'W, R = W'A), then W with the new H (G = HH', R = (AH')'), every coordinate in order; its violation
 * is the sum of |projected gradient| over both sweeps.  Stop when violation_init (that of iteration 1) is 0 or
 * violation / violation_init <= tol, else after max_iter iterations.  No normalisation.  update_w = 0: W stays as given, W'W and
 * W'A are formed once and only the H sweep repeats (fold-in of new columns).  fp64 against the stored values of A (dense: the
 * accurate-form product); the same bits on every call.  The host reads the violation once per iteration.
 * SMK_BAD_PARAM: a null pointer, k < 1, k > min(m, n), a negative alpha, l1_ratio outside [0, 1], tol < 0, max_iter < 1, a bad
 * view.  SMK_UNSUPPORTED: k > 128, a column shard, a single-copy dense matrix (its transpose is NOT built behind the caller's
 * back).  On an error W and H are untouched. */
typedef struct smk_cd_options { double alpha_w, alpha_h, l1_ratio, tol; int max_iter; int update_w; } smk_cd_options;
typedef struct smk_cd_stats   { int iterations; int converged; double violation_init, violation; } smk_cd_stats;
/* W (m x k) and H (k x ncols) are in/out views in device memory (SMK_DT_F64 / SMK_DT_F32, strides in elements, the caller's stream) */
int smk_nmf_cd_device(const smk_matrix* a, int k, const smk_cd_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                      void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_cd_stats* stats);
/* one sweep by itself, host fp64 arrays, as smk_nnls_blockpivot stands by itself: G k x k (G[t, r] at G[r * ldG + t]), R k x ncols,
 * X k x ncols in/out, column-major; for every column and t = 0 .. k-1 in order, with G' = G + l2 I and R' = R - l1:
 * grad = sum_r G'[t, r] x[r] - R'[t]; *violation += |x[t] == 0 ? min(0, grad) : grad|; x[t] = max(x[t] - grad / G'[t, t], 0)
 * unless G'[t, t] == 0.  k <= 128. */
int smk_cd_sweep(int k, int64_t ncols, const double* G, int64_t ldG, const double* R, int64_t ldR, double* X, int64_t ldX,
                 double l1, double l2, double* violation);
/* diagnostics of the calling thread's last smk_nmf_cd_device call: passes over A and sweeps launched */
int smk_cd_last_profile(int* products, int* sweeps);
/* measurement (tools/cd_rate.py): the average time in ms of `reps` launches of one sweep kernel on synthetic data, k x ncols, R
 * read as `slabs` partial products.  which: 0 the coordinate-descent sweep, 1 its maintained-gradient form, 2 the HALS H sweep,
 * 3 the reduction of the partial products alone.  *checksum: the violation of the last launch (which 0 / 1), else 0. */
int smk_cd_sweep_time(int which, int k, int64_t ncols, int slabs, int reps, double* ms, double* checksum);

/* ---- NMF of a sparse matrix under the generalised Kullback-Leibler divergence, by multiplicative updates ---------
 * scikit-learn's solver="mu" with beta_loss="kullback-leibler" on X = A': W_sklearn = H', components_ = W', sklearn's alpha_W is
 * alpha_h here and its alpha_H is alpha_w; l1 / l2 of H = m alpha_h l1_ratio / m alpha_h (1 - l1_ratio), of W = n alpha_w l1_ratio /
 * n alpha_w (1 - l1_ratio).  With EPS = 2^-23, over the stored entries (i, j, a) of A, one iteration is
 *   H[t, j] *= (sum over column j of a / max(w_i . h_j, EPS) W[i, t]) / (sum_i W[i, t] + l1 + l2 H[t, j])
 *   W[i, t] *= (sum over row i of a / max(w_i . h_j, EPS) H[t, j]) / (s_t + l1 + l2 W[i, t]),  s_t = sum_j H[t, j], 0 -> 1.0
 * each penalty added only if > 0, a zero denominator replaced by EPS, W below 2^-52 set to 0.  error = sqrt(2 max(D, 0)),
 * D = sum a log(a / max(w_i . h_j, EPS)) - sum a + (sum_i w_i) . (sum_j h_j); error_init is taken before iteration 1; when tol > 0
 * the error is taken at iterations 10, 20, ... and the run stops when (previous error - error) / error_init < tol, else after
 * max_iter iterations.  stats->error is that of the factors returned.  update_w = 0: W stays as given and only the H step repeats
 * (fold-in of new columns).  fp64, every sum in a fixed order: the same bits on every call.  The host reads the device on check
 * iterations only.
 * SMK_BAD_PARAM: a null pointer, k < 1, k > min(m, n), a negative alpha, l1_ratio outside [0, 1], tol < 0, max_iter < 1, a bad view,
 * a negative stored value.  SMK_UNSUPPORTED: a dense matrix, k > 128, a column shard, a matrix that stores an entry twice (the
 * divergence is not linear in a).  On an error W and H are untouched. */
typedef struct smk_kl_options { double alpha_w, alpha_h, l1_ratio, tol; int max_iter; int update_w; } smk_kl_options;
typedef struct smk_kl_stats   { int iterations; int converged; double error_init, error; } smk_kl_stats;
/* W (m x k) and H (k x ncols) are in/out views in device memory (SMK_DT_F64 / SMK_DT_F32, strides in elements, the caller's stream) */
int smk_nmf_kl_device(const smk_matrix* a, int k, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                      void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats);
/* out[0] = D (not clamped), out[1] = sum a log(a / max(w_i . h_j, EPS)), out[2] = sum WH of the given factors (views as above, only
 * read); the error returns of smk_nmf_kl_device that apply */
int smk_matrix_kl_divergence_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW,
                                    const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out);
/* diagnostics of the calling thread's last smk_nmf_kl_device call: sweeps over the stored entries that updated a factor, and
 * sweeps that formed the divergence */
int smk_kl_last_profile(int* entry_passes, int* divergence_passes);
/* measurement (tools/kl_rate.py): the average time in ms of `reps` launches on synthetic factors of rank k.  which: 0 the H step
 * (the quotient gather over CSC(A) with its update), 1 the W step (over CSC(A')), 2 / 3 the plain gather product launch_spmm_seg on
 * the same plan, rank and gathered factor as 0 / 1: one gather of the same rows without the dot product and the quotient */
int smk_kl_step_time(const smk_matrix* a, int which, int k, int reps, double* ms);

/* ---- NMF fitted to the stored entries of a sparse matrix only: masked coordinate descent --------------------------
 * An entry that the matrix does not store is "not measured" (a missing rating, a clipped bin, an entry held out on purpose), not 0.
 * Omega = the stored entries (i, j, a), stored zeros included.  Minimises  1/2 sum over Omega of (a - w_i . h_j)^2  plus the penalty
 * terms of smk_nmf_cd_device, with its orientation, options, penalty scaling and stopping rule.  One iteration sweeps H, then W with
 * the new H.  The H sweep takes every column j by itself and t = 0 .. k-1 in order, the residuals r = a - w_i . h_j of the column's
 * entries kept current:  grad = -sum W[i, t] r + l1 + l2 H[t, j],  hess = sum W[i, t]^2 + l2  (sums over the stored entries of column
 * j);  violation += |H[t, j] == 0 ? min(0, grad) : grad|;  unless hess == 0, H[t, j] = max(H[t, j] - grad / hess, 0).  A column
 * without stored entries follows the same formulas.  The W sweep is the same over the rows.  When every entry is stored this is
 * smk_nmf_cd_device's iteration up to rounding.  update_w = 0: W stays as given and only the H sweep repeats (fold-in of new
 * columns).  stats->error = sqrt(sum over Omega of (a - w_i . h_j)^2) of the factors returned.  fp64, every sum in a fixed order: the
 * same bits on every call.  The host reads the violation once per iteration.
 * SMK_BAD_PARAM: a null pointer, k < 1, k > min(m, n), a negative alpha, l1_ratio outside [0, 1], tol < 0, max_iter < 1, a bad view.
 * SMK_UNSUPPORTED: a dense matrix, k > 128, a column shard, a matrix that stores an entry twice (the mask is then not a set),
 * SMK_SPMM_SEG_LEN above 64.  Negative stored values are served, as by smk_nmf_cd_device.  On an error W and H are untouched. */
typedef struct smk_masked_stats { int iterations; int converged; double violation_init, violation, error; } smk_masked_stats;
/* W (m x k) and H (k x ncols) are in/out views in device memory (SMK_DT_F64 / SMK_DT_F32, strides in elements, the caller's stream) */
int smk_nmf_masked_device(const smk_matrix* a, int k, const smk_cd_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                          void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_masked_stats* stats);
/* out3[0] = sum over the stored entries of `a` of (a - w_i . h_j)^2, out3[1] = that of a^2, out3[2] = their number, of the given
 * factors (views as above, only read): the held-out score when `a` holds the entries withheld from the fit.  col_r / col_a (both or
 * neither): ncols doubles each in device memory, the first two sums per column.  The error returns of smk_nmf_masked_device that apply */
int smk_matrix_masked_residual_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW,
                                      const void* H, int dtH, int64_t rsH, int64_t csH, double* col_r, double* col_a, void* stream,
                                      double* out3);
/* diagnostics of the calling thread's last smk_nmf_masked_device call: sweeps over the stored entries that updated a factor, and
 * sweeps that formed the residual */
int smk_masked_last_profile(int* entry_sweeps, int* residual_sweeps);
/* measurement (tools/masked_rate.py): the average time in ms of `reps` launches on synthetic factors of rank k.  which: 0 the H sweep
 * (over CSC(A)), 1 the W sweep (over CSC(A')), 2 the H step of smk_nmf_kl_device on the same matrix and rank, 3 the plain gather product
 * launch_spmm_seg on the same plan: one gather of the same rows without the coordinate chain */
int smk_masked_step_time(const smk_matrix* a, int which, int k, int reps, double* ms);

/* ---- the same iteration on a DENSE resident matrix: the sums run over every entry of the stored matrix (bf16 or fp32
 * storage, widened exactly; a stored 0 contributes nothing), so on the same data the result is smk_nmf_kl_device's up to summation
 * order.  Each half-iteration is one streaming read of one stored copy: A for H, the stored transpose for W; two chained fp64
 * matrix-core contractions per tile, no m x n temporary.  Options, statistics, views and the stopping rule are smk_nmf_kl_device's.
 * SMK_BAD_PARAM: as there (a negative stored value included).  SMK_UNSUPPORTED: a sparse matrix, k > 128, a column shard, and a
 * single-copy matrix when update_w != 0 (the W step needs the stored transpose; the fold-in on a single copy is served).  On an
 * error W and H are untouched. */
int smk_nmf_kl_dense_device(const smk_matrix* a, int k, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                            void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats);
/* out[0 .. 2] as smk_matrix_kl_divergence_device, over every entry with a > EPS; one read of A, a single copy is served */
int smk_matrix_kl_divergence_dense_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW,
                                          const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out);
/* diagnostics of the calling thread's last smk_nmf_kl_dense_device call: streaming passes over A or A' that updated a factor, and
 * passes over A that formed the divergence */
int smk_kl_dense_last_profile(int* matrix_passes, int* divergence_passes);
/* measurement (tools/kl_dense_rate.py): the average time in ms of `reps` launches on synthetic factors of rank k.  which: 0 the H
 * step with its finish (over A), 1 the W step with its finish (over the stored transpose), 2 the residual pass of
 * smk_matrix_residual on A at the same rank: one product over the same bytes, the floor to compare with */
int smk_kl_dense_step_time(const smk_matrix* a, int which, int k, int reps, double* ms);

/* ---- NMF of a resident DENSE matrix under another beta-divergence, by multiplicative updates -------------------
 * smk_nmf_kl_dense_device for any beta >= 0 other than 2: scikit-learn's NMF(solver="mu", beta_loss=beta) on X = A', beta = 0 being
 * "itakura-saito" -- the loss of a power spectrogram.  Options, orientation, penalties, stopping rule, fold-in and results are
 * smk_nmf_kl_device's; stats->error = sqrt(2 D_beta(A || W H)).  Per entry of the stored A with d = w_i . h_j the numerator takes
 * a d^(beta - 2) and the denominator d^(beta - 1) (d clamped at 2^-23 from below where the exponent is negative), the quotient of
 * the two sums is raised to gamma = 1 / (2 - beta) below beta = 1, 1 / (beta - 1) above 2 and 1 between, and factor entries below
 * 2^-52 become zero when beta < 1.  Each half-iteration is one streaming read of one stored copy and forms both sums on the matrix
 * cores; beta = 0 costs divisions only, any other beta one double-precision pow per entry and half-iteration (DESIGN.md 21 has
 * the measured cost).  beta = 1 forwards to smk_nmf_kl_dense_device: the same bits.  The same bits on every run.
 * SMK_BAD_PARAM: as smk_nmf_kl_dense_device, a beta that is negative or not finite, a negative stored value, and for beta <= 0 a
 * stored zero (add a small value to the matrix, or use a positive beta).  SMK_UNSUPPORTED: beta = 2 (the Frobenius solvers:
 * smk_nmf_run, smk_nmf_cd_device), a sparse matrix, k > 128, a column shard, a single-copy matrix when update_w != 0.  On an error
 * W and H are untouched. */
int smk_nmf_beta_dense_device(const smk_matrix* a, int k, double beta, const smk_kl_options* o, void* W, int dtW, int64_t rsW,
                              int64_t csW, void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats);
/* out[0] = D_beta(A || W H) (not clamped) over the entries with a > 2^-23, then the sums it is formed from.  beta = 0: out[1] =
 * sum a / d, out[2] = sum log(a / d), out[3] = m n, D = out[1] - out[3] - out[2].  Other beta: out[1] = sum a^beta, out[2] =
 * sum a d^(beta - 1), out[3] = sum d^beta over every entry, D = (out[1] - beta out[2] + (beta - 1) out[3]) / (beta (beta - 1)).
 * beta = 1: smk_matrix_kl_divergence_dense_device's three numbers and out[3] = 0.  One read of A; a single copy is served. */
int smk_matrix_beta_divergence_dense_device(const smk_matrix* a, int k, double beta, const void* W, int dtW, int64_t rsW,
                                            int64_t csW, const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out);
/* diagnostics of the calling thread's last smk_nmf_beta_dense_device call (beta != 1), as smk_kl_dense_last_profile */
int smk_beta_dense_last_profile(int* matrix_passes, int* divergence_passes);
/* measurement (tools/beta_dense_rate.py), as smk_kl_dense_step_time.  which: 0 the H step with its finish (over A), 1 the W step
 * (over the stored transpose), 2 the KL step of kl_dense.hip on the same matrix and rank, 3 the residual pass.  beta != 1 */
int smk_beta_dense_step_time(const smk_matrix* a, int which, int k, double beta, int reps, double* ms);

/* ---- labels, memberships, top terms and fold-in, on the device (the device twins of smk_compute_assignments,
 * smk_compute_fuzzy_assignments and smk_top_terms below: the same comparisons in the same order, so the same integers and the
 * same membership bits; no k <= n and no height >= width requirement) -----------------------------------------------------
 * H: k x n view in device memory (SMK_DT_F64 / SMK_DT_F32, strides in elements, the caller's stream).
 * labels: n uint32; memberships: k*n float, document c at c*k, or NULL -- both device memory */
int smk_labels_device(const void* H, int dtype, int64_t rsH, int64_t csH, int k, int64_t n, void* stream,
                      void* labels, void* memberships);
/* W: m x k view.  term_indices: maxterms*k int32 in device memory, topic j at j*maxterms; min(maxterms, m) slots per topic are
 * written, in the order d[a] > d[b] || (d[a] == d[b] && a < b).  Any maxterms (above 256: a radix sort per topic). */
int smk_top_terms_device(const void* W, int dtype, int64_t rsW, int64_t csW, int64_t m, int k, int maxterms,
                         void* stream, void* term_indices);
/* the same on a solver's resident factors, no copy of H / W; normalize as in smk_solver_get_factors */
int smk_solver_labels(smk_solver* s, int normalize, void* stream, void* labels, void* memberships);
int smk_solver_top_terms(smk_solver* s, int normalize, int maxterms, void* stream, void* term_indices);
/* H := argmin_{H >= 0} ||A - W H||_F with the solver's W fixed: one exact block-pivoting solve (BPP solvers, unsharded), warm
 * start = the current H.  W, the normalisation state of W and the iteration count stay.  SMK_FAILURE: the reference's `false`
 * (rank-deficient W). */
int smk_solver_project_h(smk_solver* s);

/* bool NnlsBlockpivot(LHS, RHS, X, Y), common/include/nnls.hpp:144-244, by itself (the reference's
 * tests/src/test_bpp.cpp drives the solver this way): LHS k x k SPD, RHS k x ncols, X in/out (warm start:
 * passive set = X > 0), Y = LHS X - RHS out (may be NULL).  SMK_FAILURE = the reference's `false`
 * (pivot limit 5k reached, or a passive block that is not positive definite). */
int smk_nnls_blockpivot(int k, int64_t ncols, const double* LHS, int64_t ldL, const double* RHS, int64_t ldR,
                        double* X, int64_t ldX, double* Y, int64_t ldY);

/* measurement: HIP events around the streaming-product launches (stream of the solver).  A pair of event records costs
 * ~11 us of idle time around the launch, so passes over less than 1 GB are timed one launch in 16 and the totals scaled
 * back up (SMK_TIMING_STRIDE overrides) */
int smk_solver_enable_timing(smk_solver* s, int on);
/* which: 0 = W'A pass, 1 = H*At pass (a pass that the multi-GPU schedule cuts into chunks counts as ONE launch per group of
 * 64 factor rows; its time is the sum of its chunk launches), 2 = the per-chunk collectives of a sharded run, timed on the
 * collective stream (the sums of (AH')' and, BPP, the all-gathers of the packed W); 3 = the time the MAIN stream stood waiting
 * for events of the collective stream (each wait bracketed by two events on the main stream: the measured, not inferred, exposed
 * part of the exchange); 4 = the same bracket around a wait for an event that completed long ago (what a bracket costs by itself,
 * ~15 us: subtract brackets x its average from slot 3); 5 = the block-pivoting (NNLS) launches of BPP, sampled with the passes.
 * Total ms and count since enable. */
int smk_solver_kernel_time(smk_solver* s, int which, double* total_ms, int* launches);
/* name of the kernel pass `which` (0 = W'A, 1 = H*At) launches for this solver -- the streaming product and its variant, or which of the
 * sparse gather products the plan chose (spmm_seg_kernel on ragged columns, spmm_gather_kernel on fixed-degree graphs, ...): what
 * bench.py attributes `roofline.achieved` to.  which = 2: how the stopping-rule checks of this solver were formed so far, with counts
 * (launches of their own, or riding in the next iteration's NNLS launch and pass: DESIGN.md 6) */
int smk_solver_kernel_name(const smk_solver* s, int which, char* out, int cap);
/* diagnostics of the block-pivoting kernels (csrc/nnls.hip), live only in a process started with SMK_NNLS_STATS=1 (else
 * SMK_UNSUPPORTED): 256 counters -- [0..15] exchanges per column (nnls.hpp:192-241 trips), [16..80] size of a column's first
 * compact solve, [96..160] of its later ones, [176] / [177] solves in the complement / direct form, [178] columns, [179] / [180]
 * solves with all / no variables passive.  Synchronises the device.  reset != 0 clears the counters after the read. */
int smk_debug_nnls_stats(unsigned long long* out256, int reset);
/* algorithmic bytes / flops one launch of pass `which` moves (len*ncols*sizeof(elt), 2*k*len*ncols) */
int smk_solver_kernel_work(const smk_solver* s, int which, double* bytes, double* flops);

/* ---- multi-GPU: A and H column sharded, W replicated in the algorithm.  Exchange steps per iteration:
 *   - sum-all-reduce of HH' (k x k, fp64), beside the H*At pass;
 *   - the sum of H*At = (AH')' (k x m; fp64 on the wire, SMK_COMM_F64=0: fp32): the pass runs in row chunks and the
 *     sum of chunk j travels while the product streams chunk j + 1 -- an all-reduce for MU / HALS (replicated W
 *     update), a reduce-scatter for BPP, whose W rows are independent NNLS problems: block r of every chunk belongs
 *     to rank r (block-cyclic), every rank solves its own blocks;
 *   - BPP: sum-all-reduce of W'W (k x k) built from the own blocks, and an all-gather per chunk of the PACKED
 *     streaming operand of those blocks (4 B per entry in the fp16 form; the fp64 rows are gathered only when results
 *     or the DELTA_FNORM rule need them); the W'A pass then runs chunk by chunk down the rows as the operand lands;
 *   - one 3-element all-reduce when the stopping rule is evaluated.
 * All of them are issued from C on ONE second HIP stream per solver (a communicator is never driven from two streams)
 * and tied to the main stream by events.  Communicators:
 *   - RCCL over xGMI: one process per GPU (smk_comm_unique_id on rank 0, broadcast the 128 bytes by any means,
 *     smk_comm_init_rank everywhere) or one process driving several GPUs (smk_comm_init_all, one host thread per
 *     device -- what smk_nmf_dense_sharded does);
 *   - an in-process stand-in with the same semantics for several shards on ONE device (smk_comm_init_local: RCCL
 *     refuses two ranks on a device), used by the tests and by boxes with fewer GPUs than shards.
 * Environment: SMK_COMM_CHUNKS=1..8 (row chunks of the exchange; default: blocks of >= 4096 rows, at most 4 chunks),
 * SMK_COMM_F64=0 (fp32 on the wire), SMK_COMM_FORCE=1 (a world of ONE rank issues every collective too: tests of the real nccl* calls).
 * The reference has no distributed mode (sphinx/source/pages_installation.rst:38). */
typedef struct smk_comm smk_comm;
int smk_comm_unique_id(void* id128 /* 128 bytes out */);
int smk_comm_init_rank(smk_comm** out, const void* id128, int rank, int world);   /* on the CURRENT HIP device */
int smk_comm_init_all(smk_comm** out /* ndev handles */, int ndev, const int* devices /* NULL: 0..ndev-1 */);
int smk_comm_init_local(smk_comm** out /* nranks handles */, int nranks);
/* every rank calls it: known values through an all-reduce (fp64, fp32), an all-gather and a reduce-scatter, checked on the host */
int smk_comm_selftest(smk_comm* c);
int smk_comm_rank(const smk_comm* c);
int smk_comm_world(const smk_comm* c);
void smk_comm_destroy(smk_comm* c);
/* a rank that gives up calls this so that peers blocked in a collective are released (ncclCommAbort / the stand-in's
 * failure flag); the handle is still destroyed with smk_comm_destroy */
void smk_comm_abort(smk_comm* c);
/* attach before smk_solver_set_factors(); the communicator must outlive the solver */
int smk_solver_attach_comm(smk_solver* s, smk_comm* comm);
/* Result Nmf(...) (common/src/nmf.cpp:173-229) on `nshards` column shards, one host thread and one device per shard;
 * devices NULL: shard r on device r; local_stub != 0: all shards on the current device through the stand-in. */
int smk_nmf_dense_sharded(const smk_options* opts, const double* A, int64_t ldA, double* W, int64_t ldW, double* H,
                          int64_t ldH, smk_stats* stats, int storage, int nshards, const int* devices, int local_stub);

/* Test hook kept from round 1: the host supplies the all-reduce (e.g. torch.distributed on gloo);
 * `ptr` is device memory inside the registered workspace. */
typedef int (*smk_allreduce_fn)(void* user, void* ptr, int64_t count, int dtype /*0 f32, 1 f64*/);
int smk_solver_comm_workspace_bytes(const smk_solver* s, size_t* bytes);
int smk_solver_set_comm(smk_solver* s, int rank, int world, smk_allreduce_fn fn, void* user,
                        void* workspace, size_t workspace_bytes);

/* ---- HierNMF2: rank-2 hierarchical clustering --------------------------------------
 * Clust / ClustSparse (hierclust/include/clust.hpp:45-58, hierclust/src/clust.cpp:97-203) with
 * ClustOptions (clust.hpp:27-37), ClustStats (:20-25) and the result Tree<T> (hierclust/include/tree.hpp).
 * Every node factorisation is the RANK2 solver above on a column subset of the resident A
 * (SubMatrixColsCompact). */
typedef struct smk_clust_options {
    smk_options nmf;       /* height/width = A's; k, algorithm are forced to 2 / RANK2 */
    int maxterms;
    double unbalanced;     /* [0, 1) */
    int trial_allowance;
    int num_clusters;      /* >= 2 */
    int verbose;
    int flat;              /* also run ClustFlat (clust_flat_generic.hpp:33-74) on the leaves */
} smk_clust_options;
typedef struct smk_clust_stats { int nmf_count; int max_count; } smk_clust_stats;
typedef struct smk_tree smk_tree;
typedef struct smk_tree_node {
    double priority;
    unsigned parent, left_child, right_child;   /* SMK_TREE_NONE when absent */
    int is_valid, is_left_child, is_leaf;
    int64_t doc_count;
} smk_tree_node;
#define SMK_TREE_NONE 0xFFFFFFFFu

int smk_clust_is_valid(const smk_clust_options* opts, int validate_matrix);   /* clust_options.cpp:16-110 */
/* column subset of a resident matrix (dense: all rows kept; sparse: unused rows dropped, the kept
 * rows are listed in new_to_old_rows[0 .. *new_height), capacity = height). */
int smk_matrix_gather_cols(const smk_matrix* src, const unsigned* cols, int64_t ncols, smk_matrix** out,
                           unsigned* new_to_old_rows, int64_t* new_height);
/* Returns SMK_OK, or SMK_FLATCLUST_FAILURE with *tree still valid (opts.flat and the flat step failed:
 * fewer leaves than clusters, or NnlsHals did not converge), or an error with *tree == NULL.
 * Random initialisers: matrix i of the run is the counter-based uniform block with seed
 * `seed + 0x9E37 * (++*draws)` (W then H per attempt); `initdir` non-empty: Winit_<i>.csv / Hinit_<i>.csv
 * (full size, i = 1, 2, ...; clust_hier_util.hpp:206-241) are used instead.  `draws` may be NULL. */
int smk_clust_dense(const smk_clust_options* opts, const double* A, int64_t ldA, int storage, uint64_t seed,
                    uint64_t* draws, const char* initdir, smk_tree** tree, smk_clust_stats* stats);
int smk_clust_sparse(const smk_clust_options* opts, int64_t nnz, const unsigned* col_offsets,
                     const unsigned* row_indices, const double* data, uint64_t seed, uint64_t* draws,
                     const char* initdir, smk_tree** tree, smk_clust_stats* stats);
/* on a matrix that already lives in HBM (smk_matrix_create[_sparse]); options height/width must match it */
int smk_clust_resident(const smk_clust_options* opts, const smk_matrix* a, uint64_t seed, uint64_t* draws,
                       const char* initdir, smk_tree** tree, smk_clust_stats* stats);
void smk_tree_destroy(smk_tree* t);
int smk_tree_node_count(const smk_tree* t);
int64_t smk_tree_term_count(const smk_tree* t);
int64_t smk_tree_doc_count(const smk_tree* t);
int smk_tree_get_node(const smk_tree* t, int q, smk_tree_node* out);
int smk_tree_node_docs(const smk_tree* t, int q, unsigned* out /* doc_count */);
int smk_tree_node_topic(const smk_tree* t, int q, double* out /* term_count */);
int smk_tree_node_terms(const smk_tree* t, int q, int* out /* maxterms */);   /* returns entries written */
int64_t smk_tree_assignments(const smk_tree* t, unsigned* out /* doc_count; SMK_TREE_NONE = outlier */);
int64_t smk_tree_outliers(const smk_tree* t, unsigned* out /* NULL: count only */);
int smk_tree_write_assignments(const smk_tree* t, const char* path);            /* tree.hpp:388-423 */
/* format 0 = XML, 1 = JSON (hierclust_xml_writer.cpp / hierclust_json_writer.cpp, byte compatible) */
int smk_tree_write(const smk_tree* t, const char* path, int format, const char* const* dictionary,
                   int64_t dictionary_size);
/* opts.flat: the flat factors (W m x num_clusters, H num_clusters x n) computed after the tree search */
int smk_tree_flat_factors(const smk_tree* t, double* W, int64_t ldW, double* H, int64_t ldH);
/* the priority score of a split: compute_priority(), clust_hier_util.hpp:105-173 */
double smk_clust_priority(const double* w_parent, const double* w_child /* n x 2, ld n */, int64_t n);

/* ---- new documents down a fitted tree, on the device (tree_route.cpp) -----------------------------------------
 * The rule is the training code's (tree_partition): at a split with child topic vectors w_l, w_r document a goes left iff h0 > h1,
 * (h0, h1) = argmin_{h >= 0} ||a - [w_l w_r] h||, the closed-form rank-2 solve.  A router holds, per pair of siblings, the two
 * topic vectors interleaved in device memory: pairs * m * 16 bytes (an 8-leaf tree has 7 pairs: 112 MB over 10^6 terms).
 * A structure is the forest HierNMF2 produces: roots are nodes 0 and 1; a valid node has both children SMK_TREE_NONE (a leaf) or two
 * valid children below node_count; no node is reached twice from the roots (no second parent, no cycle); invalid or unreachable nodes
 * are ignored.  valid may be NULL (every node valid).  Anything else: SMK_BAD_PARAM, smk_last_error names the node.
 * smk_tree_router_check is host code and needs no initialised device: pairs = splits + the root pair, max_depth = decisions on the
 * longest descent. */
typedef struct smk_tree_router smk_tree_router;
int smk_tree_router_check(int node_count, const unsigned* left, const unsigned* right, const int* valid, int* pairs, int* max_depth);
/* topics_host: m x node_count fp64, column-major with ld doubles per column, on the host (column q = the topic vector of node q).
 * SMK_BAD_PARAM: a null pointer, m < 1, ld < m, a bad structure.  SMK_FAILURE: the 2 x 2 Gram matrix of a reachable pair is singular
 * by the rank-2 solve's own test (a zero topic vector, for example); the message names the pair.  SMK_DEVICE_ERROR: no memory. */
int smk_tree_router_create(int64_t m, int node_count, const unsigned* left, const unsigned* right, const int* valid,
                           const double* topics_host, int64_t ld, smk_tree_router** router);
/* the same router from a fitted tree, read through smk_tree_get_node / smk_tree_node_topic */
int smk_tree_router_from_tree(const smk_tree* t, smk_tree_router** router);
void smk_tree_router_destroy(smk_tree_router* r);
/* every output may be NULL; table_bytes = pairs * m * 16 */
int smk_tree_router_sizes(const smk_tree_router* r, int64_t* m, int* node_count, int* pairs, int* max_depth, int64_t* table_bytes);
/* the arrays create took, bit for bit (node_count entries each, topics with ld doubles per column): what a saved router keeps */
int smk_tree_router_download(const smk_tree_router* r, unsigned* left, unsigned* right, int* valid, double* topics_host, int64_t ld);
/* The columns of A_new (a resident SPARSE matrix with m rows) down the tree, one launch, synchronous.  Outputs in device memory, n =
 * columns of A_new entries each: leaf (int32: the node the document ends at, in the tree's own numbering -- smk_tree_assignments'
 * -- and never SMK_TREE_NONE: training outliers are a property of the search, not of this rule), depth (int32, may be NULL:
 * decisions taken), h (fp64, 2 per document, may be NULL: (h0, h1) of the last decision).  A document without entries goes right at
 * every level.  The same bits on every run.  stream: the caller's (the library's stream waits for it).  SMK_UNSUPPORTED: a dense
 * A_new, a column shard.  SMK_BAD_PARAM: a null pointer, A_new's height is not m, an output that is not device memory of n entries.
 * The outputs are written on success only. */
int smk_tree_route_device(const smk_tree_router* r, const smk_matrix* A_new, void* stream, void* leaf, void* depth, void* h);
/* diagnostics of the calling thread's last successful smk_tree_route_device call: kernel launches, stored entries they walked */
int smk_tree_route_last_profile(int* launches, int64_t* entries);
/* measurement (tools/route_rate.py): the average time in ms of `reps` routing launches into a workspace */
int smk_tree_route_time(const smk_tree_router* r, const smk_matrix* A_new, int reps, double* ms);

/* ---- flat clustering ------------------------------------------------------------------
 * FlatClust / FlatClustSparse (flatclust/include/flat_clust.hpp, flatclust/src/flat_clust.cpp:118-264):
 * NmfSolve<> restricted to HALS / RANK2 / BPP; same argument meaning as smk_nmf_dense / smk_nmf_sparse. */
int smk_flatclust_dense(const smk_options* opts, const double* A, int64_t ldA, double* W, int64_t ldW, double* H,
                        int64_t ldH, smk_stats* stats, int storage);
int smk_flatclust_sparse(const smk_options* opts, unsigned height, unsigned width, unsigned nz,
                         const unsigned* col_offsets, const unsigned* row_indices, const double* data, double* W,
                         int64_t ldW, double* H, int64_t ldH, smk_stats* stats);
/* NnlsHals (common/include/nnls.hpp:249-316): H-only HALS sweeps with W fixed, until
 * PG(H) < tol * PG(H after sweep 1); normalises W, H on success.  SMK_FAILURE at the iteration limit. */
int smk_solver_nnls_hals(smk_solver* s, double tol, int verbose, int max_iter, int* iterations);
/* assignments.hpp:32-113, terms.hpp:62-108 (host post-processing of the returned factors) */
int smk_compute_assignments(const double* H, unsigned ldH, unsigned k, unsigned n, unsigned* labels /* n */);
int smk_compute_fuzzy_assignments(const double* H, unsigned ldH, unsigned k, unsigned n, float* probabilities);
int smk_top_terms(int maxterms, const double* W, unsigned ldim, unsigned height, unsigned width,
                  int* term_indices /* maxterms * width */);
/* common/src/assignments.cpp:23-70; return 1 on success like the reference's bool */
int smk_write_assignments_file(const unsigned* labels, unsigned n, const char* path);
int smk_write_fuzzy_assignments_file(const float* probabilities, unsigned k, unsigned n, const char* path);
/* FlatClustWriteResults, common/src/flat_clust_output.cpp:56-141; format 0 = XML, 1 = JSON */
int smk_flatclust_write_results(const char* assignfile, const char* fuzzyfile, const char* resultfile,
                                const unsigned* assignments, unsigned num_assignments, const float* probabilities,
                                const char* const* dictionary, int64_t dictionary_size, const int* term_indices,
                                int64_t num_term_indices, int format, unsigned maxterms, unsigned num_docs,
                                unsigned num_clusters);

/* ---- CSV files: WriteDelimitedFile / LoadDelimitedFile, common/include/delimited_file.hpp:49-135 ----
 * (row-major text, scientific notation; used for w.csv / h.csv and init files) */
int smk_write_csv(const double* buf, unsigned ldim, unsigned height, unsigned width, const char* filename,
                  unsigned precision);
int smk_load_csv(const char* filename, double* out, unsigned long capacity, unsigned* height, unsigned* width);
/* MatrixMarket coordinate files -> CSC (LoadMatrixMarketFile, common/include/sparse_matrix_io.hpp:118-262:
 * real/integer/pattern x general/symmetric/skew-symmetric).  Two calls: sizes first (arrays NULL), then data.
 * Returns 1 on success, 0 on failure. */
int smk_load_matrix_market(const char* filename, unsigned* height, unsigned* width, unsigned* nnz,
                           unsigned* col_offsets /* width+1 or NULL */, unsigned* row_indices /* nnz or NULL */,
                           double* data /* nnz or NULL */);

/* ---- flat handles onto the public C++ API `namespace smallk` (include/smallk.hpp), one per entry of
 * pysmallk's extern block (pysmallk/interface/smallk_lib.pyx:42-88), for bindings that cannot call C++
 * (ctypes, cgo, JNI).  Functions that can throw return 0 = ok, 1 = std::logic_error,
 * 2 = std::runtime_error; the message is in smk_api_last_exception(). */
const char* smk_api_last_exception(void);
int smk_api_initialize(void);                /* smallk::Initialize   smallk.cpp:114-119 */
int smk_api_is_initialized(void);            /* smallk::IsInitialized */
void smk_api_finalize(void);                 /* smallk::Finalize */
void smk_api_reset(void);                    /* smallk::Reset        smallk.cpp:81-111 */
void smk_api_seed_rng(int seed);             /* smallk::SeedRNG */
unsigned smk_api_get_major_version(void);
unsigned smk_api_get_minor_version(void);
unsigned smk_api_get_patch_level(void);
int smk_api_load_matrix_file(const char* path);                                 /* LoadMatrix(string) :163 */
int smk_api_load_matrix_dense(const double* buf, unsigned ldim, unsigned height, unsigned width); /* :204 */
int smk_api_load_matrix_sparse(unsigned height, unsigned width, unsigned nz, const double* data,
                               const unsigned* row_indices, const unsigned* col_offsets);       /* :268 */
int smk_api_is_matrix_loaded(void);
int smk_api_set_output_dir(const char* dir);  /* SetOutputDir :348-380 */
const char* smk_api_get_output_dir(void);
void smk_api_set_output_precision(unsigned digits);
unsigned smk_api_get_output_precision(void);
int smk_api_set_nmf_tolerance(double tol);
double smk_api_get_nmf_tolerance(void);
void smk_api_set_max_iter(unsigned v);
unsigned smk_api_get_max_iter(void);
void smk_api_set_min_iter(unsigned v);
unsigned smk_api_get_min_iter(void);
void smk_api_set_max_threads(unsigned v);
unsigned smk_api_get_max_threads(void);
void smk_api_set_max_terms(unsigned v);
unsigned smk_api_get_max_terms(void);
void smk_api_set_output_format(int xml0_json1);
int smk_api_get_output_format(void);
int smk_api_set_hiernmf2_tolerance(double tol);
double smk_api_get_hiernmf2_tolerance(void);
void smk_api_set_device_storage(int storage);   /* extension: SMK_STORE_F32 / SMK_STORE_BF16 */
int smk_api_get_device_storage(void);
unsigned smk_api_get_iteration_count(void);
/* smallk::Nmf(k, algorithm, initfile_w, initfile_h), smallk.cpp:471-650; `algorithm` is numbered
 * like smallk::Algorithm: MU 0, BPP 1, HALS 2, RANK2 3 (smallk.hpp:34-40) */
int smk_api_nmf(unsigned k, int algorithm, const char* initfile_w, const char* initfile_h);
const double* smk_api_locked_buffer_w(unsigned* ldim, unsigned* height, unsigned* width);   /* :653-661 */
const double* smk_api_locked_buffer_h(unsigned* ldim, unsigned* height, unsigned* width);   /* :664-672 */
int smk_api_hiernmf2(unsigned num_clusters);            /* smallk::HierNmf2, smallk.cpp:859-862 */
int smk_api_hiernmf2_with_flat(unsigned num_clusters);  /* smallk::HierNmf2WithFlat, smallk.cpp:865-868 */
int smk_api_load_dictionary_file(const char* path);     /* LoadDictionary(string), smallk.cpp:675-691 */
int smk_api_load_dictionary(const char* const* terms, unsigned count);          /* smallk.cpp:694-707 */

/* ---- preprocess_tf: term-document pruning and tf-idf (preprocessor/src/preprocess.cpp:81-232) ---------------------------
 * Input: a term-count matrix in CSC, checked as smk_matrix_create_sparse checks it (row indices need not be sorted inside a
 * column).  Counts: 1 in boolean mode, 0 for a negative value, else the value truncated toward zero.  The loop prunes rows
 * (total count < docs_per_term, or an entry in every column), short columns (< terms_per_doc entries) and duplicate columns
 * (the one with the largest index survives) until nothing changes or max_iter iterations have run (max_iter = 0 is
 * accepted: scores of the input as it stands).  Returns SMK_OK, or SMK_FAILURE when every column was pruned; in both cases
 * *out is a result (on failure it holds only the iteration log and the sizes at the failure).  Everything stays on the
 * device until a download.  smk_preprocess returns with every pass finished; the accessors below run on the calling thread's
 * current context stream, so a result may be read from another context than the one that made it. */
typedef struct smk_preprocess_options {
    unsigned max_iter, docs_per_term, terms_per_doc;
    int boolean_mode;
} smk_preprocess_options;
typedef struct smk_preprocess_result smk_preprocess_result;
int smk_preprocess(const smk_preprocess_options* opts, unsigned height, unsigned width, unsigned nnz, const unsigned* col_offsets,
                   const unsigned* row_indices, const double* data, smk_preprocess_result** out);
void smk_preprocess_result_destroy(smk_preprocess_result* r);
int smk_preprocess_result_sizes(const smk_preprocess_result* r, unsigned* height, unsigned* width, unsigned* nnz,
                                unsigned* iterations);
/* the log line of each iteration ("[i] height: h, width: w, nonzeros: n"): 3 x iterations values h, w, n */
int smk_preprocess_result_log(const smk_preprocess_result* r, unsigned* out);
/* host wall times of smk_preprocess: the input upload (the host-to-device copies of offsets, rows and values; the working set
 * is allocated before it), and the device phase from the uploaded input to the resident result */
int smk_preprocess_result_timing(const smk_preprocess_result* r, double* upload_ms, double* device_ms);
/* the reduced matrix and index sets; any pointer may be NULL.  term_indices: height, doc_indices: width, col_offsets:
 * width + 1, row_indices and scores: nnz */
int smk_preprocess_result_download(const smk_preprocess_result* r, unsigned* term_indices, unsigned* doc_indices,
                                   unsigned* col_offsets, unsigned* row_indices, double* scores);
/* the reduced tf-idf matrix as a resident sparse matrix (with its transpose), built on the device: the matrix
 * smk_matrix_create_sparse builds from the downloaded arrays, for smk_clust_resident and the solver */
int smk_preprocess_result_matrix(const smk_preprocess_result* r, smk_matrix** out);
/* reduced_matrix.mtx (TermFrequencyMatrix::WriteMtxFile, term_frequency_matrix.cpp:286-320): the banner, "h w nnz", then
 * "row col score" 1-based in column order, fixed notation with `precision` digits; formatted on as many threads as the process
 * may run on (its CPU affinity, at most OMP_NUM_THREADS when set), about 2^22 lines in flight.
 * SMK_OK, or SMK_FAILURE when the file cannot be written */
int smk_preprocess_write_mtx(const smk_preprocess_result* r, const char* path, unsigned precision);

/* ---- a fitted vocabulary: new documents into the term space of a fit --------------------------------
 * A vocabulary is what a fit leaves behind for documents that arrive later: the input's term count (height_in), the surviving
 * terms (original indices, strictly ascending), their idf = log(width_fit / df) exactly as the fit computed them, and the fit's
 * boolean_mode; all on the device, with the scattered map old term -> new term.  Applying it to a CSC term-count matrix in
 * the ORIGINAL term numbering gives the matrix smk_transform needs: entries of pruned terms removed, the rest renumbered with
 * their order kept, scored (1 + log(count)) * idf[term] and every column normalised, operation for operation as the fit scores
 * its own columns -- a fit's own documents come out with the fit's bits. */
typedef struct smk_vocabulary smk_vocabulary;
/* the vocabulary of a fit; SMK_FAILURE on a failed fit and on an applied result (which keeps no idf: its vocabulary is the one
 * that was applied) */
int smk_preprocess_result_vocabulary(const smk_preprocess_result* r, smk_vocabulary** out);
/* from host arrays of `height` elements (a saved vocabulary).  Checked before anything is launched (SMK_BAD_PARAM +
 * smk_last_error): height >= 1, non-null arrays, term_indices strictly ascending and below height_in.  idf is taken as given */
int smk_vocabulary_create(unsigned height_in, unsigned height, const unsigned* term_indices, const double* idf, int boolean_mode,
                          smk_vocabulary** out);
void smk_vocabulary_destroy(smk_vocabulary* v);
int smk_vocabulary_sizes(const smk_vocabulary* v, unsigned* height_in, unsigned* height, int* boolean_mode);
/* term_indices and idf: height elements each; either may be NULL */
int smk_vocabulary_download(const smk_vocabulary* v, unsigned* term_indices, double* idf);
typedef struct smk_apply_options {
    unsigned min_terms; /* a document with fewer surviving entries is dropped; 0 keeps every document, empty ones included */
    int boolean_mode;   /* -1: the fit's */
} smk_apply_options;
/* The input is checked as smk_preprocess checks its own (rows < height_in; they need not be sorted inside a column).  *out is
 * an ordinary result: height and term_indices are the vocabulary's, doc_indices the input columns that were kept (ascending),
 * the log is empty, iterations 0, both timings filled in.  SMK_FAILURE when every column was dropped (*out then holds the
 * vocabulary's height, the input's width and the number of entries in surviving terms). */
int smk_vocabulary_apply(const smk_vocabulary* v, const smk_apply_options* opts, unsigned width, unsigned nnz,
                         const unsigned* col_offsets, const unsigned* row_indices, const double* data, smk_preprocess_result** out);
/* the same with the input in device memory, by the conventions of smk_matrix_create_sparse_device: offsets from 0, SMK_IDX_I32 /
 * SMK_IDX_I64 indices, SMK_DT_F64 / SMK_DT_F32 values, the caller's stream, the index arrays checked by a kernel before anything
 * reads through them.  The result has the bits smk_vocabulary_apply gives on the same arrays; its upload time is 0. */
int smk_vocabulary_apply_device(const smk_vocabulary* v, const smk_apply_options* opts, unsigned width, unsigned nnz,
                                const void* col_offsets, int idx_type, const void* row_indices, int row_idx_type, const void* values,
                                int dtype, void* stream, smk_preprocess_result** out);

#ifdef __cplusplus
}
#endif
#endif /* SMALLK_AMD_H */

/*
 * aps.h — C ABI of libaps_hip.so, the MI355X (gfx950) stitching hot path.
 *
 * This is the drop-in boundary for AutoPanoStitch's hot path.  The reference's only FFI is the
 * MATLAB mex gateway (PP/mex/flann_knn.cpp:118-119, PP/mex/nearest2HammingExhaustiveMEX.cpp:16);
 * every entry point below is what a mex shim for the cited reference function binds (the shims and
 * the shadowing .m wrappers are in matlab/, described in INTEGRATION.md).  "PP/" abbreviates
 * "/root/reference/Procedural Program/".
 *
 * Conventions (all functions):
 *   - extern "C", return int status: APS_OK (0) or a negative APS_E_* code; a human-readable
 *     message for the calling thread is available from aps_last_error().  Nothing throws or
 *     long-jumps across the boundary (the mex shim turns a non-zero status into
 *     mexErrMsgIdAndTxt("aps:<kind>", aps_last_error()), as flann_knn.cpp:130-166 does).
 *   - Pointers are plain pointers; each may point to HOST memory (what a mex shim holds) or to
 *     DEVICE memory (what a resident pipeline holds).  The library asks the HIP runtime which it
 *     is (hipPointerGetAttributes) and stages host buffers through HBM itself.  No torch types.
 *   - The caller owns every buffer; outputs are caller-allocated; the library keeps no pointer
 *     after return.  Data-dependent output sizes use (capacity in, count out); if the capacity
 *     is too small the call fails with APS_E_CAP and *count holds the needed size.
 *   - Matrices carry an explicit layout + leading dimension.  APS_COLMAJOR is MATLAB's layout
 *     (element (i,k) at p[i + k*ld], flann_knn.cpp:111-112); APS_ROWMAJOR is C/numpy/torch
 *     (element (i,k) at p[i*ld + k]).  Elements outside the logical result - between the rows / columns of an output whose
 *     leading dimension exceeds its extent, and rows count..cap of a capacity buffer - are not written, for host and device
 *     pointers alike.
 *   - Indices crossing the boundary are 1-based uint32 like the reference's mex outputs
 *     (flann_knn.cpp:214,248; nearest2HammingExhaustiveMEX.cpp:76); 0 means "none".
 *   - Thread-safe and re-entrant: per-thread HIP stream and workspace; no global mutable state
 *     besides the device selection of the calling thread.
 *   - There is NO CPU fallback in this library.  Without a usable gfx950 device every compute
 *     entry point returns APS_E_DEVICE.
 */
#ifndef APS_H_
#define APS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APS_VERSION 100 /* 0.1.0 */

/* ---- status codes -------------------------------------------------------------------------- */
enum {
    APS_OK = 0,
    APS_E_ARG = -1,      /* bad argument value (null pointer, negative size, unknown enum)       */
    APS_E_DIM = -2,      /* dimension mismatch (flann_knn:dim, hamm2nn:cols)                      */
    APS_E_TYPE = -3,     /* unsupported element type / layout                                     */
    APS_E_OOM = -4,      /* device or host allocation failed (renderPanorama.m:245-266 semantics) */
    APS_E_DEVICE = -5,   /* no gfx950 device / HIP runtime error                                  */
    APS_E_INTERNAL = -6, /* invariant violated inside the library                                 */
    APS_E_CAP = -7       /* output capacity too small; needed size reported through *count        */
};

enum { APS_COLMAJOR = 0, APS_ROWMAJOR = 1 };

/* ---- library / device ---------------------------------------------------------------------- */
int aps_version(void);
const char* aps_last_error(void);
/* Number of usable gfx950 devices (0 if none; never fails). */
int aps_device_count(void);
/* Select the device for the calling thread.  The selection also becomes the process-wide default that threads which
 * never called aps_set_device start on (worker pools, parpool('Threads') workers); before any call the default is env
 * APS_DEVICE, else 0. */
int aps_set_device(int device);
/* Select the device for the calling thread ONLY (the process-wide default is left alone): what a worker thread of a
 * process that drives several GPUs calls before its first entry point, so that it does not inherit whichever device
 * another thread selected last. */
int aps_set_thread_device(int device);
/* Recreate the calling thread's own stream at a priority of the device's range: level > 0 the highest, < 0 the lowest,
 * 0 the middle (the default).  For a host that runs two stages side by side from two threads and wants the short launches
 * of one not to queue behind the other's kernels (the runtime keeps separate hardware queues per priority level). */
int aps_set_thread_stream_priority(int level);
/* The device the calling thread is bound to (binding it to the default first if it has none); < 0 on error. */
int aps_get_device(void);
/* Run the calling thread's work on an existing HIP stream (e.g. torch's current stream);
 * NULL restores the library's own per-thread stream. */
int aps_set_stream(void* hip_stream);
/* Block until the calling thread's stream has drained. */
int aps_synchronize(void);
/* Release the calling thread's cached device workspace. */
int aps_release_workspace(void);
/* Per-thread event timer on the library's stream (used by bench.py for in-stream kernel timing):
 * aps_timer_begin() records an event, aps_timer_end() records another, synchronises and returns
 * the elapsed milliseconds between them. */
int aps_timer_begin(void);
int aps_timer_end(float* ms);
/* Per-kernel timing on the stream the kernels are launched on (what bench.py's `roofline` entry uses):
 * while enabled, every launch site of a named hot kernel is bracketed by HIP events.
 * aps_profile_get sums the elapsed time of all recorded launches whose name equals `name`
 * (e.g. "match2nn", "sift_blur", "warp_layer", "mb_blur", ...) and returns the launch count.
 * on = 1: every launch site; on = 2: only the per-batch sites (matching, RANSAC, coverage, crop, BA, gain) - the
 * per-image and per-tile chains issue thousands of launches per stitch and their event records cost a few percent;
 * on = 0: off. */
int aps_profile_enable(int on);
int aps_profile_reset(void);
int aps_profile_get(const char* name, double* total_ms, int* launches);
/* The recorded launches of `name` one by one, in launch order: ms[0 .. min(*count, cap) - 1]; *count = how many there are.
 * (bench.py: the dominant kernel's duration per step - its median and minimum, not only the mean.) */
int aps_profile_series(const char* name, double* ms, int cap, int* count);
/* Writes a ';'-separated list of the kernel names recorded since the last reset into buf. */
int aps_profile_names(char* buf, int buf_len);

/* ============================================================================================
 * (1) Descriptor matching — PP/featureMatching/matchFeaturesScratch.m
 * ============================================================================================ */

/* a5: nearest2SSDExhaustive (matchFeaturesScratch.m:322-366).
 *   D2(i,j) = (a2(i) + b2(j)) - 2*G(i,j),  G = A*B'  in f32;
 *   idx2(i) = argmin_j D2(i,j) (first index on ties, :356), d1 = that minimum,
 *   d2 = min over j != idx2(i) (inf if n2 == 1).
 * Arithmetic contract (the canonical order the oracle restates): G(i,j) is the k-ascending f32 fma
 * chain acc = fmaf(A(i,k), B(j,k), acc) from acc = 0 — exactly what v_mfma_f32_32x32x2_f32 computes;
 * a2/b2 are k-ascending sums s = s + x*x (separate multiply and add).
 * idx2: 1-based uint32[n1]; d1, d2: f32[n1]. */
int aps_match_2nn_ssd(const float* A, int64_t n1, int64_t lda, const float* B, int64_t n2,
                      int64_t ldb, int dim, int layout, uint32_t* idx2, float* d1, float* d2);

/* a6: nearest2ApproxFloatFast + doBlock (matchFeaturesScratch.m:442-573), the 'pca2nn' back end of Method = 'Approximate':
 *   muB = mean(B,1,'omitnan'); coeff = pca(B - muB, 'NumComponents', n_components); both sets centred with muB and
 *   projected (:480-484; skipped when use_pca == 0 or dim <= n_components, :478); rows / (sqrt(sum(row.^2)) + eps('single'))
 *   (:488-489); G = A*B'; idx2 = first argmax_j G(i,j), the second similarity = max of the rest; d = 2 - 2*sim (:552-570).
 * Arithmetic contract (the canonical order the oracle restates; MATLAB leaves it open):
 *   mean / covariance sums per chunk of 256 rows in ascending row order (the covariance chunk as the f32 fma chain of
 *   v_mfma_f32_32x32x2_f32), chunk partials added in f64 in ascending order, covariance / (n2 - 1);
 *   principal axes = eigenvectors of that covariance by cyclic Jacobi rotations in f64 on the HOST (fixed order), sorted by
 *   descending eigenvalue, each signed so that its largest-magnitude entry is positive (pca's convention), cast to f32;
 *   projection = k-ascending f32 fma chain; squared norm s = s + y*y over ascending components;
 *   G(i,j) = component-ascending f32 fma chain (one MFMA chain).
 *   Fewer than n_components + 1 rows in B: pca() returns min(n2 - 1, n_components) columns (the centred data has rank
 *   <= n2 - 1); the other columns of the basis are ZERO here, which projects every row of A and of B to exactly 0 on them -
 *   the same norms, similarities and distances as the reference's narrower basis (n2 == 1: no column at all, d1 = 2).
 * idx2: 1-based uint32[n1]; d1, d2: f32[n1] (d2 = +inf when n2 == 1).  mu_out (f32[dim]) and coeff_out (f32[dim x
 * n_components], row-major; columns min(n2 - 1, n_components) .. are zero) are optional (NULL) and filled only when the
 * projection runs.  n1, n2 >= 1. */
int aps_match_pca2nn(const float* A, int64_t n1, int64_t lda, const float* B, int64_t n2, int64_t ldb, int dim, int layout,
                     int n_components, int use_pca, uint32_t* idx2, float* d1, float* d2, float* mu_out, float* coeff_out);

/* Options of the a4 driver (matchFeaturesScratch.m:59-78 name/value pairs). */
typedef struct aps_match_opts {
    double max_ratio;       /* 'MaxRatio'       (inputs.m:59  Ratiothreshold = 0.6).  f64 like MATLAB's scalars:
                               the test is d1 <= MaxRatio^2 * d2 with MaxRatio^2 evaluated in double
                               (matchFeaturesScratch.m:170-173); a float field would move the boundary. */
    double match_threshold; /* 'MatchThreshold' (inputs.m:55  Matchingthreshold = 1.5; raw SSD), f64   */
    int unique;            /* 'Unique'         (featureMatchingPairwise.m:113: true)               */
    int normalize;         /* 0 never, 1 always, 2 = the reference's rule: L2-normalise both sets
                              iff max|A| > 2 or max|B| > 2 (matchFeaturesScratch.m:105-110)        */
} aps_match_opts;

/* a4 + a5: matchFeaturesScratch(F1, F2, 'Method','Exhaustive', ...) for float descriptors
 * (matchFeaturesScratch.m:81-215): conditional row normalisation x./(sqrt(sum(x.^2))+eps('single'))
 * (:232-233), exhaustive 2-NN, keep iff d1 <= r^2*d2 (:173-174) and d1 <= MatchThreshold (:177) and
 * both finite (:178), then greedy one-to-one by ascending d with stable order (:186-207).
 * Outputs: idx1/idx2 1-based uint32[cap], metric f32[cap], *count = K.  cap >= n1 always suffices. */
int aps_match_features(const float* F1, int64_t n1, int64_t ld1, const float* F2, int64_t n2,
                       int64_t ld2, int dim, int layout, const aps_match_opts* opts,
                       uint32_t* idx1, uint32_t* idx2, float* metric, int64_t cap, int64_t* count);

/* Diagnostics of the calling thread's most recent filtered matching call (aps_match_features / _pairwise / _pairs):
 * rows = (A row, pair) combinations the int8 screening pre-pass looked at (0 when it did not run: APS_MATCH_NO_SCREEN,
 * APS_MATCH_MODE=f32), survivors = those it could NOT prove to fail the ratio / threshold filter and handed to the exact
 * path.  The screen never changes a result (matchFeaturesScratch.m:170-178 is evaluated on exact distances for every
 * row that can pass it); the counters exist for benchmarks and for tests that guard against a silently disabled screen. */
int aps_match_screen_stats(int64_t* rows, int64_t* survivors);

/* ... and of the same call: jobs = the (A set, B set) jobs the screening pass ran, exact_jobs = those it ran on EXACT int8
 * codes.  A set whose every row is a vector of integers 0 .. 255 divided by its f32 norm, bit for bit (SIFT descriptors as
 * OpenCV quantises them and the SIFT stage hands them over; detected per row, no hint needed), is coded as u - 128 without any
 * rounding, and a job of two such sets bounds its distances from exact integer dot products: the only slack left is the
 * spread of the column set's norms.  Any other job takes the rounded codes with their error terms.  Same results either
 * way; APS_MATCH_NO_EXACT=1 switches the exact codes off (A/B).  For benchmarks and tests. */
int aps_match_screen_exact_jobs(int64_t* jobs, int64_t* exact_jobs);

/* Diagnostics: the eight statistics words the matcher's proofs take from ONE descriptor set (n x 128 f32, `normalize` != 0:
 * rows L2-normalised first as matchFeaturesScratch.m:232-233 does), as the preparation kernels compute them (maxima over
 * all rows, folded from per-workgroup maxima): stats[0] = max ||x||^2 (canonical k-ascending f32 sum), [1] = max ||x - f16(x)||
 * (rounded up), [2], [3] = residuals of the f16 norm pieces (0 for ordinary data), [4] = max x, [5] = max column-side int8
 * residual norm (rounded up), [6] = min ||x||^2, [7] = min x.  Host output.  For tests: a statistic that misses a row makes
 * a bound unsound without changing any result on ordinary data. */
int aps_match_set_stats(const float* X, int64_t n, int64_t ld, int layout, int normalize, float* stats);

/* Diagnostics of the co-residency rule: registers per lane and the workgroup bound of the int8
 * screening kernel as the LOADED code object declares them (hipFuncGetAttributes).  shape = 16 (v_mfma_i32_16x16x64_i8, the
 * default) or 32 (v_mfma_i32_32x32x32_i8, APS_SCREEN_SHAPE=32); bounds_pass != 0: the pooled matcher's instantiation.  The
 * kernels must hold 256 registers at 512 threads per workgroup so that no other kernel's waves share a SIMD with int8-MFMA
 * waves; the library refuses to launch them otherwise (APS_E_INTERNAL). */
int aps_match_screen_kernel_regs(int shape, int bounds_pass, int* num_regs, int* max_threads_per_block);

/* a3: featureMatchingPairwise (featureMatchingPairwise.m:48-63): all upper-triangular image pairs
 * in the reference's order (column-major linear index of triu(.,1): (1,2),(1,3),(2,3),(1,4),...),
 * each through aps_match_features' rule, in ONE batched launch sequence.
 *   desc[i]  : descriptors of image i, counts[i] x dim, row stride ld[i] (layout as above)
 *   pair_ptr : int64[n_pairs+1] CSR offsets into idx_i/idx_j/metric, n_pairs = n_img*(n_img-1)/2
 *   idx_i/idx_j : 1-based feature indices in image i / j (i < j), metric: SSD
 * cap >= sum over pairs of counts[i] always suffices. */
int aps_match_pairwise(const float* const* desc, const int64_t* counts, const int64_t* ld,
                       int n_img, int dim, int layout, const aps_match_opts* opts,
                       int64_t* pair_ptr, uint32_t* idx_i, uint32_t* idx_j, float* metric,
                       int64_t cap, int64_t* count);

/* The same for an explicit list of image pairs (0-based image ids, pair_a[p] != pair_b[p]); this is what
 * lets the n x n pair matrix of featureMatchingPairwise.m:48 be tiled across GPUs: every rank holds all
 * descriptors (after the all-gather) and matches its own slice of the pair list.  For each pair the rows
 * of image pair_a[p] are matched against image pair_b[p]; idx_a/idx_b are 1-based feature indices. */
int aps_match_pairs(const float* const* desc, const int64_t* counts, const int64_t* ld, int n_img,
                    int dim, int layout, const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs,
                    const aps_match_opts* opts, int64_t* pair_ptr, uint32_t* idx_a, uint32_t* idx_b,
                    float* metric, int64_t cap, int64_t* count);

/* a8 kNN: [idx, dist] = flann_knn_win(train, query, k, 'flann', trees, checks) for float
 * descriptors (flann_knn.cpp:118-253; caller featureMatchingGlobal.m:108-117), with an EXACT
 * search in place of OpenCV's randomized kd-forest: squared-L2, ascending, ties -> lower index.
 * idx: 1-based uint32 Fq x k, dist: f32 Fq x k, both in `layout` with leading dimension ldo. */
int aps_knn_global(const float* train, int64_t ft, int64_t ldt, const float* query, int64_t fq,
                   int64_t ldq, int dim, int layout, int k, uint32_t* idx, float* dist,
                   int64_t ldo);
/* The same search for featureMatchingGlobal's own use (featureMatchingGlobal.m:106-147: the pool against itself, then the
 * per-query filter at ratioThr).  pool: the normalised descriptors of all images back to back, img_off[n_img + 1] the row
 * offsets of the images (img_off[0] = 0, img_off[n_img] = f).  A query that the filter PROVABLY drops at `ratio` - an
 * int8 screening pass bounds its two smallest cross-image distances, :129-147 - may come back as k copies of itself
 * (distance 0): the filter removes them as self matches, fewer than two candidates remain, the query is skipped exactly
 * as the reference skips it.  Every other row gets its exact k nearest (k <= 4), bit-identical to aps_knn_global.  The
 * output of aps_global_filter on this table therefore equals its output on aps_knn_global's.  Pools whose (row, image)
 * table would exceed 2^31 slots (f x n_img; BASELINE configs[4]: 5.4 M rows x 500 images) are searched in several passes
 * over ranges of query images, every pass against all images: same result, bounded workspace. */
int aps_knn_global_screened(const float* pool, int64_t f, int64_t ld, int dim, int layout, const int64_t* img_off, int n_img,
                            float ratio, int k, uint32_t* idx, float* dist, int64_t ldo);
/* Diagnostics of the calling thread's most recent aps_knn_global_screened call: rows of the pool, rows that were searched. */
int aps_knn_global_screen_stats(int64_t* rows, int64_t* survivors);

/* a8 kNN, binary descriptors: [idx, dist] = flann_knn_win(train_u8, query_u8, k, 'bf' | 'flann', ...) - the uint8 branches
 * of flann_knn.cpp: cv::BFMatcher(NORM_HAMMING).knnMatch (:199-223) and the LSH index (:235-240), both replaced by ONE exact
 * brute-force Hamming k-NN (ascending distance, ties -> lower index; the LSH index is approximate and seed dependent).
 * nbytes <= 64 (ORB 32, BRISK 64).  idx: 1-based uint32 Fq x k, dist: f32 Fq x k in `layout` with leading dimension ldo;
 * a query with fewer than k train rows gets index 0 / Inf in the missing slots (:217-218). */
int aps_knn_hamming(const uint8_t* train, int64_t ft, int64_t ldt, const uint8_t* query, int64_t fq, int64_t ldq,
                    int nbytes, int layout, int k, uint32_t* idx, float* dist, int64_t ldo);

/* a8 pooling step: allDesc = allDesc ./ sqrt(sum(allDesc.^2, 2) + eps('single')) (featureMatchingGlobal.m:80-86; eps inside
 * the root, unlike matchFeaturesScratch's normalizeRowsL2).  out: n x dim f32 row-major (ld = dim), host or device. */
int aps_global_normalize(const float* X, int64_t n, int64_t ld, int dim, int layout, float* out);

/* a8 filter: the per-query loop of featureMatchingGlobal.m:123-161 (drop self, drop same-image,
 * need >= 2 left, reject iff d1/max(d2,eps('single')) > ratio, append [li lj] to pair (min,max) in
 * query order).  img_idx (1-based image id per row) and local_idx (1-based) are uint32[f].
 * Output CSR over pairs in the same pair order as aps_match_pairwise. */
int aps_global_filter(const uint32_t* nn_idx, const float* nn_dist, int64_t f, int k,
                      int64_t ldn, int layout, const uint32_t* img_idx, const uint32_t* local_idx,
                      int n_img, float ratio, int64_t* pair_ptr, uint32_t* idx_i, uint32_t* idx_j,
                      int64_t cap, int64_t* count);

/* a9: [idx2,d1,d2] = nearest2HammingExhaustiveMEX(Abytes,Bbytes)
 * (nearest2HammingExhaustiveMEX.cpp:16-80, ...OMPMEX.cpp:18-83): brute-force Hamming 2-NN on packed
 * bytes with the reference's tie rule (strict < for best, <= for second, :63-68), N2==0 -> idx 0 and
 * NaN (:42-45), single candidate -> second = nb*8 (:71-74). */
int aps_hamming_2nn(const uint8_t* A, int64_t n1, int64_t lda, const uint8_t* B, int64_t n2,
                    int64_t ldb, int nbytes, int layout, uint32_t* idx2, float* d1, float* d2);

/* Options of the binary branch of matchFeaturesScratch (matchFeaturesScratch.m:59-78 name/value pairs). */
typedef struct aps_hamming_match_opts {
    double max_ratio;       /* 'MaxRatio', linear for binary sets (matchFeaturesScratch.m:171); rounded to single for the test,
                               as MATLAB evaluates double scalar * single array */
    double match_threshold; /* 'MatchThreshold', percent of mismatched bits (:32 suggests 10 or more), rounded to single */
    int unique;             /* 'Unique' (featureMatchingPairwise.m:113: true) */
    int nbits;              /* 0 = 8 * nbytes; otherwise 1..8*nbytes: the width of unpacked-bit inputs before packBits padded
                               them to whole bytes (matchFeaturesScratch.m:618-645).  Distances are counted on the packed bytes
                               either way (the padding is zero on both sides); nbits is the divisor of the percent values and
                               the patch of :318. */
} aps_hamming_match_opts;

/* a3 + a4 + a9 for binary sets: the pair loop of featureMatchingPairwise.m:48-63 with matchFeaturesScratch's binary branch
 * inside (matchFeaturesScratch.m:81-135,170-211), every pair of the list in ONE batched launch chain.  Per pair, the rows of image
 * pair_a[p] (0-based ids, pair_a[p] != pair_b[p]) are searched in image pair_b[p]:
 *   2-NN on packed bytes with the mex's tie rule (nearest2HammingExhaustiveMEX.cpp:63-74: strict < for the best, so ties go to
 *   the lower index; a single candidate gives second = nbytes * 8); a second distance of 0 becomes nbits (:318);
 *   dBest = (d1 / nbits) * 100, dSecond = (d2 / nbits) * 100 in single, in that order (:120-121);
 *   keep iff dBest <= single(MaxRatio) * dSecond (single product, :171) and dBest <= single(MatchThreshold) (:177);
 *   unique != 0: greedy one-to-one in ascending (dBest, row) order (the stable sort of :186-207) - every row proposes one column,
 *   so a column goes to its smallest (dBest, row) - and the list is in that order; unique == 0: in row order.
 *   A pair with an empty side yields an empty list (:84-88).
 * desc[i]: counts[i] x nbytes uint8 in `layout` with leading dimension ld[i], nbytes in 1..64, one width for all sets.
 * Every array - the three tables, the pair list, the sets, the outputs - may be host or device memory.
 * Outputs: pair_ptr int64[n_pairs + 1] CSR offsets; idx_a / idx_b 1-based row indices in image pair_a[p] / pair_b[p]; metric =
 * dBest (percent).  cap >= sum over pairs of counts[pair_a[p]] always suffices.  With cap too small - cap = 0, or any of the
 * three lists NULL, asks for the count only - the call fails with APS_E_CAP, *count and pair_ptr hold the true sizes and the
 * lists are not written; elements count..cap of the lists are never written.
 * The uniqueness step keeps one 8-byte slot per column of every pair in flight: the pair list is walked in chunks whose
 * counts[pair_b[p]] sum to at most a bound (2^25 slots, 256 MiB; a single pair above it is a chunk of its own), with the same
 * result for any chunking.  Arguments are checked before any device work, apart from reading tables and pair lists that live on
 * the device; a list whose pairs all have an empty side needs no device. */
int aps_hamming_match_pairs(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                            const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, const aps_hamming_match_opts* opts,
                            int64_t* pair_ptr, uint32_t* idx_a, uint32_t* idx_b, float* metric, int64_t cap, int64_t* count);
/* The same for all upper-triangular pairs in aps_match_pairwise's order (featureMatchingPairwise.m:48), n_pairs =
 * n_img * (n_img - 1) / 2: rows of image i searched in image j, i < j. */
int aps_hamming_match_pairwise(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                               const aps_hamming_match_opts* opts, int64_t* pair_ptr, uint32_t* idx_i, uint32_t* idx_j, float* metric,
                               int64_t cap, int64_t* count);

/* ============================================================================================
 * (2) Geometric verification — PP/imageMatching/estimateTransformationRANSAC.m
 * ============================================================================================ */

/* input.transformationType (inputs.m:74) = transformType of estimateTransformationRANSAC.m:612-660; minimal samples
 * 4 / 3 / 2 / 2 / 1.  All five run through APS_ROBUST_RANSAC and through APS_ROBUST_MLESAC (whose estimators differ:
 * estimateTransformationMLESAC.m:345-510 - null vectors of the 2n x 9 / 7 / 5 systems, Kabsch for 'rigid', the mean
 * displacement for 'translation'). */
enum {
    APS_TFORM_PROJECTIVE = 0,
    APS_TFORM_AFFINE = 1,      /* estimateAffine :227-288: pseudo-inverse of the normalised design matrix        */
    APS_TFORM_SIMILARITY = 2,  /* estimateSimilarity :290-356: rotation from the 2x2 cross-covariance, median scale */
    APS_TFORM_RIGID = 3,       /* estimateRigid :358-421 (identity rotation when the cross-covariance is ill-conditioned) */
    APS_TFORM_TRANSLATION = 4  /* estimateTranslation :423-452: per-axis median displacement                      */
};

/* a12 findInliers (estimateTransformationRANSAC.m:444-516) for T hypotheses at once.
 *   Hs    : f64 3x3xT, each 3x3 column-major (MATLAB page layout)
 *   p1,p2 : f64 Mx2 column-major with leading dimension ldp (x column then y column)
 *   n_inl : int32[T]; mean_err: f64[T] (mean error over inliers, NaN if none);
 *   mask  : uint8 MxT column-major (may be NULL).
 * Projective: e = sqrt(|x2-Hx1|^2 + |x1-H^-1 x2|^2) < thr (:474-481); non-finite or |w|<eps -> inf
 * (:499-503); >=4 inliers whose centred x1 have s2/s1 < 1e-3 -> all false (:506-513,:567).
 * Affine / similarity / rigid: e = |x2 - Hx1| (:483-484); translation: the same error and the threshold both divided by
 * max(|coordinates|, 1) of the whole point set (:486-494); the collinearity test applies to affine (>= 3 inliers) only. */
int aps_ransac_score(const double* Hs, int n_hyp, const double* p1, const double* p2, int64_t m,
                     int64_t ldp, double thr, int tform_type, int32_t* n_inl, double* mean_err,
                     uint8_t* mask);

enum { APS_ROBUST_RANSAC = 0, APS_ROBUST_MLESAC = 1 };

typedef struct aps_ransac_opts {
    double max_distance; /* input.maxDistance        (inputs.m:69: 5.5)  */
    double confidence;   /* input.inliersConfidence  (inputs.m:72: 99.9) */
    int max_iter;        /* input.maxIter            (inputs.m:68: 500)  */
    int tform_type;      /* APS_TFORM_* (input.transformationType, inputs.m:74: 'projective')  */
    int method;          /* APS_ROBUST_RANSAC: estimateTransformationRANSAC.m (input.imageMatchingMethod 'ransac');
                            APS_ROBUST_MLESAC: estimateTransformationMLESAC.m:94-254 ('mlesac'): one-way distance,
                            truncated-loss score, refit on the inliers is the answer                */
} aps_ransac_opts;

/* a12 whole loop: [model, inliers, isFound] = estimateTransformationRANSAC(p1, p2, transformType, input)
 * (estimateTransformationRANSAC.m:54-183; the name dates from the projective-only rounds, opts->tform_type selects the
 * model).  The random subsets are an INPUT for every type: the first minPoints entries of a 4-column draw are the
 * sample.  sample_idx is
 * uint32 4 x n_samples column-major, 1-based, one column per loop iteration (each iteration of
 * :94-143 consumes one randperm draw, skipped ones included).  All hypotheses are fitted and scored
 * on the device in one batch; the data-dependent best/early-exit logic (:115-130) is replayed on the
 * host in order, so the result equals the sequential loop on the same draws.
 * model: f64 3x3 column-major; inlier_mask: uint8[m]; is_found: 0/1; trials_used: loop iterations
 * the sequential algorithm would have executed (may be NULL). */
int aps_ransac_homography(const double* p1, const double* p2, int64_t m, int64_t ldp,
                          const uint32_t* sample_idx, int n_samples, const aps_ransac_opts* opts,
                          double* model, uint8_t* inlier_mask, int* is_found, int* trials_used);

/* Number of pairs in the calling thread's most recent aps_ransac_homography / aps_ransac_homography_batch call whose
 * n_samples pre-drawn subsets ran out BEFORE the sequential loop's own stopping rule (trial > maxTrials, or 10*maxIter
 * skipped draws, estimateTransformationRANSAC.m:94): the reference would have kept drawing, so for those pairs the result
 * is that of a truncated loop.  Callers that want the reference's behaviour re-run with more draws (the counter-based
 * draw stream of aps_ransac_draw_samples only gets longer: earlier draws do not change). */
int aps_ransac_draws_exhausted(void);

/* The seeded stand-in for randperm(numPoints, 4) (estimateTransformationRANSAC.m:96): fills sample_idx
 * (uint32 4 x n_samples x n_pairs, 1-based) with distinct 4-subsets of 1..counts[p] from the counter-based
 * stream u = mix64(seed, keys[p] (or p if keys is NULL), 4*iteration + k) — identical to
 * imageMatching.draw_samples on the host.  A pair with counts[p] < 4 gets counts[p] distinct entries followed by ones
 * (enough for the transformTypes whose minimal sample it can still serve). */
int aps_ransac_draw_samples(const int64_t* counts, const uint64_t* keys, int n_pairs, int n_samples,
                            uint64_t seed, uint32_t* sample_idx);

/* The input of that batch, gathered on the device (imageMatching.m:121-135: keypoints{i}(matches(:,1),:) and
 * keypoints{j}(matches(:,2),:) per candidate pair): work pair q is images (img_a[q], img_b[q]); its matches are the
 * work_ptr[q+1]-work_ptr[q] entries of the resident 1-based lists idx_a / idx_b starting at list_start[q].
 *   kp       : host array of n_img DEVICE pointers, image i's keypoints as kp_count[i] x 2 f64 row-major [x y]
 *   idx_a/b  : device int32 lists (what aps_match_pairs leaves on the device)
 *   list_start, work_ptr (n_work+1), img_a, img_b: host arrays
 *   pts_a/b  : device f64, (total x 2) column-major with leading dimension ldp >= total = work_ptr[n_work];
 *              an index outside its image's table yields NaN coordinates (such a pair then fails RANSAC). */
int aps_gather_match_points(const double* const* kp, const int64_t* kp_count, int n_img, const int32_t* idx_a,
                            const int32_t* idx_b, const int64_t* list_start, const int64_t* work_ptr,
                            const int32_t* img_a, const int32_t* img_b, int n_work, double* pts_a, double* pts_b,
                            int64_t ldp);

/* Batched a10/a11/a12: every candidate pair of imageMatching.m:121-156 in one device batch.
 *   pts1/pts2 : f64, pair p's matched points are rows pair_ptr[p]..pair_ptr[p+1]-1 of two
 *               (total x 2) column-major arrays with leading dimension ldp
 *   sample_idx: uint32 4 x n_samples x n_pairs (1-based, local to the pair)
 * Outputs per pair: models f64 3x3xP, mask uint8[total], found int32[P], n_inl int32[P]. */
int aps_ransac_homography_batch(const double* pts1, const double* pts2, int64_t ldp,
                                const int64_t* pair_ptr, int n_pairs, const uint32_t* sample_idx,
                                int n_samples, const aps_ransac_opts* opts, double* models,
                                uint8_t* mask, int32_t* found, int32_t* n_inl);

/* ============================================================================================
 * (3) Rendering — PP/renderPanorama/renderPanorama.m, PP/blending/ (both .m files), PP/imageProcessing/imageWarp.m
 * ============================================================================================ */

/* Canvas pixel (xp, yp), 0-based -> a = origin0 + xp / f_pan, b = origin1 + yp / f_pan -> ray ("Projection
 * contract").  Modes 0, 1 and 4 are separable in (azimuth, height); modes 2, 3, 5 and 6 are drawn about R_ref. */
enum {
    APS_PROJ_CYLINDRICAL = 0,   /* azimuth a, height b = y / hypot(x, z)                                          */
    APS_PROJ_SPHERICAL = 1,     /* azimuth a, elevation b; 'equirectangular' is an alias (renderPanorama.m:180-189,357) */
    APS_PROJ_PLANAR = 2,        /* pinhole about R_ref: ray (a, b, 1)                                             */
    APS_PROJ_STEREOGRAPHIC = 3, /* about R_ref: (a, b) = (x, y) / (1 + z) of the unit ray                         */
    APS_PROJ_MILLER = 4,        /* Miller cylindrical: azimuth a, elevation 1.25 atan(sinh(0.8 b)); poles at b = +-2.3034 */
    APS_PROJ_FISHEYE = 5,       /* equidistant azimuthal about R_ref: hypot(a, b) = angle from the axis; void beyond pi */
    APS_PROJ_PANINI = 6         /* Pannini, d = 1, about R_ref: ray (a, b, 1 - a^2 / 4); verticals stay straight  */
};
/* APS_BLEND_MULTIBAND_MAXWEIGHT: multiband over the max-weight partition (Brown & Lowe Eq. 15-19; DESIGN.md, "Max-weight
 * multiband contract"): every pixel's level-0 weight is 1 for the first layer of maximal raw weight (> 0) and 0 for the others;
 * pyramids, collapse, clamp, void paint and coverage are APS_BLEND_MULTIBAND's.  Accepted wherever APS_BLEND_MULTIBAND is. */
enum { APS_BLEND_NONE = 0, APS_BLEND_LINEAR = 1, APS_BLEND_MULTIBAND = 2, APS_BLEND_MULTIBAND_MAXWEIGHT = 3 };
enum { APS_NONE_LAST = 0, APS_NONE_FIRST = 1, APS_NONE_MAXANGLE = 2 };
enum {
    APS_IMG_U8_HWC = 0,   /* row-major interleaved H x W x C (numpy / torch)            */
    APS_IMG_U8_MATLAB = 1 /* column-major planar H x W x C (MATLAB uint8 array)        */
};

/* One source image + its camera (cameras struct: initializeCameraMatrices.m:114-122). */
typedef struct aps_image {
    const uint8_t* data; /* uint8 pixels, host or device                                        */
    int height, width, channels; /* channels: 1 or 3 (gray is replicated, loadImages.m:62)    */
    int layout;          /* APS_IMG_U8_*                                                        */
    double K[9];         /* 3x3 intrinsics, column-major                                        */
    double R[9];         /* 3x3 world->camera rotation, column-major                            */
    float gain[3];       /* per-channel gain (gainCompensationRKf output row; ones if off)      */
} aps_image;

/* Geometry of the panorama canvas: the values renderPanorama.m:125-232 derives on the host. */
typedef struct aps_canvas {
    int mode;            /* APS_PROJ_*                                                          */
    int height, width;   /* H, W (:137-146,180-189)                                             */
    double f_pan;        /* opts.fPan * opts.resScale enters only through these three:          */
    double origin0;      /* th0 (cyl/sph/miller) or u0 (planar/stereo/fisheye/panini)           */
    double origin1;      /* h0 (cyl), ph0 (sph), y0 (miller) or v0 (planar/stereo/fisheye/panini) */
    double R_ref[9];     /* cameras(refIdx).R, column-major (planar/stereo/fisheye/panini only) */
} aps_canvas;

typedef struct aps_render_opts {
    int tile_h, tile_w;    /* opts.tile — explicit, never derived from free memory */
    float angle_power;     /* opts.anglePower (displayPanorama.m:101: 2)                        */
    int blending;          /* APS_BLEND_*                                                       */
    int pyr_levels;        /* opts.pyrLevels = input.bands                                      */
    float pyr_sigma;       /* opts.pyrSigma  = input.MBBsigma                                   */
    int none_policy;       /* opts.composeNonePolicy                                            */
    int canvas_white;      /* opts.canvasColor == 'white'                                       */
} aps_render_opts;

/* a14-a17: the tile loop of renderPanorama.m:342-425 (ray generation, fuseTile, sampleOneTile,
 * sampleBlock, warpWeights, void paint, uint8 conversion), all tiles, on the device.
 *   pano    : uint8 H x W x 3 in `out_layout` (APS_IMG_U8_HWC or APS_IMG_U8_MATLAB)
 *   covered : uint8 H x W (same 2-D layout), may be NULL. */
int aps_render(const aps_image* images, int n_img, const aps_canvas* canvas,
               const aps_render_opts* opts, int out_layout, uint8_t* pano, uint8_t* covered);

/* The same, restricted to the tiles t (row-major tile index over the canvas) with t % tile_step ==
 * tile_first: tiles are independent in the reference (renderPanorama.m:342-406; pyramids are tile
 * local), so this is the unit of multi-GPU sharding.  Pixels of other tiles are left untouched. */
int aps_render_tiles(const aps_image* images, int n_img, const aps_canvas* canvas,
                     const aps_render_opts* opts, int out_layout, int tile_first, int tile_step,
                     uint8_t* pano, uint8_t* covered);

/* The same for the CONTIGUOUS tiles tile_begin <= t < tile_end of the row-major tile list: a rank that owns a run of
 * neighbouring tiles meets (and converts) only the ~20 of 64 views under its band of the canvas, where tiles dealt
 * t % p meet 47 (round 5; section 6 of DESIGN.md). */
int aps_render_tile_range(const aps_image* images, int n_img, const aps_canvas* canvas, const aps_render_opts* opts, int out_layout,
                          int tile_begin, int tile_end, uint8_t* pano, uint8_t* covered);

/* SURVEY 8(f) rank 2 -- imresize(I, s | [oh ow], 'bicubic' | 'bilinear') on a uint8 image, the preprocessing step in
 * front of SIFT (PP/imageProcessing/resizeImagesToLimits.m:57-61,103; loadImages.m:66-68).  Antialiased on shrink,
 * half-pixel centres, replicate borders, the smaller-scale dimension first, uint8 rounding after each pass.
 * scale_r/scale_c: the per-dimension scales imresize uses (s, s for the scalar form; oh/h, ow/w for the size form). */
enum { APS_RESIZE_BILINEAR = 0, APS_RESIZE_BICUBIC = 1 };
int aps_imresize_u8(const uint8_t* img, int h, int w, int c, int layout, int oh, int ow, double scale_r, double scale_c,
                    int method, uint8_t* out);

/* SURVEY 8(f) rank 3 -- the per-pair blocks of the bundle adjustment's normal equations: the parfor body of
 * accumulateNormalEqnsBlock (PP/bundleAdjustment/bundleAdjustmentRKf.m:717-741) with jacobianPair (:793-899),
 * computeSingleResidual (:1641-1686), computeJacobianWrtCamera (:1688-1783) and huberWeight (:1806-1829).
 * Ui, Uj: total x 2 f64, column-major with leading dimension ldu (x at [k], y at [ldu + k]): the matched points on image
 * i and j of all pairs back to back; pair p owns rows pair_ptr[p] .. pair_ptr[p+1]-1.  cams: per pair four cameras
 * (base i, base j, incremented i, incremented j), 12 f64 each: f, cx, cy, R (3 x 3 column-major, world -> camera).
 * out: per pair 59 f64 = Hii, Hjj, Hij (4 x 4 column-major over [dthx dthy dthz df]), gi, gj (4), E, r2sum, rcnt.
 * A camera with fewer parameters uses the leading rows/columns, as the reference's J(:, 1:numel(cols)) does.
 * both_directions = !opts.OneDirection.  The LM loop, prior, sparse assembly and solve stay with the caller. */
int aps_ba_pair_blocks(const double* Ui, const double* Uj, int64_t ldu, const int64_t* pair_ptr, int n_pairs,
                       const double* cams, double sigma_huber, int both_directions, double* out);

/* The same blocks for a resident problem, assembled on the device: the normal-equation evaluation of the LM loop of
 * bundleAdjustmentRKf (accumulateNormalEqnsBlock, :609-791), a few thousand times per set.
 * aps_ba_problem_create uploads the matched points of every verified pair once (host memory; Ui, Uj, ldu, pair_ptr laid
 * out as for aps_ba_pair_blocks).  pair_ij: 2 x n_pairs int32, the 0-based cameras (i, j) of pair p with i < j < n_cams,
 * pairs sorted by (i, j) without repeats.
 * aps_ba_normal_eqns evaluates at the cameras base_cams (the linearisation point) and lin_cams (base + increments), both
 * n_cams x 12 f64 packed as for aps_ba_pair_blocks.  col_start[k]: camera k's first column of H, or -1 when k is not in
 * camList; n_params[k]: 1 for the seed, 4 otherwise.  The active cameras must tile the columns 0 .. P-1 exactly.  A pair
 * takes part when both its cameras are active and it has matches.  Outputs (host memory): H dense P x P column-major, g
 * (P), stats = {E, rmse}.  want_H = 0: energy only (the LM trial step, :553-555): no Jacobians, H and g untouched (may be
 * NULL), the same E and rmse bits as want_H = 1.
 * Bit contract: H, g, E and rmse equal the host loop of accumulateNormalEqnsBlock over these blocks for a sorted camList
 * (bundleAdjustment.py): every cell and sum starts at +0.0 and takes its blocks in ascending (i, j) order.
 * Errors: APS_E_ARG for a NULL handle, a non-positive sigma, a column map that overlaps or does not cover P. */
typedef struct aps_ba_problem aps_ba_problem;
int aps_ba_problem_create(const double* Ui, const double* Uj, int64_t ldu, const int64_t* pair_ptr, const int* pair_ij,
                          int n_pairs, int n_cams, aps_ba_problem** handle);
int aps_ba_problem_destroy(aps_ba_problem* handle);
int aps_ba_normal_eqns(aps_ba_problem* handle, const double* base_cams, const double* lin_cams, const int* col_start,
                       const int* n_params, int P, double sigma_huber, int both_directions, int want_H, double* H, double* g,
                       double* stats);

/* The data term of bundleAdjustmentH's one-direction residualsJacobian (PP/bundleAdjustment/bundleAdjustmentH.m:282-436,
 * computeUnidirResiduals :512-590, computeJacobianBatch :685-737) on the same resident problem: the refinement of planar
 * sets, whose LM loop (adaptiveLM, :147-279), regulariser rows and solve stay on the host (bundleAdjustment.py).
 * G: n_cams x 9 f64, host memory, row-major absolute homographies with G[9 k + 8] == 1 (n_cams must be the problem's).
 * For match k of pair (i, j): Y = G_i [u v 1]', res = Y_i(1:2) / Y_i(3) - Y_j(1:2) / Y_j(3); Huber weight w = delta / |res|
 * when |res| >= delta (else 1), delta = max(0, huber), 0 turns it off, and w multiplies res itself (as the reference
 * does); the rows of image i are ((dY/dp) Y3 - Y (dY3/dp)) / Y3^2 * w over p = [a b c d e f g h] (row-major, H(3,3) = 1),
 * those of image j the same formula negated.  The seed owns no columns, every other image k the 8 columns from
 * 8 * blk(k), blk counting the non-seed images in index order: P = 8 (n_cams - 1).  Every pair with matches takes part; a
 * pair with the seed adds to the other image's diagonal block and g only.
 * Outputs (host memory): H = J'J dense P x P column-major, g = J'r (P), stats = {sum (w res)^2, sum |res|^2, match count}.
 * want_H = 0: energy only (adaptiveLM's trial step, :211): no Jacobians, H and g untouched (may be NULL), the same stats bits.
 * Bit contract: per pair every sum is 64 lane-strided partials (match k on lane k mod 64, in ascending k; per match the
 * row u term, then the row v term) combined by an xor butterfly (offsets 32, 16, .., 1), every partial starting at +0.0;
 * blocks assembled in ascending (i, j) pair order into cells that start at +0.0, a lone off-diagonal block written as
 * 0.0 + x, the stats summed in pair order.  No fma.  bundleAdjustment.hNormalEqnsMirror restates it in numpy.
 * Errors: APS_E_ARG for a NULL handle or output, a wrong n_cams (or fewer than two), a seed out of range, a non-finite
 * huber, a G that is not host memory or has G[9 k + 8] != 1. */
int aps_ba_h_normal_eqns(aps_ba_problem* handle, const double* G, int n_cams, int seed, double huber, int want_H, double* H,
                         double* g, double* stats);

/* SURVEY 8(f) rank 4 -- the crop rectangle of PP/imageProcessing/panoramaCropper.m:73-165: rgb2gray + imbinarize against
 * `range` (input.blackRange, or input.whiteRange with canvas_white = 1 and the mask complemented), imfill(.,'holes'), and
 * the line-by-line largest-rectangle scan (first maximum in (line, column) order, the last column never part of a
 * rectangle, as in the reference).  img: h x w x 3 uint8 (layout as for the renderers).  rect[0..3] = offsetx, offsety,
 * cropW, cropH, 1-based as in :153-157; the reference then takes rows offsety..offsety+cropH and columns
 * offsetx..offsetx+cropW.  *valid = 0 when that range leaves the image (the reference warns and returns the input). */
int aps_crop_rect(const uint8_t* img, int64_t h, int64_t w, int layout, int canvas_white, double range, int32_t* rect,
                  int32_t* valid);

/* a20: [panoCropped, rect, didCrop] = cropNonzeroBbox(panorama, canvasColor) (renderPanorama.m:1459-1504), the step
 * renderPanorama runs on its output when opts.cropBorder is set (:430-432; displayPanorama.m:101 sets it): bounding box of
 * rgb2gray(panorama) > 0 (black canvas) or < 255 (white canvas), padded by 6 pixels and clipped to the image.
 * img: h x w x 3 uint8 (layout as for the renderers, host or device).  rect = {r1, r2, c1, c2}, 1-based inclusive;
 * *did_crop = 0 and rect = the whole image when there is no foreground.  The caller slices (no pixels are moved here). */
int aps_crop_nonzero_bbox(const uint8_t* img, int64_t h, int64_t w, int layout, int canvas_white, int64_t* rect,
                          int* did_crop);

/* rgbAnnotation of renderPanorama (renderPanorama.m:438-477; planar scans :653-679): the panorama with every image's warped
 * outline (insertShape 'Polygon', LineWidth 2) and its number in a red box at the centroid (insertText), drawn on the device.
 * Both toolbox calls are closed; the raster rule is this library's own ("Annotation contract"; parity with MATLAB
 * unpinned), integer arithmetic throughout, restated byte for byte by tests/annotate_mirror.py.
 *   src, dst : uint8 h x w x 3, APS_IMG_U8_HWC, host or device memory each; dst == src draws in place, otherwise the two must
 *              not overlap and src is never written.
 *   polys    : f64 n x 4 x 2, the corners of polygon p as x then y in 1-based canvas coordinates (pixel (r, c) has its centre
 *              at x = c, y = r); anchors: f64 n x 2 (x, y), where label p's box has its top-left corner; colors: uint8 n x 3.
 *              Host or device memory (they are read on the host: the edges are binned to canvas tiles there).
 *   A polygon is valid when its eight coordinates are finite and |v| <= 2^20; the others are skipped and NOT numbered: the
 *   labels are 1 .. *n_drawn in order of the valid polygons (the reference numbers 1:numel(valid) the same way, :474).
 *   line_width in 1..64: an edge paints every pixel whose centre lies within line_width / 2 of the closed segment between its
 *   corners quantised to 1/16 px (round caps and joins); a later polygon paints over an earlier one; labels (5 x 7 digit font
 *   scaled by 3, box (255, 0, 0) at 60 %, text white) come after all outlines in ascending order; everything is clipped.
 *   *n_drawn (host memory): the number of valid polygons.
 * Cost: one copy src -> dst (none in place), then one workgroup per 64 x 64 canvas tile that an edge or a label touches; one
 * host synchronisation, at the end of the call (a resident result is complete on return).
 * Errors, all before any device work: APS_E_ARG for a NULL pointer (the three tables may be NULL when n == 0), h or w < 1 (or
 * above 2^31 - 1), n < 0, line_width outside 1..64, partially overlapping src / dst. */
int aps_annotate_panorama(const uint8_t* src, int64_t h, int64_t w, const double* polys, const double* anchors,
                          const uint8_t* colors, int n, int line_width, uint8_t* dst, int* n_drawn);

/* Marks on an image: the drawing under showMatchedFeatures(I1, I2, p1, p2, 'montage') as refineMatch calls it with
 * input.showKeypointsPlot (imageMatching.m:257-269), and under keypoint plots.  The toolbox call is closed; the raster rule is
 * this library's own ("Mark contract"; parity with MATLAB unpinned), integer arithmetic throughout, restated byte
 * for byte by tests/marks_mirror.py.  A mark is a segment or a ring with its own line width and opaque colour. */
#define APS_MARK_SEGMENT 0
#define APS_MARK_RING    1
typedef struct aps_mark {
    double x0, y0, x1, y1;   /* ring: x1 = radius, y1 unused */
    int32_t kind, line_width;
    uint8_t rgb[3], reserved;
} aps_mark;

/*   src, dst : uint8 h x w x 3, APS_IMG_U8_HWC, host or device memory each; dst == src draws in place, otherwise the two must
 *              not overlap and src is never written.
 *   marks    : n marks, HOST memory.  Coordinates are 1-based f64, x = column (pixel (r, c) has its centre at x = c, y = r),
 *              quantised to 1/16 px.  A segment paints every pixel whose centre lies within line_width / 2 of the closed segment
 *              (round caps; equal end points give a dot).  A ring paints every pixel whose centre lies between radius -
 *              line_width / 2 (not below 0) and radius + line_width / 2 of the centre (x0, y0), both closed; radius 0 is a disc.
 *   A mark is valid when its coordinates are finite with |v| <= 2^20 and, for a ring, the radius is finite with
 *   0 <= radius <= 4096 (y1 is not looked at); the others are skipped and not counted.  Marks are drawn in ascending index: where
 *   they overlap the highest index wins.  Everything is clipped; a valid mark wholly outside the canvas counts.
 *   *n_drawn (host memory, may be NULL): the number of valid marks.  n = 0 is a plain copy.
 * Cost: one copy src -> dst (none in place), then one workgroup per 64 x 64 tile that a mark can touch; one host
 * synchronisation, at the end of the call (a resident result is complete on return).  Runs on the calling thread's stream.
 * Errors, all before any device work and with nothing written: APS_E_ARG for a NULL pointer (marks may be NULL when n == 0),
 * h or w < 1 (or above 2^31 - 1), n < 0, any mark with a kind other than 0 / 1 or a line_width outside 1..64, partially
 * overlapping src / dst, or tile lists of 2^31 - 1 entries or more. */
int aps_draw_marks(const uint8_t* src, int64_t h, int64_t w, const aps_mark* marks, int64_t n, uint8_t* dst,
                   int64_t* n_drawn);

/* The 'montage' of showMatchedFeatures: dst = uint8 max(h1, h2) x (w1 + w2) x 3 with img1 (h1 x w1 x 3) in rows 1..h1, columns
 * 1..w1, img2 in rows 1..h2, columns w1 + 1..w1 + w2, and 0 everywhere else.  Each pointer is host or device memory; dst must
 * not overlap either source.  Two strided copies and a fill on the calling thread's stream; complete on return.
 * Errors: APS_E_ARG for a NULL pointer, a size below 1 (or a destination side above 2^31 - 1), or an overlapping destination. */
int aps_montage_pair(const uint8_t* img1, int64_t h1, int64_t w1, const uint8_t* img2, int64_t h2, int64_t w2, uint8_t* dst);

/* SURVEY 8(f) rank 1 -- the overlap statistics of gainCompensationRKf (PP/gainCompensation/gainCompensationRKf.m:96-149,
 * 239-367): every `stride`-th canvas point (1-based coordinates, :106-107) that two images i < j both cover
 * (front, inside, tent weight > 0) adds 1 to n_ij(i,j) and the two bilinear RAW (0..255) colour samples to
 * sum_ci(i,j,:) / sum_cj(i,j,:).  Outputs: f64 N x N and N x N x 3, column-major, upper triangle, zero elsewhere.
 * The N x N solve for the gains (:151-238) stays on the host.  Sums are added in an unspecified order: compare
 * them with a relative tolerance (the reference itself sums in single per tile); counts are exact. */
int aps_gain_overlap_stats(const aps_image* images, int n_img, const aps_canvas* canvas, int stride,
                           double* n_ij, double* sum_ci, double* sum_cj);

/* SURVEY 8(f) rank 1, planar scans -- the overlap statistics of gainCompensationH
 * (PP/gainCompensation/gainCompensationH.m:45-52,78-149; caller renderPanorama.m:584-588).  iw[k]: the k-th image warped to
 * the common canvas, f32 height x width x channels; ww[k]: its weight map, f32 height x width (host or device memory, like
 * every other buffer of this library; layout APS_ROWMAJOR = interleaved rows as C / numpy hold them, APS_COLMAJOR = MATLAB's
 * planar column-major arrays).  Every `downsample`-th row and column of the canvas is sampled (1:ds:end, :45-52); a sample
 * is valid for image k when ww[k] > 0 and all channels are finite (:117); each pair i < j valid there adds 1 to n_ij(i,j)
 * and its two colours to sum_ci(i,j,:) / sum_cj(i,j,:), accumulated in double (:126-146).  Outputs as aps_gain_overlap_stats:
 * f64 N x N and N x N x 3, column-major, upper triangle.  Sums are added in an unspecified order (compare with a relative
 * tolerance); counts are exact.  The edge selection and the N x N solve (:152-223) stay on the host. */
int aps_gain_overlap_stats_warped(const float* const* iw, const float* const* ww, int n_img, int64_t height, int64_t width,
                                  int channels, int layout, int downsample, double* n_ij, double* sum_ci, double* sum_cj);

/* a15/a16 for ONE tile, layers out (for tests): rows r0..r0+ht-1, cols c0..c0+wt-1 (0-based) of
 * the canvas sampled from ONE image.  S: f32 ht x wt x 3 row-major interleaved, Wang/Wf: f32 ht x wt,
 * M: uint8 ht x wt (sampleOneTile, renderPanorama.m:1063-1146). */
int aps_warp_tile(const aps_image* image, const aps_canvas* canvas, int r0, int c0, int ht, int wt,
                  float angle_power, float* S, uint8_t* M, float* Wang, float* Wf);

/* a21: F = multiBandBlending(Ci, Wi, levels, onGPU, sigma) (multiBandBlending.m:45-171).
 *   C: f32 K x h x w x 3 (row-major interleaved per layer), Wt: f32 K x h x w, F: f32 h x w x 3. */
int aps_multiband_blend(const float* C, const float* Wt, int k, int h, int w, int levels,
                        float sigma, float* F);

/* The max-weight partition, the stand-alone partner of aps_multiband_blend ("Max-weight multiband contract"):
 * out[k] = 1.0f at the pixels where layer k is the FIRST layer of maximal weight and that maximum is > 0 (written `w > best`,
 * so a NaN never owns), 0.0f elsewhere; a pixel without a positive weight has no owner.
 *   Wt, out: f32 k x h x w as aps_multiband_blend takes Wt, host or device memory; out may alias Wt.  No cap on k.
 * Errors: APS_E_ARG for a NULL pointer, k < 1, h < 1 or w < 1, before any device work. */
int aps_maxweight_weights(const float* Wt, int k, int h, int w, float* out);

/* a22: linearBlending (linearBlending.m:46-115) on f32 layers: sum(I.*W)/max(sum(W),eps('single')). */
int aps_linear_blend(const float* C, const float* Wt, int k, int h, int w, float* F);

/* a19: warped = imageWarp(image, tform, outputView, 'bilinear') (imageWarp.m:39-168) for uint8 or
 * f32 images: inverse homography warp onto an imref2d-like grid, valid only when all four taps are
 * inside (:133), fill value elsewhere.
 *   H: f64 3x3 column-major; x0,y0,sx,sy: outputView.XWorldLimits(1), YWorldLimits(1),
 *   PixelExtentInWorldX/Y (:36-41).  in/out: row-major interleaved h x w x c. */
int aps_image_warp_h_u8(const uint8_t* in, int in_h, int in_w, int c, const double* H, int out_h,
                        int out_w, double x0, double y0, double sx, double sy, uint8_t fill,
                        uint8_t* out);
int aps_image_warp_h_f32(const float* in, int in_h, int in_w, int c, const double* H, int out_h,
                         int out_w, double x0, double y0, double sx, double sy, float fill,
                         float* out);
/* The same with options.method: 'nearest' (imageWarp.m:109-123: round(src), valid inside [1,w] x [1,h]), 'bilinear'
 * (:125-168) or 'bicubic' (:170-264: Keys kernel bicubicKernel :275-301 on the 4 x 4 taps around floor(src), valid for
 * 2 <= floor(src) <= size - 2, x direction first, result clamped to [0, 255] and rounded for uint8, to [0, 1] for f32, where a NaN gives 1: MATLAB's min and max skip it). */
enum { APS_WARP_NEAREST = 0, APS_WARP_BILINEAR = 1, APS_WARP_BICUBIC = 2 };
int aps_image_warp_u8(const uint8_t* in, int in_h, int in_w, int c, const double* H, int out_h, int out_w, double x0,
                      double y0, double sx, double sy, uint8_t fill, int method, uint8_t* out);
int aps_image_warp_f32(const float* in, int in_h, int in_w, int c, const double* H, int out_h, int out_w, double x0,
                       double y0, double sx, double sy, float fill, int method, float* out);

/* Planar scans -- pureNonRotationalPanoramas on the device (PP/renderPanorama/renderPanorama.m:519-699; the warp of
 * PP/imageProcessing/imageWarp.m:125-168; the statistics of PP/gainCompensation/gainCompensationH.m).  One call takes the uint8
 * images and their H2refined homographies and returns the uint8 panorama; no canvas-sized array visits the host.
 *   images[k]: uint8 img_h[k] x img_w[k] x img_c[k] (c = 1 or 3), row-major interleaved, host or device memory like every other
 *   buffer of this library; sizes may differ per image.  H: n_img 3x3 f64 matrices, column-major each, as aps_image_warp_* takes
 *   them.  out_h, out_w, x0, y0, sx, sy: the canvas (imref2dScratch: ImageSize, XWorldLimits(1), YWorldLimits(1),
 *   PixelExtentInWorldX/Y); its size is the caller's computation (outputLimitsScratch, :547-575) and is not re-derived here.
 *   blending: APS_BLEND_*; levels, sigma: multiBandBlending's (used by APS_BLEND_MULTIBAND and APS_BLEND_MULTIBAND_MAXWEIGHT
 *   only; the byte formulas return for the latter what they return for the former).  white_canvas: void pixels
 *   (no image has weight > 0 there) become 255 instead of 0.  gains: f32 n_img x 3 row-major, or NULL for ones (:584-591: one
 *   f32 multiply per channel after the warp).  pano: uint8 out_h x out_w x 3 row-major interleaved (a single-channel image is
 *   replicated); covered (optional, may be NULL): uint8 out_h x out_w, 1 where some image has weight > 0.
 * Per canvas pixel and image: source value (float)u8 / 255, the inverse map, validity test and four-tap f64 sum of
 * aps_image_warp_f32 'bilinear' (fill 0), the weight = the same warp of warpWeights' tent map (:1282-1312) clamped to [0, 1];
 * 'none' = the first image of maximal weight, 'linear' = linearBlending, 'multiband' = multiBandBlending and max(0, min(1, .));
 * then uint8(round(255 * v)) with the product in f64 and MATLAB's round.  The result equals, byte for byte, what
 * aps_image_warp_f32 + aps_multiband_blend / aps_linear_blend and the host arithmetic between them give.  Every image is
 * written and read inside its footprint only (the canvas bounding box of its forward-mapped border, grown conservatively; the
 * whole canvas when the homography's denominator changes sign over the image); APS_PLANAR_NO_CULL=1 in the environment forces
 * whole-canvas footprints (same bytes).
 * Before its first launch the call compares aps_planar_composite_bytes(...) with the free device memory and returns APS_E_OOM
 * with a message naming both figures when the composite cannot fit (renderPanorama.m:245-266: skip this panorama).
 * Errors: APS_E_ARG for a NULL argument, n_img < 1, an unknown blending, levels < 1, sigma <= 0 (or one whose filter has more
 * than 9 taps), non-positive sx / sy, a singular or non-finite homography; APS_E_DIM for a bad image or canvas size and for more
 * than 64 images (the limit of the weight normalisation's layer mask, as in the tiled renderer).  None of them reaches a launch. */
int aps_planar_composite(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                         const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int blending, int levels,
                         float sigma, int white_canvas, const float* gains, uint8_t* pano, uint8_t* covered);
/* Host only (no device needed): the device memory aps_planar_composite requests for these shapes, in bytes, or a negative
 * APS_E_* code for arguments the composite would refuse.  With P = out_h * out_w and sum over the images:
 *   sum(h*w*c) + 4 * sum(h + w)      staged images, tent tables
 *   + 160 * n + 16 * n * P           job table, float4 layers
 *   + P + 3 * P                      coverage, panorama
 * and for APS_BLEND_MULTIBAND, with L = max(1, min(levels, floor(log2(min(out_h, out_w))))), P_0 = P, P_l the pixels of level l
 * (each side max(1, floor(side / 2)) of the level above), D = P_1 + .. + P_(L-1), I = P_1 + .. + P_(L-2):
 *   + 16 * P                         blended image
 *   + 16 * n * D                     Gaussian levels 1..L-1 of every layer
 *   + 16 * min(n, 16) * P if L > 1   blurred level of one batch of layers
 *   + 16 * (P + D) + 16 * I          numerator pyramid, collapse buffers
 * (Requests are rounded up to 256 bytes each by the workspace pool; images and outputs already in device memory are not
 * staged, so the figure is an upper bound for them.) */
int64_t aps_planar_composite_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, int out_h, int out_w,
                                   int blending, int levels);
/* gainCompensationH's overlap statistics (gainCompensationH.m:45-52,78-149) from the same resident layers, before gains: every
 * `downsample`-th row and column of the canvas, valid = weight > 0 and finite colour, pairs i < j whose footprints intersect.
 * Arguments as aps_planar_composite, outputs as aps_gain_overlap_stats_warped (f64 N x N and N x N x 3, column-major, upper
 * triangle; counts exact, sums in an unspecified order).  The N x N solve stays with the caller, who passes the gains to
 * aps_planar_composite; that call warps again and applies them with the same single f32 multiply. */
int aps_planar_gain_stats(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                          const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                          double* n_ij, double* sum_ci, double* sum_cj);
/* The footprint-compact planar compositor (PP/renderPanorama/renderPanorama.m:519-699, PP/imageProcessing/imageWarp.m:125-168,
 * PP/blending/multiBandBlending.m:72-167, PP/gainCompensation/gainCompensationH.m:45-52,78-149): arguments, semantics, argument
 * errors and result BYTES of aps_planar_composite, for scan sets that call cannot take -- many views, each covering a small part
 * of a large canvas.  Every layer is stored inside its footprint only (its own pitch), at level 0 and at every pyramid level
 * (the footprint grown by the filter radius, mapped through the resize, clipped to the level: the rectangles the dense call
 * confines its kernels to); a horizon-crossing homography makes that one layer canvas-sized; APS_PLANAR_NO_CULL=1 makes them
 * all canvas-sized (same bytes).  The host builds, per level and 64 x 64 block of the canvas, the ascending list of images
 * whose footprint meets the block and uploads the lists once; weight normalisation, 'none', 'linear', the Laplacian
 * accumulation (one pass per level for all contributors) and the gain statistics walk the list of their block, so the work
 * per pixel follows the overlap and not n_img.  Per pixel the layer arithmetic is the dense call's (one shared device
 * function), every sum runs in ascending image order from +0.0, the Gaussian and resize chains are those of the dense
 * pyramid, the uint8 tail is the same.
 * Limits: no cap on n_img other than int32 indexing: n_img * (2 * L - 1) and the total length of the contributor lists (below)
 * must stay under 2^31 (APS_E_DIM otherwise); out_h * out_w < 2^31 as in the dense call.
 * Before its first launch the call compares aps_planar_composite_compact_bytes(...) with the free device memory and returns
 * APS_E_OOM naming both figures.  One host synchronisation, at the end of the call. */
int aps_planar_composite_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                 const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int blending,
                                 int levels, float sigma, int white_canvas, const float* gains, uint8_t* pano, uint8_t* covered);
/* Host only (no device needed): the device memory aps_planar_composite_compact requests, in bytes, or a negative APS_E_* code
 * for arguments the composite would refuse.  The footprints depend on the homographies and the canvas, so they are arguments.
 * With P = out_h * out_w, L = 1 for 'none' / 'linear' and max(1, min(levels, floor(log2(min(out_h, out_w))))) for multiband,
 * G(l,k) the footprint of image k at level l (G(0,k) = aps_planar_footprints; B(l,k) = G(l,k) grown by r = 4 on every side and
 * clipped to the level; G(l+1,k) = the output pixels of the resize that can see B(l,k)), |.| the pixels of a
 * rectangle, blocks(l) = ceil(h_l / 64) * ceil(w_l / 64), entries(l) = sum over k of the 64 x 64 blocks G(l,k) meets:
 *   sum(h*w*c) + 4 * sum(h + w)                      staged images, tent tables
 *   + 160 * n + 32 * n * (2 * L - 1)                 job table, layer tables (levels and blurred levels)
 *   + 16 * sum_l sum_k |G(l,k)|                      float4 layers, every level, inside their footprints
 *   + 16 * max_(l < L-1) sum_k |B(l,k)|              blurred layers of one level (0 for L = 1)
 *   + 4 * sum_l (blocks(l) + 1 + entries(l))         contributor lists
 *   + P + 3 * P                                      coverage, panorama
 * and for APS_BLEND_MULTIBAND, with D and I as in aps_planar_composite_bytes:
 *   + 16 * P + 16 * (P + D) + 16 * I                 blended image, numerator pyramid, collapse buffers
 * No term multiplies n by P.  r = 4 is the radius of the widest filter built (9 taps): the formula does not take sigma, and a
 * narrower filter requests less. */
int64_t aps_planar_composite_compact_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, const double* H,
                                           int out_h, int out_w, double x0, double y0, double sx, double sy, int blending,
                                           int levels);
/* aps_planar_gain_stats from the compact layers (gainCompensationH.m:45-52,78-149): same arguments, outputs and tolerance
 * contract (counts exact, sums in an unspecified order); the pairs of a sampled point are taken from its block's list.
 * n_img <= 65535 (a pair is keyed i * n_img + j + 1 in 32 bits; the three outputs hold 7 * n_img^2 doubles); APS_E_DIM above. */
int aps_planar_gain_stats_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                  const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                                  double* n_ij, double* sum_ci, double* sum_cj);
/* Host only, for tests and callers that plan memory: the footprints aps_planar_composite uses (without APS_PLANAR_NO_CULL).
 * rects: int n_img x 4 = (x0, y0, x1, y1), 0-based half-open canvas columns and rows, clipped to the canvas; whole (optional):
 * 1 where the whole-canvas fallback was taken (horizon across or too close to the image). */
int aps_planar_footprints(int n_img, const int* img_h, const int* img_w, const double* H, int out_h, int out_w, double x0, double y0,
                          double sx, double sy, int* rects, int* whole);
/* Host only: warpWeights' 1-D tent factor of length n (renderPanorama.m:1282-1312), f32, as the composite builds it. */
int aps_planar_tent(int n, float* t);

/* ============================================================================================
 * (4) SIFT — PP/featureMatching/getFeaturePoints.m:36-40,71-74
 * ============================================================================================ */

typedef struct aps_sift_params {
    double sigma;              /* input.Sigma              (inputs.m:34: 1.6)     */
    int n_layers;              /* input.NumLayersInOctave  (inputs.m:35: 4)       */
    double contrast_threshold; /* input.ContrastThreshold  (inputs.m:36: 0.00133) */
    double edge_threshold;     /* input.EdgeThreshold      (inputs.m:40: 6)       */
    int max_features;          /* capacity guard; 0 = library default (262144)    */
} aps_sift_params;

/* a1: [features, validPts] = getFeaturePoints(input, img) for detector 'SIFT': rgb2gray, Lowe/OpenCV
 * SIFT (detectSIFTFeatures + extractFeatures are closed toolbox code; the algorithm restated is
 * OpenCV's cv::SIFT, which the toolbox is documented to wrap — see DESIGN.md "SIFT contract").
 *   desc : f32 count x 128, `desc_layout` with leading dimension ldd, unit L2 norm
 *   loc  : f64 count x 2 [x y], 1-based sub-pixel, column-major with leading dimension ldl
 *   aux  : f32 count x 4 row-major [scale(size), angle_deg, response, octave_layer] or NULL
 * cap = rows available in desc/loc/aux; *count = features found (APS_E_CAP if cap is too small).
 * Feature order is canonical: ascending (octave, layer, row, col, orientation bin). */
int aps_sift_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_sift_params* params, float* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_sift_extract for a group of views of one shape (height x width x channels, img_layout): every stage runs once for the group -
 * one launch per pyramid plane, one extrema sweep, one launch of each per-keypoint kernel - where n_views single calls run it
 * n_views times.  The rows of view k are bit for bit those of aps_sift_extract on views[k].img, in the same order. */
#define APS_SIFT_MAX_VIEWS 16
typedef struct aps_sift_view {
    const uint8_t* img;   /* H x W x channels, host or device, as aps_sift_extract */
    float* desc; double* loc; float* aux;   /* per-view outputs, host or device; aux may be NULL */
    int64_t cap;          /* rows of room in this view's outputs */
    int64_t count;        /* out: rows found (on APS_E_CAP: rows needed) */
} aps_sift_view;
/* n_views in 1..APS_SIFT_MAX_VIEWS (else APS_E_ARG, as for a NULL views or a NULL views[k].img).  desc_layout, ldd and ldl hold for
 * every view; count-only mode, padding, layouts and host / device pointers behave as aps_sift_extract's, view by view.  When any
 * view's rows exceed its cap nothing is written and the call returns APS_E_CAP with EVERY view's count set to the rows it needs, so
 * one retry is enough.  A view without features gets count = 0 and does not touch the others.  params->max_features is the candidate
 * capacity of each view.  The pyramids of the group live side by side: n_views x 1.24 GB of workspace for 4K views.  The call runs on
 * the calling thread's stream with that thread's workspace. */
int aps_sift_extract_batch(aps_sift_view* views, int n_views, int height, int width, int channels,
                           int img_layout, const aps_sift_params* params,
                           int desc_layout, int64_t ldd, int64_t ldl);

/* SIFT strongest-N (DESIGN.md "Strongest-N for SIFT and SURF"; cv::SIFT's nfeatures, selectStrongest): of the rows aps_sift_extract
 * returns for the same image and parameters (the candidates, in canonical order), keep the first min(n_strongest, candidates) by
 * (aux's response = the keypoint's contrast descending, compared as f32; canonical index ascending).  No quota per octave.  The unit
 * is the output row: the orientations of one keypoint tie and the lower orientation bin stays. */
typedef struct aps_sift_strongest_params {
    aps_sift_params sift;      /* sift.max_features keeps its meaning: the candidate capacity of the detection */
    int n_strongest;           /* N >= 1; anything else is APS_E_ARG before any device work */
} aps_sift_strongest_params;

/* Arguments, count-only mode, padding, layouts and pointers behave as aps_sift_extract's.  *count = rows kept;
 * cap >= min(candidates, n_strongest) always suffices.  With cap below the rows kept nothing is written (APS_E_CAP, *count = rows
 * kept).  The kept rows come in canonical order, and descriptor, location and aux of a kept row are bit for bit those of the same row
 * of aps_sift_extract; only kept rows are described.  n_strongest >= candidates gives aps_sift_extract's result. */
int aps_sift_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_sift_strongest_params* params, float* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_sift_extract_strongest for a group of views of one shape: aps_sift_extract_batch's chain with the selection as one more stage
 * of the group.  The rows of view k (descriptor, location, aux, order and count) are bit for bit those of aps_sift_extract_strongest
 * on views[k].img with the same params, whatever the other views contain; views[k].count = rows kept, and
 * views[k].cap >= min(candidates_k, n_strongest) always suffices.  When any view's kept rows exceed its cap nothing is written and the
 * call returns APS_E_CAP with EVERY view's count set to the rows it needs.  A view without features gets count = 0 and does not touch
 * the others; sift.max_features stays the candidate capacity of each view.  Before any device work: n_strongest < 1, n_views outside
 * 1..APS_SIFT_MAX_VIEWS, a NULL views, params or views[k].img are APS_E_ARG.  Count-only mode, padding, layouts and host / device
 * pointers behave view by view as aps_sift_extract_batch's.  One sort, one flag pass, one ballot and scan and one compaction select
 * for all the views, with no read-back beyond aps_sift_extract_batch's; only kept rows are described. */
int aps_sift_extract_batch_strongest(aps_sift_view* views, int n_views, int height, int width, int channels,
                                     int img_layout, const aps_sift_strongest_params* params,
                                     int desc_layout, int64_t ldd, int64_t ldl);

/* ============================================================================================
 * (4b) SURF — PP/featureMatching/getFeaturePoints.m:54-55,71-74
 * ============================================================================================ */

typedef struct aps_surf_params {
    double metric_threshold;   /* detectSURFFeatures MetricThreshold (1000) */
    int n_octaves;             /* getFeaturePoints.m:55: 8 */
    int n_scale_levels;        /* 4 (>= 3) */
    int upright;               /* 0 */
    int max_features;          /* capacity guard; 0 = library default (none beyond cap) */
} aps_surf_params;

/* [features, validPts] = getFeaturePoints(input, img) for detector 'SURF' (getFeaturePoints.m:54-55,71-74): rgb2gray,
 * detectSURFFeatures(gray, 'NumOctaves', 8), extractFeatures.  Both toolbox calls are closed code; the algorithm restated is
 * SURF of Bay et al. (2008) with the parameters that call implies — see DESIGN.md "SURF contract", which fixes every
 * operation and its order (parity with MATLAB is unpinned).
 *   desc : f32 count x 64, `desc_layout` with leading dimension ldd >= 64 (row-major) / >= cap (column-major), unit L2 norm;
 *          row-major with ldd >= 128: columns 64..127 are zeroed as well, so resident rows feed the 128-wide matchers
 *   loc  : f64 count x 2 [x y], 1-based sub-pixel, column-major with leading dimension ldl >= cap
 *   aux  : f32 count x 4 row-major [scale, angle_deg, metric, sign_of_laplacian] or NULL
 * cap = rows available in desc/loc/aux; *count = features found (APS_E_CAP if cap is too small; desc = NULL or cap = 0 counts).
 * Images with height * width * 255 >= 2^32 are refused with APS_E_ARG (the integral image holds exact 32-bit sums).
 * Host and device pointers are accepted; the call runs on the calling thread's library stream.
 * Feature order is canonical: ascending (octave, level, row, col). */
int aps_surf_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_surf_params* params, float* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* SURF strongest-N (DESIGN.md "Strongest-N for SIFT and SURF"; selectStrongest): of the rows aps_surf_extract returns for the same
 * image and parameters (the candidates, in canonical order), keep the first min(n_strongest, candidates) by (aux's metric descending,
 * compared as f32; canonical index ascending).  No quota per octave. */
typedef struct aps_surf_strongest_params {
    aps_surf_params surf;      /* surf.max_features keeps its meaning: the call fails when the detection finds more candidates */
    int n_strongest;           /* N >= 1; anything else is APS_E_ARG before any device work */
} aps_surf_strongest_params;

/* Arguments, count-only mode, padding, layouts, pointers and the zeroing of columns 64..127 behave as aps_surf_extract's.
 * *count = rows kept; cap >= min(candidates, n_strongest) always suffices.  With cap below the rows kept nothing is written
 * (APS_E_CAP, *count = rows kept).  The kept rows come in canonical order, and descriptor, location and aux of a kept row are those of
 * the same row of aps_surf_extract; only kept rows are described.  n_strongest >= candidates gives aps_surf_extract's result.
 * The call reads back the candidate count, then the final count. */
int aps_surf_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_surf_strongest_params* params, float* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_surf_extract for a group of views of one shape (height x width x channels, img_layout): every stage runs once for the group -
 * the three integral-image launches, one detection launch per octave, one scan, one compaction, one per-keypoint launch - where
 * n_views single calls run it n_views times.  The rows of view k (descriptor, location, aux, order and count) are bit for bit those
 * of aps_surf_extract on views[k].img with the same params, whatever the other views hold. */
#define APS_SURF_MAX_VIEWS 16
typedef struct aps_surf_view {
    const uint8_t* img;   /* H x W x channels, host or device, as aps_surf_extract */
    float* desc; double* loc; float* aux;   /* per-view outputs, host or device; aux may be NULL */
    int64_t cap;          /* rows of room in this view's outputs */
    int64_t count;        /* out: rows found (on APS_E_CAP: rows needed) */
} aps_surf_view;
/* n_views in 1..APS_SURF_MAX_VIEWS (else APS_E_ARG, as for a NULL views, params or views[k].img, an image the 32-bit integral image
 * cannot hold and every parameter range aps_surf_extract checks - all before any device work).  desc_layout, ldd and ldl hold for
 * every view; host / device pointers, row-major / column-major layout, padding, the rows count..cap that are never written and the
 * zeroing of columns 64..127 with ldd >= 128 behave as aps_surf_extract's, view by view.  When any view's rows exceed its cap (a
 * view with desc = NULL or cap = 0 only counts) nothing is written and the call returns APS_E_CAP with EVERY view's count set to the
 * rows it needs, so one retry is enough.  A view without features gets count = 0 and does not touch the others.
 * params->max_features keeps its meaning per view.  The call reads back once, for all counts; it runs on the calling thread's
 * stream with that thread's workspace, which holds the views' integral images side by side: 8 bytes per pixel and view. */
int aps_surf_extract_batch(aps_surf_view* views, int n_views, int height, int width, int channels,
                           int img_layout, const aps_surf_params* params,
                           int desc_layout, int64_t ldd, int64_t ldl);

/* aps_surf_extract_strongest for a group of views of one shape: aps_surf_extract_batch's chain with the selection as one more stage
 * of the group, the view being the selection's group.  The rows of view k are bit for bit those of aps_surf_extract_strongest on
 * views[k].img with the same params, whatever the other views hold; views[k].count = rows kept, and
 * views[k].cap >= min(candidates_k, n_strongest) always suffices.  Arguments, capacities, APS_E_CAP with nothing written and every
 * count set, and the checks are aps_surf_extract_batch's, with n_strongest < 1 refused (APS_E_ARG) before any device work;
 * surf.max_features is tested against each view's candidates.  One sort, one flag pass, one ballot and scan and one compaction
 * select for all the views.  The call reads back twice, as aps_surf_extract_strongest does: the views' candidate counts, then the
 * counts kept. */
int aps_surf_extract_batch_strongest(aps_surf_view* views, int n_views, int height, int width, int channels,
                                     int img_layout, const aps_surf_strongest_params* params,
                                     int desc_layout, int64_t ldd, int64_t ldl);

/* ============================================================================================
 * (4c) FAST + FREAK — PP/featureMatching/getFeaturePoints.m:51-52,71-74
 * ============================================================================================ */

typedef struct aps_fast_params {
    int threshold;             /* t = floor(MinContrast * 255), evaluated by the caller (detectFASTFeatures: MinContrast 0.2 -> 51) */
    int quality_num;           /* MinQuality as the rational quality_num / quality_den (0.1 -> 100000 / 1000000) */
    int quality_den;
    int max_features;          /* capacity guard; 0 = none beyond cap */
} aps_fast_params;

/* [features, validPts] = getFeaturePoints(input, img) for detector 'FAST' (getFeaturePoints.m:51-52,71-74): rgb2gray,
 * detectFASTFeatures(gray), extractFeatures - which describes corner points with FREAK: 512 bits in 64 bytes, the binary
 * family of inputs.m:31-33 that matchFeaturesScratch.m:81-135,170-171 and featureMatchingGlobal.m:54-120 take as
 * binaryFeatures.  Both toolbox calls are closed code; the algorithms restated are FAST-9 (Rosten & Drummond) and FREAK
 * (Alahi, Ortiz & Vandergheynst) - see DESIGN.md "FAST/FREAK contract", which fixes every operation in integer arithmetic
 * (parity with MATLAB is unpinned).
 *   desc : u8 count x 64, `desc_layout` with leading dimension ldd >= 64 (row-major) / >= cap (column-major); bit i of a
 *          descriptor is bit (i % 8), LSB first, of byte i / 8
 *   loc  : f64 count x 2 [x y], 1-based, integer-valued, column-major with leading dimension ldl >= cap
 *   aux  : f32 count x 4 row-major [metric = FAST score, orientation bin 0..255, 0, 0] or NULL
 * cap = rows available in desc/loc/aux; *count = features found (APS_E_CAP if cap is too small; desc = NULL or cap = 0 counts).
 * Elements outside the logical result (padding of ldd / ldl, rows count..cap) are not written.
 * Images with height * width * 255 >= 2^32 are refused with APS_E_ARG (the integral image holds exact 32-bit sums).
 * Host and device pointers are accepted; the call runs on the calling thread's library stream.
 * Feature order is canonical: ascending (row, col). */
int aps_fast_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_fast_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* FAST/FREAK over a scale pyramid (DESIGN.md "FAST/FREAK scale pyramid"; the parameter names are detectORBFeatures' NumLevels and
 * ScaleFactor).  ScaleFactor is the rational scale_num / scale_den = round(ScaleFactor * 10^6) / 10^6, evaluated by the caller;
 * scale_den < scale_num <= 2 * scale_den and n_levels in 1..16, everything else is APS_E_ARG. */
typedef struct aps_fast_pyramid_params {
    aps_fast_params fast;
    int n_levels;              /* NumLevels: levels asked for; the plan ends earlier where a level has no admissible pixel */
    int scale_num;             /* ScaleFactor (1.2 -> 1200000 / 1000000) */
    int scale_den;
} aps_fast_pyramid_params;

/* aps_fast_extract on every level of the plan: level 0 is the rgb2gray plane, level l is level l - 1 resampled (bilinear, half-pixel
 * centres, 8-bit weights, integer arithmetic), and each level goes through the FAST/FREAK contract unchanged, with its own s_max.
 * Arguments, capacity, count-only mode, padding and pointers behave as aps_fast_extract's.  Differences in the outputs:
 *   loc  : the pixel's centre in level-0 coordinates, 1-based: f64((2 x_l + 1) * width) / f64(2 * w_l) + 0.5, and y alike
 *          (level 0: x_l + 1 exactly)
 *   aux  : [FAST score, orientation bin, level, 0]
 * Feature order is canonical: ascending (level, row, col).  A corner may be reported at several levels.
 * n_levels = 1 gives aps_fast_extract's result. */
int aps_fast_extract_pyramid(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_fast_pyramid_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_fast_extract_pyramid for a group of views of one shape (n_levels = 1: aps_fast_extract's plan): every stage runs once for the
 * group - the integral-image launches and one resampling launch per level, one detection launch, one segmented maximum for the
 * quality gate's s_max per (view, level), one gate, one scan, one compaction, one FREAK launch - where n_views single calls run it
 * n_views times.  The views share one plan; planes, score planes, integral images and bitmap words are packed [view][level].  The
 * rows of view k (descriptor, location, aux = [score, bin, level, 0], order and count) are byte for byte those of
 * aps_fast_extract_pyramid on views[k].img with the same params, whatever the other views hold. */
#define APS_FAST_MAX_VIEWS 16
typedef struct aps_fast_view {
    const uint8_t* img;   /* H x W x channels, host or device, as aps_fast_extract */
    uint8_t* desc; double* loc; float* aux;   /* per-view outputs, host or device; aux may be NULL */
    int64_t cap;          /* rows of room in this view's outputs */
    int64_t count;        /* out: rows found (on APS_E_CAP: rows needed) */
} aps_fast_view;
/* n_views in 1..APS_FAST_MAX_VIEWS (else APS_E_ARG, as for a NULL views, params or views[k].img, an image the 32-bit integral image
 * cannot hold and every parameter range aps_fast_extract_pyramid checks - all before any device work).  desc_layout, ldd and ldl
 * hold for every view; host / device pointers, row-major / column-major layout, padding and the rows count..cap that are never
 * written behave as aps_fast_extract's, view by view.  When any view's rows exceed its cap (a view with desc = NULL or cap = 0 only
 * counts) nothing is written and the call returns APS_E_CAP with EVERY view's count set to the rows it needs, so one retry is
 * enough.  A view without features gets count = 0 and does not touch the others.  fast.max_features keeps its meaning per view.
 * The call reads back once, for all counts; it runs on the calling thread's stream with that thread's workspace.
 * aps_fast_extract_strongest and aps_fast_extract_uniform have no group form: their selection group is a level, and a group of
 * views would need views x levels of them. */
int aps_fast_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels,
                           int img_layout, const aps_fast_pyramid_params* params,
                           int desc_layout, int64_t ldd, int64_t ldl);

/* The plan of that call (host only, needs no device): h_0 = height, h_l = floor((2 h_{l-1} scale_den + scale_num) / (2 scale_num)),
 * widths alike; the plan ends before the first level with min(h_l, w_l) < 2 * margin + 1 (aps_freak_pattern's margin) or at
 * n_levels; level 0 always exists.  heights / widths: host int[n_levels] or NULL; *n_used = levels in the plan. */
int aps_fast_pyramid_plan(int height, int width, int n_levels, int scale_num, int scale_den, int* heights, int* widths, int* n_used);

/* Test hook: the u8 level planes of aps_fast_extract_pyramid, packed one after the other, each row-major, to a host or device
 * pointer `out` of cap_bytes bytes (APS_E_CAP if too small).  *bytes = the sum of h_l * w_l; out = NULL reports it without device
 * work.  It tells a resampling error from a detection error. */
int aps_fast_pyramid_planes(const uint8_t* img, int height, int width, int channels, int img_layout,
                            const aps_fast_pyramid_params* params, uint8_t* out, int64_t cap_bytes, int64_t* bytes);

/* FAST/FREAK strongest-N (DESIGN.md "FAST/FREAK strongest-N"; detectORBFeatures' nfeatures, selectStrongest): of the rows
 * aps_fast_extract_pyramid returns for the same image and parameters (the candidates), keep at most n_strongest - per level a quota
 * q_l = floor(N (h_l + w_l) / sum (h + w)) (+ 1 on the first N - sum q_l levels), a short coarse level handing its unused quota to the
 * finer ones, and within a level the candidates that come first by (Harris response descending, canonical index ascending).  The
 * response is the integer R = 25 (A B - C^2) - (A + B)^2 of the 3 x 3 Sobel gradients summed over the 7 x 7 window of the level's plane. */
typedef struct aps_fast_strongest_params {
    aps_fast_pyramid_params pyramid;   /* n_levels = 1: aps_fast_extract's plan */
    int n_strongest;                   /* N >= 1; anything else is APS_E_ARG before any device work */
} aps_fast_strongest_params;

/* Arguments, capacity, count-only mode, padding, layouts and pointers behave as aps_fast_extract_pyramid's.  *count = rows kept;
 * cap >= min(candidates, n_strongest) always suffices; pyramid.fast.max_features is checked against the rows kept.  With cap below
 * the rows kept nothing is written (APS_E_CAP, *count = rows kept).  The kept rows come in canonical (level, row, col) order; descriptor,
 * location, score, bin and level of a kept row are those of the same row of aps_fast_extract_pyramid, and
 *   aux  : [FAST score, orientation bin, level, f32(R)] (the int64 R rounded to nearest)
 * With at most n_strongest candidates every one is kept.  The count can stay below n_strongest while candidates are dropped: what a
 * short level 0 leaves of its quota goes to no other level.  The call reads back the candidate counts, then the final count. */
int aps_fast_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_fast_strongest_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* The quotas q_l of that call's plan (host only, needs no device).  quota: host int[n_levels] or NULL; *n_used = levels in the plan. */
int aps_fast_strongest_quota(int height, int width, int n_levels, int scale_num, int scale_den, int n_strongest,
                             int* quota, int* n_used);

/* Test hook: R of every candidate, in candidate order, as int64 to a host or device pointer `response` of cap elements (APS_E_CAP if
 * too small).  *count = candidates; response = NULL reports the count alone.  It tells a Harris error from a selection error. */
int aps_fast_harris(const uint8_t* img, int height, int width, int channels, int img_layout,
                    const aps_fast_pyramid_params* params, int64_t* response, int64_t cap, int64_t* count);

/* The integer FREAK tables the extractor uses (tests restate the contract on them; needs no device).  Every pointer may be
 * NULL.  All arrays are host int32, row-major:
 *   fields    [256][43][3]  per orientation bin and receptive field: centre offset dx, dy (pixels) and box half-side r
 *   pairs     [512][2]      the descriptor's field pairs (a, b): bit i = mean(a) > mean(b)
 *   ori_pairs [45][2]       the orientation's field pairs
 *   ori_dir   [45][2]       their unit directions (ux, uy) scaled by 2^10
 *   cos_sin   [256][2]      (c_k, s_k) = round(2^14 * cos / sin(2 pi k / 256))
 *   margin                  largest max(|dx|, |dy|) + r + 1 of `fields`: pixels closer than this to the edge are never corners */
int aps_freak_pattern(int32_t* fields, int32_t* pairs, int32_t* ori_pairs, int32_t* ori_dir, int32_t* cos_sin, int* margin);

/* FAST corners with ORB descriptors (DESIGN.md "FAST/ORB contract"; extractFeatures' Method = 'ORB'): the candidates, their order
 * and the selections are exactly those of the FAST/FREAK entries for the same image and parameters - count, loc, aux[0], aux[2] and
 * aux[3] are bit for bit theirs - and each kept row is described with the intensity-centroid orientation and a steered BRIEF
 * descriptor of 256 bits on its level's plane, integer arithmetic throughout:
 *   desc : u8 count x 32, leading dimension ldd >= 32 (row-major) / >= cap (column-major); bit i = S(a_i) < S(b_i), LSB first in
 *          byte i / 8, S the 5 x 5 box sum on the steered point
 *   aux  : [FAST score, ORB bin 0..255, level, f32(R) with a selection else 0]
 * select = 0 is aps_fast_extract_pyramid's chain, 1 aps_fast_extract_strongest's with N = n_select, 2 aps_fast_extract_uniform's with
 * N = n_select on the grid_rows x grid_cols grid.  Capacity, count-only mode, padding, host and device pointers, both layouts,
 * max_features and APS_E_CAP with nothing written behave as in those entries.  APS_E_ARG before any device work: select outside 0..2,
 * n_select < 1 with a selection, a grid value outside 1..32 with select = 2, NULL params, and whatever those entries refuse. */
typedef struct aps_fast_orb_params {
    aps_fast_pyramid_params pyramid;   /* n_levels = 1: aps_fast_extract's plan */
    int select;                        /* 0 none | 1 strongest-N | 2 uniform-N */
    int n_select;                      /* N >= 1 when select != 0 */
    int grid_rows, grid_cols;          /* 1..32 each when select == 2 */
} aps_fast_orb_params;
int aps_fast_orb_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                         const aps_fast_orb_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                         double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_fast_extract_batch with ORB descriptors: the group's protocol (all-or-nothing capacity, counts, one read-back) is that entry's;
 * the rows of view k are byte for byte those of aps_fast_orb_extract with select = 0 on views[k].img, whatever the other views hold. */
int aps_fast_orb_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels,
                               int img_layout, const aps_fast_pyramid_params* params,
                               int desc_layout, int64_t ldd, int64_t ldl);

/* The integer ORB tables the extractor uses (tests restate the contract on them; host only, needs no device).  Every pointer may be
 * NULL.  All arrays are host int32, row-major:
 *   tests  [256][4]        the generated test pattern (xa, ya, xb, yb), unsteered
 *   table  [256][256][4]   per orientation bin the steered tests (dxa, dya, dxb, dyb)
 *   disc   [709][2]        the offsets (u, v), u^2 + v^2 <= 225, of the orientation's moments, in ascending (v, u) order
 *   reach                  largest |d| of `table` + 2 (the box) + 1 = 16, at most aps_freak_pattern's margin */
int aps_orb_pattern(int32_t* tests, int32_t* table, int32_t* disc, int* reach);

/* Corner detector x descriptor (DESIGN.md "Harris corner contract"): one entry states the whole family of the FAST chains.
 * corner = APS_CORNER_FAST gives, byte for byte, the existing entry for the same descriptor and selection (aps_fast_extract_pyramid,
 * aps_fast_extract_strongest, aps_fast_extract_uniform, aps_fast_orb_extract; the group form aps_fast_extract_batch,
 * aps_fast_orb_extract_batch).  corner = APS_CORNER_HARRIS replaces the detector alone: on every level plane of the same plan the
 * integer Harris response R = 25 (A B - C^2) - (A + B)^2 of aps_fast_harris (Sobel 3 x 3, 7 x 7 window, k = 0.04) at every pixel;
 * a pixel at least aps_freak_pattern's margin from every edge is a candidate iff R > 0 and R exceeds the R of its eight neighbours;
 * a candidate stays iff R * quality_den >= Rmax * quality_num, exactly, Rmax the largest candidate R of the (view, level).
 * chain.pyramid.fast.threshold is checked as ever and not read.  Order, locations, description, selections (strength R), capacity
 * protocol, count-only mode, layouts, padding, host and device pointers, max_features and APS_E_CAP with nothing written are those
 * of the FAST entries.
 *   aux : [f32(R), orientation bin, level, f32(R) with a selection else 0]
 * APS_E_ARG before any device work: corner or descriptor out of range, the group form with chain.select != 0, and whatever the
 * existing entries refuse. */
enum { APS_CORNER_FAST = 0, APS_CORNER_HARRIS = 1 };
enum { APS_DESC_FREAK = 0, APS_DESC_ORB = 1 };
typedef struct aps_corner_params {
    aps_fast_orb_params chain;   /* pyramid, select, n_select, grid */
    int corner;                  /* APS_CORNER_* */
    int descriptor;              /* APS_DESC_* */
} aps_corner_params;
int aps_corner_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                       const aps_corner_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                       double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);
int aps_corner_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels,
                             int img_layout, const aps_corner_params* params,
                             int desc_layout, int64_t ldd, int64_t ldl);

/* Test hook: the dense response R of every level plane of aps_fast_extract_pyramid's plan, before suppression and gate, packed like
 * aps_fast_pyramid_planes (one int64 per pixel, host or device); 0 at pixels closer than 4 to an edge, where the 9 x 9 patch leaves
 * the plane.  out = NULL: *count = the pixels of all levels, no device work; cap < *count is APS_E_CAP. */
int aps_harris_planes(const uint8_t* img, int height, int width, int channels, int img_layout,
                      const aps_fast_pyramid_params* params, int64_t* out, int64_t cap, int64_t* count);

/* ============================================================================================
 * (4d) Uniform-N selection for SIFT, SURF and FAST — selectUniform next to selectStrongest
 * ============================================================================================ */
/* DESIGN.md "Uniform-N selection".  Candidates, strength, groups (one; for FAST one per level) and canonical order are those of the
 * detector's _strongest entry, and so is the budget of a group: min(N, candidates), for FAST the rows the _strongest call keeps on
 * the level.  The budget is spread over the cells of a grid_rows x grid_cols grid on the group's plane (the image; for FAST the
 * level's plane) by water-filling: with counts c_k and budget Q, t is the largest integer with sum_k min(c_k, t) <= Q, cell k keeps
 * min(c_k, t) rows, and the first Q - sum_k min(c_k, t) cells in ascending k with c_k > t keep one more.  Within a cell the rows that
 * come first by (strength descending, canonical index ascending) stay.  The cell of a candidate is that of a 0-based pixel (py, px):
 *   SIFT  px = clamp((int)floor(x) - 1, 0, width - 1) of the row's 1-based f64 location, py alike
 *   SURF  the candidate's detection sample (i * step, j * step), before refinement
 *   FAST  the candidate's pixel on its level
 * A 1 x 1 grid gives the _strongest result. */
typedef struct aps_sift_uniform_params {
    aps_sift_strongest_params strongest;   /* strongest.n_strongest is N >= 1 */
    int grid_rows, grid_cols;              /* each in 1..32; anything else is APS_E_ARG before any device work */
} aps_sift_uniform_params;
typedef struct aps_surf_uniform_params {
    aps_surf_strongest_params strongest;   /* strongest.n_strongest is N >= 1 */
    int grid_rows, grid_cols;              /* each in 1..32; anything else is APS_E_ARG before any device work */
} aps_surf_uniform_params;
typedef struct aps_fast_uniform_params {
    aps_fast_strongest_params strongest;   /* strongest.n_strongest is N >= 1 */
    int grid_rows, grid_cols;              /* each in 1..32; anything else is APS_E_ARG before any device work */
} aps_fast_uniform_params;

/* Arguments, capacity, count-only mode, APS_E_CAP with nothing written, padding, layouts, host and device pointers, the meaning of
 * max_features and the read-backs are those of the matching _strongest entry, and so is *count.  The kept rows come in canonical order;
 * every byte of descriptor, location and aux of a kept row is that of the same row of the call without selection (FAST: aux[3] = f32(R)
 * as in aps_fast_extract_strongest); only kept rows are described. */
int aps_sift_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_sift_uniform_params* params, float* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);
int aps_surf_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_surf_uniform_params* params, float* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);
int aps_fast_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_fast_uniform_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* aps_sift_extract_uniform for a group of views of one shape, as aps_sift_extract_batch_strongest is for aps_sift_extract_strongest:
 * the rows of view k (descriptor, location, aux, order and count) are bit for bit those of aps_sift_extract_uniform on views[k].img
 * with the same params, whatever the other views contain; the budget of view k is min(candidates_k, N), spread over the cells of its
 * own grid.  Arguments, capacities, APS_E_CAP and the checks are aps_sift_extract_batch_strongest's, with a grid value outside 1..32
 * refused (APS_E_ARG) before any device work.  The selection of the whole group is one sort and one pass of each of its kernels, with
 * no read-back beyond aps_sift_extract_batch's. */
int aps_sift_extract_batch_uniform(aps_sift_view* views, int n_views, int height, int width, int channels,
                                   int img_layout, const aps_sift_uniform_params* params,
                                   int desc_layout, int64_t ldd, int64_t ldl);

/* aps_surf_extract_uniform for a group of views of one shape, as aps_surf_extract_batch_strongest is for aps_surf_extract_strongest:
 * the rows of view k are bit for bit those of aps_surf_extract_uniform on views[k].img with the same params, whatever the other
 * views hold; the budget of view k is min(candidates_k, N), spread over the cells of its own grid.  Arguments, capacities,
 * APS_E_CAP, the checks and the two read-backs are aps_surf_extract_batch_strongest's, with a grid value outside 1..32 refused
 * (APS_E_ARG) before any device work.  The selection of the whole group is one sort and one pass of each of its kernels. */
int aps_surf_extract_batch_uniform(aps_surf_view* views, int n_views, int height, int width, int channels,
                                   int img_layout, const aps_surf_uniform_params* params,
                                   int desc_layout, int64_t ldd, int64_t ldl);

/* The water-filling of that rule (host only, needs no device; the function the device kernel calls): keep[k] of n_cells cells (1..1024)
 * with counts[k] in 0..2^32-1 under min(budget, sum counts).  counts and keep: host int64[n_cells]. */
int aps_uniform_quota(const int64_t* counts, int n_cells, int64_t budget, int64_t* keep);

/* The cell of the 0-based pixel (py, px) of a plane_h x plane_w plane (host only, needs no device; the function the device kernels call):
 * *cell = (py * grid_rows / plane_h) * grid_cols + px * grid_cols / plane_w, integer divisions.  A pixel outside the plane or a grid
 * value outside 1..32 is APS_E_ARG. */
int aps_uniform_cell(int py, int px, int plane_h, int plane_w, int grid_rows, int grid_cols, int* cell);

/* ============================================================================================
 * (4e) KAZE — PP/featureMatching/getFeaturePoints.m:63-64,71-74
 * ============================================================================================ */

#define APS_KAZE_DIFFUSION_REGION 0      /* Perona-Malik g2, 1 / (1 + |grad|^2 / k^2): detectKAZEFeatures' default, the one built */
#define APS_KAZE_DIFFUSION_SHARPEDGE 1   /* g1 = exp(-|grad|^2 / k^2): not built (APS_E_ARG) */
#define APS_KAZE_DIFFUSION_EDGE 2        /* Weickert's: not built (APS_E_ARG) */

typedef struct aps_kaze_params {
    double threshold;          /* detectKAZEFeatures Threshold (0.0001), >= 0 */
    int num_octaves;           /* NumOctaves (3), 1..4 */
    int num_scale_levels;      /* NumScaleLevels (4), 3..10 */
    int diffusion;             /* APS_KAZE_DIFFUSION_*: only _REGION is built */
    int max_features;          /* capacity guard; 0 = library default (none beyond cap) */
} aps_kaze_params;

/* [features, validPts] for detector 'KAZE' (getFeaturePoints.m:63-64,71-74): rgb2gray, detectKAZEFeatures(gray), extractFeatures.
 * Both toolbox calls are closed code; the algorithm restated is KAZE of Alcantarilla, Bartoli and Davison (ECCV 2012) with the
 * parameters that call implies — see DESIGN.md "KAZE contract", which fixes every operation and its order (parity with MATLAB is
 * unpinned); tests/kaze_mirror.py restates it in NumPy, bit for bit.  num_octaves * num_scale_levels evolution levels, all at full
 * resolution; keypoints are strict 3x3x3 maxima of the scale-normalised Hessian determinant above `threshold` on the levels between
 * the first and the last, refined as SURF's are.
 *   desc : f32 count x 64 oriented M-SURF rows, `desc_layout` with leading dimension ldd >= 64 (row-major) / >= cap (column-major),
 *          unit L2 norm; row-major with ldd >= 128: columns 64..127 are zeroed as well, so resident rows feed the 128-wide matchers
 *   loc  : f64 count x 2 [x y], 1-based sub-pixel, column-major with leading dimension ldl >= cap
 *   aux  : f32 count x 4 row-major [scale (sigma, pixels), angle_deg, metric (the response), level] or NULL
 * cap = rows available in desc/loc/aux; *count = features found (APS_E_CAP if cap is too small, with the true count and nothing
 * written; desc = NULL or cap = 0 counts).  Rows beyond the count are never written.  Every argument is checked before any device
 * work: NULL img / params / count, num_octaves outside 1..4, num_scale_levels outside 3..10, threshold < 0, a diffusion other than
 * APS_KAZE_DIFFUSION_REGION and height * width >= 2^31 are APS_E_ARG.  An image too small for level 1's margin gives
 * count 0, not an error.  Host and device pointers are accepted; the call runs on the calling thread's library stream with that
 * thread's workspace (4 bytes x (5 + 3 levels) planes: 1.36 GB for a 3840 x 2160 view at the defaults) and reads back once, the count.
 * Feature order is canonical: ascending (level, row, col).
 * Not built: the 'sharpedge' and 'edge' diffusivities, 128-D rows, group (batch) entries and a MATLAB gateway command.  Upright and
 * the NumStrongest / NumUniform selections are aps_kaze_extract_select's, below. */
int aps_kaze_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_kaze_params* params, float* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

typedef struct aps_kaze_select_params {
    aps_kaze_params kaze;      /* what aps_kaze_extract takes: the candidates are its rows */
    int select;                /* 0 none, 1 strongest-N, 2 uniform-N (aps_fast_orb_params' convention) */
    int n_select;              /* N (NumStrongest / NumUniform), >= 1 with a selection; not read with select == 0 */
    int grid_rows;             /* UniformGrid rows, 1..32; read with select == 2 */
    int grid_cols;             /* UniformGrid columns, 1..32; read with select == 2 */
    int upright;               /* 0 | 1: extractFeatures' Upright */
} aps_kaze_select_params;

/* aps_kaze_extract with a selection of its rows and / or upright descriptors (DESIGN.md "KAZE selection and Upright").  The
 * candidates are the rows aps_kaze_extract returns for the same image and `kaze`, in canonical order; their strength is `metric`
 * (aux[:, 2]), in one group with no quota per level.
 *   select == 1  keeps the first min(n_select, candidates) by (metric descending, canonical index ascending): the rule of
 *                aps_surf_extract_strongest
 *   select == 2  keeps Q = min(n_select, candidates) rows spread over the grid_rows x grid_cols cells of the image by water-filling
 *                (aps_uniform_quota), the largest metric first within a cell; a row's cell is aps_uniform_cell of its detection
 *                pixel, before refinement: the rule of aps_surf_extract_uniform.  A 1 x 1 grid is select == 1's result
 *   upright == 1 skips the orientation: the descriptor is the oriented one's arithmetic at (cos, sin) = (1.0f, 0.0f) and angle_deg
 *                is +0.0; count, loc, scale, metric and level are the oriented call's bits
 * Kept rows come out in canonical order, and every byte of a kept row (with upright == 0) is that row's of the unselected call;
 * n_select at or above the candidates gives the unselected result.  With select == 0 and upright == 0 the call is aps_kaze_extract.
 * Outputs, layouts, host / device pointers and the capacity protocol are aps_kaze_extract's, with *count = rows kept: cap >=
 * min(candidates, n_select) suffices.  kaze.max_features > 0 limits the candidates found, before the selection (APS_E_CAP with the
 * candidate count), as in aps_surf_extract_strongest.  With a selection the call reads back twice: the candidates, then the rows
 * the device kept.  No atomics in the selection; the result is the same from run to run.
 * Errors, all before any device work: every refusal of aps_kaze_extract, and APS_E_ARG for NULL params, select outside 0..2,
 * n_select < 1 with a selection, a grid value outside 1..32 with select == 2, upright outside 0..1. */
int aps_kaze_extract_select(const uint8_t* img, int height, int width, int channels, int img_layout,
                            const aps_kaze_select_params* params, float* desc, int desc_layout, int64_t ldd,
                            double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count);

/* ============================================================================================
 * Lens distortion: undistortImage / undistortPoints of the Computer Vision Toolbox ("Lens distortion contract")
 * ============================================================================================ */
/* A lens without skew.  Coordinates are the library's 1-based pixel coordinates (the frame of keypoints, of K and of
 * aps_image_warp_u8): the 0-based pixel (row i, column j) sits at (u, v) = (j + 1, i + 1).  A two-term radial model has k3 = 0.
 * The forward (distorting) map of a point (u, v) of the ideal image, in f64, evaluated exactly as parenthesised, no contraction:
 *     x = (u - cx) / fx;  y = (v - cy) / fy;  r2 = x*x + y*y
 *     rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *     dx = ((2*p1)*x)*y + p2*(r2 + (2*x)*x)
 *     dy = p1*(r2 + (2*y)*y) + ((2*p2)*x)*y
 *     ud = fx*(x*rad + dx) + cx;  vd = fy*(y*rad + dy) + cy
 * tests/undistort_mirror.py restates the three entries below in NumPy, bit for bit.  Domain: moderate lenses, normalised
 * radius below about 1; no fisheye. */
typedef struct aps_lens {
    double fx, fy, cx, cy, k1, k2, k3, p1, p2;
} aps_lens;

/* undistortImage: output pixel (i, j), 0-based, of the out_h x out_w view has the ideal coordinates (u, v) = (x0 + j, y0 + i)
 * and samples the distorted image img (h x w x c uint8, c = 1 or 3, img_layout APS_IMG_U8_HWC or APS_IMG_U8_MATLAB; out has
 * the same layout) at (ud, vd).  The sample is valid iff 1 <= ud <= w and 1 <= vd <= h (a NaN fails); then x1 = floor(ud),
 * x2 = min(x1 + 1, w), wx = ud - x1, likewise in y, and the value is that of aps_image_warp_u8's bilinear branch:
 * ((w11*p11 + w12*p12) + w21*p21) + w22*p22 with w11 = (1-wx)*(1-wy), w12 = (1-wx)*wy, w21 = wx*(1-wy), w22 = wx*wy and
 * p11 = (y1, x1), p12 = (y2, x1), p21 = (y1, x2), p22 = (y2, x2), rounded half away from zero and clamped to 0..255.  An
 * invalid sample gives `fill`.  A lens whose five coefficients are all zero copies the input into the view (ud = u, vd = v,
 * decided on the host).  img and out: host or device memory each, not overlapping.  One launch on the calling thread's stream, one lane per output
 * pixel; complete on return.
 * Errors, all before any device work: APS_E_ARG for a NULL pointer, fx or fy not finite or not above 0, any other field not
 * finite, fill outside 0..255, an origin of 2^24 or more in magnitude; APS_E_DIM for a non-positive size, c other than 1 or 3,
 * an image of 2^31 / 3 pixels or more; APS_E_TYPE for an unknown layout. */
int aps_undistort_image_u8(const uint8_t* img, int h, int w, int c, int img_layout, const aps_lens* lens, int out_h, int out_w,
                           int x0, int y0, int fill, uint8_t* out);

/* undistortPoints: the inverse map of n distorted points by exactly 20 fixed-point steps from x = xd = (ud - cx) / fx,
 * y = yd = (vd - cy) / fy: each step is x <- (xd - dx(x, y)) / rad(x, y), y <- (yd - dy(x, y)) / rad(x, y), both from the
 * previous (x, y); then u = fx*x + cx, v = fy*y + cy.  There is no convergence test.  pts and out: f64, x at [k] and y at
 * [ld + k] (the layout of the extractors' loc), host or device memory each; the entries n..ld-1 of out are not written.
 * n = 0 is a no-op.  Errors, before any device work: the lens errors above, APS_E_DIM for n < 0 or ld < n, APS_E_ARG for a
 * NULL pointer when n > 0. */
int aps_undistort_points(const double* pts, int64_t n, int64_t ld, const aps_lens* lens, double* out);

/* The 'valid' output view of an h x w image: with (ux, uy) the aps_undistort_points images (the same kernel, on the device) of
 * the pixel centres of the four border rows and columns, *x0 = ceil(max ux over the left column), x1 = floor(min ux over the
 * right column), *y0 = ceil(max uy over the top row), y1 = floor(min uy over the bottom row), *out_h = y1 - *y0 + 1,
 * *out_w = x1 - *x0 + 1 (host memory; the host takes the extrema).  Errors: the lens errors above, APS_E_DIM for a
 * non-positive size, APS_E_ARG for a NULL pointer, a border that does not map to finite points, or an empty rectangle. */
int aps_undistort_valid_view(int h, int w, const aps_lens* lens, int* x0, int* y0, int* out_h, int* out_w);

/* ============================================================================================
 * Bench / test support — NOT part of the reference boundary
 * ============================================================================================ */
/* One uint8 H x W x 3 (row-major interleaved) view of the seeded procedural world used by bench.py and the
 * pipeline tests, through the pinhole camera (K, R), both 3x3 ROW-major here.  See synth.py. */
int aps_synth_view(const double* K_rowmajor, const double* R_rowmajor, int height, int width,
                   unsigned seed, float finest_px, float gain, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* APS_H_ */

/*
 * xhist_amd.h — C ABI of the MI355X-native xhistogram hot path (libxhist_amd.so).
 *
 * The reference (xgcm/xhistogram) is pure Python and has NO FFI; its hot path sits behind plain
 * Python calls.  This header is the boundary a maintainer would bind (ctypes) in place of the body
 * of `_bincount_2d_vectorized` — see INTEGRATION.md for the stub.  Every entry point cites the
 * reference lines whose work it replaces (paths relative to /root/reference).
 *
 * Contract of the path (xhistogram/core.py:137-194):
 *   D sample arrays of identical logical shape [M rows, C cols], D edge arrays (sorted, length
 *   E_d >= 1), optional weights [M, C]  ->  out[M, nb_0, ..., nb_{D-1}],  nb_d = E_d - 1.
 *   bin k of a dimension holds  edges[k] <= x < edges[k+1];  the last bin also holds
 *   x == edges[E-1];  NaN, x < edges[0], x > edges[E-1] drop the sample (in ANY dimension).
 *   Unweighted -> exact int64 counts.  Weighted -> float64 sums of weights (cast to f64 first).
 *   The first input is the slowest-varying bin axis (C order), as `ravel_multi_index` at
 *   core.py:178-181.  Comparisons are made in float64 (XHIST_CMP_F64: every sample is converted
 *   to double first, which is what numpy's searchsorted does for f32/int data against f64 edges)
 *   or exactly in int64 (XHIST_CMP_I64: integer / datetime64 data against integer edges).
 *
 * Ownership: the caller owns every input and output buffer; the library owns plans and scratch.
 * Threading: all entry points are thread-safe; one plan may be executed from many threads.
 * Errors: functions return XHIST_OK (0) or a negative xhist_status; xhist_last_error() returns a
 * thread-local description.  The library never aborts and never falls back to a CPU path: without
 * a usable HIP device every compute call fails with XHIST_ERR_NO_DEVICE.
 */
#ifndef XHIST_AMD_H
#define XHIST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XHIST_ABI_VERSION 11
#define XHIST_MAX_DIMS 8 /* max number of sample arrays (histogram dimensionality) */

typedef enum {
  XHIST_OK = 0,
  XHIST_ERR_INVALID = -1,     /* bad argument: null pointer, bad dtype tag, sizes < 0, D out of range */
  XHIST_ERR_UNSUPPORTED = -2, /* legal for the reference but not for this build (documented)        */
  XHIST_ERR_NO_DEVICE = -3,   /* no HIP device visible / device index out of range                   */
  XHIST_ERR_HIP = -4,         /* HIP runtime error (message in xhist_last_error)                      */
  XHIST_ERR_NOMEM = -5,       /* host or device allocation failed                                     */
  XHIST_ERR_EDGES = -6,       /* edges decrease somewhere or contain NaN (numpy: ValueError)          */
  XHIST_ERR_COMM = -7         /* RCCL not loadable / a collective failed (message in xhist_last_error) */
} xhist_status;

/* element type tags (numpy dtypes the reference accepts for samples / weights) */
typedef enum {
  XHIST_F64 = 0, XHIST_F32 = 1, XHIST_F16 = 2,
  XHIST_I64 = 3, XHIST_I32 = 4, XHIST_I16 = 5, XHIST_I8 = 6,
  XHIST_U64 = 7, XHIST_U32 = 8, XHIST_U16 = 9, XHIST_U8 = 10,
  XHIST_BOOL = 11
} xhist_dtype;

typedef enum { XHIST_CMP_F64 = 0, XHIST_CMP_I64 = 1 } xhist_cmp_domain;
/* Per-input domains (a datetime64 axis next to a float axis): cmp_domain = XHIST_CMP_PER_DIM | mask,
 * bit d of mask set <=> input d compares in int64 (its edge array is int64), else in float64.
 * numpy digitizes every argument on its own (core.py:163-174), so such mixtures are legal there. */
#define XHIST_CMP_PER_DIM 0x100
/* OR-ed onto XHIST_CMP_I64 / XHIST_CMP_PER_DIM: the int64-domain inputs are UNSIGNED 64-bit — their
 * edge arrays hold uint64 values and their samples (uint8..uint64, bool) compare as unsigned
 * (numpy: uint64 data against uint64 edges). */
#define XHIST_CMP_UNSIGNED 0x200
/* XHIST_MEM_HOST_TO_DEVICE: samples / weights are HOST pointers (staged by the library), `out` is a DEVICE buffer on the plan's GPU:
 * the partial histogram of a host-resident block stays on the GPU that computed it, for the sum over blocks and GPUs
 * (xhist_buffer_add, xhist_comm_allreduce) that replaces dask's `.sum(drop_axes)` (core.py:439) */
typedef enum { XHIST_MEM_HOST = 0, XHIST_MEM_DEVICE = 1, XHIST_MEM_HOST_TO_DEVICE = 2 } xhist_mem_kind;

/* A logical [M, C] array addressed as data[row_offset(r) + c * col_stride] (strides in ELEMENTS):
 *   row_offset(r) = r * row_stride                                                  if inner_rows == 0
 *                 = (r / inner_rows) * outer_stride + (r % inner_rows) * row_stride  otherwise.
 * row_stride == 0 or col_stride == 0 express numpy broadcasting without materialising it
 * (core.py:366 broadcast_arrays).  The grouped form expresses an N-D array whose reduced axes
 * sit BETWEEN kept axes — (time, LAT, lon) histogrammed over lat: rows = (time, lon) pairs,
 * inner_rows = n_lon, outer_stride = n_lat * n_lon — so that the reference's moveaxis + reshape
 * copy (core.py:211-229) is never made. */
typedef struct {
  const void* data;
  int32_t dtype; /* xhist_dtype */
  int32_t reserved;
  int64_t row_stride;
  int64_t col_stride;
  int64_t inner_rows;   /* rows per group; 0 = ungrouped */
  int64_t outer_stride; /* stride between groups of rows */
} xhist_array;

typedef struct xhist_plan xhist_plan; /* opaque: device-resident edge tables + launch geometry */

/* ---- library / device queries ------------------------------------------------------------ */
int xhist_abi_version(void);
const char* xhist_last_error(void);
int xhist_device_count(int* count);
/* name (may be NULL) receives the gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
int xhist_device_info(int device, char* name, size_t name_cap, int* compute_units, size_t* total_mem_bytes);

/* ---- plans ------------------------------------------------------------------------------- */
/* Upload D edge arrays (HOST pointers; float64 for XHIST_CMP_F64, int64 for XHIST_CMP_I64, per input
 * for XHIST_CMP_PER_DIM) and
 * build the per-dimension bucket->edge-range tables used by the branch-free digitize.
 * Replaces the per-call edge handling of core.py:154-155, 163-174. */
int xhist_plan_create(int device, int n_inputs, const void* const* edges, const int64_t* n_edges,
                      int cmp_domain, xhist_plan** plan);
int xhist_plan_destroy(xhist_plan* plan);

/* The fused hot path — replaces core.py:137-194 (_bincount_2d_vectorized: searchsorted 170-173,
 * ravel_multi_index 178-181, _dispatch_bincount/_bincount_2d 73-134, trim 189-192) in ONE kernel.
 *   samples[n_inputs], weights (NULL = unweighted): xhist_array views, all HOST or all DEVICE (mem_kind).
 *   out: contiguous [n_rows, prod(nb_d)];  out_dtype XHIST_I64 (unweighted) or XHIST_F64 (weighted).
 *   accumulate != 0: add into `out` instead of overwriting it — this is the reference's
 *     "sum over blocks" (dask `.sum(drop_axes)`, core.py:439) fused into the kernel's flush.
 *   stream: hipStream_t (NULL = default stream).  XHIST_MEM_DEVICE calls are asynchronous on
 *     `stream`; XHIST_MEM_HOST calls stage through device memory and return when `out` is final
 *     (with stream NULL they run on the calling thread's own stream, so concurrent host callers —
 *     dask's threaded scheduler — overlap one block's staging copy with another block's kernel).
 * Named roctx ranges wrap plan creation, execute and the exchange calls when a roctx library is
 * mapped in the process (rocprofv3 --marker-trace) or XHIST_AMD_ROCTX=1.
 */
int xhist_plan_execute(xhist_plan* plan, const xhist_array* samples, const xhist_array* weights,
                       int64_t n_rows, int64_t n_cols, void* out, int out_dtype, int mem_kind,
                       int accumulate, void* stream);

/* Two weight arrays binned in ONE pass over the samples: out_a = histogram weighted by weights_a,
 * out_b by weights_b (both float64 [n_rows, prod(nb_d)]).  The idiom behind it is the ratio of two
 * histograms, "mean of A in the bins of x" = hist(x, weights=A*w) / hist(x, weights=w): the
 * reference runs the whole path twice (its own TODO, xarray.py:106); here the samples are read and
 * digitized once when the arrays are device-resident and the vector kernels apply, and the call
 * degrades to two xhist_plan_execute passes otherwise — same results either way. */
int xhist_plan_execute_two_weights(xhist_plan* plan, const xhist_array* samples, const xhist_array* weights_a,
                                   const xhist_array* weights_b, int64_t n_rows, int64_t n_cols, void* out_a,
                                   void* out_b, int mem_kind, int accumulate, void* stream);

/* Per-bin minimum and maximum of `values` (ABI v10): which samples count is exactly what xhist_plan_execute counts (same
 * digitize, last bin closed, NaN / out-of-range samples dropped); each counted sample contributes its value converted to
 * float64.  NaN values are ignored (np.fmin / np.fmax), values are ordered totally with -0.0 < +0.0, and a bin that received
 * no value is NaN in both outputs.  Results are exact.
 *   values: an xhist_array of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_min, out_max: contiguous float64 [n_rows, prod(nb_d)], DEVICE buffers; they double as the kernels' working space.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   accumulate != 0: combine into the existing outputs (NaN there = empty) instead of overwriting them — chunked inputs.
 *   Asynchronous on `stream`. */
int xhist_plan_execute_extrema(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                               int64_t n_rows, int64_t n_cols, double* out_min, double* out_max,
                               int mem_kind, int accumulate, void* stream);

/* Where each bin's minimum and maximum of `values` lie (added within ABI v11): the samples that count, the conversion of the
 * values, the NaN rule and the total order (-0.0 < +0.0) are xhist_plan_execute_extrema's, and out_values equals its two
 * outputs bit for bit.  out_index holds, per bin, the column index (0 .. n_cols - 1 inside the bin's row) of the FIRST counted
 * sample whose value is the bin's minimum (plane 0) or maximum (plane 1), and -1 where the bin received no value.  Exact and
 * deterministic: pass 1 finds the extreme keys, pass 2 takes the smallest index among the samples whose key equals them.
 *   out_values: contiguous float64 [2, n_rows, prod(nb_d)] (minimum, maximum), a DEVICE buffer; it doubles as working space.
 *   out_index: contiguous int64 [2, n_rows, prod(nb_d)], a DEVICE buffer.  Both are overwritten (no accumulate mode).
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live. */
int xhist_plan_execute_argextrema(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                  int64_t n_rows, int64_t n_cols, double* out_values, int64_t* out_index,
                                  int mem_kind, void* stream);

/* Per-bin count and sum of `values` that do not depend on the order of arrival (added within ABI v11): which samples count is
 * exactly what xhist_plan_execute_mean_var counts (a counted sample whose value is not NaN contributes that value converted to
 * float64), and out_count is its count.  out_total is defined on integers, per (row, bin):
 *   A = the largest |v| of the bin (pass 1 is xhist_plan_execute_extrema's); E = frexp(A)'s exponent, U = max(E - 96, -1074);
 *   a value v = s * m * 2^e (m the 53-bit integer significand, e = -1074 for subnormals) becomes q = m << (e - U), or m >> (U - e)
 *   truncated towards zero (0 once the shift reaches 64); q < 2^96 is split into three unsigned 32-bit limbs, and s * limb_j is
 *   added into three int64 accumulators; out_total = RN_even((L0 + L1 * 2^32 + L2 * 2^64) * 2^U), one rounding in integer
 *   arithmetic, overflowing to +-inf as IEEE does, a zero result +0.0.  An empty bin gives +0.0.  A bin that holds an infinity
 *   gives that infinity, or NaN where it holds both.
 * The result is the same bits for any order of the samples, launch geometry and run.  Every value within a factor 2^43 of its
 * bin's largest magnitude is converted exactly, and a bin of such values gets the correctly rounded exact sum; in general
 * |out_total - exact| <= ulp(out_total) / 2 + n * 2^(E - 96).  No intermediate overflows.
 *   values: an xhist_array of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   n_cols must be below 2^31 (the accumulators hold that many limbs): XHIST_ERR_UNSUPPORTED otherwise, before any device work.
 *   out_count (int64), out_total (float64): contiguous [n_rows, prod(nb_d)] DEVICE buffers, overwritten (no accumulate mode);
 *   five 8-byte scratch blocks of that size are taken for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live
 *   ("sum pass1=extrema_... pass2=sum_..."). */
int xhist_plan_execute_sum(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                           int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_total,
                           int mem_kind, void* stream);

/* Per-bin count, mean and sum of squared deviations of `values` (ABI v11): which samples count is exactly what
 * xhist_plan_execute counts (same digitize, last bin closed, NaN / out-of-range samples dropped); each counted sample whose
 * value is not NaN contributes that value converted to float64.  Two passes (Chan, Golub & LeVeque): n and S = sum(v), then
 * d = v - S/n in float64 and M2 = max(0, sum(d*d) - sum(d)^2 / n).  mean = S/n and M2 are NaN where n == 0; the variance is
 * M2 / (n - ddof), left to the caller.  Float64 atomics add in arbitrary order: the last bits can differ between runs, except
 * for data whose sums are exact in every order.
 *   values: an xhist_array of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_count (int64), out_mean, out_m2 (float64): contiguous [n_rows, prod(nb_d)] DEVICE buffers, overwritten (no
 *   accumulate mode); one float64 scratch block of that size is taken for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live. */
int xhist_plan_execute_mean_var(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_m2,
                                int mem_kind, void* stream);

/* Per-bin sum of weights, weighted mean and weighted sum of squared deviations of `values` (added within ABI v11): which
 * samples count is exactly what xhist_plan_execute_mean_var counts; each counted sample whose value is not NaN contributes the
 * pair (w, v), both converted to float64 (frequency weights).  Two passes: W = sum(w) and S = sum(w*v), then d = v - S/W in
 * float64 and M2 = max(0, sum(w*d*d) - sum(w*d)^2 / W).  mean = S/W and M2 are NaN where W == 0 (empty bins, and bins whose
 * weights sum to 0); a NaN weight makes its bin's W, mean and M2 NaN.  Negative weights are not checked: the formulas apply,
 * the clamp of M2 at 0 included.  The variance is M2 / (W - ddof), left to the caller.  Float64 atomics add in arbitrary
 * order: the last bits can differ between runs, except for data whose sums are exact in every order.
 *   values, weights: xhist_arrays of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_wsum, out_mean, out_m2 (float64): contiguous [n_rows, prod(nb_d)] DEVICE buffers, overwritten (no accumulate mode);
 *   one float64 scratch block of that size is taken for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live
 *   ("mean_var_w pass1=mvw_sum_..."). */
int xhist_plan_execute_mean_var_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                         const xhist_array* weights, int64_t n_rows, int64_t n_cols, double* out_wsum,
                                         double* out_mean, double* out_m2, int mem_kind, void* stream);

/* Per-bin count, mean and second, third and fourth central moments of `values` (added within ABI v11): the samples that count,
 * pass 1 (n, S = sum(v)) and mean = S/n are exactly those of xhist_plan_execute_mean_var.  Pass 2 forms d = v - mean in float64,
 * the terms t1 = d, t2 = t1*d, t3 = t2*d, t4 = t3*d in this order of products, and D = sum(t1), Q2 = sum(t2), Q3 = sum(t3),
 * Q4 = sum(t4).  With delta = D/n, every product and sum rounded on its own:
 *   M2 = max(0, Q2 - (D*D)/n)            (xhist_plan_execute_mean_var's expression: on equal sums, its bits)
 *   d2 = delta*delta, d3 = d2*delta, d4 = d2*d2
 *   M3 = (Q3 - (3*delta)*Q2) + (2*n)*d3  (not clamped)
 *   M4 = max(0, ((Q4 - (4*delta)*Q3) + (6*d2)*Q2) - (3*n)*d4)
 * The mean and the three moments are NaN where n == 0, and a NaN stays NaN.  Variance, skewness and kurtosis (M3/n / (M2/n)^1.5,
 * M4/n / (M2/n)^2) are left to the caller.  Float64 atomics add in arbitrary order: the last bits can differ between runs,
 * except for data whose sums are exact in every order.
 *   values: an xhist_array of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_count (int64), out_mean (float64): contiguous [n_rows, prod(nb_d)]; out_moments (float64): contiguous [3, n_rows,
 *   prod(nb_d)], M2, M3, M4.  DEVICE buffers, overwritten (no accumulate mode); one float64 scratch block of [n_rows, prod(nb_d)]
 *   is taken for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live
 *   ("skew_kurt pass1=mv_sum_... pass2=sk_dev_..."). */
int xhist_plan_execute_skew_kurt(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                 int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_moments,
                                 int mem_kind, void* stream);

/* The same with frequency weights (added within ABI v11): the samples that count, pass 1 (W = sum(w), S = sum(w*v)) and mean =
 * S/W are exactly those of xhist_plan_execute_mean_var_weighted.  Pass 2 forms t1 = w*d and then t2, t3, t4 as above; the
 * formulas above hold with W in the place of n.  The mean and the moments are NaN where W == 0; a NaN weight makes its bin NaN.
 * Negative weights are not checked.
 *   values, weights: xhist_arrays of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_wsum, out_mean (float64): contiguous [n_rows, prod(nb_d)]; out_moments (float64): contiguous [3, n_rows, prod(nb_d)].
 *   Otherwise as above ("skew_kurt_w pass1=mvw_sum_... pass2=skw_dev_..."). */
int xhist_plan_execute_skew_kurt_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                          const xhist_array* weights, int64_t n_rows, int64_t n_cols, double* out_wsum,
                                          double* out_mean, double* out_moments, int mem_kind, void* stream);

/* Per-bin covariance of two value arrays (added within ABI v11): which samples count is exactly what
 * xhist_plan_execute_mean_var counts, and a counted sample contributes its pair (a, b), both converted to float64, only if
 * neither is NaN (pairwise-complete).  Two passes over the three streams, the corrected two-pass form of
 * xhist_plan_execute_mean_var: n, Sa = sum(a), Sb = sum(b); then da = a - Sa/n, db = b - Sb/n in float64 and
 *   M2_a = max(0, sum(da*da) - sum(da)^2 / n),  C_ab = sum(da*db) - sum(da) sum(db) / n,  M2_b = max(0, sum(db*db) - sum(db)^2 / n).
 * C_ab is not clamped: a covariance may be negative.  The means and the three moments are NaN where n == 0; variances and
 * covariance are M2 / (n - ddof) and C_ab / (n - ddof), left to the caller.  Float64 atomics add in arbitrary order: the last
 * bits can differ between runs, except for data whose sums are exact in every order.
 *   values_a, values_b: xhist_arrays of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   out_count (int64): contiguous [n_rows, prod(nb_d)]; out_mean (float64): contiguous [2, n_rows, prod(nb_d)], mean_a then
 *   mean_b; out_comoment (float64): contiguous [3, n_rows, prod(nb_d)], M2_a, C_ab, M2_b.  DEVICE buffers, overwritten (no
 *   accumulate mode); two float64 scratch blocks of [n_rows, prod(nb_d)] are taken from the library's allocator for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live
 *   ("cov pass1=cov_sum_..."). */
int xhist_plan_execute_cov(xhist_plan* plan, const xhist_array* samples, const xhist_array* values_a,
                           const xhist_array* values_b, int64_t n_rows, int64_t n_cols, int64_t* out_count,
                           double* out_mean, double* out_comoment, int mem_kind, void* stream);

/* Weighted per-bin covariance of two value arrays (added within ABI v11): which samples count is exactly what
 * xhist_plan_execute_cov counts, and a counted sample contributes its triple (w, a, b), all converted to float64, only if
 * neither a nor b is NaN, whatever its weight (pairwise-complete; frequency weights, as xhist_plan_execute_mean_var_weighted's).
 * Two passes over the four streams: W = sum(w), Swa = sum(w*a), Swb = sum(w*b); then da = a - Swa/W, db = b - Swb/W in
 * float64, wda = w*da, wdb = w*db and
 *   M2_a = max(0, sum(wda*da) - sum(wda)^2 / W),  C_ab = sum(wda*db) - sum(wda) sum(wdb) / W,  M2_b = max(0, sum(wdb*db) - sum(wdb)^2 / W).
 * C_ab is not clamped.  The means and the three moments are NaN where W == 0 (empty bins, and bins whose weights sum to 0); a
 * NaN weight on a complete pair makes its bin NaN.  Negative weights are not checked.  Variances and covariance are
 * M2 / (W - ddof) and C_ab / (W - ddof), left to the caller.  Float64 atomics add in arbitrary order: the last bits can differ
 * between runs, except for data whose sums are exact in every order.
 *   values_a, values_b, weights: xhist_arrays of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0
 *   broadcast); all three are validated before any device work.
 *   out_wsum (float64): contiguous [n_rows, prod(nb_d)]; out_mean (float64): contiguous [2, n_rows, prod(nb_d)], mean_a then
 *   mean_b; out_comoment (float64): contiguous [3, n_rows, prod(nb_d)], M2_a, C_ab, M2_b.  DEVICE buffers, overwritten (no
 *   accumulate mode); two float64 scratch blocks of [n_rows, prod(nb_d)] are taken from the library's allocator for the call.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`.  xhist_plan_describe then names the kernel family of each pass and where its slots live
 *   ("cov_w pass1=covw_sum_..."). */
int xhist_plan_execute_cov_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values_a,
                                    const xhist_array* values_b, const xhist_array* weights, int64_t n_rows, int64_t n_cols,
                                    double* out_wsum, double* out_mean, double* out_comoment, int mem_kind, void* stream);

/* Per-bin quantiles of `values`, exact: every output element is what np.nanquantile(values of that bin as float64, q[i],
 * method=...) gives, bit for bit, NaN for a bin with no value.  Which samples count is exactly what xhist_plan_execute counts
 * (same digitize, last bin closed, NaN / out-of-range samples dropped); NaN values are ignored.  Rows of at most 4096 values
 * are sorted in LDS, a few whole rows per workgroup; longer rows take an exact radix select on order-preserving keys of the
 * values, in a fixed number of streaming passes, its working state in row chunks of at most 256 MiB (one row at least).
 *   values: an xhist_array of any real dtype, same logical [n_rows, n_cols] shape as the samples (strides 0 broadcast).
 *   q: HOST array of n_q values in [0, 1] (not checked here); method: one of the XHIST_Q_* codes (numpy's method names).
 *   out: contiguous float64 [n_q, n_rows, prod(nb_d)] DEVICE buffer, overwritten.  Scratch comes from the library's allocator.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Asynchronous on `stream`, no host synchronisation.  xhist_plan_describe then names the family, the kernel family and home
 *   of the passes, the digit width d, the number of passes and the row chunks; the radix line ends with the successor pass of
 *   the interpolating methods, successor=<family>/<home>/<lds_bytes> (its home may differ from pass 0's: it keeps one window per
 *   target of a group where pass 0 keeps one per bin). */
#define XHIST_Q_LINEAR 0
#define XHIST_Q_LOWER 1
#define XHIST_Q_HIGHER 2
#define XHIST_Q_MIDPOINT 3
#define XHIST_Q_NEAREST 4
int xhist_plan_execute_quantile(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                int64_t n_rows, int64_t n_cols, const double* q, int n_q, int method, double* out,
                                int mem_kind, void* stream);

/* Weighted per-bin quantiles of `values` (added within ABI v11): numpy's method="inverted_cdf" with weights.  Samples and
 * values count as for xhist_plan_execute_quantile; each brings its weight, converted to float64.  Per bin, with C(x) the sum
 * of the weights of the values <= x and W the sum of all: the smallest value x with C(x) / W >= q[i] (one float64 division) and
 * C(x) > 0, or the largest value of positive weight if rounding leaves none.  NaN where the bin has no value, W is not finite
 * and positive, or a weight of the bin is NaN or negative.  On weights whose float64 sums are exact in any order every element
 * equals np.nanquantile(values of the bin, q[i], weights=..., method="inverted_cdf") bit for bit (zeros by value); on other
 * weights the order of the sums moves C and W in their last bits and the result may be a neighbouring value of the bin.
 *   weights: an xhist_array of any real dtype, shaped like the values (strides 0 broadcast).  The fast kernels take weights of
 *   the sample dtype with unit column stride; anything else runs the generic family.  Rows of at most 2048 values are sorted
 *   in LDS.  q, out, mem_kind, stream and scratch are those of xhist_plan_execute_quantile.  xhist_plan_describe then starts
 *   with "weighted_quantile family=...". */
int xhist_plan_execute_quantile_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                         const xhist_array* weights, int64_t n_rows, int64_t n_cols, const double* q, int n_q,
                                         double* out, int mem_kind, void* stream);

/* The per-sample maps (added within ABI v11: a new entry, every earlier one unchanged): from a per-bin result back to the
 * samples.  One 8-byte element per sample, into `out`, a DENSE row-major [n_rows, n_cols] DEVICE block whatever the strides of
 * the inputs are: element (r, c) is the result of the sample at (r, c) of the views.  Which samples count is exactly what
 * xhist_plan_execute counts (same digitize, last bin closed, NaN / out-of-range samples dropped, in ANY dimension).
 *   XHIST_MAP_INDEX    int64: the C-order flat index of the sample's bin over the plan's bin axes (the first input slowest:
 *                      np.ravel_multi_index), -1 for a sample that is not counted.  values, centre and scale must be NULL.
 *   XHIST_MAP_TAKE     float64: centre[r, bin], NaN for a sample that is not counted.  values and scale must be NULL.
 *   XHIST_MAP_ANOMALY  float64: (double)values[r, c] - centre[r, bin], one IEEE subtraction; where scale is given, divided by
 *                      scale[r, bin], one IEEE division.  NaN for a sample that is not counted; a NaN value stays NaN.
 *   values: an xhist_array of any real dtype, shaped like the samples (strides 0 broadcast); XHIST_MAP_ANOMALY only.
 *   centre, scale: contiguous float64 [n_rows, prod(nb_d)] DEVICE tables, read only (the outputs of
 *   xhist_plan_execute_mean_var, for instance: they need not leave the device).
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Every element of `out` is written exactly once and nothing outside it; nothing is accumulated.  Asynchronous on `stream`.
 *   A plan without bins (an edge array of a single edge) counts no sample: the block is then filled with -1 / NaN, the NaN
 *   being the all-ones bit pattern.
 *   xhist_plan_describe then reads "map op=index|take|anomaly family=fast|generic|none table=lds|global|none scan=.. cmp=..
 *   segs=.. block=.. lds_bytes=..": the kernel family (none: a plan without bins or a call without columns) and where the table
 *   row of a workgroup lives. */
#define XHIST_MAP_INDEX 0
#define XHIST_MAP_TAKE 1
#define XHIST_MAP_ANOMALY 2
int xhist_plan_execute_map(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, int64_t n_rows,
                           int64_t n_cols, int op, const double* centre, const double* scale, void* out, int mem_kind,
                           void* stream);

/* bin_order (added within ABI v11: a new entry, every earlier one unchanged): the stable group-by of every row's samples by
 * bin, a counting sort of the keys xhist_plan_execute_map gives with XHIST_MAP_INDEX (the same samples count, in the same
 * bins; a sample that is not counted has key -1, which sorts behind every bin).  With B = prod(nb_d), per row r:
 *   out_order[r, :]    int64, a permutation of 0 .. n_cols - 1: the columns sorted by key, columns of equal keys ascending
 *                      (np.argsort(key, kind="stable") with -1 replaced by B).
 *   out_offsets[r, b]  int64, b = 0 .. B: the number of columns whose key is below b.  The columns of bin b are
 *                      out_order[r, out_offsets[r, b] : out_offsets[r, b + 1]], the columns that are not counted
 *                      out_order[r, out_offsets[r, B] :], and the differences of a row are xhist_plan_execute's counts.
 *   out_order, out_offsets: contiguous DEVICE blocks [n_rows, n_cols] and [n_rows, B + 1]; every element of both is written
 *   exactly once and nothing outside them.  n_cols == 0 gives offsets of 0.  A plan without bins (an edge array of a single
 *   edge) gives out_offsets [n_rows, 1] of 0 and out_order[r, c] = c.
 *   n_cols must be below 2^31 and (B + 1) * 4 bytes must fit the LDS of a workgroup (B <= 40959 on an MI355X):
 *   XHIST_ERR_UNSUPPORTED otherwise, before any launch.
 *   Scratch of the call: n_rows * n_cols * 8 bytes of keys and a counter table of at most a quarter of that wherever a row is
 *   cut into several chunks, with 1/64 of the table again for the totals of 64 chunks (n_rows * (B + 1) * 4 bytes where a row
 *   is one chunk).
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Exact and deterministic: no result depends on the order in which waves arrive.  Asynchronous on `stream`.
 *   xhist_plan_describe then reads "group keys=fast|generic|none bits=.. waves=.. block=.. chunks=.. chunk=.. lds_bytes=..
 *   rows_per_launch=.. D=.. cmp=..": the kernel family that made the keys (none: a plan without bins or a call without
 *   columns), the ballots of a step, the waves of a workgroup, and how a row was cut. */
int xhist_plan_execute_group(xhist_plan* plan, const xhist_array* samples, int64_t n_rows, int64_t n_cols,
                             int64_t* out_order, int64_t* out_offsets, int mem_kind, void* stream);

/* bin_sort (added within ABI v11: a new entry, every earlier one unchanged): every row's samples grouped by bin as
 * xhist_plan_execute_group groups them and, inside each bin, sorted by value.  With key[c] the bin key of column c (-1 replaced
 * by B) and vk[c] the order-preserving uint64 key of values[c] taken as float64 (unsigned order is the total order of the values
 * with -0.0 < +0.0; its bits are complemented when `descending` is nonzero; 2^64 - 1 for a NaN in either direction, so NaN is
 * last in its bin either way), per row r:
 *   out_order[r, :]    int64, a permutation of 0 .. n_cols - 1: np.lexsort((vk, key)), by bin, then by value, ties in
 *                      ascending column.  The columns that are not counted, out_order[r, out_offsets[r, B] :], are sorted by
 *                      value too.
 *   out_offsets[r, b]  int64, b = 0 .. B: the number of columns whose key is below b, as xhist_plan_execute_group's.
 *   out_order, out_offsets: contiguous DEVICE blocks [n_rows, n_cols] and [n_rows, B + 1]; every element of both is written
 *   exactly once and nothing outside them.  n_cols == 0 gives offsets of 0.  A plan without bins gives out_offsets
 *   [n_rows, 1] of 0 and every row sorted by value.
 *   values: any real dtype, any strides.  n_cols must be below 2^31 and B + 1 at most 2^32: XHIST_ERR_UNSUPPORTED otherwise,
 *   before any launch.  There is no bound from the LDS: a stable least-significant-digit radix sort on 8-bit digits, first of
 *   the value keys (digits the dtype of the values makes constant are not launched: 8 passes for float64 and 64-bit integers,
 *   5 for float32, 3 for float16, 6 / 4 / 3 / 2 for integers of 32 / 16 / 8 bits and bool), then of the gathered bin keys in
 *   ceil(log2(B + 1) / 8) passes, every pass with 256 counters per wave.
 *   Scratch of the call: 32 bytes per sample (8 of bin keys, two blocks of 8-byte keys, two of 4-byte positions; 24 for a plan
 *   without bins) and at most 256 MiB of counters, 1 KiB per (row, chunk) of a launch.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Exact and deterministic: the place of a record is a function of the keys alone.  Asynchronous on `stream`.
 *   xhist_plan_describe then reads "sort keys=fast|generic|none value_passes=.. bin_passes=.. waves=.. block=.. chunks=..
 *   chunk=.. slices=.. rows_per_launch=.. D=.. cmp=.. vdtype=..": the kernel family that made the bin keys (none: a plan
 *   without bins or a call without columns), the passes of each phase, and how a row was cut. */
int xhist_plan_execute_sort(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, int64_t n_rows,
                            int64_t n_cols, int descending, int64_t* out_order, int64_t* out_offsets, int mem_kind,
                            void* stream);

/* bin_rank (added within ABI v11: a new entry, every earlier one unchanged): the rank of every sample's value among the values
 * of its bin.  Per row r, with S the columns of bin b that xhist_plan_execute counts and whose value, taken as float64, is not
 * NaN, n = |S|, the values of S in ascending order (descending when `descending` is nonzero) and ties decided by IEEE == (so
 * -0.0 and +0.0 tie), for a column c of S with value v: lt the number of values of S strictly before v in that order, eq the
 * number equal to v, d the number of distinct values up to and including v, D the number of distinct values of S.
 *   out[r, c] = (2 lt + eq + 1) / 2   XHIST_RANK_AVERAGE
 *               lt + 1                XHIST_RANK_MIN
 *               lt + eq               XHIST_RANK_MAX
 *               d                     XHIST_RANK_DENSE
 *               i - out_offsets[r, b] + 1 for out_order[r, i] == c of xhist_plan_execute_sort on the same arguments
 *                                     XHIST_RANK_ORDINAL: ties in ascending column, -0.0 before +0.0 (after it when descending)
 *   and with `pct` nonzero that rank divided once, in IEEE float64, by n (by D for XHIST_RANK_DENSE).  NaN (0x7ff8000000000000)
 *   for a column that is not counted and for a column whose value is NaN.  Every rank is an integer or a half-integer below
 *   2^31: every result is exact.
 *   out: a contiguous DEVICE block [n_rows, n_cols] of float64, a row's columns in position order; every element is written
 *   exactly once and nothing outside it.  A plan without bins counts no sample: the block is filled with NaN, the all-ones bit
 *   pattern.
 *   values: any real dtype, any strides.  An unknown method is XHIST_ERR_INVALID.  n_cols must be below 2^31 and B + 1 at most
 *   2^32: XHIST_ERR_UNSUPPORTED otherwise, before any launch.
 *   The call is xhist_plan_execute_sort into scratch and six kernels over its sorted order: head and NaN bits of every sorted
 *   position from two ballots per 64 positions (the only gather of the values), a scan of the head words per row in three
 *   launches (tiles of 1024 words), the divisors per (row, bin) when pct, and the ranks scattered to out.  No kernel waits for
 *   another workgroup.
 *   Scratch of the call, on top of xhist_plan_execute_sort's: 8 bytes per sample of order, n_rows * (B + 1) * 8 bytes of
 *   offsets, 28 bytes per 64 samples of a row (two 8-byte words of bits and three uint32), 12 bytes per 65536 samples of a row
 *   (a tile's three uint32), and n_rows * B * 8 bytes of divisors when pct; XHIST_ERR_NOMEM where it cannot be had.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Exact and deterministic.  Asynchronous on `stream`.
 *   xhist_plan_describe then reads "rank method=average|min|max|dense|ordinal pct=.. descending=.. words=.. rows_per_launch=..
 *   | " followed by xhist_plan_execute_sort's own line ("none" for a call without columns or a plan without bins): the words of
 *   64 positions of a row and the rows of one launch. */
typedef enum {
  XHIST_RANK_AVERAGE = 0,
  XHIST_RANK_MIN,
  XHIST_RANK_MAX,
  XHIST_RANK_DENSE,
  XHIST_RANK_ORDINAL
} xhist_rank_method;
int xhist_plan_execute_rank(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, int64_t n_rows,
                            int64_t n_cols, int method, int descending, int pct, double* out, int mem_kind, void* stream);

/* histogram_mode (added within ABI v11: a new entry, every earlier one unchanged): per bin the most frequent value, how often it
 * occurs and how many different values there are: the statistic of categorical values.  Per row r and bin b, with S the columns
 * of bin b that xhist_plan_execute counts and whose value, taken as float64, is not NaN, and equality of values decided by IEEE
 * == (so -0.0 and +0.0 are one value):
 *   out_count[r, b]      = |S|, xhist_plan_execute_mean_var's count bit for bit
 *   out_nunique[r, b]    = the number of distinct values of S
 *   out_mode_count[r, b] = the largest number of columns of S that hold one value
 *   out_mode[r, b]       = that value; among several values that occur that often the smallest.  Its bits are those of the
 *                          first column of the value in xhist_plan_execute_sort's ascending order on the same arguments: where
 *                          the value is a zero that S holds with both signs, -0.0.
 *   An empty bin (|S| == 0, a bin of only NaN values included) gets 0, 0, 0 and NaN (0x7ff8000000000000).
 *   The four outputs are contiguous DEVICE blocks [n_rows, B], int64 but out_mode, which is float64; every element of each is
 *   written exactly once and nothing outside them.  A NULL output is XHIST_ERR_INVALID.
 *   values: any real dtype, any strides.  n_cols must be below 2^31 and B + 1 at most 2^32: XHIST_ERR_UNSUPPORTED otherwise,
 *   before any launch.
 *   The call is xhist_plan_execute_sort into scratch, the head and NaN bits and the scan of the head words of
 *   xhist_plan_execute_rank, and two kernels over them.  In the sorted order the columns of one value of one bin are a run
 *   between two head bits.  One wave per 64 positions packs every run that starts there as (length << 32 | 2^32 - 1 - start),
 *   takes the maximum per bin across its lanes and issues at most one 64-bit atomic maximum per (64 positions, bin), and only
 *   where it improves on the slot it read first; the maximum of integers does not depend on the order of arrival.  One thread
 *   per (row, bin) then finds the end of the bin's non-NaN values by bisection, takes the distinct values as a difference of two
 *   head counts and gathers the one value at the winning run's start.  No kernel waits for another workgroup.  A call without
 *   columns launches the second kernel alone.
 *   Scratch of the call, on top of xhist_plan_execute_sort's: xhist_plan_execute_rank's without the divisors, that is 8 bytes
 *   per sample of order, n_rows * (B + 1) * 8 bytes of offsets, 28 bytes per 64 samples of a row and 12 bytes per 65536 samples
 *   of a row; XHIST_ERR_NOMEM where it cannot be had.  The slots of the atomic maximum are the out_mode_count block itself,
 *   zeroed by the call and finished in place.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Exact and deterministic.  Asynchronous on `stream`.
 *   xhist_plan_describe then reads "mode words=.. rows_per_launch=.. | " followed by xhist_plan_execute_sort's own line ("none"
 *   for a call without columns): the words of 64 positions of a row and the rows of one launch. */
int xhist_plan_execute_mode(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                            int64_t* out_count, int64_t* out_nunique, double* out_mode, int64_t* out_mode_count, int mem_kind,
                            void* stream);

/* bin_unique (added within ABI v11: a new entry, every earlier one unchanged): per row the distinct values of every bin and how
 * often each occurs, in CSR form: np.unique(v_bin, return_counts=True, return_inverse=True) per bin.  Per row r and bin b, with S
 * the columns of bin b that xhist_plan_execute counts and whose value, taken as float64, is not NaN, and equality of values
 * decided by IEEE == (so -0.0 and +0.0 are one value); B the number of bins, W = size:
 *   out_offsets[r, b]  = the number of distinct values in the bins below b, for b = 0 .. B; np.diff of a row is
 *                        xhist_plan_execute_mode's out_nunique bit for bit, and U = out_offsets[r, B] the row's number of
 *                        distinct (bin, value) pairs.  It always tells the truth, whatever `size` is.
 *   out_uniques[r, u]  for out_offsets[r, b] <= u < out_offsets[r, b + 1]: the distinct values of S, ascending.  The bits of an
 *                        entry are those of the value's first column in xhist_plan_execute_sort's ascending order on the same
 *                        arguments: a zero that S holds with both signs reads -0.0.
 *   out_counts[r, u]   = the number of columns of S whose value == out_uniques[r, u]
 *   Entries min(U, W) <= u < W are padding: 0x7ff8000000000000 in out_uniques and 0 in out_counts.  Entries u >= W are stored
 *   nowhere: silent truncation, which the caller sees as out_offsets[r, B] > size.
 *   out_inverse[r, c]  (NULL: none) = the entry u of column c's value, also where u >= W; -1 for a column that is not counted
 *                        and for a column whose value is NaN.
 *   out_offsets is a contiguous DEVICE block [n_rows, B + 1] of int64, out_uniques [n_rows, size] of float64, out_counts
 *   [n_rows, size] of int64, out_inverse [n_rows, n_cols] of int64 with a row's columns in position order.  Every element of
 *   each is written and nothing outside them.  A NULL out_offsets, and with size > 0 a NULL out_uniques or out_counts, is
 *   XHIST_ERR_INVALID, and so is a negative size.  A plan without bins gives offsets of 0, padding only and an inverse of -1; a
 *   call without columns offsets of 0 and padding only.
 *   values: any real dtype, any strides.  n_cols must be below 2^31 and B + 1 at most 2^32: XHIST_ERR_UNSUPPORTED otherwise,
 *   before any launch.
 *   The call is xhist_plan_execute_sort into scratch, the head and NaN bits and the scan of the head words of
 *   xhist_plan_execute_rank, and up to five kernels over them.  Inside a bin the values precede the NaNs and a bin's first
 *   position is a head, so the entry of a position is the offset of its bin plus the heads from the bin's start up to it.  One
 *   thread per (row, bin) writes the bin's distinct values into out_offsets, one workgroup per row scans them in place, one wave
 *   per 64 positions stores the value (the one gather besides the head pass's) and the run length of every head below W, the
 *   padding is written, and with an inverse one wave per 64 positions scatters the entries.  No kernel waits for another
 *   workgroup and none issues an atomic.
 *   Scratch of the call, on top of xhist_plan_execute_sort's: xhist_plan_execute_rank's without the divisors; XHIST_ERR_NOMEM
 *   where it cannot be had.
 *   mem_kind must be XHIST_MEM_DEVICE (host data: upload it first); anything else is XHIST_ERR_INVALID.
 *   Exact and deterministic.  Asynchronous on `stream`, no synchronisation with the host.
 *   xhist_plan_describe then reads "unique size=.. inverse=0|1 words=.. rows_per_launch=.. | " followed by
 *   xhist_plan_execute_sort's own line ("none" for a call without columns or a plan without bins). */
int xhist_plan_execute_unique(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                              int64_t size, double* out_uniques, int64_t* out_counts, int64_t* out_offsets, int64_t* out_inverse,
                              int mem_kind, void* stream);

/* bin_weighted_unique (added within ABI v11: a new entry, every earlier one unchanged): xhist_plan_execute_unique with a weight
 * per column and one output more, for samples that are not equal (a grid cell's area or volume).  out_uniques, out_counts,
 * out_offsets and out_inverse are xhist_plan_execute_unique's on the same arguments, bit for bit, with its rules for `size`,
 * padding and truncation.
 *   out_weight_sums[r, u] = the float64 sum of float64(weights[r, c]) over the columns c that out_counts[r, u] counts.  A
 *                           column whose value is NaN belongs to no entry, whatever its weight.  Padding entries are +0.0,
 *                           entries u >= size are stored nowhere.  Weights are not checked: a zero weight still counts in
 *                           out_counts, negative weights add, a NaN weight makes its own entry NaN and no other, and +inf and
 *                           -inf in one entry give NaN.
 *   out_weight_sums is a contiguous DEVICE block [n_rows, size] of float64; every element is written and nothing outside it.
 *   With size > 0 a NULL out_uniques, out_counts or out_weight_sums is XHIST_ERR_INVALID, and so are a NULL out_offsets, NULL
 *   weights and a negative size.  weights: any real dtype, any strides (stride 0: broadcast).
 *   The order of the additions is part of the interface.  The columns of an entry are one run of the sorted order, in ascending
 *   column inside it.  One wave per 64 positions gathers the weights (the call's only gather of them), takes an inclusive
 *   segmented sum between the head bits in six shuffle steps, stores every run that starts and ends inside its 64 positions,
 *   and leaves two sums: of the lanes before its first head and from its last head on.  A segmented scan over these, in tiles of
 *   1024 words as the scan of the head words goes, gives every word the sum of the run that enters it, and the word in which
 *   that run ends stores it.  There is no floating-point atomic, no kernel waits for another workgroup, and the tree of a run
 *   depends on its first and last sorted position in its row alone: the same bits run to run, on any stream, for any grid and
 *   any rows_per_launch, with and without an inverse and for any size.  On weights whose partial sums are all exact in float64
 *   every sum is the exact one; otherwise it is within 2 * gamma(n) * sum |w| of it, n the entry's count.
 *   Scratch of the call, on top of xhist_plan_execute_unique's and only for size > 0: 16 bytes per 64 samples of a row and 16
 *   bytes per 65536 samples of a row; XHIST_ERR_NOMEM where it cannot be had.
 *   mem_kind must be XHIST_MEM_DEVICE; anything else is XHIST_ERR_INVALID.  Asynchronous on `stream`, no synchronisation with
 *   the host.
 *   xhist_plan_describe then reads "wunique size=.. inverse=0|1 words=.. rows_per_launch=.. | " followed by
 *   xhist_plan_execute_sort's own line ("none" for a call without columns or a plan without bins). */
int xhist_plan_execute_unique_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values,
                                       const xhist_array* weights, int64_t n_rows, int64_t n_cols, int64_t size, double* out_uniques,
                                       int64_t* out_counts, double* out_weight_sums, int64_t* out_offsets, int64_t* out_inverse,
                                       int mem_kind, void* stream);

/* histogram_weighted_mode (added within ABI v11: a new entry, every earlier one unchanged): per bin the value that carries the
 * most weight.  out_count and out_nunique are xhist_plan_execute_mode's, bit for bit.  With the entries of bin b as
 * xhist_plan_execute_unique_weighted gives them for size = n_cols:
 *   out_mode_weight[r, b] = the largest out_weight_sums entry of the bin, compared as IEEE compares (-0.0 and +0.0 are equal);
 *                           bitwise the first entry of the segment that holds the maximum
 *   out_mode[r, b]        = out_uniques of that entry, by bits: among equal sums the smallest value
 *   Where any entry sum of the bin is NaN, both are 0x7ff8000000000000.  An empty bin (a bin of only NaN values included) gets
 *   0, 0, NaN (0x7ff8000000000000) and +0.0.  With all weights 1 out_mode is xhist_plan_execute_mode's by bits and
 *   out_mode_weight == out_mode_count.
 *   The four outputs are contiguous DEVICE blocks [n_rows, B], int64 the first two, float64 the others; every element of each
 *   is written exactly once and nothing outside them.  A NULL output and NULL weights are XHIST_ERR_INVALID.  n_cols must be
 *   below 2^31 and B + 1 at most 2^32: XHIST_ERR_UNSUPPORTED otherwise, before any launch.
 *   The call is xhist_plan_execute_mode's up to the scan of the head words, then the run sums of
 *   xhist_plan_execute_unique_weighted, each stored at its run's first sorted position, and three kernels: one wave per 64
 *   positions takes the maximum per bin of an order-preserving 64-bit key of the sums (-0.0 as +0.0, NaN the largest) and issues
 *   at most one 64-bit integer atomic maximum per (64 positions, bin), read first; a second walk has the runs whose key equals
 *   the slot take an integer atomic minimum of their start; one thread per (row, bin) writes the four outputs and gathers the
 *   one value.  Integer atomics only: neither result depends on the order of arrival.
 *   Scratch of the call, on top of xhist_plan_execute_mode's: 8 bytes per sample, 16 bytes per 64 samples of a row and 16 bytes
 *   per 65536 samples of a row; XHIST_ERR_NOMEM where it cannot be had.  The slots of the atomics are the out_mode_weight and
 *   out_mode blocks, filled by the call and finished in place.
 *   mem_kind must be XHIST_MEM_DEVICE.  Deterministic.  Asynchronous on `stream`.
 *   xhist_plan_describe then reads "wmode words=.. rows_per_launch=.. | " followed by xhist_plan_execute_sort's own line ("none"
 *   for a call without columns). */
int xhist_plan_execute_mode_weighted(xhist_plan* plan, const xhist_array* samples, const xhist_array* values, const xhist_array* weights,
                                     int64_t n_rows, int64_t n_cols, int64_t* out_count, int64_t* out_nunique, double* out_mode,
                                     double* out_mode_weight, int mem_kind, void* stream);

/* One-shot form of the two calls above with an internal plan cache keyed on (device, edges). */
int xhist_bincount_rows(int device, int n_inputs, const xhist_array* samples,
                        const xhist_array* weights, int64_t n_rows, int64_t n_cols,
                        const void* const* edges, const int64_t* n_edges, int cmp_domain, void* out,
                        int out_dtype, int mem_kind, int accumulate, void* stream);

/* min / max over a logical [M, C] array, NaN-propagating like numpy's a.min()/a.max(): feeds
 * np.histogram_bin_edges' (first_edge, last_edge) when bins is an int and range is None
 * (core.py:383-388).  result[0] = min, result[1] = max, as float64 (HOST pointer). */
int xhist_minmax(int device, const xhist_array* a, int64_t n_rows, int64_t n_cols, double* result,
                 int mem_kind, void* stream);

/* count / min / max / mean / sum of squared deviations of the elements of a DEVICE-resident [M, C] array that lie in
 * [lo, hi] (use_range != 0; NaN never does) or of all of them: what numpy's bin-width estimators need of the data —
 * np.histogram_bin_edges with bins = "sqrt" | "sturges" | "rice" | "scott" (core.py:383-388 hands it the whole array,
 * which for a GPU-resident array would mean a copy to the host).  result (HOST, 5 doubles) = {count, min, max, mean, M2};
 * min / max are NaN when a counted element is NaN (numpy then rejects the range); M2 only when want_m2 != 0 (a second
 * pass over the data with the mean of the first).  Synchronises `stream`. */
int xhist_moments(int device, const xhist_array* a, int64_t n_rows, int64_t n_cols, int use_range, double lo, double hi,
                  int want_m2, double* result, int mem_kind, void* stream);

/* ---- exchange between GPUs (one process per GPU; RCCL over xGMI) ---------------------------- */
/* Sharded inputs produce one partial histogram per GPU; what the reference does with dask's
 * `bin_counts.sum(drop_axes)` (core.py:439) is ONE in-place all-reduce of that small buffer
 * (shards cut along a reduced axis) or an all-gather of rows (shards cut along a kept axis:
 * disjoint output rows).  These calls wrap RCCL, which is dlopen-ed on first use (an RCCL the
 * process has mapped already is shared; XHIST_AMD_RCCL overrides the path), so single-GPU users and
 * hosts that bring their own collective never load it.
 *   rank 0: xhist_comm_unique_id -> hand the 128 bytes to every rank by any out-of-band means
 *   (the host's launcher, a file, MPI) -> every rank: xhist_comm_create (collective).
 * Buffers are DEVICE pointers on the comm's device; calls are asynchronous on `stream` and must be
 * issued in the same order on every rank.  int64 sums are exact and order-independent. */
#define XHIST_COMM_ID_BYTES 128
typedef enum { XHIST_REDUCE_SUM = 0, XHIST_REDUCE_MIN = 1, XHIST_REDUCE_MAX = 2 } xhist_reduce_op;
typedef struct xhist_comm xhist_comm; /* opaque: one RCCL communicator bound to one device */
int xhist_comm_unique_id(void* id, size_t cap);
int xhist_comm_create(int device, int rank, int world_size, const void* id, size_t id_bytes, xhist_comm** out);
/* any of rank / world_size / device / rccl_version may be NULL */
int xhist_comm_info(const xhist_comm* comm, int* rank, int* world_size, int* device, int* rccl_version);
/* in place; dtype XHIST_I64 (counts), XHIST_F64 or XHIST_F32 (weighted sums; min / max of the data
 * for bins=int: the reference's np.histogram_bin_edges sees the whole array, core.py:383-388) */
int xhist_comm_allreduce(xhist_comm* comm, void* buf, int64_t count, int dtype, int op, void* stream);
/* recv holds world_size * count elements, rank r's block at offset r * count */
int xhist_comm_allgather(xhist_comm* comm, const void* send, void* recv, int64_t count, int dtype, void* stream);
/* Deadlines: xhist_comm_create (the rendezvous) and xhist_comm_wait (the completion of collectives) do not wait for a
 * peer for ever: XHIST_AMD_COMM_TIMEOUT_S seconds (environment, default 300; <= 0: no deadline;
 * XHIST_AMD_COMM_CREATE_TIMEOUT_S, when set, overrides it for the rendezvous alone).  On expiry, or on an
 * asynchronous RCCL error, the communicator is aborted (ncclCommAbort: kernels of a collective in flight return), the call
 * returns XHIST_ERR_COMM with a message naming rank, world size and what was waited for, and every later call on the
 * communicator returns XHIST_ERR_COMM at once; xhist_comm_destroy is still due.
 * xhist_comm_wait: block until everything enqueued on `stream` has completed — the host-side synchronisation point of
 * an exchange, in place of a bare hipStreamSynchronize that a dead peer would hang. */
int xhist_comm_wait(xhist_comm* comm, void* stream);
int xhist_comm_destroy(xhist_comm* comm);

/* ---- device buffers ------------------------------------------------------------------------ */
/* Partial histograms that stay on their GPU between the kernel and the exchange, for hosts without a
 * device allocator of their own (the Python shim with numpy inputs; a C host).  What they carry is the
 * per-block result of `_bincount` (core.py:197-247) on its way into the sum over blocks (core.py:439).
 *   xhist_buffer_copy direction: 0 host -> device, 1 device -> host (both final when the call returns),
 *   2 device -> device on `device` (asynchronous on `stream`).
 *   xhist_buffer_add: dst[i] += src[i] on `device`, int64 or float64, asynchronous on `stream` — the sum
 *   of the partials of the blocks one GPU processed, before the all-reduce adds up the GPUs. */
int xhist_buffer_alloc(int device, size_t bytes, void** dptr);
int xhist_buffer_free(int device, void* dptr);
int xhist_buffer_copy(int device, void* dst, const void* src, size_t bytes, int direction, void* stream);
int xhist_buffer_add(int device, void* dst, const void* src, int64_t count, int dtype, void* stream);

/* Strided N-D copy between device buffers of `device`, asynchronous on `stream`: element (i_0 … i_{ndim-1}) of the source
 * (byte strides `src_strides`, 0 and negative allowed) goes to the same index of the destination (`dst_strides`).
 * ndim <= 8.  dst_dtype == src_dtype copies raw elements; dst_dtype == XHIST_F64 converts every supported dtype to float64
 * (numpy's promotion inside searchsorted, core.py:170).  This is what blocks of a device-resident dask array need around
 * the path: the moveaxis + reshape copy of core.py:218-226 for layouts no three strides describe, slices, and the
 * concatenation of unaligned chunks (test_chunking.py:104-146) — without a host round trip and without torch. */
int xhist_buffer_copy_nd(int device, int ndim, const int64_t* shape, const void* src, int src_dtype, const int64_t* src_strides,
                         void* dst, int dst_dtype, const int64_t* dst_strides, void* stream);
/* GPU a device pointer belongs to (for arrays that arrive through __cuda_array_interface__, which does not say) */
int xhist_pointer_device(const void* ptr, int* device);

/* ---- diagnostics / tuning (not part of the reference contract) ----------------------------- */
/* keys: "block_threads", "grid_blocks" (0 = auto), "force_global" (0/1), "force_generic" (0/1),
 *       "partition" (0 auto / 1 prefer / -1 never: multi-pass mode for histograms beyond LDS),
 *       "fused" (0 auto / 1 always / -1 never: that mode in one routing pass instead of count + prefix + scatter),
 *       "records48" (0 auto / -1 never: that pass moves float64 weights as 8-byte records — 36 mantissa bits next to the bin code,
 *       2^-37 relative per weight — while a call's weights have one sign, decided on the GPU; both signs fall back to full
 *       float64 records in the same call; XHIST_AMD_EXACT_RECORDS=1 is the process-wide "never"; full float64 records of a joint
 *       histogram travel through the rings of the "exchange" mode too, as 12-byte records in two tagged words — the weight bit
 *       for bit, any sign mixture),
 *       "exchange" (0 auto / 1 whenever the kernel can run / -1 never: such packed records never written to HBM — one persistent
 *       workgroup per compute unit keeps rows of a window of the histogram in LDS and records travel through rings inside each
 *       XCD; auto = float64 samples + float64 weights on numpy.linspace-style edges, one row of >= 2^25 samples, a chip of
 *       8 x 32 compute units, and a window that a probe on the GPU finds to hold 88 % of the call's samples; setting the key
 *       also re-admits a plan at once that an exchange aborted IN FLIGHT had taken off the mode — otherwise such a plan stays
 *       on the classic passes for its next 16 eligible calls, twice as many after every further abort, and is admitted again),
 *       "exchange_arrive_us" (0 = 200: how long the mode's 256 workgroups wait for one another to START — a compute unit held
 *       by another stream's or process's kernel keeps one out; after that nothing has been produced and the classic passes queued
 *       behind take the call; such calls are counted in the description, "exchange_arrival_misses", and do not take the plan off
 *       the mode), "exchange_budget_ms" (0 = 500: how long a workgroup waits for its peers ONCE RECORDS TRAVEL before the mode is
 *       switched off for the call and the classic passes take it; -1: not at all — tests), "exchange_min_pct" (0 = 88: the window
 *       coverage, per cent of the probe's samples, from which the mode takes a call),
 *       "lanes" (0 auto / 1 prefer / -1 never: one-row-per-lane kernels for many short rows),
 *       "arith" (0 auto / 1 prefer / -1 never: table-free digitize for numpy.linspace-style edges),
 *       "arith32" (0 auto / 1 prefer / -1 never: float32 samples on such edges digitized in float32 arithmetic),
 *       "pack" (0 auto / 1 whenever the plan has them / -1 never: packed 16-byte bucket entries — one LDS read per sample and
 *       dimension — for float64 / float32 samples on non-uniform edges, on a linear or a float-bit-pattern (logarithmic) grid),
 *       "route_grid", "acc_grid" (workgroups of the routing / adding-up pass of the multi-pass mode; 0 auto),
 *       "slices" (0 auto / 1 prefer / -1 never: histograms of a few times the LDS capacity in bin slices),
 *       "route_spl" (0 auto / 4: never the long 8-samples-per-lane tile) and "min_parts"
 *       (0 auto = 16 / 1 = as few as the histogram's size asks for / up to 128: partitions per row) shape the routing pass of
 *       the multi-pass mode; "route_pool_pct" (tests: its chunk pool cut to this percentage),
 *       "flat_rows" (0 auto / 1 for any row length below 65536 / -1 never: many dense short rows streamed as one array),
 *       "lds_copies" (0 = auto), "profile" (0 = off, R = keep the last R kernel timings),
 *       "profile_stride" (S >= 1: time every S-th execute only — for microsecond kernels, where the two event records of
 *       the profile mode cost as much as the launch itself) */
int xhist_plan_set_param(xhist_plan* plan, const char* key, int64_t value);
/* human-readable description of the last launch (kernel family, LDS bytes, copies, grid...) */
int xhist_plan_describe(xhist_plan* plan, char* buf, size_t cap);
/* "profile" = R > 0 keeps HIP-event pairs (recorded on the caller's stream, tightly around the
 * histogram kernel launch(es), after the output memset) for the R most recent device executes.
 * This call synchronises them, writes up to `cap` durations (ms, oldest first) and resets. */
int xhist_plan_profile_read(xhist_plan* plan, float* ms, int cap, int* n_out);

/* the library's scratch cache on `device` (staging buffers, record streams of the partitioned mode, transposes): stats[0] = bytes
 * cached (free, kept for reuse), [1] = bytes callers hold right now, [2] = bytes the cache may keep — twice what the largest
 * recent call held at once, at least 64 MiB, at most half of the device; $XHIST_AMD_POOL_KEEP_GB fixes it — [3] = that recent peak. */
int xhist_scratch_stats(int device, uint64_t* stats, int n);

/* TEST SUPPORT (ABI v9) — stands in for "somebody else's kernel holds compute units" (an RCCL kernel of a collective on another
 * stream, another process on the GPU): launches `workgroups` workgroups of 64 threads with `lds_bytes` of LDS each on `stream`,
 * which do nothing but wait until `microseconds` have passed.  With lds_bytes >= 64 KiB no 158 KB workgroup of the exchange mode
 * (the persistent kernel behind BASELINE C5's path, /root/reference/xhistogram/core.py:73-83 beyond LDS) can share their compute
 * units, which is what tests/test_gpu_exchange.py needs to show that such a call fails fast instead of waiting for a deadline.
 * Asynchronous; replaces nothing of the reference. */
int xhist_debug_hold_cus(int device, int workgroups, int lds_bytes, int64_t microseconds, void* stream);

/* TEST SUPPORT (added within ABI v11) — xhist_plan_execute_sum's integer arithmetic on the HOST, over one bin: the `n` values
 * (HOST pointer; NaN ignored) go through the very functions the kernels compile (the unit from the extremes, the limbs, the one
 * rounding), the accumulators plain int64 additions.  Needs no device; n < 2^31. */
int xhist_debug_sum_host(const double* values, int64_t n, int64_t* out_count, double* out_total);
/* ... and the one rounding alone: *out = RN_even((L0 + L1 * 2^32 + L2 * 2^64) * 2^U), -1074 <= U <= 1023. */
int xhist_debug_sum_round(int64_t L0, int64_t L1, int64_t L2, int U, double* out);

/* free cached plans and scratch on every device */
int xhist_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* XHIST_AMD_H */

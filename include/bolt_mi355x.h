/*
 * bolt_mi355x.h -- C ABI of libbolt_mi355x.so, the MI355X (gfx950) execution
 * backend for bolt's Spark-mode data-parallel hot path.
 *
 * The reference (beautifulNow1992/bolt v0.7.1) is pure Python; its "FFI" for
 * this path is the pyspark RDD API that the bolt/spark modules call.  Every entry
 * point below replaces one of those call sites; the ctypes binding a bolt
 * maintainer would add is bolt_amd/_lib.py.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch / numpy types cross this ABI.
 *   - Device buffers are owned by the caller (PyTorch allocations passed as
 *     tensor.data_ptr()).  The library allocates no device memory: scratch
 *     comes from a caller-provided workspace.
 *   - All work is stream-ordered on the caller's HIP stream (`stream` is a
 *     hipStream_t; NULL = the legacy default stream).  No call synchronises
 *     the device.
 *   - Every function returns 0 on success and a negative BM_E* code on
 *     failure; the message is available from bm_last_error() (thread-local).
 *     Nothing throws or aborts across this boundary.
 *   - Strides and shapes are in ELEMENTS, int64, C order (outermost first).
 */
#ifndef BOLT_MI355X_H
#define BOLT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM_ABI_VERSION 1

/* status codes */
#define BM_OK 0
#define BM_E_ARG (-1)    /* invalid argument (shape, stride, dtype, ...)   */
#define BM_E_HIP (-2)    /* a HIP runtime call failed (launch, ...)       */
#define BM_E_WS (-3)     /* workspace too small                            */
#define BM_E_COMM (-4)   /* communicator failed: async RCCL error, timeout or abort */

/* element dtypes understood by the reductions (numpy kinds) */
#define BM_BOOL 0
#define BM_U8 1
#define BM_I8 2
#define BM_U16 3
#define BM_I16 4
#define BM_U32 5
#define BM_I32 6
#define BM_U64 7
#define BM_I64 8
#define BM_F16 9
#define BM_F32 10
#define BM_F64 11

/* statistics (bolt/spark/array.py:_stat names + reduce(add)) */
#define BM_STAT_MEAN 0   /* StatCounter.mean      statcounter.py:109-112 */
#define BM_STAT_VAR 1    /* StatCounter.variance  statcounter.py:119-125 */
#define BM_STAT_STD 2    /* StatCounter.stdev     statcounter.py:127-130 */
#define BM_STAT_SUM 3    /* reduce(operator.add)  array.py:243-282, :381-395 */
#define BM_STAT_MAX 4    /* reduce(numpy.maximum) array.py:397-411 (NaN propagates) */
#define BM_STAT_MIN 5    /* reduce(numpy.minimum) array.py:413-427 (NaN propagates) */
/* reduce(func) with a numpy ufunc, array.py:243-282 (treeReduce(func)) */
#define BM_STAT_PROD 6   /* numpy.multiply / operator.mul (bool: logical and)   */
#define BM_STAT_LAND 7   /* numpy.logical_and -> bool                           */
#define BM_STAT_LOR 8    /* numpy.logical_or  -> bool                           */
#define BM_STAT_BAND 9   /* numpy.bitwise_and / operator.and_ (int, bool)       */
#define BM_STAT_BOR 10   /* numpy.bitwise_or  / operator.or_  (int, bool)       */
#define BM_STAT_BXOR 11  /* numpy.bitwise_xor / operator.xor  (int, bool)       */
#define BM_STAT_FMAX 12  /* numpy.fmax (NaN ignored unless all NaN)             */
#define BM_STAT_FMIN 13  /* numpy.fmin                                          */

/* Version of this ABI (BM_ABI_VERSION).  Host code refuses a mismatch. */
int bm_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char *bm_last_error(void);

/* Number of compute units of the current device (for sizing), or <0. */
int bm_device_cus(void);

/*
 * bm_host_writable -- *ok = 1 if [p, p + bytes) is page-locked host memory that
 * the current device addresses at the same pointer, else 0.  Statistics with
 * small results (mean/var/std/sum over most axes, array.py:284-395) pass such
 * a buffer as bm_reduce's `out`: the kernel stores the result into host
 * memory and the separate device-to-host copy (collect, array.py:1012-1014)
 * disappears.
 */
int bm_host_writable(const void *p, size_t bytes, int *ok);

/*
 * bm_copy_strided -- dst[i] = src[i] over an N-d index space.
 *
 * The single data-movement primitive of the backend.  It replaces every
 * record-moving call site of the Spark path:
 *   - the ingest transpose + parallelize    bolt/spark/construct.py:55-69
 *   - ChunkedArray._chunk flatMap (pack)    bolt/spark/chunk.py:131-142
 *   - ChunkedArray.unchunk / removepad      bolt/spark/chunk.py:146-200, :514-550
 *   - keys_to_values partitionBy+_rebuild   bolt/spark/chunk.py:202-289
 *   - values_to_keys flatMap(_extract)      bolt/spark/chunk.py:291-347
 *   - Keys.transpose / Values.transpose     bolt/spark/shapes.py:66-89, :136-159
 *   - the multi-GPU swap's pack and unpack around the all-to-all
 *   - basic indexing, BoltArraySpark._getbasic  bolt/spark/array.py:480-512
 * Element i = (i_0..i_{n-1}) is read at src + sum(i_k*src_strides[k]) and
 * written at dst + sum(i_k*dst_strides[k]) (strides in elements; source
 * strides may be negative -- a reversed slice, BoltArraySpark.__getitem__
 * array.py:480-676 -- destination strides are >= 0; dst must not overlap
 * itself or src).
 * elem_bytes: any positive size (1/2/4/8/16 are native; others are moved
 * as bytes).  Data is moved bit-exactly.  ndim <= 24.
 */
int bm_copy_strided(const void *src, void *dst, int ndim, const int64_t *shape,
                    const int64_t *src_strides, const int64_t *dst_strides,
                    int elem_bytes, void *stream);

/*
 * bm_copy_strided_moments -- bm_copy_strided of a float32 / float64 array
 * whose destination is `nrows` rows of `R` elements, `row_pitch` (>= R)
 * elements apart, which also leaves the BM_STAT_VAR state of every row
 * (mean[nrows] then M2[nrows], float64: what bm_reduce_state(BM_STAT_VAR)
 * of the written rows gives, from other arithmetic) in `state`, so that a
 * later mean / var / std over the rows is
 *   bm_reduce_combine(stat, in_dtype, state, counts = {R}, nparts = 1, nrows, ...)
 * and does not read the array again (swap, then statistics over the moved
 * key axis: array.py:716-763 followed by _stat, array.py:284-334).
 *
 * The state is written (*fused = 1) only when the copy is a tile transpose
 * on 16-B vectors whose destination-contiguous dim is the row itself (its
 * extent is R), every row starts at a multiple of row_pitch elements below
 * nrows * row_pitch, and the row spans at most 256 tiles; the transpose
 * kernel then emits the state of every (row, tile) -- a pivot, mean - pivot
 * and M2, float64 -- into `workspace` and a merge kernel combines them in
 * tile order.  In every other case the call is
 * exactly bm_copy_strided: *fused = 0 and `state` is not touched.  The bytes
 * written to dst are bm_copy_strided's in both cases.
 * workspace: bm_copy_strided_moments_workspace_bytes of the same arguments
 * (0: this copy never fuses; the pointer may then be NULL).  state_bytes >=
 * bm_reduce_state_bytes(BM_STAT_VAR, in_dtype, nrows).
 * BM_E_ARG, before anything is launched: in_dtype not BM_F32 / BM_F64 or
 * elem_bytes not its size, state or fused NULL, state_bytes too small,
 * row_pitch < R, or prod(shape) != nrows * R.  BM_E_WS: the copy fuses and
 * the workspace is too small.
 */
int bm_copy_strided_moments_workspace_bytes(int ndim, const int64_t *shape,
                                            const int64_t *src_strides,
                                            const int64_t *dst_strides, int elem_bytes,
                                            int in_dtype, int64_t R, int64_t row_pitch,
                                            int64_t nrows, size_t *bytes);
int bm_copy_strided_moments(const void *src, void *dst, int ndim, const int64_t *shape,
                            const int64_t *src_strides, const int64_t *dst_strides,
                            int elem_bytes, int in_dtype, int64_t R, int64_t row_pitch,
                            int64_t nrows, void *workspace, size_t workspace_bytes,
                            void *state, size_t state_bytes, int *fused, void *stream);

/*
 * bm_permute -- dst = ascontiguousarray(src.transpose(perm)) for a
 * C-contiguous src of `shape`.  This is BoltArraySpark.swap
 * (bolt/spark/array.py:716-763) and .transpose / .T / .swapaxes
 * (array.py:765-833) collapsed into their net permutation; one kernel,
 * bit-exact for every dtype.
 */
int bm_permute(const void *src, void *dst, int ndim, const int64_t *shape,
               const int32_t *perm, int elem_bytes, void *stream);

/*
 * bm_gather_rows -- dst[a, j, :] = src[a, idx[j], :] for a C-contiguous src
 * viewed as [n_outer][src_rows][row_bytes]; dst is [n_outer][n_idx][row_bytes].
 * idx is a DEVICE array of n_idx int64 row numbers in [0, src_rows) (the host
 * checks bounds, as BoltArraySpark.__getitem__ does, array.py:652-659).
 * The non-strided selections of __getitem__ (bolt/spark/array.py:514-593):
 *   _getmixed    one index list on one axis (x.take(idx, axis)),
 *   _getadvanced one list per axis -> a point gather (row = one element).
 * Bit-exact for every dtype.
 */
int bm_gather_rows(const void *src, void *dst, int64_t n_outer, int64_t src_rows,
                   int64_t row_bytes, const int64_t *idx, int64_t n_idx, void *stream);

/*
 * bm_record_gather -- dst[r*dst_rec + o] = src[r*src_rec + map[o]] for
 * r < nrec, o < dst_rec (sizes in elements of elem_bytes = 1/2/4/8).
 * map is a DEVICE array of dst_rec int32 indices in [0, src_rec), shared by
 * every record.  The pack and unpack of ChunkedArray for small records:
 *   pack   ChunkedArray._chunk flatMap     bolt/spark/chunk.py:131-142
 *          (map: packed chunk element -> dense value index, halos included)
 *   unpack ChunkedArray.unchunk/removepad  bolt/spark/chunk.py:146-200, :514-550
 *          (map: dense value index -> packed element of its chunk's core)
 * A source record of <= 64 KiB is staged whole in LDS; bit-exact.
 * parts (HOST array, nparts <= 8; nparts 0 or 1 = the whole record): the
 * destination record split into ranges, part p = {dlo, dhi, slo, shi}:
 * dst[dlo, dhi) reads only src[slo, shi) (every map entry of the range lies
 * there; the caller guarantees it), staged alone -- a smaller LDS tile.  The
 * ranges must tile [0, dst_rec) in order.
 */
int bm_record_gather(const void *src, void *dst, int64_t nrec, int64_t src_rec,
                     int64_t dst_rec, const int32_t *map, int nparts,
                     const int64_t *parts, int elem_bytes, void *stream);

/*
 * Reductions over a C-contiguous array viewed as [O][R][I]: the middle axis
 * (R records) is reduced, O*I outputs are produced in [O][I] order.  This is
 * the aligned layout that BoltArraySpark._align (array.py:85-115) builds
 * before StatCounter / treeReduce run (array.py:269, :321-323).
 *
 * Arithmetic: floating inputs and every mean/var/std accumulate in float64
 * (combined across lanes, waves, blocks and chunks in a fixed order:
 * deterministic) and round once to out_dtype.  SUM over integer dtypes is modular in the input width
 * (numpy add of same-dtype arrays wraps: the reference's treeReduce(add));
 * SUM over BM_BOOL is logical OR (numpy bool add).  MAX / MIN compare in the
 * input dtype with numpy.maximum / numpy.minimum semantics (a NaN wins),
 * FMAX / FMIN with numpy.fmax / numpy.fmin (a NaN loses).  PROD over floats
 * accumulates in float64, over integers is modular in the input width, over
 * BM_BOOL is logical AND.  LAND / LOR test x != 0 and write BM_BOOL;
 * BAND / BOR / BXOR act on the element bits (integer and bool dtypes only).
 * out_dtype: BM_F16/BM_F32/BM_F64 for MEAN/VAR/STD and float SUM/PROD;
 * BM_BOOL for LAND/LOR; in_dtype otherwise.
 * var / std: batched Welford -- each lane reduces a batch of up to 32 values
 * around a pivot drawn from the batch, merged by Chan's formula
 * (statcounter.py:51-59, :85-96) -- so the relative error of M2 stays
 * O(32 eps) whatever the offset or outliers of the data.
 * Population variance (M2/n), std = sqrt(var), as statcounter.py:119-130.
 */
/*
 * bm_record_gather_masked -- bm_record_gather whose (record, part) tiles
 * stage only the 16-B units of their source range that the map reads:
 * stage_mask (DEVICE, nparts x mask_words uint32) has bit k of part p set
 * when unit k (bytes [16k, 16k + 16) from the part's slo) holds an element
 * the part's map entries name.  values_to_keys drops the moved axis' halo
 * rows, which then stay in HBM (bolt/spark/chunk.py:291-347, removepad
 * :514-550).  A NULL mask stages everything (= bm_record_gather).
 */
int bm_record_gather_masked(const void *src, void *dst, int64_t nrec, int64_t src_rec,
                            int64_t dst_rec, const int32_t *map, int nparts,
                            const int64_t *parts, const uint32_t *stage_mask,
                            int mask_words, int elem_bytes, void *stream);

/*
 * bm_record_scatter -- the packed -> packed moves whose source record is read
 * whole, as one stream: for record r < nrec (src_rec elements each, records
 * contiguous) and element p,
 *     dst[(r / group) * dst_group_stride + map_a[p] + (r % group) * map_b[p]]
 *         = src[r * src_rec + p]                    (map_a[p] < 0: dropped)
 * map_a / map_b: DEVICE int32 arrays of src_rec entries (map_b may be NULL:
 * 0).  Replaces, for small records,
 *   - keys_to_values of the trailing keys (group = their extent, map_b = the
 *     chunk box sizes)                     bolt/spark/chunk.py:202-289
 *   - values_to_keys (group 1)             bolt/spark/chunk.py:291-347
 *   - unchunk, padding dropped (group 1)   bolt/spark/chunk.py:146-200
 * vec: elements per vector (power of two, vec * elem_bytes <= 16); the caller
 * guarantees every aligned vec-group of source elements is dropped whole or
 * lands on vec consecutive, vec-aligned destinations.  Bit-exact.
 */
int bm_record_scatter(const void *src, void *dst, int64_t nrec, int64_t src_rec,
                      int64_t group, int64_t dst_group_stride, const int32_t *map_a,
                      const int32_t *map_b, int vec, int elem_bytes, void *stream);

/*
 * bm_record_runs -- bm_record_scatter's moves when every source record is a
 * few long runs (no maps): run b of record r = g * group + k is copied whole,
 *     dst[g * dst_group_stride + a_b + k * m_b + j] = src[r * src_rec + s_b + j]
 * for j < len_b.  runs: DEVICE int64 array [s_b, len_b, a_b, m_b] x nruns,
 * in units of vec_bytes-byte vectors (vec_bytes a power of two in
 * [elem_bytes, 16] dividing every record, stride and run; the caller checks
 * the runs lie inside the records and the destination).  src_rec and
 * dst_group_stride are in elements; nrec must be a multiple of group.
 * flags: BM_RUNS_TILED when the runs tile every new record (m_b = len_b and
 * the regions [a_b, a_b + group * len_b), sorted by a_b, lie back to back
 * from 0 to dst_group_stride; at most 64 runs): the kernel then walks the
 * destination in order, whole lines per wave, each lane finding its source;
 * the flag on runs that do not tile gives wrong bytes (every read stays inside
 * a run of a source record of the group, the runs themselves inside the
 * records as above).  Without the flag: one wave per (record, run).
 * C5's keys_to_values((2,)): 16 chunk boxes of 2.6-3.2 KB per record
 * (bolt/spark/chunk.py:202-289).  Bit-exact.
 */
#define BM_RUNS_TILED 1
int bm_record_runs(const void *src, void *dst, int64_t nrec, int64_t src_rec,
                   int64_t group, int64_t dst_group_stride, int nruns,
                   const int64_t *runs, int vec_bytes, int flags, int elem_bytes,
                   void *stream);

int bm_reduce_workspace_bytes(int stat, int in_dtype, int64_t O, int64_t R,
                              int64_t I, size_t *bytes);

int bm_reduce(int stat, const void *src, int in_dtype, int64_t O, int64_t R,
              int64_t I, void *out, int out_dtype, void *workspace,
              size_t workspace_bytes, void *stream);

/*
 * bm_reduce over rows of a padded layout (I = 1): row o is the R elements at
 * src + o * row_pitch (row_pitch >= R, in elements; the pad is never read).
 * The per-record statistics of a transposed result -- mean / std over the
 * time axis after swap((0,),(0,1)), bolt/spark/array.py:284-334 over
 * statcounter.py -- when the swap wrote its rows at a line-aligned pitch
 * (a row of 2000 float32 at 8000 B starts 64 B into a line every other row;
 * padded to 8192 B the transpose and this read both run whole lines).
 * Results identical to bm_reduce on the compacted rows when row_pitch keeps
 * the rows' 16-B vector width (a pitch in whole vectors: every padded layout
 * the array makes; other pitches read narrower vectors, another summation
 * order); the same workspace (bm_reduce_workspace_bytes with I = 1 covers
 * every pitch).
 */
int bm_reduce_rows(int stat, const void *src, int in_dtype, int64_t O, int64_t R,
                   int64_t row_pitch, void *out, int out_dtype, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * bm_reduce_moments -- mean, variance and standard deviation of one read of
 * src: what the reference's StatCounter holds after one pass over a partition
 * (stats='all': n, mu and m2 together, bolt/spark/statcounter.py:30-48), which
 * _stat (bolt/spark/array.py:284-334) reads one moment of per call.  The
 * layout is bm_reduce's [O][R][I]; with I == 1, row_pitch >= R reads padded
 * rows as bm_reduce_rows does (row_pitch = R otherwise).  out_mean / out_var /
 * out_std receive O*I values of out_dtype (a float dtype) each; any may be
 * NULL (not all), and any may be a bm_host_writable host buffer.  The launches,
 * workspace (bm_reduce_workspace_bytes of BM_STAT_VAR) and summation order are
 * those of bm_reduce(BM_STAT_VAR): var and std are bit-identical to
 * bm_reduce's, the mean is the Welford mean of the same state (S1 / n for 1-
 * and 2-byte integers), within rounding of bm_reduce(BM_STAT_MEAN)'s.
 */
int bm_reduce_moments(const void *src, int in_dtype, int64_t O, int64_t R,
                      int64_t I, int64_t row_pitch, void *out_mean, void *out_var,
                      void *out_std, int out_dtype, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * bm_reduce_keep -- bm_reduce / bm_reduce_rows of a mean, variance or standard
 * deviation that keeps what its read saw: the reference's _stat
 * (bolt/spark/array.py:284-334) builds the whole StatCounter (n, mu, m2:
 * bolt/spark/statcounter.py:30-48) on every call and reads one moment of it;
 * an array's records never change, so the counter of (array, axes) is kept
 * and a later var / std is bm_reduce_combine of it (one part, count R) with
 * no read of the array.  stat is BM_STAT_MEAN, BM_STAT_VAR or BM_STAT_STD;
 * the layout, row_pitch, out and out_dtype (a float dtype) are
 * bm_reduce_moments'; the workspace is bm_reduce_workspace_bytes of stat.
 * out receives exactly the bytes bm_reduce / bm_reduce_rows writes.  state
 * (bm_reduce_state_bytes(BM_STAT_VAR, in_dtype, O*I) bytes, device memory)
 * receives from the same read the two planes bm_reduce_state(BM_STAT_VAR)
 * stores, bit for bit -- absolute mean[O*I], then M2[O*I] -- and *kept = 1.
 * Integer inputs and plans that split R into chunks run the plain launches:
 * state is left untouched and *kept = 0.
 */
int bm_reduce_keep(int stat, const void *src, int in_dtype, int64_t O, int64_t R,
                   int64_t I, int64_t row_pitch, void *out, int out_dtype,
                   void *state, int *kept, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * bm_standardize_rows -- center / z-score of rows in one read and one write:
 *   dst[o*dst_pitch + r] = (src[o*src_pitch + r] - mean_o) [/ std_o],  r < R,
 * mean_o and std_o (population, ddof = 0: bolt/spark/statcounter.py:109-130)
 * over row o's R elements; scale = 0 subtracts the mean only, scale = 1 also
 * divides.  No reference call site: the reference has no center / zscore (an
 * API addition, like bm_reduce_moments' stats()); the pipelines built on it
 * subtract and divide on the host from what mean() / std() return
 * (bolt/spark/array.py:336-379).  Pitches are in elements, >= R; the pad is
 * neither read nor written.  out_dtype must be the statistics dtype of
 * in_dtype (float16 / float32 keep theirs, every other dtype gives float64).
 * Each row is held in registers between its read and its write -- one wave per
 * row, or one 256-thread block per longer row; the moments are float64
 * two-pass sums over the held values, the subtraction and the (true) division
 * are float64, rounded once to out_dtype; the same input gives the same bytes.
 * A row of zero variance centres to zeros and scales to nan (0/0); a nan makes
 * its whole row nan.  *taken = 1 when the rows were written; *taken = 0 and
 * nothing launched when a row is longer than the kernels hold on chip, or
 * when longer rows are too few to give each a block (bm_reduce_moments, then
 * bm_standardize_apply, serve those).  O == 0 or R == 0 writes nothing
 * (*taken = 1).  Arguments are checked before any launch.
 */
int bm_standardize_rows(const void *src, int in_dtype, int64_t O, int64_t R,
                        int64_t src_pitch, void *dst, int out_dtype,
                        int64_t dst_pitch, int scale, int *taken, void *stream);

/*
 * bm_standardize_apply -- the elementwise half of center / z-score for every
 * layout bm_standardize_rows does not take: over bm_reduce's [O][R][I],
 *   dst[o,r,i] = (src[o,r,i] - mean[o*I+i]) [/ std[o*I+i]],
 * mean / std being float64 device planes of O*I values (bm_reduce_moments or
 * bm_reduce_combine_moments with out_dtype BM_F64); std NULL: centre only.
 * No reference call site (an API addition, see bm_standardize_rows).  With
 * I == 1 the rows of src / dst are src_pitch / dst_pitch elements apart
 * (>= R); with I > 1 both pitches must be R.  out_dtype and the arithmetic
 * are bm_standardize_rows'.  The planes are read through the cache, the array
 * with streaming loads and stores: one read and one write of the array.
 * Any of O, R, I == 0 writes nothing.  Arguments are checked before any launch.
 */
int bm_standardize_apply(const void *src, int in_dtype, int64_t O, int64_t R,
                         int64_t I, int64_t src_pitch, const double *mean,
                         const double *std, void *dst, int out_dtype,
                         int64_t dst_pitch, void *stream);

/*
 * bm_detrend_rows -- every row minus its least-squares polynomial of degree
 * `order` (1..BM_DETREND_MAX_ORDER, and < R) in one read and one write:
 *   dst[o*dst_pitch + r] = d_r - sum_{k=1..order} C_k p_k(t_r),  r < R,
 * d_r = src[o*src_pitch + r] - mean_o.  No reference call site: the reference
 * has no detrend (an API addition, like bm_standardize_rows' center / zscore);
 * thunder's Series.detrend fits every record on the host.  The convention is
 * scipy.signal.detrend's: the mean goes with the trend.  Pitches are in
 * elements, >= R; the pad is neither read nor written.  out_dtype must be the
 * statistics dtype of in_dtype (float16 / float32 keep theirs, every other
 * dtype gives float64).  Numerics, all float64: no Vandermonde matrix is
 * formed; p_k are the discrete orthonormal (Gram) polynomials on the row's R
 * positions, t_r = r - (R-1)/2, b_k = (k/2) sqrt((R-k)(R+k) / (4k^2-1)),
 *   p_0 = 1/sqrt(R), p_1 = t p_0 / b_1, p_{k+1} = (t p_k - b_k p_{k-1}) / b_{k+1}
 * (b_k and 1/b_k formed on the host, the kernel multiplies by the reciprocal;
 * no table is read: every lane walks the recurrence over the positions it
 * holds); mean_o is bm_standardize_rows' two-pass mean about the row's first
 * element, C_k = sum_r d_r p_k(t_r) summed in a fixed order (the same input
 * gives the same bytes), the fit is summed k ascending and the result rounded
 * once to out_dtype.  Each row is held in registers between its read and its
 * write, as bm_standardize_rows holds it, and *taken follows the same plan:
 * 1 when the rows were written; 0 and nothing launched when a row is longer
 * than the kernels hold on chip, or when longer rows are too few to give each
 * a block (bm_comoment_state with the basis as the signals, then
 * bm_detrend_apply, serve those).  A constant row gives exact zeros; a nan or
 * an infinity makes its whole row nan.  O == 0 or R == 0 writes nothing
 * (*taken = 1).  Arguments are checked before any launch; a refused call
 * leaves *taken alone.
 */
#define BM_DETREND_MAX_ORDER 8   /* two batches of BM_COMOMENT_MAX_SIGNALS */
int bm_detrend_rows(const void *src, int in_dtype, int64_t O, int64_t R,
                    int64_t src_pitch, int order, void *dst, int out_dtype,
                    int64_t dst_pitch, int *taken, void *stream);

/*
 * bm_detrend_apply -- the elementwise half of detrend for every layout
 * bm_detrend_rows does not take: over bm_reduce's [O][R][I],
 *   dst[o,r,i] = (src[o,r,i] - mean[o*I+i]) - sum_{k<order} coef[k*O*I + o*I+i] * basis[k*R + r],
 * mean being a float64 device plane of O*I values, coef `order` such planes
 * (bm_comoment_state's mean and C planes against the basis) and basis
 * order x R float64 values in device memory, signal-major: p_1..p_order of
 * bm_detrend_rows at the R positions.  No reference call site (an API
 * addition, see bm_detrend_rows).  With I == 1 the rows of src / dst are
 * src_pitch / dst_pitch elements apart (>= R); with I > 1 both pitches must be
 * R.  out_dtype is bm_detrend_rows'; the subtraction of the mean, the fit
 * (summed k ascending) and its subtraction are float64, rounded once.  Planes
 * and basis are read through the cache, the array with streaming loads and
 * stores: one read and one write of the array.  order outside
 * 1..BM_DETREND_MAX_ORDER gives BM_E_ARG; order >= R is taken, unlike
 * bm_detrend_rows: the table is the caller's, and R may be one rank's slab of
 * a record that is spread over ranks, shorter than the fit has terms.  Any of
 * O, R, I == 0 writes nothing.  Arguments are checked before any launch.
 */
int bm_detrend_apply(const void *src, int in_dtype, int64_t O, int64_t R,
                     int64_t I, int64_t src_pitch, const double *mean,
                     const double *coef, const double *basis, int order,
                     void *dst, int out_dtype, int64_t dst_pitch, void *stream);

/*
 * Partial reduction state for the multi-GPU merge (the per-partition
 * StatCounter of array.py:321-322).  `state` receives, for O*I outputs:
 *   MEAN/VAR/STD: two float64 planes, mean[O*I] then M2[O*I] (count = R);
 *   SUM / PROD float: one float64 plane (the sum / product);
 *   SUM / PROD int/bool, LAND / LOR / BAND / BOR / BXOR: one uint64 plane;
 *   MAX / MIN / FMAX / FMIN: one uint64 plane holding the element's bits.
 * bm_reduce_state_bytes gives the state size in bytes.
 */
int bm_reduce_state_bytes(int stat, int in_dtype, int64_t nout, size_t *bytes);

int bm_reduce_state(int stat, const void *src, int in_dtype, int64_t O,
                    int64_t R, int64_t I, void *state, void *workspace,
                    size_t workspace_bytes, void *stream);

/*
 * Combine nparts states (laid out back to back, part-major) in part order
 * -- the StatCounter.combine tree of statcounter.py:67-99 / treeReduce of
 * array.py:323, made deterministic -- and finalise into out[nout].
 * counts: host array of nparts record counts (parts with count 0 are
 * skipped).  nparts <= 256.
 */
int bm_reduce_combine(int stat, int in_dtype, const void *states,
                      const int64_t *counts, int nparts, int64_t nout,
                      void *out, int out_dtype, void *stream);

/*
 * bm_reduce_combine(BM_STAT_VAR) finalised into every moment asked for: the
 * merged StatCounter (bolt/spark/statcounter.py:30-48, :67-99) read for mean,
 * variance and stdev at once instead of once per _stat call
 * (bolt/spark/array.py:284-334).  states: nparts two-plane BM_STAT_VAR states
 * of bm_reduce_state (mean[nout] then M2[nout], part-major), merged in part
 * order exactly as bm_reduce_combine merges them.  out_mean / out_var /
 * out_std as for bm_reduce_moments; with every count 0 the mean is 0 and var /
 * std are NaN.
 */
int bm_reduce_combine_moments(int in_dtype, const void *states,
                              const int64_t *counts, int nparts, int64_t nout,
                              void *out_mean, void *out_var, void *out_std,
                              int out_dtype, void *stream);

/*
 * cov() / corr(): the co-moment of every record with fixed signals.
 * No reference call site: an API addition (the reference has neither method;
 * its users correlate on the host, record by record, through map()).  The
 * state extends the StatCounter of one partition (n, mu, m2:
 * bolt/spark/statcounter.py:30-48) by one co-moment per signal, and the merge
 * extends StatCounter.combine (bolt/spark/statcounter.py:67-99).
 */
#define BM_COMOMENT_MAX_SIGNALS 4   /* signals per call: one read of the array serves them all */
#define BM_COMOMENT_MAX_PARTS 128   /* parts per bm_comoment_combine */
#define BM_CO_COV 0    /* population covariance C / n (ddof = 0, as BM_STAT_VAR) */
#define BM_CO_CORR 1   /* Pearson r = C / sqrt(M2_x M2_y), clamped to [-1, 1]  */

/*
 * bm_comoment_workspace_bytes -- scratch bm_comoment_state needs for this
 * layout and K (the chunks' partial sums when the reduced extent is split;
 * 0 when it is not); it holds for every alignment of src and every pitch.  No reference call site: an API addition.  Monotone in
 * K; any of O, R, I == 0 gives 0.
 */
int bm_comoment_workspace_bytes(int in_dtype, int64_t O, int64_t R, int64_t I,
                                int K, size_t *bytes);

/*
 * bm_comoment_state -- one read of src ([O][R][I] as bm_reduce; with I == 1
 * rows are row_pitch >= R elements apart and the pad is never read, otherwise
 * row_pitch = R) into the co-moment state of its O*I records: (2 + K) float64
 * planes of O*I values, mean_x, M2_x, then for each signal k
 *   C_k = sum_r (x_r - mean_x) (y_k[r] - ymean_k).
 * No reference call site: an API addition; the state is the StatCounter's
 * (n = R, mu, m2) that statcounter.py:67-99 merges, with C_k added.
 * y: device memory, K*R float64, signal-major.  ymean (host, K values): what
 * each signal is centred by, the caller's float64 mean of its R values;
 * yresid (host, K values, or NULL for zeros): sum_r (y_k[r] - ymean_k), the
 * rounding residue of that mean, which the state is corrected by.  Every
 * accumulation is float64 about the record's first element, summed in a fixed
 * order (lanes, row phases, chunks: see bm_comoment.hip): the same input gives
 * the same bytes, and plane k has the bytes of the one-signal call with y_k.
 * workspace: bm_comoment_workspace_bytes (BM_E_WS if smaller).  A record
 * holding a nan or an infinity has a nan M2 and nan C_k, and the mean a sum
 * over it gives (+inf, -inf, or nan for inf - inf or a nan), wherever in the
 * record the value sits (the pivot is finite: such a first element takes 0);
 * other records are untouched.  Any of O, R, I == 0 stores
 * nothing.  Arguments are checked before any launch: null pointers, a bad
 * dtype, negative extents, a pitch below R or a pitch with I > 1, K outside
 * 1..BM_COMOMENT_MAX_SIGNALS give BM_E_ARG.
 */
int bm_comoment_state(const void *src, int in_dtype, int64_t O, int64_t R,
                      int64_t I, int64_t row_pitch, const double *y,
                      const double *ymean, const double *yresid, int K,
                      void *state, void *workspace, size_t workspace_bytes,
                      void *stream);

/*
 * bm_comoment_combine -- nparts states of bm_comoment_state (back to back,
 * part-major) merged in part order with the pairwise update of
 * statcounter.py:67-99, (mean, M2) as bm_reduce_combine merges them and
 *   C = Ca + Cb + (mean_xb - mean_xa) (ymean_b - ymean_a) na nb / (na + nb),
 * then finalised into K planes of nout values of out_dtype:
 *   what = BM_CO_COV:  C / n;
 *   what = BM_CO_CORR: C / sqrt(M2_x M2_y), clamped to [-1, 1] before the one
 *                      rounding; nan unless M2_x M2_y > 0 (a record or a
 *                      signal of zero variance, whatever rounding left in C).
 * A record that holds a nan or an infinity in any part (a nan M2 and C_k in
 * that part's state) gives nan, cov and corr alike; the merged mean is not
 * an output.
 * No reference call site: an API addition.  counts[nparts] (parts of count 0
 * are skipped; all 0: nan), ymean[nparts*K] and ym2[nparts*K] (each part's
 * own mean and sum of squared deviations of its slice of signal k, part-major)
 * are host arrays; the signals' side of the merge runs on the host.  out may
 * be a bm_host_writable buffer.  A local call is bm_comoment_state followed by
 * this with one part.  nparts <= BM_COMOMENT_MAX_PARTS.  nout == 0 stores
 * nothing.  BM_E_ARG for null pointers, what out of range, an out_dtype that
 * is not a statistics dtype (float16 / float32 / float64), K outside
 * 1..BM_COMOMENT_MAX_SIGNALS, nparts out of range, a negative count or nout.
 */
int bm_comoment_combine(int what, const void *states, const int64_t *counts,
                        const double *ymean, const double *ym2, int nparts,
                        int64_t nout, int K, void *out, int out_dtype,
                        void *stream);

/*
 * quantile() / percentile() / median(): exact order statistics of rows.
 * No reference call site: an API addition (the reference has no such method;
 * its users sort every record on the host through map()).  An order statistic
 * is one of the row's own values: both entry points select by rank on
 * order-preserving unsigned keys of the element's width (floats in IEEE order,
 * -0.0 before +0.0) and decode the selected key, so nothing is rounded but the
 * interpolation.  A call takes nq quantiles, quantile k given as
 *   ranks[k]: the 0-based rank of lo among the row's R values, and
 *   frac[k] in [0, 1): 0 gives lo; otherwise lo + (hi - lo) * frac[k] with hi
 *     the value of rank ranks[k] + 1, evaluated in float64 as three separately
 *     rounded operations (no fused multiply-add) and rounded once to out_dtype.
 * A quantile with frac != 0 takes two ranks; a call takes at most
 * BM_QUANTILE_MAX_RANKS ranks.  out: nq planes of O values, plane k at
 * out + k * O elements; it may be a bm_host_writable buffer.  out_dtype is
 * in_dtype itself (every frac 0: the selected elements, bit for bit) or the
 * statistics dtype of in_dtype (float16 / float32 keep theirs, every other
 * dtype gives float64; 64-bit integers beyond 2^53 round when converted).  A
 * row holding a NaN gives NaN in every output.  bool runs as uint8.
 */
#define BM_QUANTILE_MAX_RANKS 8

/*
 * bm_quantile_rows -- the quantiles of O rows of R elements, row_pitch >= R
 * elements apart (the pad is never read), from one read: each row is held in
 * registers as keys -- one wave per row, or one 256-thread block per longer
 * row -- and every rank is found by a binary search over the key's bits,
 * counting the keys below a candidate.  No reference call site: an API
 * addition.  *taken = 1 when the planes were written; *taken = 0 and nothing
 * launched when a row is longer than the kernels hold on chip, or when longer
 * rows are too few to give each a block (bm_quantile_select serves those).
 * O == 0 or R == 0 writes nothing (*taken = 1).  Arguments are checked before
 * any launch: null pointers, a bad dtype, an out_dtype that is neither of the
 * two above, negative extents, a pitch below R, nq outside 1..8, a frac
 * outside [0, 1), a rank (+ 1 where frac != 0) that is not below R and more
 * than BM_QUANTILE_MAX_RANKS ranks give BM_E_ARG.
 */
int bm_quantile_rows(const void *src, int in_dtype, int64_t O, int64_t R,
                     int64_t row_pitch, const int64_t *ranks,
                     const double *frac, int nq, void *out, int out_dtype,
                     int *taken, void *stream);

/*
 * bm_quantile_workspace_bytes -- scratch bm_quantile_select needs for O rows
 * and nranks ranks (nq plus one per frac != 0): the histograms, prefixes and
 * NaN counts of one batch of rows.  No reference call site: an API addition.
 * Monotone in O and nranks; O == 0 or R == 0 gives 0.
 */
int bm_quantile_workspace_bytes(int in_dtype, int64_t O, int64_t R, int nranks,
                                size_t *bytes);

/*
 * bm_quantile_select -- bm_quantile_rows' result for rows of any length: a
 * most-significant-byte-first radix select, sizeof(element) reads of the rows.
 * Each pass adds the keys that match a rank's prefix to 256-bin histograms
 * (LDS, then 64-bit integer atomics: deterministic) over rows x blocks per
 * row, so that one long row still fills the device, and a pick kernel extends
 * every prefix by the byte its rank falls in.  No reference call site: an API
 * addition.  workspace: bm_quantile_workspace_bytes (BM_E_WS if smaller or
 * NULL).  Arguments are checked as bm_quantile_rows checks them.
 */
int bm_quantile_select(const void *src, int in_dtype, int64_t O, int64_t R,
                       int64_t row_pitch, const int64_t *ranks,
                       const double *frac, int nq, void *out, int out_dtype,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * bm_normalize_rows -- every row against its own baseline b_o in one read and
 * one write (dF/F of a calcium-imaging pipeline):
 *   dst[o*dst_pitch + r] = (src[o*src_pitch + r] - b_o) / (b_o + offset),  r < R.
 * No reference call site: an API addition (thunder's Series.normalize does the
 * step on the host).  Pitches are in elements, >= R; the pad is neither read
 * nor written.  out_dtype must be the statistics dtype of in_dtype (float16 /
 * float32 keep theirs, every other dtype gives float64).  The baseline is
 *   BM_NORM_MEAN: the float64 mean of the row, formed as bm_standardize_rows
 *     forms it; rank and frac are ignored; *taken follows bm_standardize_rows'
 *     plan;
 *   BM_NORM_RANK: the order statistic given by rank and frac as one quantile
 *     of bm_quantile_rows -- frac in [0, 1), rank (+ 1 where frac != 0) below
 *     R -- that is lo, or lo + (hi - lo) * frac in float64, not rounded to
 *     out_dtype.  The row is held in registers as bm_quantile_rows' keys, the
 *     rank found by its bit search, and the held keys are decoded back to the
 *     values; *taken follows bm_quantile_rows' plan, where the vector width
 *     must also divide dst_pitch.
 * x - b, b + offset and the (true) division are three separately rounded
 * float64 operations, rounded once to out_dtype.  A row holding a NaN is NaN
 * throughout; b + offset == 0 gives what IEEE gives.  bool runs as uint8.
 * *taken = 1 when the rows were written; *taken = 0 and nothing launched when
 * the plan does not hold them (a baseline plane, then bm_standardize_apply
 * with mean = b and std = b + offset, serve those).  O == 0 or R == 0 writes
 * nothing (*taken = 1).  Arguments are checked before any launch: null
 * pointers, a bad dtype or out_dtype, negative extents, a pitch below R, a
 * baseline that is neither of the two, a bad rank or frac and a non-finite
 * offset give BM_E_ARG and leave *taken alone.
 */
#define BM_NORM_MEAN 0
#define BM_NORM_RANK 1
int bm_normalize_rows(const void *src, int in_dtype, int64_t O, int64_t R,
                      int64_t src_pitch, int baseline, int64_t rank,
                      double frac, double offset, void *dst, int out_dtype,
                      int64_t dst_pitch, int *taken, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Multi-GPU record exchange over RCCL (xGMI), one process per GPU.
 *
 * These replace the Spark shuffles that move records between executors:
 *   keys_to_values' partitionBy + _rebuild   bolt/spark/chunk.py:251-261
 *   unchunk's partitionBy (shuffle #2)       bolt/spark/chunk.py:179-191
 * (and so the swap / transpose that run through them, array.py:716-808), and
 * the driver-side merge of per-partition statistics partials
 * (treeReduce of StatCounter.combine, array.py:321-323).
 * RCCL is bound at run time (dlopen): the librccl already in the process
 * (PyTorch-ROCm's) is reused, else the system librccl.so.1.  All transfers
 * are stream-ordered on `stream`; no call blocks the host on the transfer.
 * Buffers are device memory owned by the caller; sizes and offsets in BYTES.
 */
#define BM_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */

/* Rank 0 creates the communicator id (BM_COMM_ID_BYTES) and sends it to the
 * other ranks out of band (bolt_amd sends it through the torch.distributed
 * rendezvous store). */
int bm_comm_unique_id(void *id, size_t bytes);

/* Collective over `world` ranks: every rank calls it with the same id and
 * its own rank, with its GPU current.  *comm receives an opaque handle. */
int bm_comm_init(void **comm, int world, const void *id, int rank);

/* Release a communicator (NULL is a no-op). */
int bm_comm_destroy(void *comm);

/* rank / world of a communicator and the path of the RCCL library in use
 * (lib may be NULL). */
int bm_comm_info(void *comm, int *rank, int *world, char *lib, size_t lib_bytes);

/*
 * bm_alltoallv -- block q of send (send_bytes[q] bytes at send_offs[q]) goes
 * to rank q; block s of recv (recv_bytes[s] at recv_offs[s]) arrives from rank
 * s.  The self block is a local device copy on `stream` (send_bytes[rank]
 * must equal recv_bytes[rank], else BM_E_ARG); the peers are one RCCL group of
 * ncclSend / ncclRecv pairs, every peer at once (each ordered GPU pair has its
 * own xGMI link).  The multi-GPU swap's exchange step (pack -> bm_alltoallv ->
 * unpack).  Arrays have `world` entries; send_bytes[q] must equal what rank q
 * expects (a mismatch across ranks is caught by bm_comm_wait's timeout).
 * BM_E_COMM if the communicator has failed or been aborted.
 */
int bm_alltoallv(void *comm, const void *send, const int64_t *send_bytes,
                 const int64_t *send_offs, void *recv, const int64_t *recv_bytes,
                 const int64_t *recv_offs, void *stream);

/*
 * bm_allgatherv -- rank s's send_bytes (its `send`) land at recv_offs[s] of
 * every rank's recv (recv_bytes[s] = rank s's send_bytes).  Uniform sizes at
 * packed offsets use ncclAllGather, others one group of point-to-point pairs.
 * Statistics states before bm_reduce_combine, and output slabs of reductions
 * that keep the sharded axis.
 */
int bm_allgatherv(void *comm, const void *send, int64_t send_bytes, void *recv,
                  const int64_t *recv_bytes, const int64_t *recv_offs, void *stream);

/*
 * bm_comm_wait -- block the host until all work queued on `stream` is done,
 * polling RCCL's asynchronous error meanwhile.  On an RCCL error, or when the
 * work is not done after timeout_s seconds (<= 0: no limit), the communicator
 * is aborted (ncclCommAbort: its kernels exit and the stream drains) and
 * BM_E_COMM is returned with the reason in bm_last_error() -- a lost or
 * mismatched peer becomes an error, not a hang.  This is how a failed Spark
 * shuffle (chunk.py:251-261) surfaces: as an exception on the driver.
 */
int bm_comm_wait(void *comm, void *stream, double timeout_s);

/* Non-blocking: BM_OK, or BM_E_COMM (communicator aborted) after an
 * asynchronous RCCL error or an earlier abort. */
int bm_comm_check(void *comm);

/* Abort now: pending exchanges stop, later calls return BM_E_COMM.
 * bm_comm_destroy still releases the handle. */
int bm_comm_abort(void *comm);

#ifdef __cplusplus
}
#endif

#endif /* BOLT_MI355X_H */

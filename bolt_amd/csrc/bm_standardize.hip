// bm_standardize.hip -- center / zscore of libbolt_mi355x (gfx950): every
// record minus its mean [over its standard deviation] along an axis.
//
// No reference call site: the reference has no such method (an API addition,
// like stats()); the pipelines built on it do the step on the host from the
// arrays mean() / std() return (bolt/spark/array.py:336-379).
//
// The result has the array's shape, so the floor is one read and one write.
//   rows kernel (the reduced axis is the last one, rows dense or padded): the
//     row is loaded once into registers -- one wave per row, or the four waves
//     of a block for longer rows -- its moments are taken from the registers,
//     and the held values are standardised and stored: one read, one write.
//   apply kernel (every other layout, and rows too long to hold): elementwise
//     over [O][R][I] with the float64 mean / std planes of a reduction that
//     ran before it (bm_reduce_moments): two reads and one write in all.
// Numerics (all float64): the row is in hand, so the moments are the
//   two-pass sums -- mean = P + sum(x - P) / n around the row's first element
//   P (0 if that is not finite, so a row with an infinity has numpy's mean
//   whatever the column it is in), then with d = x - mean, M2 = sum d^2 - (sum d)^2 / n (the second term
//   removes the rounding of the mean) and std = sqrt(M2 / n), the population
//   value of statcounter.py:109-130.  Lanes add their values in register order
//   and fold through DPP in lane order (wave_fold), waves through LDS in wave
//   order: deterministic.  d and d / std are formed in float64 (a true
//   division) and rounded once to the output dtype.  A row of zero variance
//   centres to exact zeros (d is x - x) and its z-score is 0/0 = nan, as numpy
//   gives; a nan in a row reaches its mean and so every output of the row.
// The rows kernel also serves bm_normalize_rows' mean baseline (bm_quantile.hip
//   holds the entry point): mode 2 divides d by mean + offset instead of std,
//   so the second pass over the held values is not run.
#include "bm_common.h"
#include "bm_host.h"
#include "bm_wave.h"
#include "../../include/bolt_mi355x.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
// Plan of bm_standardize_rows.  All three thresholds are UNMEASURED: they are
// set from the register budget, not from A/B runs.
//   a thread holds lane_vecs(vec) = min(8, 32 / vec) vectors, that is
//   min(8 * vec, 32) elements: 8 vectors of 16 B for 4- and 8-byte elements
//   (32 data registers; with the float64 temporaries the float32 kernel takes
//   104 registers, four waves a SIMD), 32 elements for narrower ones (their
//   float64 values are what fills the registers);
//   wave per row: rows up to 64 * that (2048 float32 at 16-B vectors, which
//   covers C2's 2000); block per row: rows up to 256 * that (8192 float32);
//   longer rows are not taken (*taken = 0: the caller's two-pass path);
//   a block per row with fewer than kBlockMinRows rows leaves CUs of the 256
//   without a block while each block waits on its own row: not taken either,
//   the two-pass kernels split such rows over the whole device.
constexpr int lane_vecs(int vec) { return vec * 8 <= 32 ? 8 : 32 / vec; }
constexpr int64_t kBlockMinRows = 256;
// -DBM_STD_RECIP (a variant build for A/B runs, Makefile EXTRA): the rows kernel
// multiplies by 1 / std instead of dividing -- what the division costs
#ifdef BM_STD_RECIP
constexpr bool kRecip = true;
#else
constexpr bool kRecip = false;
#endif
constexpr int kMaxVec = 8;  // elements per vector at most (1-byte inputs: 8-B loads, 64 B of float64 out)

// ------------------------------------------------------------------ rows --
struct RowsArgs {
  int64_t O, R;
  int64_t sp, dp;  // elements between row starts of src / dst (>= R)
  int64_t row0;    // first row of this launch (launches split at the grid limit)
  int32_t scale;   // 0: x - mean, 1: (x - mean) / std, 2: (x - mean) / (mean + offset)
  double offset;   // scale 2 (bm_normalize_rows' mean baseline)
};

// WPR waves per row (1, or the block's 4), each thread holding NV vectors of
// VEC elements: R <= 64 * WPR * VEC * NV (the host's plan), R % VEC == 0.
template <typename T, int VEC, int NV, int WPR>
__global__ void __launch_bounds__(kThreads)
    k_std_rows(const T *__restrict__ src, typename OutOf<T>::t *__restrict__ dst, RowsArgs a) {
  typedef typename OutOf<T>::t OT;
  __shared__ double sm[WPR];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int RPB = kThreads / 64 / WPR;  // rows per block
  const int64_t row = a.row0 + (int64_t)rows_block() * RPB + (WPR == 1 ? wave : 0);
  // wave per row: whole waves leave, and no barrier follows; block per row: the whole block leaves
  if (row >= a.O) return;
  const T *s = src + row * a.sp;
  OT *o = dst + row * a.dp;
  constexpr int64_t stride = (int64_t)64 * WPR * VEC;
  const int64_t j0 = (int64_t)(WPR == 1 ? lane : (int)threadIdx.x) * VEC;

  // the one read: j < R leaves a whole vector inside the row (R % VEC == 0)
  T v[NV][VEC];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[u][k] = T(0);
    if (j0 + u * stride < a.R) vload_nt<T, VEC>(s + j0 + u * stride, v[u]);
  }
  const double n = (double)a.R;
  const double P = finite_or_zero(to_f64(s[0]));  // (an infinite first value: the mean is the sum's, inf or nan)
  double s1 = 0.0;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const bool in = j0 + u * stride < a.R;
#pragma unroll
    for (int k = 0; k < VEC; ++k) s1 += in ? to_f64(v[u][k]) - P : 0.0;
  }
  const double mean = P + row_sum<WPR>(s1, lane, wave, sm) / n;
  double sd = 1.0;
  if (a.scale == 2) {
    sd = mean + a.offset;  // bm_normalize_rows: the baseline is the mean
  } else if (a.scale) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const bool in = j0 + u * stride < a.R;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double d = in ? to_f64(v[u][k]) - mean : 0.0;
        t1 += d;
        t2 = fma(d, d, t2);
      }
    }
    t1 = row_sum<WPR>(t1, lane, wave, sm);
    t2 = row_sum<WPR>(t2, lane, wave, sm);
    const double m2 = fma(-t1, t1 / n, t2);
    sd = sqrt((m2 < 0.0 ? 0.0 : m2) / n);  // (a nan stays a nan)
  }
  // the one write
  const bool recip = kRecip && a.scale == 1;
  const double inv = recip ? 1.0 / sd : 0.0;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    if (j0 + u * stride < a.R) {
      OT ov[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double d = to_f64(v[u][k]) - mean;
        ov[k] = (OT)(a.scale ? (recip ? d * inv : d / sd) : d);
      }
      store_out_nt<OT, VEC>(o + j0 + u * stride, ov);
    }
  }
}

// ----------------------------------------------------------------- apply --
// rows of one column vector a thread of the column kernel takes with the
// vector's mean / std held in registers: the planes' traffic (16 B of float64
// per element and plane) falls to 1/16 of the array's.  zscore of C2's columns
// (2000, 512, 512) over axis 0: 1.755 ms with one row per thread, 1.110 ms with
// 16 (profiles/standardize_ab.log); other values UNMEASURED
constexpr int kApplyRows = 16;

struct ApplyArgs {
  int64_t R, I;
  int64_t sp, dp;   // ROWS: elements between row starts of src / dst
  FastDiv nv;       // vectors per row (ROWS: R / VEC, else I / VEC)
  FastDiv nrc;      // columns: chunks of kApplyRows rows per o
  uint64_t total;   // work items: vectors (ROWS), (o, row chunk, column vector) (columns)
};

template <typename T, typename OT, int VEC>
__device__ __forceinline__ void apply_vec(const T (&v)[VEC], const double (&m)[VEC], const double (&s)[VEC],
                                          bool scale, OT (&ov)[VEC]) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const double d = to_f64(v[k]) - m[k];
    ov[k] = (OT)(scale ? d / s[k] : d);
  }
}

// ROWS (I == 1): vectors along R, one mean / std per row o.  Columns (I > 1):
// vectors along I, mean / std at [o * I + i], kApplyRows rows per thread.  The
// planes are read through the cache (neighbouring work items read the same
// values), the array streams.
template <typename T, int VEC, bool ROWS>
__global__ void __launch_bounds__(kThreads)
    k_std_apply(const T *__restrict__ src, typename OutOf<T>::t *__restrict__ dst, const double *__restrict__ mean,
                const double *__restrict__ sd, ApplyArgs a) {
  typedef typename OutOf<T>::t OT;
  const uint64_t step = (uint64_t)gridDim.x * kThreads;
  for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < a.total; idx += step) {
    const uint64_t q = fd_div(idx, a.nv);
    const int64_t j = (int64_t)(idx - q * a.nv.d) * VEC;
    double m[VEC], s[VEC];
    T v[VEC];
    OT ov[VEC];
    if constexpr (ROWS) {
      const int64_t row = (int64_t)q;
#pragma unroll
      for (int k = 0; k < VEC; ++k) { m[k] = mean[row]; s[k] = sd ? sd[row] : 1.0; }
      vload_nt<T, VEC>(src + row * a.sp + j, v);
      apply_vec<T, OT, VEC>(v, m, s, sd != nullptr, ov);
      store_out_nt<OT, VEC>(dst + row * a.dp + j, ov);
    } else {
      const uint64_t o = fd_div(q, a.nrc);
      const int64_t r0 = (int64_t)(q - o * a.nrc.d) * kApplyRows;
      const int64_t r1 = r0 + kApplyRows < a.R ? r0 + kApplyRows : a.R;
      const int64_t pl = (int64_t)o * a.I + j;
#pragma unroll
      for (int k = 0; k < VEC; ++k) { m[k] = mean[pl + k]; s[k] = sd ? sd[pl + k] : 1.0; }
      const int64_t e = ((int64_t)o * a.R + r0) * a.I + j;
      const T *p = src + e;
      OT *w = dst + e;
#pragma unroll 4
      for (int64_t r = r0; r < r1; ++r, p += a.I, w += a.I) {
        vload_nt<T, VEC>(p, v);
        apply_vec<T, OT, VEC>(v, m, s, sd != nullptr, ov);
        store_out_nt<OT, VEC>(w, ov);
      }
    }
  }
}

// -------------------------------------------------------------- dispatch --
// the widest vector (elements, a power of two) that every row start and both
// pointers allow: n (the vectorised extent) and both pitches in whole
// vectors, src aligned to its vector, dst to its stores of at most 16 B
int std_vec(int ies, int oes, int64_t n, int64_t sp, int64_t dp, const void *src, const void *dst) {
  return pick_vec(std::min(16 / ies, kMaxVec), {n, sp, dp}, {{src, ies}, {dst, oes}});
}

template <typename T, int VEC>
void launch_rows_v(bool block, const void *src, void *dst, RowsArgs a, hipStream_t st) {
  typedef typename OutOf<T>::t OT;
  const int rpb = block ? 1 : kThreads / 64;
  for_block_runs(cdiv(a.O, rpb), kThreads, [&](int64_t b0, int g) {
    a.row0 = b0 * rpb;
    if (block)
      k_std_rows<T, VEC, lane_vecs(VEC), kThreads / 64><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
    else
      k_std_rows<T, VEC, lane_vecs(VEC), 1><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
  });
}

template <typename T, int VEC>
void launch_apply_v(bool rows, const void *src, void *dst, const double *mean, const double *sd, ApplyArgs a,
                    hipStream_t st) {
  typedef typename OutOf<T>::t OT;
  // grid-stride: at most 2^20 blocks, each thread a few vectors on the largest arrays
  const int g = (int)std::min<int64_t>((int64_t)1 << 20, cdiv((int64_t)a.total, kThreads));
  if (rows)
    k_std_apply<T, VEC, true><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, mean, sd, a);
  else
    k_std_apply<T, VEC, false><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, mean, sd, a);
}

// the kernels of the runtime dtype (checked by check_dtypes) and vec (std_vec's)
void launch_rows(int dt, int vec, bool block, const void *src, void *dst, const RowsArgs &a, hipStream_t st) {
  for_dtype(dt, [&](auto t) {
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVec>(vec, [&](auto v) { launch_rows_v<T, decltype(v)::value>(block, src, dst, a, st); });
  });
}
void launch_apply(int dt, int vec, bool rows, const void *src, void *dst, const double *mean, const double *sd,
                  const ApplyArgs &a, hipStream_t st) {
  for_dtype(dt, [&](auto t) {
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVec>(vec, [&](auto v) {
      launch_apply_v<T, decltype(v)::value>(rows, src, dst, mean, sd, a, st);
    });
  });
}

int check_dtypes(const char *who, int in_dtype, int out_dtype) {
  if (dtype_size(in_dtype) == 0) {
    bm_set_error("%s: bad dtype %d", who, in_dtype);
    return BM_E_ARG;
  }
  if (out_dtype != stat_dtype(in_dtype)) {
    bm_set_error("%s: out_dtype %d is not the statistics dtype %d of dtype %d (float16 / float32 keep "
                 "theirs, every other dtype gives float64)", who, out_dtype, stat_dtype(in_dtype), in_dtype);
    return BM_E_ARG;
  }
  return BM_OK;
}

}  // namespace

// bm_standardize_rows behind its argument checks: the plan and the launch.
// Also bm_normalize_rows' mean baseline (bm_quantile.hip), mode 2 with `offset`.
int bm_standardize_rows_checked(const char *who, const void *src, int in_dtype, int64_t O, int64_t R,
                                int64_t src_pitch, void *dst, int out_dtype, int64_t dst_pitch, int mode,
                                double offset, int *taken, hipStream_t stream) {
  *taken = 1;
  if (O == 0 || R == 0) return BM_OK;  // nothing to write
  const int ies = dtype_size(in_dtype), oes = dtype_size(out_dtype);
  const int vec = std_vec(ies, oes, R, src_pitch, dst_pitch, src, dst);
  const int64_t held = (int64_t)vec * lane_vecs(vec);  // elements a thread holds
  const bool wave = R <= 64 * held;
  if (!wave && (R > kThreads * held || O < kBlockMinRows)) {
    *taken = 0;  // rows beyond the registers, or too few of them for a block each (see the plan above)
    return BM_OK;
  }
  RowsArgs a{};
  a.O = O; a.R = R; a.sp = src_pitch; a.dp = dst_pitch; a.scale = mode; a.offset = offset;
  launch_rows(in_dtype, vec, !wave, src, dst, a, stream);
  return check_launch(who);
}

extern "C" int bm_standardize_rows(const void *src, int in_dtype, int64_t O, int64_t R, int64_t src_pitch,
                                   void *dst, int out_dtype, int64_t dst_pitch, int scale, int *taken,
                                   void *stream) {
  const char *who = "bm_standardize_rows";
  if (!src || !dst || !taken) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_dtypes(who, in_dtype, out_dtype);
  if (rc) return rc;
  if (scale != 0 && scale != 1) { bm_set_error("%s: scale %d is not 0 or 1", who, scale); return BM_E_ARG; }
  if (O < 0 || R < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld)", who, (long long)O, (long long)R);
    return BM_E_ARG;
  }
  if (src_pitch < R || dst_pitch < R) {
    bm_set_error("%s: pitch below the row length (src_pitch=%lld dst_pitch=%lld R=%lld)", who,
                 (long long)src_pitch, (long long)dst_pitch, (long long)R);
    return BM_E_ARG;
  }
  return bm_standardize_rows_checked(who, src, in_dtype, O, R, src_pitch, dst, out_dtype, dst_pitch, scale, 0.0, taken,
                                     (hipStream_t)stream);
}

extern "C" int bm_standardize_apply(const void *src, int in_dtype, int64_t O, int64_t R, int64_t I,
                                    int64_t src_pitch, const double *mean, const double *std, void *dst,
                                    int out_dtype, int64_t dst_pitch, void *stream) {
  const char *who = "bm_standardize_apply";
  if (!src || !dst || !mean) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_dtypes(who, in_dtype, out_dtype);
  if (rc) return rc;
  if (O < 0 || R < 0 || I < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld I=%lld)", who, (long long)O, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  if (src_pitch < R || dst_pitch < R || (I > 1 && (src_pitch != R || dst_pitch != R))) {
    bm_set_error("%s: pitches %lld / %lld do not fit R=%lld, I=%lld (>= R, and R itself unless I == 1)", who,
                 (long long)src_pitch, (long long)dst_pitch, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  if (O == 0 || R == 0 || I == 0) return BM_OK;  // nothing to write
  const int ies = dtype_size(in_dtype), oes = dtype_size(out_dtype);
  const bool rows = I == 1;
  const int vec = rows ? std_vec(ies, oes, R, src_pitch, dst_pitch, src, dst) : std_vec(ies, oes, I, 0, 0, src, dst);
  ApplyArgs a{};
  a.R = R; a.I = I; a.sp = src_pitch; a.dp = dst_pitch;
  const int64_t nv = (rows ? R : I) / vec;
  const int64_t nrc = cdiv(R, kApplyRows);
  a.nv = make_fastdiv((uint64_t)nv);
  a.nrc = make_fastdiv((uint64_t)nrc);
  a.total = (uint64_t)(rows ? O : O * nrc) * (uint64_t)nv;
  launch_apply(in_dtype, vec, rows, src, dst, mean, std, a, (hipStream_t)stream);
  return check_launch(who);
}

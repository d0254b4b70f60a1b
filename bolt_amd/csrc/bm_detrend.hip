// bm_detrend.hip -- detrend of libbolt_mi355x (gfx950): every record minus its
// least-squares polynomial of degree `order` along an axis.
//
// No reference call site: the reference has no such method (an API addition,
// like center / zscore); thunder's Series.detrend does the step per record
// with a polyfit on the host.
//
// The result has the array's shape, so the floor is one read and one write.
//   rows kernel (the reduced axis is the last one, rows dense or padded):
//     k_std_rows' structure (bm_standardize.hip) -- the row is loaded once into
//     registers, one wave per row or the four waves of a block for longer
//     rows, its mean and its co-moments with the basis are taken from the
//     registers, and the held values are detrended and stored: one read, one
//     write.
//   apply kernel (every other layout, and rows too long to hold): elementwise
//     over [O][R][I] with the float64 mean / coefficient planes of a
//     bm_comoment_state that ran before it and the basis table: one more read
//     per batch of signals, and one write.
// Numerics (all float64): no Vandermonde matrix is formed.  The basis is the
//   discrete orthonormal (Gram) polynomials on the record's n positions,
//   t_r = r - (n-1)/2, b_k = (k/2) sqrt((n-k)(n+k) / (4k^2-1)):
//     p_0 = 1/sqrt(n), p_1 = t p_0 / b_1, p_{k+1} = (t p_k - b_k p_{k-1}) / b_{k+1};
//   the entry point forms b_k and 1/b_k on the host and the kernel multiplies
//   by the reciprocal.  mean = P + sum(x - P) / n around the row's first
//   element P as k_std_rows forms it, d = x - mean, C_k = sum d p_k(t_r) for
//   k = 1..order -- lanes add in register order and fold through DPP in lane
//   order (wave_fold), waves through LDS in wave order: deterministic -- and
//   y_r = d_r - sum_k C_k p_k(t_r), k ascending, rounded once to the output
//   dtype.  Projecting d, not x, keeps the digits of data with a large offset.
//   A constant row gives exact zeros (d is x - x); a nan or an infinity in a
//   row reaches its co-moments and so every output of the row.
#include "bm_common.h"
#include "bm_host.h"
#include "bm_wave.h"
#include "../../include/bolt_mi355x.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxOrder = BM_DETREND_MAX_ORDER;
// Plan of bm_detrend_rows: bm_standardize_rows' (pick_vec, lane_vecs,
// kBlockMinRows), set from the register budget.  MEASURED at C2's shape only
// (float32 (512, 512, 2000) at a pitch of 2048, wave per row;
// profiles/detrend_ab.log, medians of 9 interleaved rounds): orders 1 / 3 / 5 /
// 8 run 0.722 / 0.933 / 1.470 / 2.118 ms against 1.113 / 1.831 / 2.658 / 3.458
// ms of the two-pass path on the same rows, the spreads below 0.1 ms, so every
// order is taken; zscore of the same buffer 0.698 ms, a copy 0.685 ms.  The
// block-per-row limit and kBlockMinRows are UNMEASURED.
//   a thread holds lane_vecs(vec) = min(8, 32 / vec) vectors, min(8 * vec, 32)
//   elements; wave per row: rows up to 64 * that (2048 float32 at 16-B
//   vectors, which covers C2's 2000); block per row: rows up to 256 * that with
//   at least kBlockMinRows rows; everything else is not taken (*taken = 0: the
//   caller's co-moment state and bm_detrend_apply).
constexpr int lane_vecs(int vec) { return vec * 8 <= 32 ? 8 : 32 / vec; }
constexpr int64_t kBlockMinRows = 256;
constexpr int kMaxVec = 8;       // rows: elements per vector at most, as bm_standardize_rows
constexpr int kMaxVecApply = 4;  // apply: a thread of the column kernel holds order x vec coefficients

// the recurrence's constants, uniform over the launch (scalar registers)
struct Basis {
  double half;             // (n - 1) / 2
  double p0;               // 1 / sqrt(n)
  double b[kMaxOrder + 1];   // b_k, k = 1..order (b[0] unused)
  double rb[kMaxOrder + 1];  // 1 / b_k
};

struct RowsArgs {
  int64_t O, R;
  int64_t sp, dp;  // elements between row starts of src / dst (>= R)
  int64_t row0;    // first row of this launch (launches split at the grid limit)
  int32_t order;
  Basis g;
};

// p_1(t).  The following values come from next_p: (p_{k-1}, p_k) -> p_{k+1}.
__device__ __forceinline__ double first_p(const Basis &g, double t) { return t * g.p0 * g.rb[1]; }
__device__ __forceinline__ double next_p(const Basis &g, int k, double t, double pk, double pm) {
  return (t * pk - g.b[k] * pm) * g.rb[k + 1];
}

// WPR waves per row (1, or the block's 4), each thread holding NV vectors of
// VEC elements: R <= 64 * WPR * VEC * NV (the host's plan), R % VEC == 0.
// The co-moments C[] are indexed by unrolled loops only (a uniform k <= order
// guard ends them), so they stay in registers: no instantiation uses scratch
// (-Rpass-analysis=kernel-resource-usage: 0 bytes a lane in all 66).  VGPRs,
// wave per row / block per row: float32 and every other type at vec 4
// 138 / 178 (3 / 2 waves a SIMD; k_std_rows takes 104), vec 8 130 / 178, vec 2
// 104-106 / 120 (4 waves), vec 1 86 / 86 (5).  The eight co-moments and the
// recurrence's temporaries are what the kernel holds on top of k_std_rows.
template <typename T, int VEC, int NV, int WPR>
__global__ void __launch_bounds__(kThreads)
    k_detrend_rows(const T *__restrict__ src, typename OutOf<T>::t *__restrict__ dst, RowsArgs a) {
  typedef typename OutOf<T>::t OT;
  __shared__ double sm[WPR];
  __shared__ double smc[kMaxOrder][WPR];
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
  const int order = a.order;

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

  // C_k = sum d p_k(t): every lane walks the recurrence over its held positions
  double C[kMaxOrder];
#pragma unroll
  for (int q = 0; q < kMaxOrder; ++q) C[q] = 0.0;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const bool in = j0 + u * stride < a.R;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const double d = in ? to_f64(v[u][k]) - mean : 0.0;
      const double t = (double)(j0 + u * stride + k) - a.g.half;
      double pm = a.g.p0, pk = first_p(a.g, t);
      C[0] = fma(d, pk, C[0]);
#pragma unroll
      for (int q = 1; q < kMaxOrder; ++q) {
        if (q >= order) break;
        const double pn = next_p(a.g, q, t, pk, pm);
        pm = pk;
        pk = pn;
        C[q] = fma(d, pk, C[q]);
      }
    }
  }
  // lanes in lane order, then the row's waves in wave order through LDS
#pragma unroll
  for (int q = 0; q < kMaxOrder; ++q) {
    if (q >= order) break;
    C[q] = wave_fold(C[q], lane, [](double x, double y) { return x + y; });
    if constexpr (WPR == 1) {
      C[q] = lane_of<kFoldLane>(C[q]);
    } else {
      if (lane == kFoldLane) smc[q][wave] = C[q];
    }
  }
  if constexpr (WPR > 1) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxOrder; ++q) {
      if (q >= order) break;
      double t = smc[q][0];
#pragma unroll
      for (int w = 1; w < WPR; ++w) t += smc[q][w];
      C[q] = t;
    }
  }

  // the one write
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    if (j0 + u * stride < a.R) {
      OT ov[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double d = to_f64(v[u][k]) - mean;
        const double t = (double)(j0 + u * stride + k) - a.g.half;
        double pm = a.g.p0, pk = first_p(a.g, t);
        double fit = C[0] * pk;
#pragma unroll
        for (int q = 1; q < kMaxOrder; ++q) {
          if (q >= order) break;
          const double pn = next_p(a.g, q, t, pk, pm);
          pm = pk;
          pk = pn;
          fit = fma(C[q], pk, fit);
        }
        ov[k] = (OT)(d - fit);
      }
      store_out_nt<OT, VEC>(o + j0 + u * stride, ov);
    }
  }
}

// ----------------------------------------------------------------- apply --
// rows of one column vector a thread of the column kernel takes with the
// vector's mean and coefficients held in registers (k_std_apply's kApplyRows;
// UNMEASURED here)
constexpr int kApplyRows = 16;

struct ApplyArgs {
  int64_t R, I;
  int64_t sp, dp;   // ROWS: elements between row starts of src / dst
  int64_t plane;    // O * I: values per mean / coefficient plane
  int32_t order;
  FastDiv nv;       // vectors per row (ROWS: R / VEC, else I / VEC)
  FastDiv nrc;      // columns: chunks of kApplyRows rows per o
  uint64_t total;   // work items: vectors (ROWS), (o, row chunk, column vector) (columns)
};

// ROWS (I == 1): vectors along R, one mean and `order` coefficients per row o,
// the basis at the vector's positions.  Columns (I > 1): vectors along I, mean
// and coefficients at [o * I + i] held over kApplyRows rows, one basis value
// per row and k.  Planes and basis are read through the cache (neighbouring
// work items read the same values), the array streams.
template <typename T, int VEC, bool ROWS>
__global__ void __launch_bounds__(kThreads)
    k_detrend_apply(const T *__restrict__ src, typename OutOf<T>::t *__restrict__ dst,
                    const double *__restrict__ mean, const double *__restrict__ coef,
                    const double *__restrict__ basis, ApplyArgs a) {
  typedef typename OutOf<T>::t OT;
  const int order = a.order;
  const uint64_t step = (uint64_t)gridDim.x * kThreads;
  for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < a.total; idx += step) {
    const uint64_t q = fd_div(idx, a.nv);
    const int64_t j = (int64_t)(idx - q * a.nv.d) * VEC;
    T v[VEC];
    OT ov[VEC];
    if constexpr (ROWS) {
      const int64_t row = (int64_t)q;
      const double m = mean[row];
      double fit[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) fit[e] = 0.0;
#pragma unroll
      for (int k = 0; k < kMaxOrder; ++k) {
        if (k >= order) break;
        const double c = coef[k * a.plane + row];
        const double *b = basis + k * a.R + j;
#pragma unroll
        for (int e = 0; e < VEC; ++e) fit[e] = fma(c, b[e], fit[e]);
      }
      vload_nt<T, VEC>(src + row * a.sp + j, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) ov[e] = (OT)((to_f64(v[e]) - m) - fit[e]);
      store_out_nt<OT, VEC>(dst + row * a.dp + j, ov);
    } else {
      const uint64_t o = fd_div(q, a.nrc);
      const int64_t r0 = (int64_t)(q - o * a.nrc.d) * kApplyRows;
      const int64_t r1 = r0 + kApplyRows < a.R ? r0 + kApplyRows : a.R;
      const int64_t pl = (int64_t)o * a.I + j;
      double m[VEC], c[kMaxOrder][VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[e] = mean[pl + e];
#pragma unroll
      for (int k = 0; k < kMaxOrder; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) c[k][e] = k < order ? coef[k * a.plane + pl + e] : 0.0;
      }
      const int64_t e0 = ((int64_t)o * a.R + r0) * a.I + j;
      const T *p = src + e0;
      OT *w = dst + e0;
      for (int64_t r = r0; r < r1; ++r, p += a.I, w += a.I) {
        vload_nt<T, VEC>(p, v);
        double fit[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) fit[e] = 0.0;
#pragma unroll
        for (int k = 0; k < kMaxOrder; ++k) {
          if (k >= order) break;
          const double b = basis[k * a.R + r];
#pragma unroll
          for (int e = 0; e < VEC; ++e) fit[e] = fma(c[k][e], b, fit[e]);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) ov[e] = (OT)((to_f64(v[e]) - m[e]) - fit[e]);
        store_out_nt<OT, VEC>(w, ov);
      }
    }
  }
}

// -------------------------------------------------------------- dispatch --
// the widest vector (elements, a power of two <= cap) that every row start and
// both pointers allow (bm_standardize.hip's std_vec)
int det_vec(int cap, int ies, int oes, int64_t n, int64_t sp, int64_t dp, const void *src, const void *dst) {
  return pick_vec(std::min(16 / ies, cap), {n, sp, dp}, {{src, ies}, {dst, oes}});
}

template <typename T, int VEC>
void launch_rows_v(bool block, const void *src, void *dst, RowsArgs a, hipStream_t st) {
  typedef typename OutOf<T>::t OT;
  const int rpb = block ? 1 : kThreads / 64;
  for_block_runs(cdiv(a.O, rpb), kThreads, [&](int64_t b0, int g) {
    a.row0 = b0 * rpb;
    if (block)
      k_detrend_rows<T, VEC, lane_vecs(VEC), kThreads / 64><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
    else
      k_detrend_rows<T, VEC, lane_vecs(VEC), 1><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
  });
}

template <typename T, int VEC>
void launch_apply_v(bool rows, const void *src, void *dst, const double *mean, const double *coef,
                    const double *basis, ApplyArgs a, hipStream_t st) {
  typedef typename OutOf<T>::t OT;
  // grid-stride: at most 2^20 blocks, each thread a few vectors on the largest arrays
  const int g = (int)std::min<int64_t>((int64_t)1 << 20, cdiv((int64_t)a.total, kThreads));
  if (rows)
    k_detrend_apply<T, VEC, true><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, mean, coef, basis, a);
  else
    k_detrend_apply<T, VEC, false><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, mean, coef, basis, a);
}

int check_common(const char *who, int in_dtype, int out_dtype, int order) {
  if (dtype_size(in_dtype) == 0) {
    bm_set_error("%s: bad dtype %d", who, in_dtype);
    return BM_E_ARG;
  }
  if (out_dtype != stat_dtype(in_dtype)) {
    bm_set_error("%s: out_dtype %d is not the statistics dtype %d of dtype %d (float16 / float32 keep "
                 "theirs, every other dtype gives float64)", who, out_dtype, stat_dtype(in_dtype), in_dtype);
    return BM_E_ARG;
  }
  if (order < 1 || order > kMaxOrder) {
    bm_set_error("%s: order %d is outside 1..%d", who, order, kMaxOrder);
    return BM_E_ARG;
  }
  return BM_OK;
}

int check_order_fits(const char *who, int order, int64_t R) {
  if (R > 0 && order >= R) {
    bm_set_error("%s: order %d needs more than %lld positions (order < R)", who, order, (long long)R);
    return BM_E_ARG;
  }
  return BM_OK;
}

}  // namespace

extern "C" int bm_detrend_rows(const void *src, int in_dtype, int64_t O, int64_t R, int64_t src_pitch, int order,
                               void *dst, int out_dtype, int64_t dst_pitch, int *taken, void *stream) {
  const char *who = "bm_detrend_rows";
  if (!src || !dst || !taken) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_common(who, in_dtype, out_dtype, order);
  if (rc) return rc;
  if (O < 0 || R < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld)", who, (long long)O, (long long)R);
    return BM_E_ARG;
  }
  if (src_pitch < R || dst_pitch < R) {
    bm_set_error("%s: pitch below the row length (src_pitch=%lld dst_pitch=%lld R=%lld)", who,
                 (long long)src_pitch, (long long)dst_pitch, (long long)R);
    return BM_E_ARG;
  }
  rc = check_order_fits(who, order, R);
  if (rc) return rc;
  *taken = 1;
  if (O == 0 || R == 0) return BM_OK;  // nothing to write
  const int ies = dtype_size(in_dtype), oes = dtype_size(out_dtype);
  const int vec = det_vec(kMaxVec, ies, oes, R, src_pitch, dst_pitch, src, dst);
  const int64_t held = (int64_t)vec * lane_vecs(vec);  // elements a thread holds
  const bool wave = R <= 64 * held;
  if (!wave && (R > kThreads * held || O < kBlockMinRows)) {
    *taken = 0;  // rows beyond the registers, or too few of them for a block each (see the plan above)
    return BM_OK;
  }
  RowsArgs a{};
  a.O = O; a.R = R; a.sp = src_pitch; a.dp = dst_pitch; a.order = order;
  const double n = (double)R;
  a.g.half = (n - 1.0) / 2.0;
  a.g.p0 = 1.0 / std::sqrt(n);
  for (int k = 1; k <= kMaxOrder; ++k) {
    // (beyond the order the values are not used; they stay finite)
    const double kk = (double)k;
    const double bk = k <= order ? kk / 2.0 * std::sqrt((n - kk) * (n + kk) / (4.0 * kk * kk - 1.0)) : 1.0;
    a.g.b[k] = bk;
    a.g.rb[k] = 1.0 / bk;
  }
  a.g.b[0] = a.g.rb[0] = 0.0;
  for_dtype(in_dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVec>(vec, [&](auto v) {
      launch_rows_v<T, decltype(v)::value>(!wave, src, dst, a, (hipStream_t)stream);
    });
  });
  return check_launch(who);
}

extern "C" int bm_detrend_apply(const void *src, int in_dtype, int64_t O, int64_t R, int64_t I, int64_t src_pitch,
                                const double *mean, const double *coef, const double *basis, int order, void *dst,
                                int out_dtype, int64_t dst_pitch, void *stream) {
  const char *who = "bm_detrend_apply";
  if (!src || !dst || !mean || !coef || !basis) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_common(who, in_dtype, out_dtype, order);
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
  // (order >= R is not refused here: the basis is the caller's table, and a rank's slab of a record
  // that is spread over ranks may hold fewer positions than the fit has terms)
  if (O == 0 || R == 0 || I == 0) return BM_OK;  // nothing to write
  const int ies = dtype_size(in_dtype), oes = dtype_size(out_dtype);
  const bool rows = I == 1;
  const int vec = rows ? det_vec(kMaxVecApply, ies, oes, R, src_pitch, dst_pitch, src, dst)
                       : det_vec(kMaxVecApply, ies, oes, I, 0, 0, src, dst);
  ApplyArgs a{};
  a.R = R; a.I = I; a.sp = src_pitch; a.dp = dst_pitch; a.plane = O * I; a.order = order;
  const int64_t nv = (rows ? R : I) / vec;
  const int64_t nrc = cdiv(R, kApplyRows);
  a.nv = make_fastdiv((uint64_t)nv);
  a.nrc = make_fastdiv((uint64_t)nrc);
  a.total = (uint64_t)(rows ? O : O * nrc) * (uint64_t)nv;
  for_dtype(in_dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVecApply>(vec, [&](auto v) {
      launch_apply_v<T, decltype(v)::value>(rows, src, dst, mean, coef, basis, a, (hipStream_t)stream);
    });
  });
  return check_launch(who);
}

// bm_reduce.hip -- sum / mean / var / std reductions of libbolt_mi355x (gfx950).
//
// Replaces the Spark path's per-partition StatCounter (bolt/spark/
// statcounter.py:38-59, driven by array.py:321-322), its treeReduce of
// StatCounter.combine (statcounter.py:67-99, array.py:323) and the
// treeReduce(add) of reduce/sum (array.py:243-282).
//
// Layout: a C-contiguous array viewed as [O][R][I]; R is reduced.
//   cols kernel (I > 1): lanes own VEC adjacent columns, 16-B loads along I,
//     row phases stride R; phases are Chan-combined through LDS.
//   rows kernel (I == 1): one wave per (row, chunk), 16-B loads along R,
//     lane states folded across the 64 lanes through DPP moves (wave_fold).
//   Long R is split into chunks over blocks (enough waves to fill 256 CUs);
//   chunk states go to a workspace and a combine kernel merges them in chunk
//   order (deterministic) and finalises.
// Numerics (all float64):
//   var / std: batched Welford.  Each lane reduces the B values of one load
//     batch (B = vectors in flight x vector width, 1..32) around a pivot that
//     is one of those values, so the batch's M2 = S2 - S1^2/B carries at most
//     O(B eps) relative error whatever the data's offset or outliers; the
//     batch state (B, mean_b, M2_b) is then merged into the lane's running
//     (n, mean, M2) by Chan's formula (statcounter.py:85-96), as are lanes,
//     row phases, chunks and ranks, always in a fixed order (deterministic).
//   mean: pivot-shifted sums around the (row, chunk)'s first element,
//     mean = K + S1/n (no cancellation: the error is eps-relative to max|x|).
//   Pivots are finite: a first element that is an infinity or a NaN takes 0
//     (finite_or_zero), so a row with such a value has the mean a sum over it
//     gives (numpy's: inf, -inf, or NaN for inf - inf or a NaN) wherever the
//     value sits, and NaN var / std (m2_out).  Welford and Chan means that come
//     out NaN are recomputed as sums, on that path only.  (Overflow of x - K
//     for finite values near +-1.8e308 is not handled.)
//   SUM over floats is a float64 sum; over integers a uint64 modular sum
//   truncated to the input width; over bool an OR.
// All are HBM-bound: algorithmic bytes = N*elem_bytes + nout*out_bytes.
#include "bm_common.h"
#include "bm_host.h"
#include "bm_wave.h"
#include "../../include/bolt_mi355x.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
// Shipped parameters (the A/B runs that chose them are cited; the rejected
// values live in git history and tools/microbench/):
// rows in flight per lane in the column reductions: 8 over 4 +1.2-1.4% on the
// 64 GiB target mean / std and C2-shape columns, 2 -4-8% (profiles/r02_ab_cols.log);
// on round 6's 64-vector tiles 16 is within +0.2..+1.4% of 8 (two placements,
// profiles/r06l_ab_cols_unroll.log): 8 stays (half the load registers)
constexpr int kColsUnroll = 8;
// split R over blocks below this many column tiles; column vectors per block
// at most (the rest of the 256 lanes are row phases); the narrowest tile taken
// to reach kColsBlocks before chunking R (profiles/r03zb_ab_tcv.log, r03zc_ab_tcv_rule.log).
// Round 6: 64-vector tiles (four row phases per block) for every shape, not
// only the few-tile ones: the 64 GiB target's mean / std over axis 0
// +0.8..+1.8% on two placements, 128-vector tiles +0.7..+1.7%, C2 / C4
// columns +-0.3% (profiles/r06j_ab_cols_tiles.log, r06k_ab_cols_tiles.log; the
// column kernels had 4x the rows kernel's DRAM read-credit stalls per byte,
// r06i_cols_vs_rows_counters.md); 32 B per lane lost 6-12%
constexpr int64_t kColsBlocks = 2048;
constexpr int64_t kColsTcv = 64;
constexpr int64_t kColsTcvMin = 64;
// 16-B vectors in flight per lane in the rows kernel: 2 beats 4 by 4%, 8 by 25%
// (profiles/r01_ab1.log; 3: equal, 4: -5% again on padded rows, r05z_rows_unroll.txt)
constexpr int kRowsUnroll = 2;
// exact-integer column var: rows in flight per lane (C4 var 3.76 -> 3.47 ms over 4, profiles/r02_ab_int.log)
constexpr int kIntUnroll = 8;
// rows kernel: blocks dealt to one XCD take consecutive rows (C2 mean / std
// +3-4%, profiles/r02_ab_redxcd.log); column kernels: blocks dealt to one XCD
// take consecutive column tiles (C4 var +1.1%, 64 GiB-target-shaped mean / std
// over axis 0 +2.2% / +1.6%, profiles/r05h_ab_cols_xcd.log)

enum Mode {
  M_MEAN = 0, M_MOM = 1, M_FSUM = 2, M_ISUM = 3, M_OR = 4, M_MAX = 5, M_MIN = 6,
  M_FPROD = 7, M_IPROD = 8, M_LAND = 9, M_BAND = 10, M_BOR = 11, M_BXOR = 12, M_FMAX = 13, M_FMIN = 14,
  // mean into `out` and the var / std state into the kept planes from one read
  // (bm_reduce_keep): M_MEAN's and M_MOM's accumulations side by side on the
  // same loaded registers, each with its own arithmetic and order
  M_MEANMOM = 15
};
template <int MODE> constexpr bool mean_part() { return MODE == M_MEAN || MODE == M_MEANMOM; }
template <int MODE> constexpr bool mom_part() { return MODE == M_MOM || MODE == M_MEANMOM; }

// "bit modes" keep a uint64 accumulator: modular integer sum / product,
// logical OR (bool sum, logical_or) / AND, bitwise and / or / xor, and
// max / min / fmax / fmin holding the element's own bits (typed compares).
template <int MODE> constexpr bool bit_mode() {
  return MODE == M_ISUM || MODE == M_OR || MODE == M_MAX || MODE == M_MIN || MODE == M_IPROD ||
         MODE == M_LAND || MODE == M_BAND || MODE == M_BOR || MODE == M_BXOR || MODE == M_FMAX ||
         MODE == M_FMIN;
}
// float-accumulating modes: a float64 sum or product
template <int MODE> constexpr bool facc_mode() { return MODE == M_FSUM || MODE == M_FPROD; }
template <int MODE> __device__ __forceinline__ double fident() { return MODE == M_FPROD ? 1.0 : 0.0; }
template <int MODE> __device__ __forceinline__ double fop(double a, double b) {
  return MODE == M_FPROD ? a * b : a + b;
}
// modes meaningless for floating inputs (numpy raises for bitwise ufuncs)
template <int MODE> constexpr bool int_only_mode() {
  return MODE == M_ISUM || MODE == M_IPROD || MODE == M_BAND || MODE == M_BOR || MODE == M_BXOR;
}

template <typename T> __device__ __forceinline__ uint64_t to_u64(T x) {
  return (uint64_t)(int64_t)x;  // sign-extends signed types: modular sums stay exact
}
template <> __device__ __forceinline__ uint64_t to_u64<uint64_t>(uint64_t x) { return x; }
template <> __device__ __forceinline__ uint64_t to_u64<uint8_t>(uint8_t x) { return x; }
template <> __device__ __forceinline__ uint64_t to_u64<uint16_t>(uint16_t x) { return x; }
template <> __device__ __forceinline__ uint64_t to_u64<uint32_t>(uint32_t x) { return x; }

template <typename T> __device__ __forceinline__ uint64_t bits_of(T x) {
  uint64_t u = 0;
  __builtin_memcpy(&u, &x, sizeof(T));
  return u;
}
template <typename T> __device__ __forceinline__ T from_bits(uint64_t u) {
  T x;
  __builtin_memcpy(&x, &u, sizeof(T));
  return x;
}
template <typename T> __device__ __forceinline__ bool is_nan(T x) { return x != x; }

// numpy.maximum / numpy.minimum: a NaN operand wins (NaNs propagate)
template <typename T, bool MAX> __device__ __forceinline__ T pick(T a, T b) {
  if (is_nan(a)) return a;
  if (is_nan(b)) return b;
  return MAX ? (b > a ? b : a) : (b < a ? b : a);
}
// numpy.fmax / numpy.fmin: a NaN operand loses (NaN only if both are NaN)
template <typename T, bool MAX> __device__ __forceinline__ T pickf(T a, T b) {
  if (is_nan(a)) return b;
  if (is_nan(b)) return a;
  return MAX ? (b > a ? b : a) : (b < a ? b : a);
}
template <typename T> __device__ __forceinline__ T qnan() { return T(0); }
template <> __device__ __forceinline__ _Float16 qnan<_Float16>() { return (_Float16)__builtin_nanf(""); }
template <> __device__ __forceinline__ float qnan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double qnan<double>() { return __builtin_nan(""); }
template <typename T> constexpr bool is_float_t() {
  return std::is_same<T, _Float16>::value || std::is_same<T, float>::value || std::is_same<T, double>::value;
}

template <typename T> struct Lim;
template <> struct Lim<uint8_t> { static __device__ uint8_t lo() { return 0; } static __device__ uint8_t hi() { return 0xff; } };
template <> struct Lim<int8_t> { static __device__ int8_t lo() { return -128; } static __device__ int8_t hi() { return 127; } };
template <> struct Lim<uint16_t> { static __device__ uint16_t lo() { return 0; } static __device__ uint16_t hi() { return 0xffff; } };
template <> struct Lim<int16_t> { static __device__ int16_t lo() { return -32768; } static __device__ int16_t hi() { return 32767; } };
template <> struct Lim<uint32_t> { static __device__ uint32_t lo() { return 0; } static __device__ uint32_t hi() { return 0xffffffffu; } };
template <> struct Lim<int32_t> { static __device__ int32_t lo() { return (-2147483647 - 1); } static __device__ int32_t hi() { return 2147483647; } };
template <> struct Lim<uint64_t> { static __device__ uint64_t lo() { return 0; } static __device__ uint64_t hi() { return ~0ull; } };
template <> struct Lim<int64_t> { static __device__ int64_t lo() { return (-9223372036854775807ll - 1); } static __device__ int64_t hi() { return 9223372036854775807ll; } };
template <> struct Lim<_Float16> { static __device__ _Float16 lo() { return -__builtin_inff16(); } static __device__ _Float16 hi() { return __builtin_inff16(); } };
template <> struct Lim<float> { static __device__ float lo() { return -__builtin_inff(); } static __device__ float hi() { return __builtin_inff(); } };
template <> struct Lim<double> { static __device__ double lo() { return -__builtin_inf(); } static __device__ double hi() { return __builtin_inf(); } };

// identity, element conversion and combination of the bit modes
template <typename T, int MODE> __device__ __forceinline__ uint64_t bident() {
  if (MODE == M_MAX) return bits_of<T>(Lim<T>::lo());
  if (MODE == M_MIN) return bits_of<T>(Lim<T>::hi());
  // fmax / fmin: NaN is the identity of floats (all-NaN -> NaN)
  if (MODE == M_FMAX) return bits_of<T>(is_float_t<T>() ? qnan<T>() : Lim<T>::lo());
  if (MODE == M_FMIN) return bits_of<T>(is_float_t<T>() ? qnan<T>() : Lim<T>::hi());
  if (MODE == M_IPROD || MODE == M_LAND) return 1;
  if (MODE == M_BAND) return ~0ull;
  return 0;
}
template <typename T, int MODE> __device__ __forceinline__ uint64_t belem(T x) {
  if (MODE == M_ISUM || MODE == M_IPROD) return to_u64(x);
  if (MODE == M_OR || MODE == M_LAND) return (uint64_t)(x != 0);
  return bits_of<T>(x);
}
template <typename T, int MODE> __device__ __forceinline__ uint64_t bop(uint64_t a, uint64_t b) {
  if (MODE == M_ISUM) return a + b;
  if (MODE == M_IPROD) return a * b;  // modular: the low bits depend only on the low bits
  if (MODE == M_OR || MODE == M_BOR) return a | b;
  if (MODE == M_LAND || MODE == M_BAND) return a & b;
  if (MODE == M_BXOR) return a ^ b;
  if (MODE == M_FMAX || MODE == M_FMIN)
    return bits_of<T>(pickf<T, MODE == M_FMAX>(from_bits<T>(a), from_bits<T>(b)));
  return bits_of<T>(pick<T, MODE == M_MAX>(from_bits<T>(a), from_bits<T>(b)));
}

// Per-lane accumulator for one output column.
template <int MODE> struct Acc;

template <> struct Acc<M_MEAN> {
  // two interleaved partial sums share the pivot: halves the add chain
  double K, S1, S1b;
  int64_t n;
  __device__ void init() { K = 0; S1 = 0; S1b = 0; n = 0; }
  __device__ void first(double x) { K = x; S1 = 0; S1b = 0; n = 1; }
  __device__ void pivot(double k) { K = k; S1 = 0; S1b = 0; n = 0; }
  __device__ double s1() const { return S1 + S1b; }
  __device__ double s2() const { return 0.0; }
  __device__ void add(double x) { S1 += x - K; ++n; }
  __device__ void add2(double x, double y) { S1 += x - K; S1b += y - K; n += 2; }
  __device__ double mean() const { return n ? K + (S1 + S1b) / (double)n : 0.0; }
  __device__ double m2() const { return 0.0; }
};

// (n, K, S1) of pivot-shifted sums -> mean
__device__ __forceinline__ double mean_from_sums(double n, double K, double s1) {
  return n > 0.0 ? K + s1 / n : 0.0;
}

// Batch moments of B values around the pivot K = x[0] (one of the values, so
// S2 <= (1 + B) M2_b and the subtraction loses at most log2(B+1) bits),
// returned in the frame shifted by the row's pivot P: mb = mean_b - P.
// K - P is exact for values within a factor of two of P (offset data) and
// otherwise rounds once, at the data's own scale.
template <int B>
__device__ __forceinline__ void batch_moments(const double (&x)[B], double P, double &mb, double &qb) {
  const double K = x[0];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = 1; i < B; ++i) {
    const double d = x[i] - K;
    s1 += d;
    s2 = fma(d, d, s2);
  }
  constexpr double inv = 1.0 / (double)B;  // B is a power of two: exact
  mb = fma(s1, inv, K - P);
  const double q = fma(-s1, s1 * inv, s2);
  qb = q > 0.0 ? q : 0.0;
}

// Chan merge of a batch (nb values, mean mb, M2 qb) into (mean, m2) holding
// na values, with f = nb / (na + nb) and nf = na * f precomputed by the caller
// (shared by the VEC columns of a lane).  na == 0 gives f = 1, nf = 0: the
// batch is taken as is.
__device__ __forceinline__ void merge_batch(double &mean, double &m2, double mb, double qb, double f,
                                            double nf) {
  const double delta = mb - mean;
  mean = fma(delta, f, mean);
  m2 = m2 + qb + delta * delta * nf;
}

__device__ __forceinline__ void batch_weights(double na, double nb, double &f, double &nf) {
  if (na == nb) {
    f = 0.5;  // equal halves (the butterfly and phase trees): no division
  } else {
    f = nb / (na + nb);
  }
  nf = na * f;
}

// 1/k for the k-th equal batch of a lane's main loop: f = B / ((k+1) B) =
// 1/(k+1), the same correctly rounded value the division gives, from a table.
constexpr int kInvN = 512;
struct InvTab {
  double v[kInvN];
  constexpr InvTab() : v() {
    for (int i = 1; i < kInvN; ++i) v[i] = 1.0 / (double)i;
  }
};
__device__ constexpr InvTab kInvTab{};

__device__ __forceinline__ void uniform_weights(int64_t kb, double B, double &f, double &nf) {
  f = kb + 1 < kInvN ? kInvTab.v[kb + 1] : 1.0 / (double)(kb + 1);
  nf = ((double)kb * B) * f;
}

// Running Welford state of one output (rows kernel), in the frame shifted by
// the row's pivot P.
struct Wel {
  double n, mean, m2;
  int64_t kb;  // equal main-loop batches merged so far
  __device__ void init() { n = 0.0; mean = 0.0; m2 = 0.0; kb = 0; }
  template <int B> __device__ void add_main(const double (&x)[B], double P) {
    double mb, qb, f, nf;
    batch_moments<B>(x, P, mb, qb);
    uniform_weights(kb, (double)B, f, nf);
    merge_batch(mean, m2, mb, qb, f, nf);
    ++kb;
    n += (double)B;
  }
  template <int B> __device__ void add_batch(const double (&x)[B], double P) {
    double mb, qb, f, nf;
    batch_moments<B>(x, P, mb, qb);
    batch_weights(n, (double)B, f, nf);
    merge_batch(mean, m2, mb, qb, f, nf);
    n += (double)B;
  }
  __device__ void add1(double y) {  // Welford's own update (statcounter.py:51-59), y = x - P
    n += 1.0;
    const double delta = y - mean;
    mean += delta / n;
    m2 = fma(delta, y - mean, m2);
  }
};

// Chan et al. pairwise combination of (n, mean, M2) -- statcounter.py:85-96
// in its exact form (no 10x heuristic needed in float64).
__device__ __forceinline__ void chan(double &na, double &ma, double &qa, double nb, double mb,
                                     double qb, bool need_m2) {
  if (nb == 0.0) return;
  if (na == 0.0) {
    na = nb; ma = mb; qa = qb;
    return;
  }
  const double n = na + nb;
  const double delta = mb - ma;
  double f;
  if (na == nb) {
    f = 0.5;
  } else {
    f = nb / n;
  }
  ma = fma(delta, f, ma);
  if (need_m2) qa = qa + qb + delta * delta * (na * f);
  na = n;
}

__device__ __forceinline__ void store_out(void *out, int64_t idx, double v, int dt) {
  switch (dt) {
    case BM_F16: ((_Float16 *)out)[idx] = (_Float16)v; break;
    case BM_F32: ((float *)out)[idx] = (float)v; break;
    default: ((double *)out)[idx] = v; break;
  }
}

__device__ __forceinline__ void store_int(void *out, int64_t idx, uint64_t v, int dt) {
  switch (dt) {  // the low bytes of v, by the element width
    case BM_BOOL:
    case BM_U8:
    case BM_I8: ((uint8_t *)out)[idx] = (uint8_t)v; break;
    case BM_U16:
    case BM_I16:
    case BM_F16: ((uint16_t *)out)[idx] = (uint16_t)v; break;
    case BM_U32:
    case BM_I32:
    case BM_F32: ((uint32_t *)out)[idx] = (uint32_t)v; break;
    default: ((uint64_t *)out)[idx] = v; break;
  }
}

__device__ __forceinline__ double finish(int stat, double mean, double m2, double n) {
  if (stat == BM_STAT_MEAN) return mean;
  const double var = n > 0.0 ? m2 / n : __builtin_nan("");
  return stat == BM_STAT_VAR ? var : sqrt(var);
}

// Output sink: either final values or state planes (p0, p1) at index e.
constexpr int kFinalMoments = 2;  // final_out: mean / var / std planes, each optional (bm_reduce_moments)
struct Sink {
  void *out;        // final output (final_out == 1)
  int out_dtype;
  int stat;
  int final_out;    // 0: state planes, 1: `out`, kFinalMoments: om / ov / os
  double *p0;       // state plane 0 (mean / fsum) or uint64 plane (isum / or)
  double *p1;       // state plane 1 (M2)
  double *p2;       // var / std chunk partials: the row's pivot P per output
  int shifted;      // var / std: p0 holds mean - P (chunk partials in the workspace)
  void *om, *ov, *os;  // kFinalMoments: mean / var / std outputs (NULL: not asked for)
  double *k0, *k1;  // bm_reduce_keep: the BM_STAT_VAR state (absolute mean, M2) next to `out` (NULL: not kept)
};

// M2 as it leaves a kernel: not below 0 (rounding of S2 - S1^2 / n), and NaN
// where the mean is not finite -- a NaN or an infinity among the values, for
// which numpy's var / std are NaN.  (The sums of such a row give a NaN M2,
// which a plain ``m2 > 0 ? m2 : 0`` turned into 0.)
__device__ __forceinline__ double m2_out(double m2, double mean) {
  return mean - mean == 0.0 ? (m2 > 0.0 ? m2 : 0.0) : __builtin_nan("");
}

// The NaN path of a Welford mean.  An infinity among the values leaves the
// state's mean NaN unless it is in the last batch merged (the batch's own
// pivot, then every merge's delta, is inf - inf), where a sum over the values
// gives the infinity.  So a mean that came out NaN is formed again as
// sum(x - P) / n over the n values `stride` apart (P is finite): +-inf, or
// NaN for inf - inf or a NaN among them.  Finite data never comes here.
template <typename T>
__device__ __forceinline__ double summed_mean_y(const T *p, int64_t stride, int64_t n, double P) {
  double s = 0.0;
  for (int64_t r = 0; r < n; ++r) s += to_f64(p[r * stride]) - P;
  return s / (double)n;
}

// the kept copy of the var / std state of output idx: bm_reduce_state's values
__device__ __forceinline__ void emit_kept(const Sink &sk, int64_t idx, double mean_y, double m2, double P) {
  sk.k0[idx] = P + mean_y;
  sk.k1[idx] = m2_out(m2, P + mean_y);
}

// var / std output of one (output, chunk): the Welford state is kept around
// the pivot P (an element of the output's first row), mean_y = mean - P.
// Final: var / std (M2 only), or every moment asked for from the one state
// (the StatCounter of statcounter.py:30-48 holds n, mu and m2 together: mean
// = P + mean_y, var = M2 / n, std = sqrt(var), the var / std arithmetic of
// the single-statistic sink); state: mean, M2 -- shifted for the workspace
// partials (chunk 0 records P), absolute for bm_reduce_state.
__device__ __forceinline__ void emit_mom(const Sink &sk, int64_t idx, int64_t e, int64_t c, double n,
                                         double mean_y, double m2, double P) {
  m2 = m2_out(m2, P + mean_y);
  if (sk.k0) emit_kept(sk, idx, mean_y, m2, P);
  if (sk.final_out == kFinalMoments) {
    if (sk.om) store_out(sk.om, idx, n > 0.0 ? P + mean_y : 0.0, sk.out_dtype);
    if (sk.ov) store_out(sk.ov, idx, finish(BM_STAT_VAR, 0.0, m2, n), sk.out_dtype);
    if (sk.os) store_out(sk.os, idx, finish(BM_STAT_STD, 0.0, m2, n), sk.out_dtype);
    return;
  }
  if (sk.final_out) {
    store_out(sk.out, idx, finish(sk.stat, 0.0, m2, n), sk.out_dtype);
    return;
  }
  sk.p0[idx] = sk.shifted ? mean_y : P + mean_y;
  sk.p1[idx] = m2;
  if (sk.shifted && c == 0) sk.p2[e] = P;
}

template <int MODE>
__device__ __forceinline__ void emit(const Sink &sk, int64_t e, double n, double mean, double m2,
                                     uint64_t u) {
  if (bit_mode<MODE>()) {
    if (sk.final_out) store_int(sk.out, e, u, sk.out_dtype);
    else ((uint64_t *)sk.p0)[e] = u;
  } else if (facc_mode<MODE>()) {
    if (sk.final_out) store_out(sk.out, e, mean, sk.out_dtype);
    else sk.p0[e] = mean;
  } else {
    if (sk.final_out) store_out(sk.out, e, finish(sk.stat, mean, m2, n), sk.out_dtype);
    else {
      sk.p0[e] = mean;
      if (MODE == M_MOM) sk.p1[e] = m2;
    }
  }
}

// ------------------------------------------------------------------ cols --
// (the XCD-aware block order, xcd_block, is in bm_wave.h)
struct ColsDesc {
  int64_t O, R, I;
  int64_t rchunk;
  int64_t nchunks;
  int32_t tcv;  // threads across columns (power of two <= 256)
  int32_t nph;  // row phases = 256 / tcv
  FastDiv ntc;  // column tiles per O
  int64_t tile0;  // first (o, column tile) of this launch (launches split at the grid limit)
};

template <typename T, int VEC, int MODE>
__global__ void __launch_bounds__(kThreads)
    k_red_cols(const T *__restrict__ src, ColsDesc d, Sink sk) {
  // row-phase merge buffers, dynamic: sized only when the block has more
  // than one row phase (cols_lds_bytes), so the wide-output case (C4's var,
  // one phase) keeps the occupancy of an LDS-free kernel
  extern __shared__ double smem[];
  double *sm0 = smem;
  double *sm1 = smem + kThreads * VEC;
  double *smn = smem + 2 * kThreads * VEC;
  const uint64_t ot = (uint64_t)d.tile0 + xcd_block();
  const uint64_t o = fd_div(ot, d.ntc);
  const uint64_t tc = ot - o * d.ntc.d;
  const int64_t c = blockIdx.y;
  const int64_t r_lo = c * d.rchunk;
  const int64_t r_hi = min(d.R, r_lo + d.rchunk);
  const int cv = threadIdx.x % d.tcv;
  const int ph = threadIdx.x / d.tcv;
  const int64_t col0 = ((int64_t)tc * d.tcv + cv) * VEC;
  const bool active = col0 < d.I;
  const int64_t nph = d.nph;

  Acc<M_MEAN> acc[VEC];
  double fs[VEC];
  uint64_t us[VEC];
  // var / std: the lane's Welford state per column; the VEC columns share n
  double wm[VEC], wq[VEC];
  double wn = 0.0;
  int64_t wkb = 0;  // equal main-loop batches merged
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    acc[k].init(); fs[k] = fident<MODE>(); us[k] = bident<T, MODE>(); wm[k] = 0.0; wq[k] = 0.0;
  }

  double P[VEC];  // var / std: pivot per column, the column's element in row 0
#pragma unroll
  for (int k = 0; k < VEC; ++k) P[k] = 0.0;
  if (active) {
    const T *base = src + ((int64_t)o * d.R) * d.I + col0;
    int64_t r = r_lo + ph;
    if (mom_part<MODE>()) {
      T p0v[VEC];
      vload<T, VEC>(base, p0v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) P[k] = finite_or_zero(to_f64(p0v[k]));
    }
    if (MODE == M_MEANMOM) {
      // never chunked (r_lo == 0): the mean's pivot, the chunk's first row, is P
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k].pivot(P[k]);
    }
    if (MODE == M_MEAN) {
      // one pivot per column for every row phase of the block (the chunk's
      // first row): the phases then combine by plain sums, no divisions
      T k0[VEC];
      vload<T, VEC>(base + r_lo * d.I, k0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k].pivot(finite_or_zero(to_f64(k0[k])));
    }
    if constexpr (mean_part<MODE>() || MODE == M_MOM || facc_mode<MODE>()) {
      // kColsUnroll rows in flight per lane; the adds stay in row order
      for (; r + (kColsUnroll - 1) * nph < r_hi; r += kColsUnroll * nph) {
        T v[kColsUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kColsUnroll; ++u) vload_nt<T, VEC>(base + (r + u * nph) * d.I, v[u]);
        if constexpr (mom_part<MODE>()) {
          // one Welford batch of kColsUnroll rows per column
          double f, nf;
          uniform_weights(wkb, (double)kColsUnroll, f, nf);
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            double x[kColsUnroll];
#pragma unroll
            for (int u = 0; u < kColsUnroll; ++u) x[u] = to_f64(v[u][k]);
            if constexpr (MODE == M_MEANMOM) {
              // M_MEAN's adds below: each column's sum takes its rows in order
#pragma unroll
              for (int u = 0; u < kColsUnroll; ++u) acc[k].add(x[u]);
            }
            double mb, qb;
            batch_moments<kColsUnroll>(x, P[k], mb, qb);
            merge_batch(wm[k], wq[k], mb, qb, f, nf);
          }
          ++wkb;
          wn += (double)kColsUnroll;
          continue;
        }
#pragma unroll
        for (int u = 0; u < kColsUnroll; ++u) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            if (facc_mode<MODE>()) fs[k] = fop<MODE>(fs[k], to_f64(v[u][k]));
            else acc[k].add(to_f64(v[u][k]));
          }
        }
      }
    }
    for (; r + 3 * nph < r_hi; r += 4 * nph) {
      T v0[VEC], v1[VEC], v2[VEC], v3[VEC];
      vload_nt<T, VEC>(base + r * d.I, v0);
      vload_nt<T, VEC>(base + (r + nph) * d.I, v1);
      vload_nt<T, VEC>(base + (r + 2 * nph) * d.I, v2);
      vload_nt<T, VEC>(base + (r + 3 * nph) * d.I, v3);
      double f = 0.0, nf = 0.0;
      if (mom_part<MODE>()) batch_weights(wn, 4.0, f, nf);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (mom_part<MODE>()) {
          const double x[4] = {to_f64(v0[k]), to_f64(v1[k]), to_f64(v2[k]), to_f64(v3[k])};
          double mb, qb;
          batch_moments<4>(x, P[k], mb, qb);
          merge_batch(wm[k], wq[k], mb, qb, f, nf);
        }
        if (mean_part<MODE>()) {
          acc[k].add(to_f64(v0[k])); acc[k].add(to_f64(v1[k]));
          acc[k].add(to_f64(v2[k])); acc[k].add(to_f64(v3[k]));
        } else if (facc_mode<MODE>()) {
          fs[k] = fop<MODE>(fs[k], to_f64(v0[k])); fs[k] = fop<MODE>(fs[k], to_f64(v1[k]));
          fs[k] = fop<MODE>(fs[k], to_f64(v2[k])); fs[k] = fop<MODE>(fs[k], to_f64(v3[k]));
        } else if (!mom_part<MODE>()) {
          us[k] = bop<T, MODE>(us[k], bop<T, MODE>(bop<T, MODE>(belem<T, MODE>(v0[k]), belem<T, MODE>(v1[k])),
                                                   bop<T, MODE>(belem<T, MODE>(v2[k]), belem<T, MODE>(v3[k]))));
        }
      }
      if (mom_part<MODE>()) wn += 4.0;
    }
    for (; r < r_hi; r += nph) {
      T v[VEC];
      vload_nt<T, VEC>(base + r * d.I, v);
      if (mom_part<MODE>()) wn += 1.0;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (mom_part<MODE>()) {  // Welford's single-value update
          const double x = to_f64(v[k]) - P[k];
          const double delta = x - wm[k];
          wm[k] += delta / wn;
          wq[k] = fma(delta, x - wm[k], wq[k]);
        }
        if (mean_part<MODE>()) acc[k].add(to_f64(v[k]));
        else if (facc_mode<MODE>()) fs[k] = fop<MODE>(fs[k], to_f64(v[k]));
        else if (!mom_part<MODE>()) us[k] = bop<T, MODE>(us[k], belem<T, MODE>(v[k]));
      }
    }
  }

  if constexpr (mom_part<MODE>()) {
    // row phases: Chan merges in a fixed binary tree over the phases (phase
    // p absorbs p + s at stride s), through LDS
    for (int s = 1; s < nph; s <<= 1) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        sm0[threadIdx.x * VEC + k] = wm[k];
        sm1[threadIdx.x * VEC + k] = wq[k];
      }
      smn[threadIdx.x] = wn;
      __syncthreads();
      if ((ph & (2 * s - 1)) == 0 && ph + s < nph) {
        const int other = (ph + s) * d.tcv + cv;
        const double nb = smn[other];
        if (nb > 0.0) {
          double f, nf;
          batch_weights(wn, nb, f, nf);
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            merge_batch(wm[k], wq[k], sm0[other * VEC + k], sm1[other * VEC + k], f, nf);
          wn += nb;
        }
      }
    }
    if constexpr (MODE == M_MOM) {
      if (ph != 0 || !active) return;
      const double ntot = (double)(r_hi - r_lo);
      const int64_t plane = d.O * d.I;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const int64_t e = (int64_t)o * d.I + col0 + k;
        const int64_t idx = sk.final_out ? e : (c * plane + e);
        if (wm[k] != wm[k])  // a non-finite value in the column: the mean a sum gives
          wm[k] = summed_mean_y(src + ((int64_t)o * d.R + r_lo) * d.I + col0 + k, d.I, r_hi - r_lo, P[k]);
        emit_mom(sk, idx, e, c, ntot, wm[k], wq[k], P[k]);
      }
      return;
    }
    // M_MEANMOM: phase 0 holds the columns' states; the sums below reuse sm0
    if (nph > 1) __syncthreads();
  }

  // other modes: combine the row phases of each column through LDS (phase
  // order); mean carries the shared-pivot sum S1 until the end
  double m_[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    if (mean_part<MODE>()) m_[k] = acc[k].s1();
    else if (facc_mode<MODE>()) m_[k] = fs[k];
    else m_[k] = __builtin_bit_cast(double, us[k]);
  }
  if (nph > 1) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) sm0[threadIdx.x * VEC + k] = m_[k];
    __syncthreads();
    if (ph == 0) {
      for (int p = 1; p < nph; ++p) {
        const int other = p * d.tcv + cv;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const double mb = sm0[other * VEC + k];
          if (mean_part<MODE>() || facc_mode<MODE>()) {
            m_[k] = fop<MODE>(m_[k], mb);
          } else {
            m_[k] = __builtin_bit_cast(double, bop<T, MODE>(__builtin_bit_cast(uint64_t, m_[k]),
                                                            __builtin_bit_cast(uint64_t, mb)));
          }
        }
      }
    }
  }
  if (ph != 0 || !active) return;
  const double ntot = (double)(r_hi - r_lo);
  const int64_t plane = d.O * d.I;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    if (mean_part<MODE>()) m_[k] = mean_from_sums(ntot, acc[k].K, m_[k]);
    const int64_t e = (int64_t)o * d.I + col0 + k;
    const int64_t idx = sk.final_out ? e : (c * plane + e);
    emit<MODE>(sk, idx, ntot, m_[k], 0.0, __builtin_bit_cast(uint64_t, m_[k]));
    // (a NaN Welford mean -- a non-finite value in the column -- gives way to the sums')
    if constexpr (MODE == M_MEANMOM) emit_kept(sk, idx, wm[k] == wm[k] ? wm[k] : m_[k] - P[k], wq[k], P[k]);
  }
}

// ------------------------------------------------------------------ rows --
// (the XCD-aware block order, rows_block, is in bm_wave.h)
struct RowsDesc {
  int64_t O, R;
  int64_t P;       // elements between row starts (R, or a padded row pitch >= R)
  int64_t rchunk;
  FastDiv nchunks;
  int64_t nitems;  // O * nchunks
  int64_t item0;   // first item of this launch (launches split at the grid limit)
};

template <typename T, int VEC, int MODE>
__global__ void __launch_bounds__(kThreads)
    k_red_rows(const T *__restrict__ src, RowsDesc d, Sink sk) {
  const int lane = threadIdx.x & 63;
  const uint64_t bid = rows_block();
  const int64_t item = d.item0 + (int64_t)bid * (kThreads / 64) + (threadIdx.x >> 6);
  if (item >= d.nitems) return;  // whole wave exits; no block barrier below
  const uint64_t o = fd_div((uint64_t)item, d.nchunks);
  const int64_t c = item - (int64_t)o * (int64_t)d.nchunks.d;
  const int64_t r_lo = c * d.rchunk;
  const int64_t r_hi = min(d.R, r_lo + d.rchunk);
  const T *row = src + (int64_t)o * d.P;

  Acc<M_MEAN> acc;
  acc.init();
  Wel w;  // var / std
  w.init();
  double fs = fident<MODE>();
  uint64_t us = bident<T, MODE>();
  int64_t j = r_lo + (int64_t)lane * VEC;
  const int64_t stride = 64 * VEC;
  // mean: one pivot for the whole (row, chunk) -- its first element -- so the
  // 64 lanes combine by plain sums (no per-step division, see butterfly).
  // var / std: every value is shifted by the row's first element P (shared
  // by all chunks of the row), so the Welford means stay near zero and keep
  // their digits on offset data (1e6 + N(0,1)); batches bound outliers.
  // (both pivots finite, see finite_or_zero)
  if (mean_part<MODE>()) acc.pivot(finite_or_zero(to_f64(row[r_lo])));
  const double P = mom_part<MODE>() ? finite_or_zero(to_f64(row[0])) : 0.0;
  // kRowsUnroll 16-B vectors in flight per lane (HBM latency cover), over
  // whole wave-wide steps only: every lane runs the same iterations, so a
  // step ends on a line boundary of a line-aligned row and no 128-B line is
  // split between a main-loop load and a tail load issued later (padded C2
  // rows: the split line was fetched from HBM twice about 60% of the time,
  // 1.018x read traffic)
  // (chunks shorter than one step keep the per-lane bound, so the Welford
  // batches still cover most of them)
  const int64_t step = kRowsUnroll * stride;
  const int64_t main_end = r_hi - r_lo >= step ? r_lo + (r_hi - r_lo) / step * step
                                               : r_hi - VEC - (kRowsUnroll - 1) * stride + 1;
  for (; j < main_end; j += step) {
    T v[kRowsUnroll][VEC];
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) vload_nt<T, VEC>(row + j + u * stride, v[u]);
    if constexpr (mom_part<MODE>()) {
      // the kRowsUnroll * VEC values in hand form one Welford batch
      double x[kRowsUnroll * VEC];
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u)
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[u * VEC + k] = to_f64(v[u][k]);
      if constexpr (MODE == M_MEANMOM) {
        // M_MEAN's adds below, in their order, on the converted values
        if constexpr (VEC % 2 == 0) {
#pragma unroll
          for (int i = 0; i < kRowsUnroll * VEC; i += 2) acc.add2(x[i], x[i + 1]);
        } else {
#pragma unroll
          for (int i = 0; i < kRowsUnroll * VEC; ++i) acc.add(x[i]);
        }
      }
      w.add_main<kRowsUnroll * VEC>(x, P);
      continue;
    }
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      if constexpr (mean_part<MODE>() && VEC % 2 == 0) {
#pragma unroll
        for (int k = 0; k < VEC; k += 2) acc.add2(to_f64(v[u][k]), to_f64(v[u][k + 1]));
        continue;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (mean_part<MODE>()) acc.add(to_f64(v[u][k]));
        else if (facc_mode<MODE>()) fs = fop<MODE>(fs, to_f64(v[u][k]));
        else us = bop<T, MODE>(us, belem<T, MODE>(v[u][k]));
      }
    }
  }
  // var / std: the rest of the row and the cross-lane merge run as sums
  // around one wave-wide pivot C = lane 0's Welford mean (lane 0 holds 1/64
  // of the main-loop data, so n (mean - C)^2 <= 64 M2 and S2 - S1^2/n loses
  // at most ~6 bits): plain adds, no division per lane or per butterfly step
  const double C = mom_part<MODE>() ? lane0_of(w.mean) : 0.0;
  double t1 = 0.0, t2 = 0.0;
  for (; j < r_hi; j += stride) {
    if (j + VEC <= r_hi) {
      T v[VEC];
      vload_nt<T, VEC>(row + j, v);
      if constexpr (mom_part<MODE>()) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const double y = (to_f64(v[k]) - P) - C;
          t1 += y;
          t2 = fma(y, y, t2);
        }
        if constexpr (MODE == M_MOM) continue;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (mean_part<MODE>()) acc.add(to_f64(v[k]));
        else if (facc_mode<MODE>()) fs = fop<MODE>(fs, to_f64(v[k]));
        else us = bop<T, MODE>(us, belem<T, MODE>(v[k]));
      }
    } else {
      for (int64_t k = j; k < r_hi; ++k) {
        if (mom_part<MODE>()) {
          const double y = (to_f64(row[k]) - P) - C;
          t1 += y;
          t2 = fma(y, y, t2);
        }
        if (mean_part<MODE>()) acc.add(to_f64(row[k]));
        else if (facc_mode<MODE>()) fs = fop<MODE>(fs, to_f64(row[k]));
        else if (!mom_part<MODE>()) us = bop<T, MODE>(us, belem<T, MODE>(row[k]));
      }
    }
  }

  // wave combination: DPP fold into lane 63 in lane order (deterministic).
  // mean: shared pivot, the S1 sums simply add; var / std: each lane's
  // Welford state as sums around C, which add.
  double m = facc_mode<MODE>() ? fs : acc.s1();
  double ws = 0.0, wq = 0.0;  // var / std: the wave's (S1, S2) around C
  if constexpr (mom_part<MODE>()) {
    const double dm = w.mean - C;
    const double s1 = w.n * dm;
    ws = s1 + t1;
    wq = fma(s1, dm, w.m2) + t2;
    const auto add = [](double a, double b) { return a + b; };
    ws = wave_fold(ws, lane, add);
    wq = wave_fold(wq, lane, add);
  }
  if constexpr (mean_part<MODE>() || facc_mode<MODE>()) {
    m = wave_fold(m, lane, [](double a, double b) { return fop<MODE>(a, b); });
  } else if constexpr (!mom_part<MODE>()) {
    us = wave_fold(us, lane, [](uint64_t a, uint64_t b) { return bop<T, MODE>(a, b); });
  }
  const double ntot = (double)(r_hi - r_lo);
  double my = 0.0;  // var / std: the chunk's mean - P from (S1, S2) around C
  if constexpr (MODE == M_MOM) {
    // in every lane, so that the NaN path below is taken by the whole wave: a
    // non-finite value in the chunk, whose mean the wave then sums again
    // (summed_mean_y's, the lanes striding the chunk)
    my = C + lane_of<kFoldLane>(ws) / ntot;
    if (my != my) {
      double s = 0.0;
      for (int64_t k = r_lo + lane; k < r_hi; k += 64) s += to_f64(row[k]) - P;
      my = wave_fold(s, lane, [](double a, double b) { return a + b; }) / ntot;
    }
  }
  if (lane != kFoldLane) return;
  const int64_t e = (int64_t)o;
  const int64_t idx = sk.final_out ? e : (c * d.O + e);
  if constexpr (MODE == M_MOM) {
    // (S1, S2) around C -> mean - P and M2
    const double q = fma(-ws, ws / ntot, wq);
    emit_mom(sk, idx, e, c, ntot, my, q, P);
    return;
  }
  if (mean_part<MODE>()) m = mean_from_sums(ntot, acc.K, m);
  emit<MODE>(sk, idx, ntot, m, 0.0, us);
  if constexpr (MODE == M_MEANMOM) {
    const double q = fma(-ws, ws / ntot, wq);
    my = C + ws / ntot;
    // (a NaN Welford mean -- a non-finite value in the row -- gives way to the sums')
    emit_kept(sk, idx, my == my ? my : m - P, q, P);
  }
}

// ----------------------------------------------- exact integer var / std --
// 1- and 2-byte integer (and bool) inputs: var / std from exact integer sums.
// Each lane keeps S1 = sum x (int64) and S2 = sum x^2 (uint64; x^2 < 2^32);
// lanes, row phases and waves add exactly (any order gives the same bits),
// and M2 = (n S2 - S1^2) / n is formed in 128-bit integers and rounded once
// -- exact up to that rounding, cheaper than the float64 Welford path (no
// conversions, one multiply-add per element) and deterministic by
// construction.  (statcounter.py:51-59 computes the same M2 in float64.)
template <typename T> constexpr bool small_int() {
  return std::is_integral<T>::value && sizeof(T) <= 2;
}

// x^2 of a value of a 1- or 2-byte type, in 32-bit unsigned arithmetic (< 2^32)
__device__ __forceinline__ uint64_t sq32(int32_t x) {
  const uint32_t a = (uint32_t)(x < 0 ? -x : x);
  return (uint64_t)(a * a);
}

// (n, S1, S2) -> (mean, M2) with the n S2 - S1^2 difference in 128 bits.  S2
// arrives as a 128-bit (hi, lo) pair: one chunk's S2 fits 64 bits (the host
// caps a chunk at 2^31 rows, x^2 < 2^32), but the sum over chunks does not
// once an output covers 2^32 values of magnitude ~2^16 (an 8 GiB uint16
// var(axis=None)).  n < 2^38 and S2 < 2^70, so n S2 < 2^108; |S1| < 2^54.
__device__ __forceinline__ void int_moments(uint64_t n, int64_t s1, uint64_t s2, uint64_t s2_hi, double &mean,
                                            double &m2) {
  mean = n ? (double)s1 / (double)n : 0.0;
  const uint64_t a1 = (uint64_t)(s1 < 0 ? -s1 : s1);
  // n * s2 and a1 * a1 as (hi, lo)
  const uint64_t p_lo = n * s2, p_hi = __umul64hi(n, s2) + n * s2_hi;
  const uint64_t q_lo = a1 * a1, q_hi = __umul64hi(a1, a1);
  const uint64_t lo = p_lo - q_lo;
  const uint64_t hi = p_hi - q_hi - (p_lo < q_lo ? 1 : 0);
  const double num = (double)hi * 18446744073709551616.0 + (double)lo;  // >= 0 (Cauchy-Schwarz)
  m2 = n ? num / (double)n : 0.0;
}

// 128-bit running S2: (hi, lo) += v
__device__ __forceinline__ void add128(uint64_t &lo, uint64_t &hi, uint64_t v_lo, uint64_t v_hi) {
  const uint64_t t = lo + v_lo;
  hi += v_hi + (t < lo ? 1 : 0);
  lo = t;
}

// chunk partials (workspace) stay exact integer sums, merged by the combine
// kernel's integer branch; final outputs and rank states get (mean, M2)
__device__ __forceinline__ void emit_int_mom(const Sink &sk, int64_t idx, int64_t e, int64_t c, int64_t n,
                                             int64_t s1, uint64_t s2) {
  if (!sk.final_out && sk.shifted) {
    reinterpret_cast<int64_t *>(sk.p0)[idx] = s1;
    reinterpret_cast<uint64_t *>(sk.p1)[idx] = s2;
    return;
  }
  double mean, m2;
  int_moments((uint64_t)n, s1, s2, 0, mean, m2);
  emit_mom(sk, idx, e, c, (double)n, mean, m2, 0.0);
}

template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads)
    k_red_cols_int(const T *__restrict__ src, ColsDesc d, Sink sk) {
  extern __shared__ double smem[];
  uint64_t *l1 = reinterpret_cast<uint64_t *>(smem);
  uint64_t *l2 = l1 + kThreads * VEC;
  const uint64_t ot = (uint64_t)d.tile0 + xcd_block();
  const uint64_t o = fd_div(ot, d.ntc);
  const uint64_t tc = ot - o * d.ntc.d;
  const int64_t c = blockIdx.y;
  const int64_t r_lo = c * d.rchunk;
  const int64_t r_hi = min(d.R, r_lo + d.rchunk);
  const int cv = threadIdx.x % d.tcv;
  const int ph = threadIdx.x / d.tcv;
  const int64_t col0 = ((int64_t)tc * d.tcv + cv) * VEC;
  const bool active = col0 < d.I;
  const int64_t nph = d.nph;
  int64_t s1[VEC];
  uint64_t s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { s1[k] = 0; s2[k] = 0; }
  if (active) {
    const T *base = src + ((int64_t)o * d.R) * d.I + col0;
    int64_t r = r_lo + ph;
    constexpr int U = kIntUnroll;  // rows in flight per lane
    for (; r + (U - 1) * nph < r_hi; r += U * nph) {
      T v[U][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) vload_nt<T, VEC>(base + (r + u * nph) * d.I, v[u]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        int32_t t1 = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t x = (int32_t)v[u][k];
          t1 += x;
          s2[k] += sq32(x);
        }
        s1[k] += t1;
      }
    }
    for (; r < r_hi; r += nph) {
      T v[VEC];
      vload_nt<T, VEC>(base + r * d.I, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const int32_t x = (int32_t)v[k];
        s1[k] += x;
        s2[k] += sq32(x);
      }
    }
  }
  if (nph > 1) {  // row phases: exact integer sums
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      l1[threadIdx.x * VEC + k] = (uint64_t)s1[k];
      l2[threadIdx.x * VEC + k] = s2[k];
    }
    __syncthreads();
    if (ph == 0) {
      for (int p = 1; p < nph; ++p) {
        const int other = p * d.tcv + cv;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          s1[k] += (int64_t)l1[other * VEC + k];
          s2[k] += l2[other * VEC + k];
        }
      }
    }
  }
  if (ph != 0 || !active) return;
  const int64_t n = r_hi - r_lo;
  const int64_t plane = d.O * d.I;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const int64_t e = (int64_t)o * d.I + col0 + k;
    const int64_t idx = sk.final_out ? e : (c * plane + e);
    emit_int_mom(sk, idx, e, c, n, s1[k], s2[k]);
  }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads)
    k_red_rows_int(const T *__restrict__ src, RowsDesc d, Sink sk) {
  const int lane = threadIdx.x & 63;
  const uint64_t bid = rows_block();
  const int64_t item = d.item0 + (int64_t)bid * (kThreads / 64) + (threadIdx.x >> 6);
  if (item >= d.nitems) return;  // whole wave exits
  const uint64_t o = fd_div((uint64_t)item, d.nchunks);
  const int64_t c = item - (int64_t)o * (int64_t)d.nchunks.d;
  const int64_t r_lo = c * d.rchunk;
  const int64_t r_hi = min(d.R, r_lo + d.rchunk);
  const T *row = src + (int64_t)o * d.P;
  int64_t s1 = 0;
  uint64_t s2 = 0;
  const int64_t stride = 64 * VEC;
  for (int64_t j = r_lo + (int64_t)lane * VEC; j < r_hi; j += stride) {
    if (j + VEC <= r_hi) {
      T v[VEC];
      vload_nt<T, VEC>(row + j, v);
      int32_t t1 = 0;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const int32_t x = (int32_t)v[k];
        t1 += x;
        s2 += sq32(x);
      }
      s1 += t1;
    } else {
      for (int64_t k = j; k < r_hi; ++k) {
        const int32_t x = (int32_t)row[k];
        s1 += x;
        s2 += sq32(x);
      }
    }
  }
  // exact integer sums: any order gives the same bits
  s1 = wave_fold(s1, lane, [](int64_t a, int64_t b) { return a + b; });
  s2 = wave_fold(s2, lane, [](uint64_t a, uint64_t b) { return a + b; });
  if (lane != kFoldLane) return;
  const int64_t n = r_hi - r_lo;
  const int64_t e = (int64_t)o;
  const int64_t idx = sk.final_out ? e : (c * d.O + e);
  emit_int_mom(sk, idx, e, c, n, s1, s2);
}

// --------------------------------------------------------------- combine --
constexpr int kMaxParts = 256;  // parts per bm_reduce_combine (ranks of a merge); kernarg-resident counts
struct CombDesc {
  int64_t nout;
  int64_t nparts;
  int64_t part_stride;  // elements between parts in a plane
  int64_t R, rchunk;    // uniform chunk counts when explicit == 0
  int32_t explicit_counts;
  int32_t pivots;       // var / std chunk partials: p0 is mean - P, P in the plane after M2
  int32_t int_sums;     // var / std of 1-2 byte integers: partials are exact (S1, S2) sums
  int32_t pad_;
  int64_t counts[kMaxParts];
};

// The NaN path of a merged mean, as k_red_merge_tiles has it: a part whose mean
// is an infinity, followed by a finite part, makes chan's delta * f + mean
// inf - inf.  The merged mean is then the sum of the parts' means (all around
// one finite pivot, or absolute): +-inf, or NaN for inf - inf or a NaN part --
// what a sum over the values gives.
__device__ __forceinline__ double summed_part_means(const double *__restrict__ p0, const CombDesc &d, int64_t e) {
  double s = 0.0;
  for (int64_t p = 0; p < d.nparts; ++p) {
    const int64_t nb = d.explicit_counts ? d.counts[p] : min(d.R, (p + 1) * d.rchunk) - p * d.rchunk;
    if (nb > 0) s += p0[p * d.part_stride + e];
  }
  return s;
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kThreads)
    k_red_combine(const double *__restrict__ p0, const double *__restrict__ p1, CombDesc d, Sink sk) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < d.nout; e += step) {
    double n = 0.0, m = 0.0, q = 0.0;
    uint64_t u = 0;
    bool first = true;
    if constexpr (MODE == M_MOM) {
      if (d.int_sums) {  // exact: add the chunks' integer sums
        int64_t s1 = 0, cnt = 0;
        uint64_t s2 = 0, s2_hi = 0;
        for (int64_t p = 0; p < d.nparts; ++p) {
          const int64_t nb = min(d.R, (p + 1) * d.rchunk) - p * d.rchunk;
          if (nb <= 0) continue;
          const int64_t at = p * d.part_stride + e;
          s1 += reinterpret_cast<const int64_t *>(p0)[at];
          add128(s2, s2_hi, reinterpret_cast<const uint64_t *>(p1)[at], 0);
          cnt += nb;
        }
        double mean, m2;
        int_moments((uint64_t)cnt, s1, s2, s2_hi, mean, m2);
        emit_mom(sk, e, e, 1, (double)cnt, mean, m2, 0.0);
        continue;
      }
    }
    for (int64_t p = 0; p < d.nparts; ++p) {
      const double nb = d.explicit_counts
                            ? (double)d.counts[p]
                            : (double)(min(d.R, (p + 1) * d.rchunk) - p * d.rchunk);
      if (nb <= 0.0) continue;
      const int64_t at = p * d.part_stride + e;
      if (MODE == M_MEAN || MODE == M_MOM) {
        // chunk partials of var / std are all around the same pivot P
        chan(n, m, q, nb, p0[at], (MODE == M_MOM) ? p1[at] : 0.0, MODE == M_MOM);
      } else if (facc_mode<MODE>()) {
        m = first ? p0[at] : fop<MODE>(m, p0[at]);
        n += nb;
      } else {
        const uint64_t b = ((const uint64_t *)p0)[at];
        u = first ? b : bop<T, MODE>(u, b);
      }
      first = false;
    }
    if constexpr (MODE == M_MEAN || MODE == M_MOM) {
      if (m != m) m = summed_part_means(p0, d, e);
    }
    if constexpr (MODE == M_MOM) {
      const double P = d.pivots ? p1[d.nparts * d.part_stride + e] : 0.0;
      emit_mom(sk, e, e, 1, n, m, q, P);
    } else {
      emit<MODE>(sk, e, n, m, q, u);
    }
  }
}

// Few outputs, many parts (axis=None statistics: one output from hundreds of
// chunk states): one block per output.  Thread t merges the contiguous run of
// parts [t*L, (t+1)*L) in order, then the 256 partial states merge in a fixed
// binary tree through LDS (thread j absorbs j + s): deterministic, and a
// serial chain of hundreds of dependent loads and divisions becomes ~L + 8.
struct PartState {
  double n, m, q;
  uint64_t u;
  int64_t s1, cnt;
  uint64_t s2, s2_hi;  // 128-bit sum of the chunks' S2
  int any;
};

template <int MODE, typename T>
__device__ __forceinline__ void merge_state(PartState &a, const PartState &b, bool int_sums) {
  if (!b.any) return;
  if (!a.any) {
    a = b;
    return;
  }
  if (MODE == M_MOM && int_sums) {
    a.s1 += b.s1; a.cnt += b.cnt;
    add128(a.s2, a.s2_hi, b.s2, b.s2_hi);
  } else if (MODE == M_MEAN || MODE == M_MOM) {
    chan(a.n, a.m, a.q, b.n, b.m, b.q, MODE == M_MOM);
  } else if (facc_mode<MODE>()) {
    a.m = fop<MODE>(a.m, b.m);
    a.n += b.n;
  } else {
    a.u = bop<T, MODE>(a.u, b.u);
  }
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kThreads)
    k_red_combine_blk(const double *__restrict__ p0, const double *__restrict__ p1, CombDesc d, Sink sk) {
  __shared__ PartState sm[kThreads];
  const int64_t e = blockIdx.x;
  const bool int_sums = MODE == M_MOM && d.int_sums;
  const int64_t L = (d.nparts + kThreads - 1) / kThreads;
  const int64_t p_lo = (int64_t)threadIdx.x * L, p_hi = min(d.nparts, p_lo + L);
  PartState st{};
  for (int64_t p = p_lo; p < p_hi; ++p) {
    const int64_t cnt = d.explicit_counts ? d.counts[p] : min(d.R, (p + 1) * d.rchunk) - p * d.rchunk;
    if (cnt <= 0) continue;
    const int64_t at = p * d.part_stride + e;
    PartState b{};
    b.any = 1;
    b.n = (double)cnt;
    if (int_sums) {
      b.s1 = reinterpret_cast<const int64_t *>(p0)[at];
      b.s2 = reinterpret_cast<const uint64_t *>(p1)[at];
      b.cnt = cnt;
    } else if (MODE == M_MEAN || MODE == M_MOM) {
      b.m = p0[at];
      b.q = (MODE == M_MOM) ? p1[at] : 0.0;
    } else if (facc_mode<MODE>()) {
      b.m = p0[at];
    } else {
      b.u = ((const uint64_t *)p0)[at];
    }
    merge_state<MODE, T>(st, b, int_sums);
  }
  sm[threadIdx.x] = st;
  for (int s = 1; s < kThreads; s <<= 1) {
    __syncthreads();
    if ((threadIdx.x & (2 * s - 1)) == 0) {
      PartState a = sm[threadIdx.x];
      merge_state<MODE, T>(a, sm[threadIdx.x + s], int_sums);
      sm[threadIdx.x] = a;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  PartState r = sm[0];
  if constexpr (MODE == M_MEAN || MODE == M_MOM) {
    if (!int_sums && r.m != r.m) r.m = summed_part_means(p0, d, e);
  }
  if constexpr (MODE == M_MOM) {
    if (int_sums) {
      double mean, m2;
      int_moments((uint64_t)r.cnt, r.s1, r.s2, r.s2_hi, mean, m2);
      emit_mom(sk, e, e, 1, (double)r.cnt, mean, m2, 0.0);
      return;
    }
    const double P = d.pivots ? p1[d.nparts * d.part_stride + e] : 0.0;
    emit_mom(sk, e, e, 1, r.n, r.m, r.q, P);
  } else {
    emit<MODE>(sk, e, r.n, r.m, r.q, r.u);
  }
}

// ------------------------------------------------------------------ host --
int mode_of(int stat, int dt) {
  if (stat == BM_STAT_MEAN) return M_MEAN;
  if (stat == BM_STAT_VAR || stat == BM_STAT_STD) return M_MOM;
  if (stat == BM_STAT_MAX) return M_MAX;
  if (stat == BM_STAT_MIN) return M_MIN;
  if (stat == BM_STAT_PROD) return is_float(dt) ? M_FPROD : (dt == BM_BOOL ? M_LAND : M_IPROD);
  if (stat == BM_STAT_LAND) return M_LAND;
  if (stat == BM_STAT_LOR) return M_OR;
  if (stat == BM_STAT_BAND) return M_BAND;
  if (stat == BM_STAT_BOR) return M_BOR;
  if (stat == BM_STAT_BXOR) return M_BXOR;
  if (stat == BM_STAT_FMAX) return is_float(dt) ? M_FMAX : M_MAX;
  if (stat == BM_STAT_FMIN) return is_float(dt) ? M_FMIN : M_MIN;
  if (is_float(dt)) return M_FSUM;
  if (dt == BM_BOOL) return M_OR;
  return M_ISUM;
}
int planes_of(int mode) { return mode == M_MOM ? 2 : 1; }
bool bit_mode_host(int mode) {
  return mode == M_ISUM || mode == M_OR || mode == M_MAX || mode == M_MIN || mode == M_IPROD ||
         mode == M_LAND || mode == M_BAND || mode == M_BOR || mode == M_BXOR || mode == M_FMAX ||
         mode == M_FMIN;
}
// the dtype a reduction writes: logical and / or give bool (numpy's
// logical_* ufuncs; bool sum is OR, bool product AND), the other bit modes
// and float sums / products keep the input dtype, statistics are float
int out_dtype_ok(int stat, int mode, int in_dt, int out_dt) {
  if (stat == BM_STAT_LAND || stat == BM_STAT_LOR) return out_dt == BM_BOOL;
  if (bit_mode_host(mode)) return out_dt == in_dt;
  return is_float(out_dt);
}

struct RedPlan {
  bool rows;
  int vec;
  int64_t rchunk, nchunks;
  int32_t tcv, nph;
  int64_t ntc;
};

RedPlan plan_reduce(int dt, int64_t O, int64_t R, int64_t I, const void *src, int64_t P) {
  RedPlan p{};
  const int es = dtype_size(dt);
  if (I == 1) {
    p.rows = true;
    const int vec = pick_vec(16 / es, {R, P}, {{src, es}});
    p.vec = vec;
    const int64_t target_waves = 8192;
    int64_t nch = 1;
    if (O < target_waves) {
      nch = cdiv(target_waves, O);
      const int64_t maxch = std::max<int64_t>(1, R / (64 * vec * 4));
      nch = std::min(nch, maxch);
    }
    // one chunk's exact integer S2 (x^2 < 2^32 per value) must fit 64 bits:
    // at most 2^31 values per chunk (a no-op below 4 GiB per output row)
    nch = std::max<int64_t>(nch, cdiv(R, (int64_t)1 << 31));
    int64_t rc = cdiv(R, nch);
    rc = cdiv(rc, vec) * vec;
    p.rchunk = rc;
    p.nchunks = cdiv(R, rc);
  } else {
    p.rows = false;
    const int vec = pick_vec(std::min(16 / es, 8), {I}, {{src, es}});
    p.vec = vec;
    const int64_t ncolv = cdiv(I, vec);
    int tcv = 1;
    while (tcv < kColsTcv && tcv < ncolv) tcv <<= 1;
    // narrower column tiles (more row phases merged in LDS) before splitting
    // R into chunks that need a workspace and a combine launch: C4's uint16
    // var over axis 0 3.50 -> 3.17 ms with 64-vector tiles and no chunks
    // (profiles/r03zb_ab_tcv.log); the float C2 column statistics move +-2%
    while (tcv > kColsTcvMin && O * cdiv(ncolv, tcv) < kColsBlocks) tcv >>= 1;
    p.tcv = tcv;
    p.nph = 256 / tcv;
    p.ntc = cdiv(ncolv, tcv);
    const int64_t blocks = O * p.ntc;
    int64_t nch = 1;
    if (blocks < kColsBlocks) {
      nch = cdiv(kColsBlocks, blocks);
      const int64_t maxch = std::max<int64_t>(1, R / ((int64_t)p.nph * 8));
      nch = std::min(nch, maxch);
    }
    nch = std::min<int64_t>(nch, 65535);
    nch = std::max<int64_t>(nch, cdiv(R, (int64_t)1 << 31));  // exact integer S2 per chunk < 2^63
    p.rchunk = cdiv(R, nch);
    p.nchunks = cdiv(R, p.rchunk);
  }
  return p;
}

// The launches of a plan, written once for every kernel family: the rows or
// columns descriptor filled, the grid split at the launch limit, and the
// plan's vector width as a template argument.  rows(v, blocks, desc) and
// cols(v, grid, desc) launch the one kernel of that width.
template <typename T, typename FR, typename FC>
void launch_plan(const RedPlan &p, int64_t O, int64_t R, int64_t P, int64_t I, FR &&rows, FC &&cols) {
  if (p.rows) {
    RowsDesc d;
    d.O = O; d.R = R; d.P = P; d.rchunk = p.rchunk;
    d.nchunks = make_fastdiv((uint64_t)p.nchunks);
    d.nitems = O * p.nchunks;
    for_block_runs(cdiv(d.nitems, kThreads / 64), kThreads, [&](int64_t b0, int g) {
      d.item0 = b0 * (kThreads / 64);
      for_vec<T, 16>(p.vec, [&](auto v) { rows(v, g, d); });
    });
  } else {
    ColsDesc d;
    d.O = O; d.R = R; d.I = I;
    d.rchunk = p.rchunk; d.nchunks = p.nchunks;
    d.tcv = p.tcv; d.nph = p.nph;
    d.ntc = make_fastdiv((uint64_t)p.ntc);
    for_tile_runs(O * p.ntc, p.nchunks, kThreads, [&](int64_t t0, dim3 grid) {
      d.tile0 = t0;
      for_vec<T, 8>(p.vec, [&](auto v) { cols(v, grid, d); });
    });
  }
}

// dynamic LDS of a k_red_cols launch: the row-phase buffers when nph > 1
template <int MODE> size_t cols_lds_bytes(int nph, int vec) {
  if (nph <= 1) return 0;
  return (mom_part<MODE>() ? (2 * (size_t)kThreads * vec + kThreads) : (size_t)kThreads * vec) * sizeof(double);
}

template <typename T, int MODE>
void launch_main_t(const RedPlan &p, const void *src, int64_t O, int64_t R, int64_t P, int64_t I, Sink sk,
                   hipStream_t st) {
  const T *s = (const T *)src;
  if constexpr (MODE == M_MOM && small_int<T>()) {
    // exact integer var / std: the same grids as the float kernels
    launch_plan<T>(
        p, O, R, P, I,
        [&](auto v, int g, const RowsDesc &d) {
          k_red_rows_int<T, decltype(v)::value><<<g, kThreads, 0, st>>>(s, d, sk);
        },
        [&](auto v, dim3 grid, const ColsDesc &d) {
          constexpr int V = decltype(v)::value;
          const size_t lds = p.nph > 1 ? 2 * (size_t)kThreads * V * sizeof(uint64_t) : 0;
          k_red_cols_int<T, V><<<grid, kThreads, lds, st>>>(s, d, sk);
        });
    return;
  }
  // (no else: the library has always carried the M_MOM float kernels of the
  // small integer types as well, and its set of kernels is left as it is)
  launch_plan<T>(
      p, O, R, P, I,
      [&](auto v, int g, const RowsDesc &d) {
        k_red_rows<T, decltype(v)::value, MODE><<<g, kThreads, 0, st>>>(s, d, sk);
      },
      [&](auto v, dim3 grid, const ColsDesc &d) {
        constexpr int V = decltype(v)::value;
        k_red_cols<T, V, MODE><<<grid, kThreads, cols_lds_bytes<MODE>(p.nph, V), st>>>(s, d, sk);
      });
}

template <int MODE>
int launch_main_m(int dt, const RedPlan &p, const void *src, int64_t O, int64_t R, int64_t P, int64_t I,
                  Sink sk, hipStream_t st) {
  bool done = false;
  for_dtype(dt, [&](auto t) {
    typedef typename decltype(t)::type T;
    if constexpr (!(int_only_mode<MODE>() && is_float_t<T>())) {
      launch_main_t<T, MODE>(p, src, O, R, P, I, sk, st);
      done = true;
    }
  });
  if (done) return BM_OK;
  bm_set_error("bm_reduce: unsupported dtype %d for this statistic", dt);
  return BM_E_ARG;
}

int launch_main(int mode, int dt, const RedPlan &p, const void *src, int64_t O, int64_t R,
                int64_t P, int64_t I, Sink sk, hipStream_t st) {
  switch (mode) {
    case M_MEAN: return launch_main_m<M_MEAN>(dt, p, src, O, R, P, I, sk, st);
    case M_MOM: return launch_main_m<M_MOM>(dt, p, src, O, R, P, I, sk, st);
    case M_FSUM: return launch_main_m<M_FSUM>(dt, p, src, O, R, P, I, sk, st);
    case M_ISUM: return launch_main_m<M_ISUM>(dt, p, src, O, R, P, I, sk, st);
    case M_MAX: return launch_main_m<M_MAX>(dt, p, src, O, R, P, I, sk, st);
    case M_MIN: return launch_main_m<M_MIN>(dt, p, src, O, R, P, I, sk, st);
    case M_FPROD: return launch_main_m<M_FPROD>(dt, p, src, O, R, P, I, sk, st);
    case M_IPROD: return launch_main_m<M_IPROD>(dt, p, src, O, R, P, I, sk, st);
    case M_LAND: return launch_main_m<M_LAND>(dt, p, src, O, R, P, I, sk, st);
    case M_BAND: return launch_main_m<M_BAND>(dt, p, src, O, R, P, I, sk, st);
    case M_BOR: return launch_main_m<M_BOR>(dt, p, src, O, R, P, I, sk, st);
    case M_BXOR: return launch_main_m<M_BXOR>(dt, p, src, O, R, P, I, sk, st);
    case M_FMAX: return launch_main_m<M_FMAX>(dt, p, src, O, R, P, I, sk, st);
    case M_FMIN: return launch_main_m<M_FMIN>(dt, p, src, O, R, P, I, sk, st);
    default: return launch_main_m<M_OR>(dt, p, src, O, R, P, I, sk, st);
  }
}

// bm_reduce_keep(BM_STAT_MEAN): the dual kernels, float inputs only
int launch_keep_mean(int dt, const RedPlan &p, const void *src, int64_t O, int64_t R, int64_t P, int64_t I,
                     Sink sk, hipStream_t st) {
  if (!is_float(dt)) {
    bm_set_error("bm_reduce_keep: dtype %d is not a float dtype", dt);
    return BM_E_ARG;
  }
  for_dtype(dt, [&](auto t) {
    typedef typename decltype(t)::type T;
    if constexpr (is_float_t<T>()) launch_main_t<T, M_MEANMOM>(p, src, O, R, P, I, sk, st);
  });
  return BM_OK;
}

// block-per-output combine for few outputs from many parts
bool comb_blk(const CombDesc &cd) { return cd.nout <= 1024 && cd.nparts >= 8; }

template <int MODE, typename T>
void launch_combine_k(int g, const double *p0, const double *p1, const CombDesc &cd, Sink sk, hipStream_t st) {
  if (comb_blk(cd))
    k_red_combine_blk<MODE, T><<<(int)cd.nout, kThreads, 0, st>>>(p0, p1, cd, sk);
  else
    k_red_combine<MODE, T><<<g, kThreads, 0, st>>>(p0, p1, cd, sk);
}

template <int MODE>
void launch_combine_m(int dt, int g, const double *p0, const double *p1, const CombDesc &cd, Sink sk,
                      hipStream_t st) {
  for_dtype(dt, [&](auto t) {  // only max/min look at the element type
    launch_combine_k<MODE, typename decltype(t)::type>(g, p0, p1, cd, sk, st);
  });
}

int launch_combine(int mode, int dt, const double *p0, const double *p1, const CombDesc &cd, Sink sk,
                   hipStream_t st) {
  int64_t g = cdiv(cd.nout, kThreads);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  switch (mode) {
    case M_MEAN: launch_combine_k<M_MEAN, double>((int)g, p0, p1, cd, sk, st); break;
    case M_MOM: launch_combine_k<M_MOM, double>((int)g, p0, p1, cd, sk, st); break;
    case M_FSUM: launch_combine_k<M_FSUM, double>((int)g, p0, p1, cd, sk, st); break;
    case M_FPROD: launch_combine_k<M_FPROD, double>((int)g, p0, p1, cd, sk, st); break;
    case M_ISUM: launch_combine_k<M_ISUM, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_IPROD: launch_combine_k<M_IPROD, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_OR: launch_combine_k<M_OR, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_LAND: launch_combine_k<M_LAND, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_BAND: launch_combine_k<M_BAND, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_BOR: launch_combine_k<M_BOR, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_BXOR: launch_combine_k<M_BXOR, uint64_t>((int)g, p0, p1, cd, sk, st); break;
    case M_MAX: launch_combine_m<M_MAX>(dt, (int)g, p0, p1, cd, sk, st); break;
    case M_FMAX: launch_combine_m<M_FMAX>(dt, (int)g, p0, p1, cd, sk, st); break;
    case M_FMIN: launch_combine_m<M_FMIN>(dt, (int)g, p0, p1, cd, sk, st); break;
    default: launch_combine_m<M_MIN>(dt, (int)g, p0, p1, cd, sk, st); break;
  }
  return BM_OK;
}

int check_args(int stat, int dt, int64_t O, int64_t R, int64_t I, const char *who) {
  if (stat < BM_STAT_MEAN || stat > BM_STAT_FMIN || dtype_size(dt) == 0) {
    bm_set_error("%s: bad stat %d / dtype %d", who, stat, dt);
    return BM_E_ARG;
  }
  if (O < 1 || R < 1 || I < 1) {
    bm_set_error("%s: empty reduction (O=%lld R=%lld I=%lld)", who, (long long)O, (long long)R,
                 (long long)I);
    return BM_E_ARG;
  }
  return BM_OK;
}

size_t ws_bytes_for(int mode, const RedPlan &p, int64_t nout) {
  if (p.nchunks <= 1) return 0;
  // var / std: + one plane of pivots
  return ((size_t)planes_of(mode) * (size_t)p.nchunks + (mode == M_MOM ? 1 : 0)) * (size_t)nout * 8;
}

// Shared body of bm_reduce / bm_reduce_state.
// P: row pitch in elements (rows reductions, I == 1); R for a dense input.
int run_reduce(int stat, const void *src, int dt, int64_t O, int64_t R, int64_t I, Sink sk,
               void *ws, size_t ws_bytes, hipStream_t st, const char *who, int64_t P) {
  const int mode = mode_of(stat, dt);
  const RedPlan p = plan_reduce(dt, O, R, I, src, P);
  const int64_t nout = O * I;
  if (p.nchunks <= 1) {
    int rc = launch_main(mode, dt, p, src, O, R, P, I, sk, st);
    if (rc) return rc;
    return check_launch(who);
  }
  const size_t need = ws_bytes_for(mode, p, nout);
  if (!ws || ws_bytes < need) {
    bm_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    return BM_E_WS;
  }
  double *w0 = (double *)ws;
  double *w1 = w0 + (size_t)p.nchunks * nout;
  Sink part = sk;
  part.final_out = 0;
  part.p0 = w0;
  part.p1 = w1;
  part.p2 = w1 + (size_t)p.nchunks * nout;  // var / std pivots (ws_bytes_for reserves the plane)
  part.shifted = mode == M_MOM;
  int rc = launch_main(mode, dt, p, src, O, R, P, I, part, st);
  if (rc) return rc;
  CombDesc cd{};
  cd.nout = nout;
  cd.nparts = p.nchunks;
  cd.part_stride = nout;
  cd.R = R;
  cd.rchunk = p.rchunk;
  cd.explicit_counts = 0;
  cd.int_sums = mode == M_MOM && !is_float(dt) && dtype_size(dt) <= 2;
  cd.pivots = mode == M_MOM && !cd.int_sums;
  rc = launch_combine(mode, dt, w0, w1, cd, sk, st);
  if (rc) return rc;
  return check_launch(who);
}

// The b-tile states of a moments transpose (bm_copy_strided_moments) -> the
// BM_STAT_VAR state of every row.  Part p holds three planes of nrows: the
// tile's pivot K (one of the row's values), mean - K and M2, over tb values
// (the last part: the rest of R).  chan over the parts in tile order, in the
// frame shifted by the first tile's pivot, as the rows kernel keeps its
// Welford state around the row's first element: K_p - K_0 is exact for offset
// data.  The pivots are finite (a tile whose first value is not takes 0), so
// an infinity or NaN of the row is in its tile's mean - K alone.  A row with
// an infinity has an infinite tile mean, which chan's delta turns into NaN
// when a finite tile follows; its mean is then the sum of the tile means
// (inf, or NaN for inf - inf or a NaN tile), what a sum over the row gives.
__global__ void __launch_bounds__(kThreads)
    k_red_merge_tiles(const double *__restrict__ parts, int64_t nparts, int64_t tb, int64_t R, int64_t nrows,
                      double *__restrict__ state) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < nrows; e += step) {
    const double K0 = parts[e];
    double n = 0.0, m = 0.0, q = 0.0;
    for (int64_t p = 0; p < nparts; ++p) {
      const double nb = (double)(min(R, (p + 1) * tb) - p * tb);
      const double *pp = parts + 3 * p * nrows + e;
      chan(n, m, q, nb, (pp[0] - K0) + pp[nrows], pp[2 * nrows], true);
    }
    m += K0;
    if (m != m) {
      double s = 0.0;
      for (int64_t p = 0; p < nparts; ++p) s += parts[3 * p * nrows + e] + parts[(3 * p + 1) * nrows + e];
      m = s;
    }
    state[e] = m;
    state[nrows + e] = m2_out(q, m);
  }
}

}  // namespace

int bm_merge_tile_moments(const double *parts, int64_t nparts, int64_t tb, int64_t R, int64_t nrows,
                          double *state, hipStream_t stream) {
  int64_t g = cdiv(nrows, kThreads);
  if (g > 4096) g = 4096;
  k_red_merge_tiles<<<(int)g, kThreads, 0, stream>>>(parts, nparts, tb, R, nrows, state);
  return check_launch("bm_copy_strided_moments");
}

extern "C" int bm_reduce_workspace_bytes(int stat, int in_dtype, int64_t O, int64_t R, int64_t I,
                                         size_t *bytes) {
  if (!bytes) { bm_set_error("bm_reduce_workspace_bytes: null out"); return BM_E_ARG; }
  int rc = check_args(stat, in_dtype, O, R, I, "bm_reduce_workspace_bytes");
  if (rc) return rc;
  // The plan depends on the pointer only through the vector width; reserve
  // for both the 16-B-aligned plan and the scalar (unaligned) plan.
  const int mode = mode_of(stat, in_dtype);
  const size_t a = ws_bytes_for(mode, plan_reduce(in_dtype, O, R, I, nullptr, R), O * I);
  const size_t b = ws_bytes_for(mode, plan_reduce(in_dtype, O, R, I, (const void *)1, R), O * I);
  *bytes = a > b ? a : b;
  return BM_OK;
}

namespace {
// bm_reduce / bm_reduce_rows: validation, then run_reduce into `out`.
int reduce_to_out(int stat, const void *src, int in_dtype, int64_t O, int64_t R, int64_t I, int64_t P,
                  void *out, int out_dtype, void *workspace, size_t workspace_bytes, void *stream,
                  const char *who) {
  int rc = check_args(stat, in_dtype, O, R, I, who);
  if (rc) return rc;
  if (!src || !out) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  const int mode = mode_of(stat, in_dtype);
  if (!out_dtype_ok(stat, mode, in_dtype, out_dtype)) {
    bm_set_error("%s: out_dtype %d does not fit stat %d on dtype %d (float for statistics and "
                 "float sums / products, bool for logical and / or, else the input dtype)",
                 who, out_dtype, stat, in_dtype);
    return BM_E_ARG;
  }
  if (is_float(in_dtype) && (mode == M_BAND || mode == M_BOR || mode == M_BXOR)) {
    bm_set_error("%s: bitwise reductions need an integer or bool dtype", who);
    return BM_E_ARG;
  }
  Sink sk{};
  sk.out = out;
  sk.out_dtype = out_dtype;
  sk.stat = stat;
  sk.final_out = 1;
  return run_reduce(stat, src, in_dtype, O, R, I, sk, workspace, workspace_bytes,
                    (hipStream_t)stream, who, P);
}
}  // namespace

extern "C" int bm_reduce(int stat, const void *src, int in_dtype, int64_t O, int64_t R, int64_t I,
                         void *out, int out_dtype, void *workspace, size_t workspace_bytes,
                         void *stream) {
  return reduce_to_out(stat, src, in_dtype, O, R, I, R, out, out_dtype, workspace, workspace_bytes,
                       stream, "bm_reduce");
}

extern "C" int bm_reduce_rows(int stat, const void *src, int in_dtype, int64_t O, int64_t R,
                              int64_t row_pitch, void *out, int out_dtype, void *workspace,
                              size_t workspace_bytes, void *stream) {
  if (row_pitch < R) {
    bm_set_error("bm_reduce_rows: row_pitch %lld < row length %lld", (long long)row_pitch, (long long)R);
    return BM_E_ARG;
  }
  return reduce_to_out(stat, src, in_dtype, O, R, 1, row_pitch, out, out_dtype, workspace, workspace_bytes,
                       stream, "bm_reduce_rows");
}

// mean, var and std of one pass: BM_STAT_VAR's plan, workspace and launches
// (plan_reduce does not look at the statistic), the last store writing every
// moment asked for instead of one.
extern "C" int bm_reduce_moments(const void *src, int in_dtype, int64_t O, int64_t R, int64_t I,
                                 int64_t row_pitch, void *out_mean, void *out_var, void *out_std,
                                 int out_dtype, void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "bm_reduce_moments";
  int rc = check_args(BM_STAT_VAR, in_dtype, O, R, I, who);
  if (rc) return rc;
  if (!src) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (!out_mean && !out_var && !out_std) {
    bm_set_error("%s: no output asked for (out_mean, out_var and out_std are all null)", who);
    return BM_E_ARG;
  }
  if (!is_float(out_dtype)) {
    bm_set_error("%s: out_dtype %d is not a float dtype", who, out_dtype);
    return BM_E_ARG;
  }
  if (row_pitch < R || (I > 1 && row_pitch != R)) {
    bm_set_error("%s: row_pitch %lld does not fit R=%lld, I=%lld (>= R, and R itself unless I == 1)", who,
                 (long long)row_pitch, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  Sink sk{};
  sk.out_dtype = out_dtype;
  sk.stat = BM_STAT_VAR;
  sk.final_out = kFinalMoments;
  sk.om = out_mean;
  sk.ov = out_var;
  sk.os = out_std;
  return run_reduce(BM_STAT_VAR, src, in_dtype, O, R, I, sk, workspace, workspace_bytes,
                    (hipStream_t)stream, who, row_pitch);
}

// bm_reduce / bm_reduce_rows of a mean, var or std whose one read also leaves
// the BM_STAT_VAR state behind.  var / std: the M_MOM kernels store the state
// they finalise; mean: the M_MEANMOM kernels run both accumulations.  Integer
// inputs and chunked plans (partials in a workspace, merged by the combine
// kernel) run the plain launches: *kept = 0.
extern "C" int bm_reduce_keep(int stat, const void *src, int in_dtype, int64_t O, int64_t R, int64_t I,
                              int64_t row_pitch, void *out, int out_dtype, void *state, int *kept,
                              void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "bm_reduce_keep";
  int rc = check_args(stat, in_dtype, O, R, I, who);
  if (rc) return rc;
  if (stat != BM_STAT_MEAN && stat != BM_STAT_VAR && stat != BM_STAT_STD) {
    bm_set_error("%s: stat %d is not mean, var or std", who, stat);
    return BM_E_ARG;
  }
  if (!src || !out || !state || !kept) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (!is_float(out_dtype)) {
    bm_set_error("%s: out_dtype %d is not a float dtype", who, out_dtype);
    return BM_E_ARG;
  }
  if (row_pitch < R || (I > 1 && row_pitch != R)) {
    bm_set_error("%s: row_pitch %lld does not fit R=%lld, I=%lld (>= R, and R itself unless I == 1)", who,
                 (long long)row_pitch, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  *kept = 0;
  Sink sk{};
  sk.out = out;
  sk.out_dtype = out_dtype;
  sk.stat = stat;
  sk.final_out = 1;
  const RedPlan p = plan_reduce(in_dtype, O, R, I, src, row_pitch);
  if (!is_float(in_dtype) || p.nchunks > 1)
    return run_reduce(stat, src, in_dtype, O, R, I, sk, workspace, workspace_bytes, (hipStream_t)stream, who,
                      row_pitch);
  sk.k0 = (double *)state;
  sk.k1 = (double *)state + O * I;
  if (stat == BM_STAT_MEAN) {
    rc = launch_keep_mean(in_dtype, p, src, O, R, row_pitch, I, sk, (hipStream_t)stream);
    if (!rc) rc = check_launch(who);
  } else {
    rc = run_reduce(stat, src, in_dtype, O, R, I, sk, workspace, workspace_bytes, (hipStream_t)stream, who,
                    row_pitch);
  }
  if (!rc) *kept = 1;
  return rc;
}

extern "C" int bm_reduce_state_bytes(int stat, int in_dtype, int64_t nout, size_t *bytes) {
  if (!bytes || nout < 0 || stat < BM_STAT_MEAN || stat > BM_STAT_FMIN || dtype_size(in_dtype) == 0) {
    bm_set_error("bm_reduce_state_bytes: bad arguments");
    return BM_E_ARG;
  }
  *bytes = (size_t)planes_of(mode_of(stat, in_dtype)) * (size_t)nout * 8;
  return BM_OK;
}

extern "C" int bm_reduce_state(int stat, const void *src, int in_dtype, int64_t O, int64_t R,
                               int64_t I, void *state, void *workspace, size_t workspace_bytes,
                               void *stream) {
  int rc = check_args(stat, in_dtype, O, R, I, "bm_reduce_state");
  if (rc) return rc;
  if (!src || !state) { bm_set_error("bm_reduce_state: null pointer"); return BM_E_ARG; }
  const int64_t nout = O * I;
  Sink sk{};
  sk.out = nullptr;
  sk.out_dtype = BM_F64;
  sk.stat = stat;
  sk.final_out = 0;
  sk.p0 = (double *)state;
  sk.p1 = (double *)state + nout;
  return run_reduce(stat, src, in_dtype, O, R, I, sk, workspace, workspace_bytes,
                    (hipStream_t)stream, "bm_reduce_state", R);
}

extern "C" int bm_reduce_combine(int stat, int in_dtype, const void *states, const int64_t *counts,
                                 int nparts, int64_t nout, void *out, int out_dtype, void *stream) {
  if (stat < BM_STAT_MEAN || stat > BM_STAT_FMIN || dtype_size(in_dtype) == 0 || nparts < 1 ||
      nparts > kMaxParts || nout < 1 || !states || !counts || !out) {
    bm_set_error("bm_reduce_combine: bad arguments");
    return BM_E_ARG;
  }
  const int mode = mode_of(stat, in_dtype);
  if (!out_dtype_ok(stat, mode, in_dtype, out_dtype)) {
    bm_set_error("bm_reduce_combine: out_dtype %d does not fit stat %d on dtype %d (float for statistics and "
                 "float sums / products, bool for logical and / or, else the input dtype)",
                 out_dtype, stat, in_dtype);
    return BM_E_ARG;
  }
  if (is_float(in_dtype) && (mode == M_BAND || mode == M_BOR || mode == M_BXOR)) {
    bm_set_error("bm_reduce_combine: bitwise reductions need an integer or bool dtype");
    return BM_E_ARG;
  }
  CombDesc cd{};
  cd.nout = nout;
  cd.nparts = nparts;
  cd.part_stride = (int64_t)planes_of(mode) * nout;
  cd.explicit_counts = 1;
  for (int p = 0; p < nparts; ++p) cd.counts[p] = counts[p];
  Sink sk{};
  sk.out = out;
  sk.out_dtype = out_dtype;
  sk.stat = stat;
  sk.final_out = 1;
  const double *p0 = (const double *)states;
  int rc = launch_combine(mode, in_dtype, p0, p0 + nout, cd, sk, (hipStream_t)stream);
  if (rc) return rc;
  return check_launch("bm_reduce_combine");
}

// bm_reduce_combine(BM_STAT_VAR, ...)'s merge, finalised into every moment asked for.
extern "C" int bm_reduce_combine_moments(int in_dtype, const void *states, const int64_t *counts, int nparts,
                                         int64_t nout, void *out_mean, void *out_var, void *out_std,
                                         int out_dtype, void *stream) {
  if (dtype_size(in_dtype) == 0 || nparts < 1 || nparts > kMaxParts || nout < 1 || !states || !counts ||
      (!out_mean && !out_var && !out_std)) {
    bm_set_error("bm_reduce_combine_moments: bad arguments");
    return BM_E_ARG;
  }
  if (!is_float(out_dtype)) {
    bm_set_error("bm_reduce_combine_moments: out_dtype %d is not a float dtype", out_dtype);
    return BM_E_ARG;
  }
  CombDesc cd{};
  cd.nout = nout;
  cd.nparts = nparts;
  cd.part_stride = (int64_t)planes_of(M_MOM) * nout;
  cd.explicit_counts = 1;
  for (int p = 0; p < nparts; ++p) cd.counts[p] = counts[p];
  Sink sk{};
  sk.out_dtype = out_dtype;
  sk.stat = BM_STAT_VAR;
  sk.final_out = kFinalMoments;
  sk.om = out_mean;
  sk.ov = out_var;
  sk.os = out_std;
  const double *p0 = (const double *)states;
  int rc = launch_combine(M_MOM, in_dtype, p0, p0 + nout, cd, sk, (hipStream_t)stream);
  if (rc) return rc;
  return check_launch("bm_reduce_combine_moments");
}

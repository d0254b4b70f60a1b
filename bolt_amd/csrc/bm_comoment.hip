// bm_comoment.hip -- cov / corr of libbolt_mi355x (gfx950): the co-moment of
// every record with up to BM_COMOMENT_MAX_SIGNALS fixed signals along an axis.
//
// No reference call site: the reference has no such method (an API addition,
// like stats() and center() / zscore()).  The state extends the StatCounter
// (n, mu, m2: bolt/spark/statcounter.py:30-48) by one co-moment per signal,
// and bm_comoment_combine extends its merge (statcounter.py:67-99).
//
// The result is K values per record, so the floor is one read of the array:
//   rows kernel (I == 1, rows dense or padded): one wave per (row, chunk of at
//     most kRowsChunk elements), 16-B non-temporal loads over whole wave-wide
//     steps, blocks in rows_block() order.  The waves of a block (four; eight
//     with four signals) take the same chunk of different rows and walk up to kRowsWalk rows each: the
//     block stages its chunk of the centred signals in LDS once (float64,
//     16 KiB per signal) and every row reads it from there, so the signal
//     costs one L2 read per 32 or 64 rows and no second HBM stream.
//     Staging through LDS at every K * R, rather than registers for rows that
//     fit or plain cached loads for short signals, is UNMEASURED: the rule was
//     set from the register budget (a wave holding a 2000-element float64
//     signal takes 64 VGPRs per signal) and no A/B run has compared the three.
//     kRowsChunk, kRowsWalk and kRowsUnroll are UNMEASURED too.  MEASURED
//     (profiles/comoment_ab.log, C2's padded rows, the state launch alone):
//     one signal 0.331 ms against std()'s 0.330; four signals 0.803 ms with
//     four waves a block (their 64 KiB image held a CU to 2 waves / SIMD),
//     0.465 ms with eight (rows_waves).
//   columns kernel (I > 1): lanes own adjacent column vectors as k_red_cols'
//     do, 256 / tcv row phases per block; y[r] is wave-uniform when a phase
//     is a whole wave (tcv == 64: one scalar load per row and signal), else a
//     same-address cached load.  R is split into chunks over blockIdx.y when
//     O * column tiles alone give fewer than kColsBlocks blocks; the blocks the
//     hardware deals to one XCD take consecutive column tiles (xcd_block).
//     Rows in flight per lane: kColsUnroll, half of it with four signals (with
//     4 rows their scalar y values spilled 7-9 SGPRs); C2's columns MEASURED
//     at 0.365 ms (one signal) / 0.375 ms (four) against std()'s 0.394.
// Numerics (all float64): every record is summed around its first element P,
//   which all chunks and row phases of the record share, against the signal
//   centred by the caller's mean: S1 = sum(x - P), S2 = sum (x - P)^2,
//   Sxy_k = sum (x - P)(y_k - ymean_k).  Sums about one pivot simply add, so
//   lanes fold in lane order (wave_fold), row phases in phase order, chunks in
//   chunk order, and no division is taken before the end:
//     mean = P + S1 / n,  M2 = S2 - S1^2 / n,
//     C_k = Sxy_k - (S1 / n) * yresid_k,  yresid_k = sum_r (y_k[r] - ymean_k)
//   (the last term removes the rounding of ymean).  P is one of the record's
//   values, so (mean - P)^2 <= n var and S2 / M2 <= 1 + n: an outlier in first
//   place or a ramp loses log2(n) bits of M2 at most, inside the 1e-12 budget
//   for n up to 1e7.  Every signal's sums are its own and take the same order
//   whatever K is (explicit fma, no contraction across signals): plane k of a
//   K-signal call has the bits of the one-signal call.  No float atomics.
//   Non-finite records are numpy's: the pivot is finite -- a first element that
//   is an infinity or a NaN takes 0 (finite_or_zero, as in bm_reduce.hip) -- so
//   the mean plane is what a sum over the record gives (+inf, -inf, or NaN for
//   inf - inf or a NaN) wherever the value sits, and M2 = inf - inf = NaN
//   exactly when the record holds such a value.  Sxy - (S1 / n) * yresid is
//   then +-inf or NaN by the sign of a rounding residue, so store_sums makes
//   every co-moment NaN where M2 came out NaN: one compare and select per
//   output; finite records keep their bits.  k_co_combine needs no more: a NaN
//   M2 or C of any part reaches the merged values through its fmas.
#include "bm_common.h"
#include "bm_host.h"
#include "bm_wave.h"
#include "../../include/bolt_mi355x.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int KMAX = BM_COMOMENT_MAX_SIGNALS;
constexpr int kMaxParts = BM_COMOMENT_MAX_PARTS;  // parts per bm_comoment_combine: the merge tables are kernel arguments
constexpr int kMaxVec = 8;      // elements per vector at most, as bm_standardize.hip
// rows: elements of a row per chunk (the LDS image of one signal: 16 KiB), rows
// a wave walks per staged chunk at most, 16-B vectors in flight per lane
constexpr int64_t kRowsChunk = 2048;
constexpr int kRowsWalk = 8;
constexpr int kRowsUnroll = 2;
// waves of a rows block: four signals' image is 64 KiB, so eight waves share it
// (two blocks a CU: 16 waves; with four waves a block the LDS held a CU to 8)
constexpr int rows_waves(int KT) { return KT > 2 ? 8 : 4; }
// columns: blocks wanted before R is left whole, threads across column vectors, rows in flight per lane
constexpr int64_t kColsBlocks = 2048;
constexpr int kColsTcv = 64;
constexpr int kColsUnroll = 4;

// the signals' host statistics, kernel arguments
struct YStat {
  double mean[KMAX];   // what the signal is centred by
  double resid[KMAX];  // sum_r (y[r] - mean): the rounding residue of the mean
};

// the sums of one record (or one chunk of it) -> its state, or its partial
// record [P, S1, S2, Sxy_0..] in the workspace when R is split into chunks
template <int KT>
__device__ __forceinline__ void store_sums(double *__restrict__ state, double *__restrict__ part, int64_t nout,
                                           int64_t e, int64_t c, int64_t nchunks, int K, double n, double P,
                                           double s1, double s2, const double (&sxy)[KT], const YStat &ys) {
  if (nchunks > 1) {
    double *p = part + c * (3 + K) * nout + e;
    p[0] = P;
    p[nout] = s1;
    p[2 * nout] = s2;
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) p[(3 + k) * nout] = sxy[k];
    return;
  }
  const double dm = s1 / n;
  const double m2 = fma(-s1, dm, s2);
  state[e] = P + dm;  // (P is finite: an infinite S1 gives the sum's mean)
  state[nout + e] = m2 < 0.0 ? 0.0 : m2;  // (a nan stays a nan)
  // a record holding a nan or an infinity: M2 is nan (inf - inf), and so is every
  // co-moment, whatever Sxy - inf * resid came to; finite records keep their bits
  const bool spoilt = m2 != m2;
#pragma unroll
  for (int k = 0; k < KT; ++k)
    if (k < K) state[(2 + k) * nout + e] = spoilt ? m2 : fma(-dm, ys.resid[k], sxy[k]);
}

// VEC float64 values from LDS, 16 B at a time where the vector allows
template <int VEC> __device__ __forceinline__ void lds_read(const double *p, double (&o)[VEC]) {
  if constexpr (VEC == 1) {
    o[0] = p[0];
  } else {
    typedef double d2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < VEC; i += 2) {
      const d2 v = *reinterpret_cast<const d2 *>(p + i);
      o[i] = v.x;
      o[i + 1] = v.y;
    }
  }
}

// ------------------------------------------------------------------ rows --
struct RowsDesc {
  int64_t O, R;
  int64_t P;        // elements between row starts (R, or a padded row pitch >= R)
  int64_t nchunks;  // chunks of kRowsChunk elements per row
  FastDiv fchunks;
  int64_t nitems;   // row groups * nchunks
  int64_t item0;    // first item of this launch (launches split at the grid limit)
  int32_t walk;     // rows per wave
  int32_t K;
};

// R % VEC == 0 and P % VEC == 0 (the host's pick), so every chunk is whole vectors
template <typename T, int VEC, int KT>
__global__ void __launch_bounds__(64 * rows_waves(KT))
    k_co_rows(const T *__restrict__ src, const double *__restrict__ y, RowsDesc d, YStat ys,
              double *__restrict__ state, double *__restrict__ part) {
  __shared__ double sy[KT * kRowsChunk];
  constexpr int kW = rows_waves(KT);  // waves of this block
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t item = d.item0 + (int64_t)rows_block();
  // (the grid holds no block past nitems: every thread reaches the barrier)
  const uint64_t g = fd_div((uint64_t)item, d.fchunks);
  const int64_t c = item - (int64_t)g * d.nchunks;
  const int64_t r_lo = c * kRowsChunk;
  const int64_t len = min(d.R - r_lo, kRowsChunk);
  // the block's chunk of the centred signals (planes past K: zeros, their sums are not stored)
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    for (int64_t i = threadIdx.x; i < len; i += 64 * kW)
      sy[k * kRowsChunk + i] = k < d.K ? y[(int64_t)k * d.R + r_lo + i] - ys.mean[k] : 0.0;
  }
  __syncthreads();  // the only barrier: waves leave on their own below

  constexpr int64_t stride = 64 * VEC;
  constexpr int64_t step = kRowsUnroll * stride;
  const int64_t main_end = len / step * step;
  const int64_t rpb = (int64_t)kW * d.walk;
  for (int w = 0; w < d.walk; ++w) {
    // at any time the block's waves read neighbouring rows
    const int64_t row = (int64_t)g * rpb + (int64_t)w * kW + wave;
    if (row >= d.O) return;
    const T *base = src + row * d.P;
    const T *s = base + r_lo;
    const double P = finite_or_zero(to_f64(base[0]));
    double s1 = 0.0, s2 = 0.0, sxy[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) sxy[k] = 0.0;
    int64_t j = (int64_t)lane * VEC;
    // kRowsUnroll vectors in flight per lane over whole wave-wide steps (every
    // lane runs the same iterations: no 128-B line is split between a main-loop
    // load and a tail load, as in k_red_rows)
    for (; j < main_end; j += step) {
      T v[kRowsUnroll][VEC];
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u) vload_nt<T, VEC>(s + j + u * stride, v[u]);
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u) {
        double dx[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          dx[i] = to_f64(v[u][i]) - P;
          s1 += dx[i];
          s2 = fma(dx[i], dx[i], s2);
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          double yv[VEC];
          lds_read<VEC>(sy + k * kRowsChunk + j + u * stride, yv);
#pragma unroll
          for (int i = 0; i < VEC; ++i) sxy[k] = fma(dx[i], yv[i], sxy[k]);
        }
      }
    }
    for (; j < len; j += stride) {  // j + VEC <= len: the chunk is whole vectors
      T v[VEC];
      vload_nt<T, VEC>(s + j, v);
      double dx[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        dx[i] = to_f64(v[i]) - P;
        s1 += dx[i];
        s2 = fma(dx[i], dx[i], s2);
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        double yv[VEC];
        lds_read<VEC>(sy + k * kRowsChunk + j, yv);
#pragma unroll
        for (int i = 0; i < VEC; ++i) sxy[k] = fma(dx[i], yv[i], sxy[k]);
      }
    }
    // the 64 lanes in lane order, into lane 63
    const auto add = [](double a, double b) { return a + b; };
    s1 = wave_fold(s1, lane, add);
    s2 = wave_fold(s2, lane, add);
#pragma unroll
    for (int k = 0; k < KT; ++k) sxy[k] = wave_fold(sxy[k], lane, add);
    if (lane == kFoldLane)
      store_sums<KT>(state, part, d.O, row, c, d.nchunks, d.K, (double)d.R, P, s1, s2, sxy, ys);
  }
}

// ------------------------------------------------------------------ cols --
// (the XCD-aware block order, xcd_block, is in bm_wave.h)
struct ColsDesc {
  int64_t O, R, I;
  int64_t rchunk, nchunks;
  int32_t tcv;    // threads across column vectors (power of two <= 64)
  int32_t nph;    // row phases = 256 / tcv
  FastDiv ntc;    // column tiles per O
  int64_t tile0;  // first (o, column tile) of this launch
  int32_t K;
};

// rows r0, r0 + nph, ... < r_hi of one column vector.  UNI: r0 is the same in
// every lane of the wave (a phase is a whole wave), so y[r] is a scalar load.
template <typename T, int VEC, int KT, bool UNI>
__device__ __forceinline__ void cols_sums(const T *__restrict__ base, const double *__restrict__ y, const ColsDesc &d,
                                          const YStat &ys, int64_t r0, int64_t r_hi, const double (&P)[VEC],
                                          double (&s1)[VEC], double (&s2)[VEC], double (&sxy)[KT][VEC]) {
  int64_t r = r0;
  if constexpr (UNI) r = ((int64_t)__builtin_amdgcn_readfirstlane((int)(r0 >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)r0);
  const int64_t nph = d.nph;
  // rows in flight per lane: fewer with four signals, whose scalar y values fill the scalar registers
  constexpr int U = KT > 2 ? kColsUnroll / 2 : kColsUnroll;
  for (; r + (U - 1) * nph < r_hi; r += U * nph) {
    T v[U][VEC];
    double yc[U][KT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      vload_nt<T, VEC>(base + (r + u * nph) * d.I, v[u]);
#pragma unroll
      for (int k = 0; k < KT; ++k) yc[u][k] = k < d.K ? y[(int64_t)k * d.R + r + u * nph] - ys.mean[k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {  // each column's sums take its rows in order
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double dx = to_f64(v[u][i]) - P[i];
        s1[i] += dx;
        s2[i] = fma(dx, dx, s2[i]);
#pragma unroll
        for (int k = 0; k < KT; ++k) sxy[k][i] = fma(dx, yc[u][k], sxy[k][i]);
      }
    }
  }
  for (; r < r_hi; r += nph) {
    T v[VEC];
    vload_nt<T, VEC>(base + r * d.I, v);
    double yc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) yc[k] = k < d.K ? y[(int64_t)k * d.R + r] - ys.mean[k] : 0.0;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const double dx = to_f64(v[i]) - P[i];
      s1[i] += dx;
      s2[i] = fma(dx, dx, s2[i]);
#pragma unroll
      for (int k = 0; k < KT; ++k) sxy[k][i] = fma(dx, yc[k], sxy[k][i]);
    }
  }
}

// the block's row phases of one plane, summed into phase 0 in phase order
template <int VEC>
__device__ __forceinline__ void phase_sum(double *sm, const ColsDesc &d, int ph, int cv, double (&a)[VEC]) {
  __syncthreads();  // sm is free again
#pragma unroll
  for (int i = 0; i < VEC; ++i) sm[threadIdx.x * VEC + i] = a[i];
  __syncthreads();
  if (ph == 0) {
    for (int p = 1; p < d.nph; ++p) {
      const int other = p * d.tcv + cv;
#pragma unroll
      for (int i = 0; i < VEC; ++i) a[i] += sm[other * VEC + i];
    }
  }
}

template <typename T, int VEC, int KT>
__global__ void __launch_bounds__(kThreads)
    k_co_cols(const T *__restrict__ src, const double *__restrict__ y, ColsDesc d, YStat ys,
              double *__restrict__ state, double *__restrict__ part) {
  __shared__ double sm[kThreads * VEC];
  const uint64_t ot = (uint64_t)d.tile0 + xcd_block();
  const uint64_t o = fd_div(ot, d.ntc);
  const uint64_t tc = ot - o * d.ntc.d;
  const int64_t c = blockIdx.y;
  const int64_t r_lo = c * d.rchunk;
  const int64_t r_hi = min(d.R, r_lo + d.rchunk);
  const int cv = threadIdx.x % d.tcv;
  const int ph = threadIdx.x / d.tcv;
  const int64_t col0 = ((int64_t)tc * d.tcv + cv) * VEC;
  const bool active = col0 < d.I;  // I % VEC == 0: a whole vector inside the row

  double P[VEC], s1[VEC], s2[VEC], sxy[KT][VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    P[i] = 0.0; s1[i] = 0.0; s2[i] = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) sxy[k][i] = 0.0;
  }
  if (active) {
    const T *base = src + ((int64_t)o * d.R) * d.I + col0;
    T p0[VEC];
    vload<T, VEC>(base, p0);  // the pivot: the column's element in row 0, shared by chunks and phases
#pragma unroll
    for (int i = 0; i < VEC; ++i) P[i] = finite_or_zero(to_f64(p0[i]));
    if (d.tcv == 64)
      cols_sums<T, VEC, KT, true>(base, y, d, ys, r_lo + ph, r_hi, P, s1, s2, sxy);
    else
      cols_sums<T, VEC, KT, false>(base, y, d, ys, r_lo + ph, r_hi, P, s1, s2, sxy);
  }
  if (d.nph > 1) {  // (uniform: every thread takes the barriers)
    phase_sum<VEC>(sm, d, ph, cv, s1);
    phase_sum<VEC>(sm, d, ph, cv, s2);
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < d.K) phase_sum<VEC>(sm, d, ph, cv, sxy[k]);
  }
  if (ph != 0 || !active) return;
  const int64_t nout = d.O * d.I;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    double sk[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) sk[k] = sxy[k][i];
    store_sums<KT>(state, part, nout, (int64_t)o * d.I + col0 + i, c, d.nchunks, d.K, (double)d.R, P[i], s1[i],
                   s2[i], sk, ys);
  }
}

// ----------------------------------------------------------------- merge --
// the chunks' partial records of every output, summed in chunk order (they
// share the pivot), into the state
struct MergeDesc {
  int64_t nout, nchunks;
  double n;
  int32_t K;
};

__global__ void __launch_bounds__(kThreads)
    k_co_merge(const double *__restrict__ part, MergeDesc d, YStat ys, double *__restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= d.nout) return;
  const int64_t rec = (3 + d.K) * d.nout;
  const double P = part[e];
  double s1 = 0.0, s2 = 0.0, sxy[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) sxy[k] = 0.0;
  for (int64_t c = 0; c < d.nchunks; ++c) {
    const double *p = part + c * rec + e;
    s1 += p[d.nout];
    s2 += p[2 * d.nout];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < d.K) sxy[k] += p[(3 + k) * d.nout];
  }
  store_sums<KMAX>(state, nullptr, d.nout, e, 0, 1, d.K, d.n, P, s1, s2, sxy, ys);
}

// --------------------------------------------------------------- combine --
struct CombDesc {
  int64_t nout;
  int32_t nparts, K, what, pad_;
  int64_t counts[kMaxParts];
  double w[kMaxParts * 2];  // [part][k]: (ymean_b - ymean_a) na nb / (na + nb) of the part's merge
  double m2y[KMAX];         // the merged signals' sums of squared deviations
};

template <typename OT>
__global__ void __launch_bounds__(kThreads)
    k_co_combine(const double *__restrict__ states, CombDesc d, OT *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= d.nout) return;
  const int64_t stride = (int64_t)(2 + d.K) * d.nout;
  double n = 0.0, m = 0.0, q = 0.0, C[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) C[k] = 0.0;
  for (int p = 0; p < d.nparts; ++p) {
    const double cb = (double)d.counts[p];
    if (cb <= 0.0) continue;
    const double *s = states + (int64_t)p * stride + e;
    const double mb = s[0], qb = s[d.nout];
    if (n == 0.0) {
      n = cb; m = mb; q = qb;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < d.K) C[k] = s[(2 + k) * d.nout];
      continue;
    }
    const double tot = n + cb;
    const double dl = mb - m;
    m = fma(dl, cb / tot, m);
    q = fma(dl * dl, n * cb / tot, q + qb);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < d.K) C[k] = fma(dl, d.w[p * d.K + k], C[k] + s[(2 + k) * d.nout]);
    n = tot;
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < d.K) {
      double v;
      if (n == 0.0) {
        v = __builtin_nan("");
      } else if (d.what == BM_CO_COV) {
        v = C[k] / n;
      } else {
        // a record or a signal without variance has no correlation: nan, also
        // where rounding left a C != 0 beside an M2 clamped to 0 (a nan M2 fails
        // the test and gives nan too)
        const double den = q * d.m2y[k];
        v = den > 0.0 ? C[k] / sqrt(den) : __builtin_nan("");
        v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);  // (a nan stays a nan)
      }
      out[(int64_t)k * d.nout + e] = (OT)v;
    }
  }
}

// ------------------------------------------------------------------ host --
struct CoPlan {
  bool rows;
  int vec;
  int64_t rchunk, nchunks;
  int32_t tcv, nph, walk;
  int64_t ntc;
};

// src == nullptr: the workspace query.  The chunk counts, and so the
// workspace, do not depend on the pointer (rows: kRowsChunk; columns: below).
CoPlan plan_comoment(int dt, int64_t O, int64_t R, int64_t I, const void *src, int64_t P) {
  CoPlan p{};
  const int es = dtype_size(dt);
  const int cap = std::min(16 / es, kMaxVec);
  if (I == 1) {
    p.rows = true;
    p.vec = pick_vec(cap, {R, P}, {{src, es}});
    p.rchunk = kRowsChunk;
    p.nchunks = cdiv(R, kRowsChunk);
    // rows per wave: up to kRowsWalk, while the device still gets 2048 blocks
    p.walk = (int32_t)std::min<int64_t>(kRowsWalk, std::max<int64_t>(1, O * p.nchunks / (kWaves * 2048)));
  } else {
    p.rows = false;
    // the chunks of R are planned for the widest vector I allows, whatever
    // the pointer allows: the workspace (sized without the pointer) and the
    // order of the chunk sums do not depend on the source's alignment
    int64_t nch = 1;
    {
      const int64_t ncolv = I / pick_vec(cap, {I}, {});
      int tcv = 1;
      while (tcv < kColsTcv && tcv < ncolv) tcv <<= 1;
      const int64_t blocks = O * cdiv(ncolv, tcv);
      if (blocks < kColsBlocks) {
        nch = cdiv(kColsBlocks, blocks);
        nch = std::min(nch, std::max<int64_t>(1, R / ((int64_t)(kThreads / tcv) * 8)));
      }
      nch = std::min<int64_t>(nch, 65535);
    }
    p.vec = pick_vec(cap, {I}, {{src, es}});
    const int64_t ncolv = I / p.vec;
    int tcv = 1;
    while (tcv < kColsTcv && tcv < ncolv) tcv <<= 1;
    p.tcv = tcv;
    p.nph = kThreads / tcv;
    p.ntc = cdiv(ncolv, tcv);
    p.rchunk = cdiv(R, nch);
    p.nchunks = cdiv(R, p.rchunk);
  }
  return p;
}

size_t part_bytes(const CoPlan &p, int64_t nout, int K) {
  return p.nchunks > 1 ? (size_t)p.nchunks * (size_t)(3 + K) * (size_t)nout * 8 : 0;
}

template <typename T, int VEC, int KT>
void launch_v(const CoPlan &p, const void *src, const double *y, int64_t O, int64_t R, int64_t P, int64_t I, int K,
              const YStat &ys, double *state, double *part, hipStream_t st) {
  const T *s = (const T *)src;
  if (p.rows) {
    RowsDesc d{};
    d.O = O; d.R = R; d.P = P; d.nchunks = p.nchunks; d.walk = p.walk; d.K = K;
    d.fchunks = make_fastdiv((uint64_t)p.nchunks);
    constexpr int kW = rows_waves(KT);
    d.nitems = cdiv(O, (int64_t)kW * p.walk) * p.nchunks;
    for_block_runs(d.nitems, 64 * kW, [&](int64_t b0, int g) {
      d.item0 = b0;
      k_co_rows<T, VEC, KT><<<g, 64 * kW, 0, st>>>(s, y, d, ys, state, part);
    });
  } else {
    ColsDesc d{};
    d.O = O; d.R = R; d.I = I; d.rchunk = p.rchunk; d.nchunks = p.nchunks; d.tcv = p.tcv; d.nph = p.nph; d.K = K;
    d.ntc = make_fastdiv((uint64_t)p.ntc);
    for_tile_runs(O * p.ntc, p.nchunks, kThreads, [&](int64_t t0, dim3 grid) {
      d.tile0 = t0;
      k_co_cols<T, VEC, KT><<<grid, kThreads, 0, st>>>(s, y, d, ys, state, part);
    });
  }
}

// the kernels are built for 1, 2 and 4 signals; 3 run as 4 with a plane of zeros
template <typename T, int VEC, typename... A> void launch_k(int K, A... a) {
  if (K == 1) launch_v<T, VEC, 1>(a...);
  else if (K == 2) launch_v<T, VEC, 2>(a...);
  else launch_v<T, VEC, 4>(a...);
}

int check_layout(const char *who, int in_dtype, int64_t O, int64_t R, int64_t I, int K) {
  if (dtype_size(in_dtype) == 0) {
    bm_set_error("%s: bad dtype %d", who, in_dtype);
    return BM_E_ARG;
  }
  if (O < 0 || R < 0 || I < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld I=%lld)", who, (long long)O, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  if (K < 1 || K > KMAX) {
    bm_set_error("%s: K=%d signals, not 1..%d", who, K, KMAX);
    return BM_E_ARG;
  }
  return BM_OK;
}

}  // namespace

extern "C" int bm_comoment_workspace_bytes(int in_dtype, int64_t O, int64_t R, int64_t I, int K, size_t *bytes) {
  const char *who = "bm_comoment_workspace_bytes";
  if (!bytes) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_layout(who, in_dtype, O, R, I, K);
  if (rc) return rc;
  *bytes = 0;
  if (O == 0 || R == 0 || I == 0) return BM_OK;
  *bytes = part_bytes(plan_comoment(in_dtype, O, R, I, nullptr, R), O * I, K);
  return BM_OK;
}

extern "C" int bm_comoment_state(const void *src, int in_dtype, int64_t O, int64_t R, int64_t I, int64_t row_pitch,
                                 const double *y, const double *ymean, const double *yresid, int K, void *state,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "bm_comoment_state";
  if (!src || !y || !ymean || !state) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  int rc = check_layout(who, in_dtype, O, R, I, K);
  if (rc) return rc;
  if (row_pitch < R || (I > 1 && row_pitch != R)) {
    bm_set_error("%s: pitch %lld does not fit R=%lld, I=%lld (>= R, and R itself unless I == 1)", who,
                 (long long)row_pitch, (long long)R, (long long)I);
    return BM_E_ARG;
  }
  if (O == 0 || R == 0 || I == 0) return BM_OK;  // nothing to store
  const CoPlan p = plan_comoment(in_dtype, O, R, I, src, row_pitch);
  const int64_t nout = O * I;
  const size_t need = part_bytes(p, nout, K);
  if (need > workspace_bytes || (need && !workspace)) {
    bm_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
    return BM_E_WS;
  }
  if (p.nchunks > 1 && cdiv(nout, kThreads) > max_blocks(kThreads)) {
    bm_set_error("%s: %lld outputs of a chunked reduction exceed one launch", who, (long long)nout);
    return BM_E_ARG;
  }
  YStat ys{};
  for (int k = 0; k < K; ++k) {
    ys.mean[k] = ymean[k];
    ys.resid[k] = yresid ? yresid[k] : 0.0;
  }
  hipStream_t st = (hipStream_t)stream;
  for_dtype(in_dtype, [&](auto t) {  // (a dtype code: check_layout)
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVec>(p.vec, [&](auto v) {
      launch_k<T, decltype(v)::value>(K, p, src, y, O, R, row_pitch, I, K, ys, (double *)state, (double *)workspace,
                                      st);
    });
  });
  if (p.nchunks > 1) {
    MergeDesc m{};
    m.nout = nout; m.nchunks = p.nchunks; m.n = (double)R; m.K = K;
    k_co_merge<<<(int)cdiv(nout, kThreads), kThreads, 0, st>>>((const double *)workspace, m, ys, (double *)state);
  }
  return check_launch(who);
}

extern "C" int bm_comoment_combine(int what, const void *states, const int64_t *counts, const double *ymean,
                                   const double *ym2, int nparts, int64_t nout, int K, void *out, int out_dtype,
                                   void *stream) {
  const char *who = "bm_comoment_combine";
  if (!states || !counts || !ymean || !ym2 || !out) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (what != BM_CO_COV && what != BM_CO_CORR) {
    bm_set_error("%s: what=%d is neither BM_CO_COV nor BM_CO_CORR", who, what);
    return BM_E_ARG;
  }
  if (out_dtype != BM_F16 && out_dtype != BM_F32 && out_dtype != BM_F64) {
    bm_set_error("%s: out_dtype %d is not a statistics dtype (float16, float32 or float64)", who, out_dtype);
    return BM_E_ARG;
  }
  if (K < 1 || K > KMAX) { bm_set_error("%s: K=%d signals, not 1..%d", who, K, KMAX); return BM_E_ARG; }
  if (nparts < 1 || nparts > kMaxParts || nparts * K > 2 * kMaxParts) {
    bm_set_error("%s: %d parts of %d signals (at most %d parts and %d part signals)", who, nparts, K, kMaxParts,
                 2 * kMaxParts);
    return BM_E_ARG;
  }
  if (nout < 0) { bm_set_error("%s: negative extent (nout=%lld)", who, (long long)nout); return BM_E_ARG; }
  for (int p = 0; p < nparts; ++p)
    if (counts[p] < 0) { bm_set_error("%s: negative count of part %d", who, p); return BM_E_ARG; }
  if (nout == 0) return BM_OK;  // nothing to store
  CombDesc d{};
  d.nout = nout; d.nparts = nparts; d.K = K; d.what = what;
  // the signals' side of the merge is the same for every output: done here
  double n = 0.0, ym[KMAX] = {0.0}, yq[KMAX] = {0.0};
  for (int p = 0; p < nparts; ++p) {
    d.counts[p] = counts[p];
    const double cb = (double)counts[p];
    if (cb <= 0.0) continue;
    if (n == 0.0) {
      n = cb;
      for (int k = 0; k < K; ++k) { ym[k] = ymean[p * K + k]; yq[k] = ym2[p * K + k]; }
      continue;
    }
    const double tot = n + cb;
    for (int k = 0; k < K; ++k) {
      const double dl = ymean[p * K + k] - ym[k];
      d.w[p * K + k] = dl * (n * cb / tot);
      ym[k] = std::fma(dl, cb / tot, ym[k]);
      yq[k] = std::fma(dl * dl, n * cb / tot, yq[k] + ym2[p * K + k]);
    }
    n = tot;
  }
  for (int k = 0; k < K; ++k) d.m2y[k] = yq[k];
  const int64_t blocks = cdiv(nout, kThreads);
  if (blocks > max_blocks(kThreads)) { bm_set_error("%s: %lld outputs exceed one launch", who, (long long)nout); return BM_E_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const double *s = (const double *)states;
  if (out_dtype == BM_F16) k_co_combine<_Float16><<<(int)blocks, kThreads, 0, st>>>(s, d, (_Float16 *)out);
  else if (out_dtype == BM_F32) k_co_combine<float><<<(int)blocks, kThreads, 0, st>>>(s, d, (float *)out);
  else k_co_combine<double><<<(int)blocks, kThreads, 0, st>>>(s, d, (double *)out);
  return check_launch(who);
}

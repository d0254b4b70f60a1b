// bm_quantile.hip -- quantile / percentile / median of libbolt_mi355x (gfx950):
// exact order statistics of every row, up to BM_QUANTILE_MAX_RANKS ranks a launch.
//
// No reference call site: the reference has no such method (an API addition,
// like stats(), center() / zscore() and cov() / corr()).
//
// An order statistic is one of the row's own values, so nothing is summed:
// both paths select by rank on order-preserving unsigned keys of the element's
// width -- floats: all bits flipped if the sign is set, else the sign bit set
// (IEEE order, -0.0 before +0.0); signed integers: the sign bit flipped --
// and decode the selected key back to the element.  The kernels are built per
// element width; the element's kind (float, signed, unsigned) reaches them as
// the two masks a value is xor-ed with (KeyMask), kernel arguments.
//   rows kernel (the hot path): the row is loaded once, non-temporally, into
//     registers as keys -- one wave per row, or the four waves of a block for
//     longer rows, k_std_rows' lane_vecs budget -- and every rank is found by a
//     binary search over the key's bits from the top: candidate = prefix | bit,
//     count the row's keys below the candidate, keep the bit if the count is
//     at most the rank.  The count is ballot + population count per held slot:
//     the compare writes a lane mask, the sum lives in scalar registers (no
//     per-lane adds and no DPP fold).  MEASURED against per-lane counts summed
//     by one ballot per bit (-DBM_Q_LANESUM) on C2's padded rows, three rounds
//     of processes in turn (profiles/quantile_lanesum_ab.log): median 1.594
//     against 1.540 ms, three percentiles 3.821 against 3.976 ms -- 3-4 % either
//     way, no winner; the ballot form stays.  Slots past the row's end carry a
//     predicate; the search itself does not need it (they hold the all-ones
//     key, which is below no candidate, as a legal all-ones element is not),
//     the step to the next rank does.  Given the key lo of rank r, the key of
//     rank r + 1 is lo if more than r + 1 keys are at most lo, else the
//     smallest key above lo: one counted pass, no second search.  Block per
//     row: per-wave counts meet in LDS, one barrier an iteration.
//   streaming kernels (rows the registers cannot hold, or too few long rows
//     for a block each): a most-significant-byte-first radix select,
//     sizeof(element) passes.  k_q_hist reads a slice of a row and adds, for
//     every searched rank whose prefix the key matches, to a 256-bin LDS
//     histogram, flushed to a global 64-bit histogram with integer atomics
//     (deterministic); k_q_pick scans the 256 bins per (row, rank), extends
//     the prefix and reduces the remaining rank.  After the last pass the
//     prefix is the key.  The first pass has one histogram per row, shared by
//     its ranks (their prefixes are all empty).
// Both: a row holding a NaN gives NaN in every output.  The interpolation
//   lo + (hi - lo) * frac runs over the selected values only, in float64,
//   three separately rounded operations (contraction is off in this file), in
//   the rows kernel's epilogue and in k_q_finish.
// Cost: one read of the array (rows), sizeof(element) reads (streaming), no
//   write but the planes.
// bm_normalize_rows (normalize(): (x - b) / (b + offset) against a percentile
//   baseline b) lives here too: k_norm_rows is the rows kernel for one
//   quantile with a second half -- the keys are invertible, so the held row
//   is decoded, normalised in float64 and stored: one read, one write.  Its
//   mean baseline is k_std_rows' (bm_standardize.hip), mode 2.
#include "bm_common.h"
#include "bm_host.h"
#include "bm_wave.h"
#include "../../include/bolt_mi355x.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int QMAX = BM_QUANTILE_MAX_RANKS;
constexpr int kMaxVec = 8;  // elements per vector at most, as bm_standardize.hip
// Plan of bm_quantile_rows: k_std_rows' (bm_standardize.hip).  A thread holds
// lane_vecs(vec) vectors = min(8 * vec, 32) elements; wave per row up to 64 *
// that, block per row up to 256 * that and only with kBlockMinRows rows or
// more.  All UNMEASURED: set from the register budget, not from A/B runs.
constexpr int lane_vecs(int vec) { return vec * 8 <= 32 ? 8 : 32 / vec; }
constexpr int64_t kBlockMinRows = 256;
// Streaming plan, UNMEASURED too: rows per batch (bounds the histograms: 16 KiB
// a row at eight ranks), blocks wanted per batch so that one long row still
// fills the device, and the shortest slice of a row a block takes.
constexpr int64_t kStreamRows = 2048;
constexpr int64_t kStreamBlocks = 2048;
constexpr int64_t kSliceMin = 4096;
constexpr int64_t kSliceMax = (int64_t)1 << 30;  // the LDS bins are 32-bit

// -DBM_Q_LANESUM (a variant build for A/B runs, Makefile EXTRA): the rows
// kernel's search counts per lane (compare + add in the VALU) and sums the
// lanes' six-bit counts with one ballot per bit, instead of one ballot and
// population count per held slot
#ifdef BM_Q_LANESUM
constexpr bool kLaneSum = true;
#else
constexpr bool kLaneSum = false;
#endif

enum { kUnsigned = 0, kSigned = 1, kFloat = 2 };

int kind_of(int dt) {
  if (is_float(dt)) return kFloat;
  return dt == BM_I8 || dt == BM_I16 || dt == BM_I32 || dt == BM_I64 ? kSigned : kUnsigned;
}
// a float is a NaN when its bits without the sign exceed the infinity's; no integer exceeds ~0
uint64_t nan_above(int dt) {
  return dt == BM_F16 ? 0x7C00ull : dt == BM_F32 ? 0x7F800000ull : dt == BM_F64 ? 0x7FF0000000000000ull : ~0ull;
}

// element bits -> key: xor with neg where the sign bit is set, else with pos
// (floats: every bit / the sign bit; signed: the sign bit both; unsigned: 0).
// The key's top bit is set exactly where pos was applied, so the way back is
// the same xor chosen by the key's top bit.
struct KeyMask {
  uint64_t neg, pos;
  uint64_t nan_above;
};
KeyMask key_mask(int dt) {
  const int es = dtype_size(dt), kind = kind_of(dt);
  const uint64_t sign = 1ull << (8 * es - 1), all = es == 8 ? ~0ull : (1ull << (8 * es)) - 1;
  KeyMask m;
  m.neg = kind == kFloat ? all : kind == kSigned ? sign : 0;
  m.pos = kind == kUnsigned ? 0 : sign;
  m.nan_above = nan_above(dt);
  return m;
}

// the quantiles of one call: rank[k] and frac[k] as bm_quantile_rows takes them
struct QSpec {
  int32_t n;       // quantiles
  int32_t dt;      // element dtype
  int32_t odt;     // output dtype
  int32_t same;    // outputs are elements (their bits), not statistics-dtype values
  KeyMask km;
  int64_t rank[QMAX];
  double frac[QMAX];
};

// keys are held in 32 bits for elements up to 4 bytes, else in 64
template <typename K> struct Held { typedef typename std::conditional<sizeof(K) == 8, uint64_t, uint32_t>::type t; };

template <typename K> __device__ __forceinline__ typename Held<K>::t encode(K b, const KeyMask &m) {
  typedef typename Held<K>::t HK;
  constexpr HK sign = HK(1) << (8 * sizeof(K) - 1);
  const HK v = b;
  return v ^ ((v & sign) ? (HK)m.neg : (HK)m.pos);
}
template <typename K> __device__ __forceinline__ bool is_nan_bits(K b, uint64_t above) {
  constexpr uint64_t sign = 1ull << (8 * sizeof(K) - 1);
  return ((uint64_t)b & ~sign) > above;
}

// ---- epilogue: key -> element -> output, shared by both paths ----
__device__ __forceinline__ uint64_t key_bits(uint64_t key, int es, const KeyMask &m) {
  const uint64_t sign = 1ull << (8 * es - 1);
  return key ^ ((key & sign) ? m.pos : m.neg);
}
__device__ __forceinline__ double bits_f64(uint64_t b, int dt) {
  switch (dt) {
    case BM_I8: return (double)(int8_t)b;
    case BM_I16: return (double)(int16_t)b;
    case BM_I32: return (double)(int32_t)b;
    case BM_I64: return (double)(int64_t)b;
    case BM_F16: return (double)(float)__builtin_bit_cast(_Float16, (uint16_t)b);
    case BM_F32: return (double)__builtin_bit_cast(float, (uint32_t)b);
    case BM_F64: return __builtin_bit_cast(double, b);
    default: return (double)b;  // bool and the unsigned integers
  }
}
__device__ __forceinline__ int es_of(int dt) {
  switch (dt) {
    case BM_BOOL: case BM_U8: case BM_I8: return 1;
    case BM_U16: case BM_I16: case BM_F16: return 2;
    case BM_U32: case BM_I32: case BM_F32: return 4;
    default: return 8;
  }
}
// output k of row `row`: klo / khi the keys of rank[k] and rank[k] + 1 (khi is
// not looked at when frac[k] == 0)
__device__ __forceinline__ void emit(void *out, int64_t O, int64_t row, int k, const QSpec &q, uint64_t klo,
                                     uint64_t khi, bool nan) {
  const int64_t idx = (int64_t)k * O + row;
  const int es = es_of(q.dt);
  if (q.same) {
    uint64_t b = key_bits(klo, es, q.km);
    if (nan) b = es == 2 ? 0x7E00ull : es == 4 ? 0x7FC00000ull : 0x7FF8000000000000ull;  // (floats only)
    if (es == 1) ((uint8_t *)out)[idx] = (uint8_t)b;
    else if (es == 2) ((uint16_t *)out)[idx] = (uint16_t)b;
    else if (es == 4) ((uint32_t *)out)[idx] = (uint32_t)b;
    else ((uint64_t *)out)[idx] = b;
    return;
  }
  const double lo = bits_f64(key_bits(klo, es, q.km), q.dt);
  double v = lo;
  if (q.frac[k] != 0.0) {
    const double hi = bits_f64(key_bits(khi, es, q.km), q.dt);
    const double d = hi - lo;       // three roundings, none fused
    const double t = d * q.frac[k];
    v = lo + t;
  }
  if (nan) v = __builtin_nan("");
  if (q.odt == BM_F16) ((_Float16 *)out)[idx] = (_Float16)v;
  else if (q.odt == BM_F32) ((float *)out)[idx] = (float)v;
  else ((double *)out)[idx] = v;
}

// ------------------------------------------------------------------ rows --
struct RowsArgs {
  int64_t O, R;
  int64_t sp;    // elements between row starts (>= R)
  int64_t row0;  // first row of this launch (launches split at the grid limit)
};

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// a wave-uniform count summed over the row's waves, in every thread: the waves
// meet in LDS, sm[par] of the two buffers (one barrier a call: the buffer
// written now was last read two calls ago, a barrier in between)
template <int WPR> __device__ __forceinline__ uint32_t row_count(uint32_t c, int lane, int wave, uint32_t (*sm)[kWaves],
                                                                 int &par) {
  if constexpr (WPR == 1) {
    return c;
  } else {
    if (lane == 0) sm[par][wave] = c;
    __syncthreads();
    uint32_t t = sm[par][0];
#pragma unroll
    for (int w = 1; w < WPR; ++w) t += sm[par][w];
    par ^= 1;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
  }
}

// the smallest of x over the row's threads, in every thread
template <int WPR> __device__ __forceinline__ uint64_t row_min(uint64_t x, int lane, int wave, uint64_t *sm) {
  x = wave_fold(x, lane, [](uint64_t a, uint64_t b) { return a < b ? a : b; });
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, kFoldLane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), kFoldLane);
  x = ((uint64_t)hi << 32) | lo;
  if constexpr (WPR == 1) {
    return x;
  } else {
    if (lane == 0) sm[wave] = x;
    __syncthreads();
    uint64_t t = sm[0];
#pragma unroll
    for (int w = 1; w < WPR; ++w) t = sm[w] < t ? sm[w] : t;
    __syncthreads();  // sm is written again by the next rank
    return t;
  }
}

// k_q_rows' three steps on a row held as keys -- the read, the bit search and
// the step to the next rank -- as functions, for k_norm_rows.  k_q_rows keeps
// its own text below: built from these functions its register allocation
// changed (float32, 16-B vectors, wave per row: 103 VGPRs and four waves a SIMD
// instead of 73 and six), and its measured times are not to move with an
// addition.  WPR waves per row (1, or the block's 4), each thread holding NV
// vectors of VEC elements: R <= 64 * WPR * VEC * NV (the host's plan),
// R % VEC == 0.  K: the unsigned integer of the element's width.

// the one read: thread slot j0, j < R leaves a whole vector inside the row
// (R % VEC == 0).  nin: the thread's vectors inside the row, its first nin
// (one register instead of k_q_rows' NV lane masks, which would stay live
// across the search).  -> this thread saw a NaN
template <typename K, int VEC, int NV, int WPR>
__device__ __forceinline__ bool load_keys(const K *s, int64_t j0, int64_t R, const KeyMask &km,
                                          typename Held<K>::t (&key)[NV][VEC], int &nin) {
  typedef typename Held<K>::t HK;
  constexpr int64_t stride = (int64_t)64 * WPR * VEC;
  bool nan = false;
  nin = 0;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const bool in = j0 + u * stride < R;
    nin += in ? 1 : 0;
    K v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = K(0);
    if (in) vload_nt<K, VEC>(s + j0 + u * stride, v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      nan = nan || (in && is_nan_bits<K>(v[i], km.nan_above));
      key[u][i] = in ? encode<K>(v[i], km) : (HK)(K)~K(0);
    }
  }
  return nan;
}

// the key of rank `rank` among the row's keys: the binary search over the key's bits
template <typename K, int VEC, int NV, int WPR>
__device__ __forceinline__ typename Held<K>::t find_rank(const typename Held<K>::t (&key)[NV][VEC], uint32_t rank,
                                                         int lane, int wave, uint32_t (*smc)[kWaves], int &par) {
  typedef typename Held<K>::t HK;
  constexpr int BITS = 8 * sizeof(K);
  HK lo = 0;
  for (int bit = BITS - 1; bit >= 0; --bit) {
    const HK cand = lo | (HK(1) << bit);
    uint32_t c = 0;
    if constexpr (kLaneSum) {
      uint32_t cl = 0;  // at most 32: six bits
#pragma unroll
      for (int u = 0; u < NV; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) cl += key[u][i] < cand ? 1u : 0u;
      }
#pragma unroll
      for (int b = 0; b < 6; ++b) c += popc64(__builtin_amdgcn_ballot_w64((cl >> b & 1u) != 0)) << b;
    } else {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) c += popc64(__builtin_amdgcn_ballot_w64(key[u][i] < cand));
      }
    }
    c = row_count<WPR>(c, lane, wave, smc, par);
    if (c <= rank) lo = cand;
  }
  return lo;
}

// given the key lo of rank `rank`, the key of rank + 1 (rank + 1 < R: the caller's check)
template <typename K, int VEC, int NV, int WPR>
__device__ __forceinline__ uint64_t next_key(const typename Held<K>::t (&key)[NV][VEC], int nin,
                                             typename Held<K>::t lo, uint32_t rank, int lane, int wave,
                                             uint32_t (*smc)[kWaves], int &par, uint64_t *smk) {
  uint32_t cle = 0;
  uint64_t mn = ~0ull;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      cle += popc64(__builtin_amdgcn_ballot_w64(u < nin && key[u][i] <= lo));
      if (u < nin && key[u][i] > lo && (uint64_t)key[u][i] < mn) mn = key[u][i];
    }
  }
  cle = row_count<WPR>(cle, lane, wave, smc, par);
  mn = row_min<WPR>(mn, lane, wave, smk);
  return cle <= rank + 1 ? mn : (uint64_t)lo;  // rank + 1 < R: a key above lo exists
}

// WPR waves per row (1, or the block's 4), each thread holding NV vectors of
// VEC elements: R <= 64 * WPR * VEC * NV (the host's plan), R % VEC == 0.  K:
// the unsigned integer of the element's width.
template <typename K, int VEC, int NV, int WPR>
__global__ void __launch_bounds__(kThreads) k_q_rows(const K *__restrict__ src, void *__restrict__ out, RowsArgs a,
                                                      QSpec q) {
  typedef typename Held<K>::t HK;
  constexpr int BITS = 8 * sizeof(K);
  __shared__ uint32_t smc[2][kWaves];
  __shared__ uint64_t smk[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int RPB = kThreads / 64 / WPR;  // rows per block
  const int64_t row = a.row0 + (int64_t)rows_block() * RPB + (WPR == 1 ? wave : 0);
  // wave per row: whole waves leave, and no barrier follows; block per row: the whole block leaves
  if (row >= a.O) return;
  const K *s = src + row * a.sp;
  constexpr int64_t stride = (int64_t)64 * WPR * VEC;
  const int64_t j0 = (int64_t)(WPR == 1 ? lane : (int)threadIdx.x) * VEC;

  // the one read: j < R leaves a whole vector inside the row (R % VEC == 0)
  HK key[NV][VEC];
  bool in[NV];
  bool nan = false;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    in[u] = j0 + u * stride < a.R;
    K v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = K(0);
    if (in[u]) vload_nt<K, VEC>(s + j0 + u * stride, v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      nan = nan || (in[u] && is_nan_bits<K>(v[i], q.km.nan_above));
      key[u][i] = in[u] ? encode<K>(v[i], q.km) : (HK)(K)~K(0);
    }
  }
  int par = 0;
  const bool row_nan = row_count<WPR>(popc64(__builtin_amdgcn_ballot_w64(nan)), lane, wave, smc, par) != 0;

  for (int k = 0; k < q.n; ++k) {
    const uint32_t rank = (uint32_t)q.rank[k];
    HK lo = 0;
    for (int bit = BITS - 1; bit >= 0; --bit) {
      const HK cand = lo | (HK(1) << bit);
      uint32_t c = 0;
      if constexpr (kLaneSum) {
        uint32_t cl = 0;  // at most 32: six bits
#pragma unroll
        for (int u = 0; u < NV; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) cl += key[u][i] < cand ? 1u : 0u;
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) c += popc64(__builtin_amdgcn_ballot_w64((cl >> b & 1u) != 0)) << b;
      } else {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) c += popc64(__builtin_amdgcn_ballot_w64(key[u][i] < cand));
        }
      }
      c = row_count<WPR>(c, lane, wave, smc, par);
      if (c <= rank) lo = cand;
    }
    uint64_t hi = lo;
    if (q.frac[k] != 0.0) {  // (uniform)
      uint32_t cle = 0;
      uint64_t mn = ~0ull;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          cle += popc64(__builtin_amdgcn_ballot_w64(in[u] && key[u][i] <= lo));
          if (in[u] && key[u][i] > lo && (uint64_t)key[u][i] < mn) mn = key[u][i];
        }
      }
      cle = row_count<WPR>(cle, lane, wave, smc, par);
      mn = row_min<WPR>(mn, lane, wave, smk);
      if (cle <= rank + 1) hi = mn;  // rank + 1 < R: a key above lo exists
    }
    if ((WPR == 1 ? lane : (int)threadIdx.x) == 0) emit(out, a.O, row, k, q, lo, hi, row_nan);
  }
}

// ------------------------------------------------------------- normalize --
// bm_normalize_rows' percentile baseline: k_q_rows' read and search for one
// quantile, then the held keys are decoded back to the row's values,
// normalised against the baseline and stored -- one read, one write.
struct NormArgs {
  int64_t O, R;
  int64_t sp, dp;  // elements between row starts of src / dst (>= R)
  int64_t row0;    // first row of this launch (launches split at the grid limit)
  int64_t rank;    // as bm_quantile_rows' ranks[0] / frac[0]
  double frac;
  double offset;
};

// key_mask of the element type: a constant in k_norm_rows, which is built per
// element type (its outputs are), where k_q_rows takes the masks as arguments
template <typename T> __device__ constexpr KeyMask mask_of() {
  constexpr int es = sizeof(T);
  constexpr bool flt = std::is_same<T, _Float16>::value || std::is_floating_point<T>::value;
  constexpr bool sgn = !flt && std::is_signed<T>::value;
  constexpr uint64_t sign = 1ull << (8 * es - 1), all = ~0ull >> (64 - 8 * es);
  return KeyMask{flt ? all : sgn ? sign : 0, flt || sgn ? sign : 0,
                 !flt ? ~0ull : es == 2 ? 0x7C00ull : es == 4 ? 0x7F800000ull : 0x7FF0000000000000ull};
}

template <typename T> struct BitsOf {
  typedef typename std::conditional<
      sizeof(T) == 1, uint8_t,
      typename std::conditional<sizeof(T) == 2, uint16_t,
                                typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type t;
};

// the element a held key was made from, as float64 (encode's way back, then bits_f64's conversion)
template <typename T> __device__ __forceinline__ double key_f64(typename Held<typename BitsOf<T>::t>::t key,
                                                                const KeyMask &m) {
  typedef typename BitsOf<T>::t K;
  typedef typename Held<K>::t HK;
  constexpr HK sign = HK(1) << (8 * sizeof(K) - 1);
  const K b = (K)(key ^ ((key & sign) ? (HK)m.pos : (HK)m.neg));
  return to_f64(__builtin_bit_cast(T, b));
}

// The baseline b is formed by every thread from the row-uniform keys lo / hi
// (the counts and the minimum reach every wave of a block through LDS), in
// float64 exactly as emit forms it.  x - b, b + offset and the division are
// three separately rounded float64 operations (contraction is off in this
// file), rounded once to the output type.  A row holding a NaN: b is NaN, and
// so is every output.  The keys stay live until the last store; widening
// outputs (float64 from 1-, 2- and 4-byte integers) leave as 16-B stores.
template <typename T, int VEC, int NV, int WPR>
__global__ void __launch_bounds__(kThreads)
    k_norm_rows(const T *__restrict__ src, typename OutOf<T>::t *__restrict__ dst, NormArgs a) {
  typedef typename OutOf<T>::t OT;
  typedef typename BitsOf<T>::t K;
  typedef typename Held<K>::t HK;
  __shared__ uint32_t smc[2][kWaves];
  __shared__ uint64_t smk[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int RPB = kThreads / 64 / WPR;  // rows per block
  const int64_t row = a.row0 + (int64_t)rows_block() * RPB + (WPR == 1 ? wave : 0);
  // wave per row: whole waves leave, and no barrier follows; block per row: the whole block leaves
  if (row >= a.O) return;
  constexpr int64_t stride = (int64_t)64 * WPR * VEC;
  const int64_t j0 = (int64_t)(WPR == 1 ? lane : (int)threadIdx.x) * VEC;

  // this thread's first output, formed before the search: a per-lane address
  // lives in vector registers, of which the search leaves enough, where dst
  // and its pitch would wait in scalar registers, of which it does not
  OT *o = dst + row * a.dp + j0;
  asm volatile("" : "+v"(o));  // (formed here, not re-formed at the stores)
  constexpr KeyMask km = mask_of<T>();
  HK key[NV][VEC];
  int nin;
  const bool nan = load_keys<K, VEC, NV, WPR>((const K *)src + row * a.sp, j0, a.R, km, key, nin);
  int par = 0;
  const bool row_nan = row_count<WPR>(popc64(__builtin_amdgcn_ballot_w64(nan)), lane, wave, smc, par) != 0;

  const uint32_t rank = (uint32_t)a.rank;
  const HK klo = find_rank<K, VEC, NV, WPR>(key, rank, lane, wave, smc, par);
  const double lo = key_f64<T>(klo, km);
  double b = lo;
  if (a.frac != 0.0) {  // (uniform)
    const HK khi = (HK)next_key<K, VEC, NV, WPR>(key, nin, klo, rank, lane, wave, smc, par, smk);
    const double d = key_f64<T>(khi, km) - lo;  // three roundings, none fused
    const double t = d * a.frac;
    b = lo + t;
  }
  if (row_nan) b = __builtin_nan("");
  const double den = b + a.offset;

  // the one write
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    if (u < nin) {
      OT ov[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double d = key_f64<T>(key[u][i], km) - b;
        ov[i] = (OT)(d / den);
      }
      store_out_nt<OT, VEC>(o + u * stride, ov);
    }
  }
}

// ------------------------------------------------------------- streaming --
// the ranks searched: one per quantile, and rank + 1 where frac != 0
struct Search {
  int32_t S;
  int32_t lo_of[QMAX];  // quantile k's lo is search lo_of[k], its hi the next one
  int64_t rank[QMAX];
};

struct StreamArgs {
  int64_t R, P;
  int64_t row0;   // first row of this batch
  int64_t slice;  // elements of a row per block (whole vectors)
  int32_t S, pass;
  KeyMask km;
};

// workspace of a batch of B rows: hist[B][S][256] u64, prefix[B][S] u64, remain[B][S] u64, nans[B] u64
struct Work {
  unsigned long long *hist, *prefix, *remain, *nans;
};
size_t work_bytes(int64_t B, int S) { return (size_t)B * ((size_t)S * (256 + 2) + 1) * 8; }
Work work_of(void *ws, int64_t B, int S) {
  Work w;
  w.hist = (unsigned long long *)ws;
  w.prefix = w.hist + (size_t)B * S * 256;
  w.remain = w.prefix + (size_t)B * S;
  w.nans = w.remain + (size_t)B * S;
  return w;
}

// grid (blocks per row, rows of the batch); pass p looks at byte p from the top
template <typename K, int VEC>
__global__ void __launch_bounds__(kThreads) k_q_hist(const K *__restrict__ src, StreamArgs a, Work w) {
  typedef typename Held<K>::t HK;
  constexpr int BITS = 8 * sizeof(K);
  __shared__ uint32_t lh[QMAX * 256];
  const int64_t rb = blockIdx.y;
  const int S = a.pass == 0 ? 1 : a.S;  // the first pass: one histogram for all ranks
  for (int i = threadIdx.x; i < S * 256; i += kThreads) lh[i] = 0;
  HK pfx[QMAX];
#pragma unroll
  for (int sidx = 0; sidx < QMAX; ++sidx)
    pfx[sidx] = a.pass != 0 && sidx < a.S ? (HK)w.prefix[rb * a.S + sidx] : HK(0);
  __syncthreads();
  const int shift = BITS - 8 * (a.pass + 1);
  const K *s = src + (a.row0 + rb) * a.P;
  const int64_t j_end = min(a.R, ((int64_t)blockIdx.x + 1) * a.slice);
  uint32_t nans = 0;
  // j + VEC <= j_end: R and the slice are whole vectors
  for (int64_t j = (int64_t)blockIdx.x * a.slice + (int64_t)threadIdx.x * VEC; j < j_end; j += (int64_t)kThreads * VEC) {
    K v[VEC];
    vload_nt<K, VEC>(s + j, v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const HK key = encode<K>(v[i], a.km);
      const uint32_t bin = (uint32_t)(key >> shift) & 255u;
      if (a.pass == 0) {
        nans += is_nan_bits<K>(v[i], a.km.nan_above) ? 1u : 0u;
        atomicAdd(&lh[bin], 1u);
      } else {
        const HK top = (HK)((uint64_t)key >> (shift + 8));  // (shift + 8 < BITS after the first pass)
#pragma unroll
        for (int sidx = 0; sidx < QMAX; ++sidx)
          if (sidx < a.S && top == pfx[sidx]) atomicAdd(&lh[sidx * 256 + bin], 1u);
      }
    }
  }
  __syncthreads();
  if (nans) atomicAdd(&w.nans[rb], (unsigned long long)nans);
  for (int i = threadIdx.x; i < S * 256; i += kThreads)
    if (lh[i]) atomicAdd(&w.hist[(size_t)rb * a.S * 256 + i], (unsigned long long)lh[i]);
}

// one thread per (row of the batch, searched rank): the bin its rank falls in
__global__ void __launch_bounds__(kThreads) k_q_pick(int64_t B, int pass, Search sr, Work w) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * sr.S) return;
  const int64_t rb = idx / sr.S;
  const int sidx = (int)(idx - rb * sr.S);
  const unsigned long long *h = w.hist + ((size_t)rb * sr.S + (pass == 0 ? 0 : sidx)) * 256;
  unsigned long long rem = pass == 0 ? (unsigned long long)sr.rank[sidx] : w.remain[idx];
  const unsigned long long pf = pass == 0 ? 0ull : w.prefix[idx];
  int b = 0;
  for (; b < 255; ++b) {  // (the bins of this prefix hold more than rem keys: b stops in time)
    const unsigned long long c = h[b];
    if (rem < c) break;
    rem -= c;
  }
  w.prefix[idx] = (pf << 8) | (unsigned long long)b;
  w.remain[idx] = rem;
}

// one thread per row of the batch: the prefixes are the keys
__global__ void __launch_bounds__(kThreads) k_q_finish(int64_t B, int64_t row0, int64_t O, Search sr, QSpec q, Work w,
                                                        void *__restrict__ out) {
  const int64_t rb = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (rb >= B) return;
  const bool nan = w.nans[rb] != 0;
  for (int k = 0; k < q.n; ++k) {
    const int at = sr.lo_of[k];
    const uint64_t lo = w.prefix[rb * sr.S + at];
    const uint64_t hi = q.frac[k] != 0.0 ? w.prefix[rb * sr.S + at + 1] : lo;
    emit(out, O, row0 + rb, k, q, lo, hi, nan);
  }
}

// -------------------------------------------------------------- dispatch --
// f(TypeTag<unsigned integer of es bytes>)
template <typename F> void for_width(int es, F &&f) {
  switch (es) {
    case 1: f(TypeTag<uint8_t>{}); break;
    case 2: f(TypeTag<uint16_t>{}); break;
    case 4: f(TypeTag<uint32_t>{}); break;
    default: f(TypeTag<uint64_t>{}); break;
  }
}

template <typename K, int VEC> void launch_rows_v(bool block, const void *src, void *out, RowsArgs a, const QSpec &q,
                                                  hipStream_t st) {
  const int rpb = block ? 1 : kThreads / 64;
  for_block_runs(cdiv(a.O, rpb), kThreads, [&](int64_t b0, int g) {
    a.row0 = b0 * rpb;
    if (block)
      k_q_rows<K, VEC, lane_vecs(VEC), kWaves><<<g, kThreads, 0, st>>>((const K *)src, out, a, q);
    else
      k_q_rows<K, VEC, lane_vecs(VEC), 1><<<g, kThreads, 0, st>>>((const K *)src, out, a, q);
  });
}

int rows_vec(int es, int64_t R, int64_t P, const void *src) {
  return pick_vec(std::min(16 / es, kMaxVec), {R, P}, {{src, es}});
}

template <typename T, int VEC> void launch_norm_v(bool block, const void *src, void *dst, NormArgs a, hipStream_t st) {
  typedef typename OutOf<T>::t OT;
  const int rpb = block ? 1 : kThreads / 64;
  for_block_runs(cdiv(a.O, rpb), kThreads, [&](int64_t b0, int g) {
    a.row0 = b0 * rpb;
    if (block)
      k_norm_rows<T, VEC, lane_vecs(VEC), kWaves><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
    else
      k_norm_rows<T, VEC, lane_vecs(VEC), 1><<<g, kThreads, 0, st>>>((const T *)src, (OT *)dst, a);
  });
}

// rows_vec where the rows are also written: the vector divides dst's pitch and
// dst is aligned to its stores of at most 16 B (bm_standardize.hip's std_vec)
int norm_vec(int ies, int oes, int64_t R, int64_t sp, int64_t dp, const void *src, const void *dst) {
  return pick_vec(std::min(16 / ies, kMaxVec), {R, sp, dp}, {{src, ies}, {dst, oes}});
}

// the checks both entry points share; fills q (and the count of searched ranks)
int check_spec(const char *who, const void *src, int in_dtype, int64_t O, int64_t R, int64_t pitch,
               const int64_t *ranks, const double *frac, int nq, const void *out, int out_dtype, QSpec *q, Search *sr) {
  if (!src || !ranks || !frac || !out) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (dtype_size(in_dtype) == 0) { bm_set_error("%s: bad dtype %d", who, in_dtype); return BM_E_ARG; }
  if (out_dtype != in_dtype && out_dtype != stat_dtype(in_dtype)) {
    bm_set_error("%s: out_dtype %d is neither dtype %d itself nor its statistics dtype %d (float16 / float32 "
                 "keep theirs, every other dtype gives float64)", who, out_dtype, in_dtype, stat_dtype(in_dtype));
    return BM_E_ARG;
  }
  if (O < 0 || R < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld)", who, (long long)O, (long long)R);
    return BM_E_ARG;
  }
  if (pitch < R) {
    bm_set_error("%s: pitch below the row length (row_pitch=%lld R=%lld)", who, (long long)pitch, (long long)R);
    return BM_E_ARG;
  }
  if (nq < 1 || nq > QMAX) { bm_set_error("%s: %d quantiles, not 1..%d", who, nq, QMAX); return BM_E_ARG; }
  *q = QSpec{};
  *sr = Search{};
  q->n = nq; q->dt = in_dtype; q->odt = out_dtype; q->km = key_mask(in_dtype);
  // an element itself where the dtypes agree and it is no statistics dtype (float16 / float32 / float64: either way the same bytes)
  q->same = out_dtype == in_dtype ? 1 : 0;
  int S = 0;
  for (int k = 0; k < nq; ++k) {
    const bool two = frac[k] != 0.0;
    if (!(frac[k] >= 0.0 && frac[k] < 1.0)) {
      bm_set_error("%s: frac[%d]=%g is not in [0, 1)", who, k, frac[k]);
      return BM_E_ARG;
    }
    if (two && q->same && out_dtype != stat_dtype(in_dtype)) {
      bm_set_error("%s: frac[%d] != 0 needs the statistics dtype %d as out_dtype, got %d", who, k,
                   stat_dtype(in_dtype), out_dtype);
      return BM_E_ARG;
    }
    if (ranks[k] < 0 || (O > 0 && ranks[k] + (two ? 1 : 0) >= R)) {
      bm_set_error("%s: rank %lld%s of quantile %d is not below the row length R=%lld", who, (long long)ranks[k],
                   two ? " (+ 1: frac != 0)" : "", k, (long long)R);
      return BM_E_ARG;
    }
    if (S + (two ? 2 : 1) > QMAX) {
      bm_set_error("%s: more than %d ranks (a quantile with frac != 0 takes two)", who, QMAX);
      return BM_E_ARG;
    }
    q->rank[k] = ranks[k];
    q->frac[k] = frac[k];
    sr->lo_of[k] = S;
    sr->rank[S++] = ranks[k];
    if (two) sr->rank[S++] = ranks[k] + 1;
  }
  sr->S = S;
  // interpolated float outputs are values, not bits
  for (int k = 0; k < nq; ++k)
    if (frac[k] != 0.0) q->same = 0;
  return BM_OK;
}

int64_t stream_rows(int64_t O) { return std::min(O, kStreamRows); }

}  // namespace

extern "C" int bm_quantile_rows(const void *src, int in_dtype, int64_t O, int64_t R, int64_t row_pitch,
                                const int64_t *ranks, const double *frac, int nq, void *out, int out_dtype,
                                int *taken, void *stream) {
  const char *who = "bm_quantile_rows";
  if (!taken) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  QSpec q;
  Search sr;
  int rc = check_spec(who, src, in_dtype, O, R, row_pitch, ranks, frac, nq, out, out_dtype, &q, &sr);
  if (rc) return rc;
  *taken = 1;
  if (O == 0 || R == 0) return BM_OK;  // nothing to write
  const int es = dtype_size(in_dtype);
  const int vec = rows_vec(es, R, row_pitch, src);
  const int64_t held = (int64_t)vec * lane_vecs(vec);  // elements a thread holds
  const bool wave = R <= 64 * held;
  if (!wave && (R > kThreads * held || O < kBlockMinRows)) {
    *taken = 0;  // rows beyond the registers, or too few of them for a block each: bm_quantile_select
    return BM_OK;
  }
  RowsArgs a{};
  a.O = O; a.R = R; a.sp = row_pitch;
  for_width(es, [&](auto t) {
    typedef typename decltype(t)::type K;
    for_vec<K, kMaxVec>(vec, [&](auto v) {
      launch_rows_v<K, decltype(v)::value>(!wave, src, out, a, q, (hipStream_t)stream);
    });
  });
  return check_launch(who);
}

extern "C" int bm_normalize_rows(const void *src, int in_dtype, int64_t O, int64_t R, int64_t src_pitch, int baseline,
                                 int64_t rank, double frac, double offset, void *dst, int out_dtype,
                                 int64_t dst_pitch, int *taken, void *stream) {
  const char *who = "bm_normalize_rows";
  if (!src || !dst || !taken) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (dtype_size(in_dtype) == 0) { bm_set_error("%s: bad dtype %d", who, in_dtype); return BM_E_ARG; }
  if (out_dtype != stat_dtype(in_dtype)) {
    bm_set_error("%s: out_dtype %d is not the statistics dtype %d of dtype %d (float16 / float32 keep "
                 "theirs, every other dtype gives float64)", who, out_dtype, stat_dtype(in_dtype), in_dtype);
    return BM_E_ARG;
  }
  if (O < 0 || R < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld)", who, (long long)O, (long long)R);
    return BM_E_ARG;
  }
  if (src_pitch < R || dst_pitch < R) {
    bm_set_error("%s: pitch below the row length (src_pitch=%lld dst_pitch=%lld R=%lld)", who,
                 (long long)src_pitch, (long long)dst_pitch, (long long)R);
    return BM_E_ARG;
  }
  if (baseline != BM_NORM_MEAN && baseline != BM_NORM_RANK) {
    bm_set_error("%s: baseline %d is not BM_NORM_MEAN or BM_NORM_RANK", who, baseline);
    return BM_E_ARG;
  }
  if (!std::isfinite(offset)) { bm_set_error("%s: offset %g is not finite", who, offset); return BM_E_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (baseline == BM_NORM_MEAN)
    return bm_standardize_rows_checked(who, src, in_dtype, O, R, src_pitch, dst, out_dtype, dst_pitch, 2, offset,
                                       taken, st);
  const bool two = frac != 0.0;
  if (!(frac >= 0.0 && frac < 1.0)) { bm_set_error("%s: frac=%g is not in [0, 1)", who, frac); return BM_E_ARG; }
  if (rank < 0 || (O > 0 && R > 0 && rank + (two ? 1 : 0) >= R)) {
    bm_set_error("%s: rank %lld%s is not below the row length R=%lld", who, (long long)rank,
                 two ? " (+ 1: frac != 0)" : "", (long long)R);
    return BM_E_ARG;
  }
  *taken = 1;
  if (O == 0 || R == 0) return BM_OK;  // nothing to write
  const int ies = dtype_size(in_dtype), oes = dtype_size(out_dtype);
  const int vec = norm_vec(ies, oes, R, src_pitch, dst_pitch, src, dst);
  const int64_t held = (int64_t)vec * lane_vecs(vec);  // elements a thread holds
  const bool wave = R <= 64 * held;
  if (!wave && (R > kThreads * held || O < kBlockMinRows)) {
    *taken = 0;  // bm_quantile_rows' plan: the caller forms the baseline plane, then bm_standardize_apply
    return BM_OK;
  }
  NormArgs a{};
  a.O = O; a.R = R; a.sp = src_pitch; a.dp = dst_pitch; a.rank = rank; a.frac = frac; a.offset = offset;
  for_dtype(in_dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    for_vec<T, kMaxVec>(vec, [&](auto v) { launch_norm_v<T, decltype(v)::value>(!wave, src, dst, a, st); });
  });
  return check_launch(who);
}

extern "C" int bm_quantile_workspace_bytes(int in_dtype, int64_t O, int64_t R, int nranks, size_t *bytes) {
  const char *who = "bm_quantile_workspace_bytes";
  if (!bytes) { bm_set_error("%s: null pointer", who); return BM_E_ARG; }
  if (dtype_size(in_dtype) == 0) { bm_set_error("%s: bad dtype %d", who, in_dtype); return BM_E_ARG; }
  if (O < 0 || R < 0) {
    bm_set_error("%s: negative extent (O=%lld R=%lld)", who, (long long)O, (long long)R);
    return BM_E_ARG;
  }
  if (nranks < 1 || nranks > QMAX) { bm_set_error("%s: %d ranks, not 1..%d", who, nranks, QMAX); return BM_E_ARG; }
  *bytes = O == 0 || R == 0 ? 0 : work_bytes(stream_rows(O), nranks);
  return BM_OK;
}

extern "C" int bm_quantile_select(const void *src, int in_dtype, int64_t O, int64_t R, int64_t row_pitch,
                                  const int64_t *ranks, const double *frac, int nq, void *out, int out_dtype,
                                  void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "bm_quantile_select";
  QSpec q;
  Search sr;
  int rc = check_spec(who, src, in_dtype, O, R, row_pitch, ranks, frac, nq, out, out_dtype, &q, &sr);
  if (rc) return rc;
  if (O == 0 || R == 0) return BM_OK;  // nothing to write
  const int64_t Bmax = stream_rows(O);
  const size_t need = work_bytes(Bmax, sr.S);
  if (!workspace || need > workspace_bytes) {
    bm_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
    return BM_E_WS;
  }
  const int es = dtype_size(in_dtype);
  const int vec = rows_vec(es, R, row_pitch, src);
  hipStream_t st = (hipStream_t)stream;
  StreamArgs a{};
  a.R = R; a.P = row_pitch; a.S = sr.S; a.km = q.km;
  for (int64_t r0 = 0; r0 < O; r0 += Bmax) {
    const int64_t B = std::min(Bmax, O - r0);
    // blocks per row: the batch fills the device, no slice is shorter than kSliceMin or longer than kSliceMax
    int64_t bpr = std::min(cdiv(kStreamBlocks, B), std::max<int64_t>(1, R / kSliceMin));
    bpr = std::max(bpr, cdiv(R, kSliceMax));
    a.slice = cdiv(cdiv(R, vec), bpr) * vec;
    bpr = cdiv(R, a.slice);
    a.row0 = r0;
    const Work w = work_of(workspace, B, sr.S);
    for (int pass = 0; pass < es; ++pass) {
      a.pass = pass;
      // the histograms start from zero; the first pass also counts the NaNs (prefix and remain lie between)
      if (pass == 0) {
        if (hipMemsetAsync(w.hist, 0, work_bytes(B, sr.S), st) != hipSuccess) return check_launch(who);
      } else if (hipMemsetAsync(w.hist, 0, (size_t)B * sr.S * 256 * 8, st) != hipSuccess) {
        return check_launch(who);
      }
      for_width(es, [&](auto t) {
        typedef typename decltype(t)::type K;
        for_vec<K, kMaxVec>(vec, [&](auto v) {
          k_q_hist<K, decltype(v)::value><<<dim3((unsigned)bpr, (unsigned)B), kThreads, 0, st>>>((const K *)src, a, w);
        });
      });
      k_q_pick<<<(int)cdiv(B * sr.S, kThreads), kThreads, 0, st>>>(B, pass, sr, w);
    }
    k_q_finish<<<(int)cdiv(B, kThreads), kThreads, 0, st>>>(B, r0, O, sr, q, w, out);
  }
  return check_launch(who);
}

// bm_wave.h -- device helpers shared by the kernels of bm_reduce.hip,
// bm_standardize.hip and bm_comoment.hip (gfx950 only): the float64 element
// conversion, the deterministic DPP fold of the 64 lanes and the XCD-aware
// block orders of the row kernels (rows_block) and the column kernels
// (xcd_block).  Their host-side counterpart is bm_host.h.
#pragma once

#include "bm_common.h"

template <typename T> __device__ __forceinline__ double to_f64(T x) { return (double)x; }
template <> __device__ __forceinline__ double to_f64<_Float16>(_Float16 x) { return (double)(float)x; }

// A pivot that sums are shifted by must be finite: x - K around an infinite or
// NaN K is NaN (or the other infinity) for every x of the row, where a sum over
// the row gives the infinity itself.  Such a first value takes 0 instead; a
// finite one is kept as it is, so finite rows keep their bits.
__device__ __forceinline__ double finite_or_zero(double k) { return k - k == 0.0 ? k : 0.0; }

// ---- the statistics dtype of an element type, and its stores ----
// the dtype of record - 0.0 (plan.stat_dtype): float16 / float32 stay, the rest float64
template <typename T> struct OutOf { typedef double t; };
template <> struct OutOf<_Float16> { typedef _Float16 t; };
template <> struct OutOf<float> { typedef float t; };

// VEC output elements as non-temporal stores of at most 16 B each
template <typename OT, int VEC> __device__ __forceinline__ void store_out_nt(OT *p, const OT (&o)[VEC]) {
  if constexpr (VEC * sizeof(OT) <= 16) {
    vstore_nt<OT, VEC>(p, o);
  } else {
    constexpr int PER = 16 / sizeof(OT);
#pragma unroll
    for (int c = 0; c < VEC / PER; ++c) {
      OT part[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) part[k] = o[c * PER + k];
      vstore_nt<OT, PER>(p + c * PER, part);
    }
  }
}

// ---- wave fold through DPP ----
// A 64-bit lane value moved by a DPP modifier of v_mov (two 32-bit halves, the
// same source lane): the cross-lane read stays in the VALU, no LDS round trip
// as __shfl_xor's ds_bpermute takes.  Controls (GFX9 DPP): quad_perm [1,0,3,2]
// = 0xB1 (lane ^ 1), [2,3,0,1] = 0x4E (lane ^ 2), row_half_mirror 0x141
// (lane 7-i of its 8), row_mirror 0x140 (lane 15-i of its row), row_bcast15
// 0x142 (lane 15 of row r -> row r+1), row_bcast31 0x143 (lane 31 -> rows 2, 3).
template <int CTRL, typename V> __device__ __forceinline__ V dpp_mov(V v) {
  static_assert(sizeof(V) == 8, "64-bit lane values");
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(V, ((uint64_t)hi << 32) | lo);
}
// dpp_mov where all 64 lanes are active and CTRL gives every lane a source lane
// (the mirrors and quad_perms): no lane keeps an old value, so none is set up
// -- dpp_mov's zero costs a v_mov per 32-bit half in front of each move.
template <int CTRL, typename V> __device__ __forceinline__ V dpp_mov_all(V v) {
  static_assert(sizeof(V) == 8, "64-bit lane values");
  static_assert(CTRL == 0xB1 || CTRL == 0x4E || CTRL == 0x141 || CTRL == 0x140, "a source lane for every lane");
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, true);
  return __builtin_bit_cast(V, ((uint64_t)hi << 32) | lo);
}
// Lane 63 receives op over all 64 lanes, combined in lane order: every step
// combines (lower lanes, upper lanes), so the result equals a left fold over
// lanes 0..63 for any associative op (first NaN / first of equal values wins,
// as in a sequential scan).  Steps 1-4 leave identical bits in the lanes that
// feed the next step (both lanes of a pair form op(lower, upper)); steps 5-6
// fold the four 16-lane rows.  Requires all 64 lanes active.
template <typename V, typename F> __device__ __forceinline__ V wave_fold(V v, int lane, F op) {
  V p = dpp_mov<0xB1>(v);
  v = (lane & 1) ? op(p, v) : op(v, p);
  p = dpp_mov<0x4E>(v);
  v = (lane & 2) ? op(p, v) : op(v, p);
  p = dpp_mov<0x141>(v);
  v = (lane & 4) ? op(p, v) : op(v, p);
  p = dpp_mov<0x140>(v);
  v = (lane & 8) ? op(p, v) : op(v, p);
  p = dpp_mov<0x142>(v);
  if (lane & 16) v = op(p, v);  // lane 31 = rows 0+1, lane 63 = rows 2+3
  p = dpp_mov<0x143>(v);
  if (lane & 32) v = op(p, v);  // lane 63 = (rows 0+1) + (rows 2+3)
  return v;
}
constexpr int kFoldLane = 63;
// lane L's value in every lane (v_readlane into a scalar register)
template <int L> __device__ __forceinline__ double lane_of(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, L);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), L);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane0_of(double v) { return lane_of<0>(v); }

// The sum of x over the threads of a row held by WPR waves of a block (1, or
// all of the block's), in every thread: lanes in lane order (wave_fold), then
// the row's waves in wave order through sm (WPR doubles of LDS; every thread of
// the block must call).  The rows kernels of bm_standardize.hip and bm_detrend.hip.
template <int WPR> __device__ __forceinline__ double row_sum(double x, int lane, int wave, double *sm) {
  x = wave_fold(x, lane, [](double a, double b) { return a + b; });
  if constexpr (WPR == 1) {
    return lane_of<kFoldLane>(x);
  } else {
    if (lane == kFoldLane) sm[wave] = x;
    __syncthreads();
    double t = sm[0];
#pragma unroll
    for (int w = 1; w < WPR; ++w) t += sm[w];
    __syncthreads();  // sm is written again by the next sum
    return t;
  }
}

// ---- block order of the row kernels ----
// Round-robin dispatch puts block b on XCD b % 8: give XCD x the x-th
// contiguous eighth of the rows, so the 128-B lines two neighbouring rows
// share are fetched into one L2 instead of two (runs of 16 / 128 / 1024
// blocks per XCD in turn: no better, padded rows 5% worse at 16,
// profiles/r05w_xcd_runs.txt).  XCD x starts its eighth x * SKEW blocks in
// and wraps, so the eight XCDs are never a power-of-two distance apart: on
// C2's padded rows (8192-B pitch, eighths 256 MiB apart) mean / std
// -1.2% / -1.0% over 3 alternating rounds (profiles/r05zd_xcd_skew.txt)
constexpr uint64_t kRedXcdSkew = 37;
__device__ __forceinline__ uint64_t rows_block() {
  uint64_t bid = blockIdx.x;
  const uint64_t g8 = gridDim.x / 8 * 8;
  if (bid < g8) {
    const uint64_t E = g8 / 8;
    bid = (bid % 8) * E + (bid / 8 + (bid % 8) * kRedXcdSkew) % E;
  }
  return bid;
}

// ---- block order of the column kernels ----
// blockIdx.x, with the blocks the hardware deals to one XCD (every 8th)
// remapped to consecutive indices (a bijection of the grid): each XCD then
// reads one contiguous range of every row, its blocks taking consecutive
// column tiles (C4 var +1.1%, 64 GiB-target-shaped mean / std over axis 0
// +2.2% / +1.6%, profiles/r05h_ab_cols_xcd.log).  The rows kernel's rotated
// start (rows_block) does not help the columns: -0.1...-0.6% on the 64 GiB
// target / C4 / C2 column statistics, profiles/r05zf_ab_colskew.log
__device__ __forceinline__ uint64_t xcd_block() {
  uint64_t bid = blockIdx.x;
  const uint64_t g8 = gridDim.x / 8 * 8;
  if (bid < g8) bid = (bid % 8) * (g8 / 8) + bid / 8;
  return bid;
}

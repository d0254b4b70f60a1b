// bm_host.h -- host-side launch plumbing shared by the .hip files of
// libbolt_mi355x: dtype codes, the launch limit and its two grid-splitting
// loops, the dtype and vector-width dispatchers, and the vector pick.  Host
// code only; the kernels, their descriptors and their plans stay in their files.
#pragma once

#include "bm_common.h"
#include "../../include/bolt_mi355x.h"

#include <algorithm>
#include <initializer_list>
#include <type_traits>

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bytes of an element of a BM_* dtype code; 0: not a dtype code
static inline int dtype_size(int dt) {
  switch (dt) {
    case BM_BOOL: case BM_U8: case BM_I8: return 1;
    case BM_U16: case BM_I16: case BM_F16: return 2;
    case BM_U32: case BM_I32: case BM_F32: return 4;
    case BM_U64: case BM_I64: case BM_F64: return 8;
    default: return 0;
  }
}
static inline bool is_float(int dt) { return dt == BM_F16 || dt == BM_F32 || dt == BM_F64; }
// the dtype of record - 0.0 (plan.stat_dtype): float16 / float32 stay, the rest float64
static inline int stat_dtype(int dt) { return dt == BM_F16 || dt == BM_F32 ? dt : BM_F64; }

// blocks of `threads` threads one launch takes at most (HIP: grid * block threads < 2^32)
constexpr int64_t max_blocks(int threads) { return 0xffffffffLL / threads; }

// after a function's launches: the first launch error, as the function's return code
static inline int check_launch(const char *who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    bm_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return BM_E_HIP;
  }
  return BM_OK;
}

// ---- dispatch: a runtime dtype code / vector width -> a template argument ----
// The callable is a generic lambda taking the tag by value:
//   [&](auto t) { typedef typename decltype(t)::type T; ... }
//   [&](auto v) { constexpr int V = decltype(v)::value; ... }
template <typename T> struct TypeTag { typedef T type; };

// f(TypeTag<element type of dt>); bool runs through the uint8 kernels (its
// values are 0 / 1).  False, and f not called: dt is not a dtype code.
template <typename F> bool for_dtype(int dt, F &&f) {
  switch (dt) {
    case BM_BOOL:
    case BM_U8: f(TypeTag<uint8_t>{}); return true;
    case BM_I8: f(TypeTag<int8_t>{}); return true;
    case BM_U16: f(TypeTag<uint16_t>{}); return true;
    case BM_I16: f(TypeTag<int16_t>{}); return true;
    case BM_U32: f(TypeTag<uint32_t>{}); return true;
    case BM_I32: f(TypeTag<int32_t>{}); return true;
    case BM_U64: f(TypeTag<uint64_t>{}); return true;
    case BM_I64: f(TypeTag<int64_t>{}); return true;
    case BM_F16: f(TypeTag<_Float16>{}); return true;
    case BM_F32: f(TypeTag<float>{}); return true;
    case BM_F64: f(TypeTag<double>{}); return true;
    default: return false;
  }
}

// f(std::integral_constant<int, vec>) for vec elements of T per vector, a
// power of two up to CAP (16 or 8).  Only widths of at most 16 B are
// instantiated: vec comes from pick_vec under the same bound, and a width
// outside it launches nothing.
template <typename T, int CAP, typename F> void for_vec(int vec, F &&f) {
  switch (vec) {
    case 16: if constexpr (CAP >= 16 && 16 * sizeof(T) <= 16) { f(std::integral_constant<int, 16>{}); } break;
    case 8: if constexpr (CAP >= 8 && 8 * sizeof(T) <= 16) { f(std::integral_constant<int, 8>{}); } break;
    case 4: if constexpr (4 * sizeof(T) <= 16) { f(std::integral_constant<int, 4>{}); } break;
    case 2: if constexpr (2 * sizeof(T) <= 16) { f(std::integral_constant<int, 2>{}); } break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
}

// The widest vector (elements, a power of two <= cap) such that every extent
// or pitch in `whole` is a whole number of vectors and every pointer is
// aligned to its access: vec * es bytes, 16 at most (wider vectors go out as
// 16-B pieces).  A null pointer counts as aligned: the workspace queries plan
// without one.
struct VecPtr { const void *p; int es; };
static inline int pick_vec(int cap, std::initializer_list<int64_t> whole, std::initializer_list<VecPtr> ptrs) {
  int vec = cap;
  for (; vec > 1; vec >>= 1) {
    bool ok = true;
    for (int64_t n : whole) ok = ok && n % vec == 0;
    for (const VecPtr &q : ptrs) ok = ok && (uintptr_t)q.p % (size_t)std::min(16, vec * q.es) == 0;
    if (ok) break;
  }
  return vec;
}

// ---- launches split at the launch limit ----
// f(first block, blocks of this launch): `blocks` blocks of `threads` threads
// in runs of at most max_blocks(threads)
template <typename F> void for_block_runs(int64_t blocks, int threads, F &&f) {
  const int64_t maxb = max_blocks(threads);
  for (int64_t b0 = 0; b0 < blocks; b0 += maxb) f(b0, (int)std::min(maxb, blocks - b0));
}
// f(first tile, grid of this launch): `tiles` (o, column tile) pairs in x by
// nchunks chunks in y, split over x so that grid.x * grid.y stays under the limit
template <typename F> void for_tile_runs(int64_t tiles, int64_t nchunks, int threads, F &&f) {
  const int64_t per = std::max<int64_t>(1, max_blocks(threads) / nchunks);
  for (int64_t t0 = 0; t0 < tiles; t0 += per)
    f(t0, dim3((unsigned)std::min(per, tiles - t0), (unsigned)nchunks));
}

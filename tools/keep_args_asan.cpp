// Host-side sanitizer run of bm_reduce_keep's argument validation: every call
// below is refused before any device work, so this runs without a GPU.
//
//   cd bolt_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/keep_args_asan.cpp bm_reduce.hip bm_api.hip -ldl -o /tmp/keep_args_asan && /tmp/keep_args_asan
//
// Exit status 0 and "keep_args_asan ok" when every call returned what it
// should and the sanitizers reported nothing.
#include <cstdio>
#include <cstring>

#include "bolt_mi355x.h"

static int fails = 0;

static void expect(int rc, int want, const char *msg_part, const char *what) {
  const char *err = bm_last_error();
  if (rc != want || (msg_part && !strstr(err, msg_part))) {
    fprintf(stderr, "FAIL %s: rc %d (want %d), error \"%s\" (want \"%s\")\n", what, rc, want, err,
            msg_part ? msg_part : "");
    ++fails;
  }
}

int main() {
  static char buf[4096];  // never dereferenced by the library: every call fails its checks
  void *p = buf;
  int kept = 7;
  const int F32 = BM_F32, F64 = BM_F64, I32 = BM_I32;
  expect(bm_reduce_keep(BM_STAT_MEAN, nullptr, F32, 2, 8, 1, 8, p, F32, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "null pointer", "null src");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, F32, 2, 8, 1, 8, nullptr, F32, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "null pointer", "null out");
  expect(bm_reduce_keep(BM_STAT_VAR, p, F32, 2, 8, 1, 8, p, F32, nullptr, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "null pointer", "null state");
  expect(bm_reduce_keep(BM_STAT_STD, p, F32, 2, 8, 1, 8, p, F32, p, nullptr, nullptr, 0, nullptr), BM_E_ARG,
         "null pointer", "null kept");
  expect(bm_reduce_keep(BM_STAT_STD, nullptr, F32, 2, 8, 1, 8, nullptr, F32, nullptr, nullptr, nullptr, 0, nullptr),
         BM_E_ARG, "null pointer", "all null");
  const int bad_stats[] = {BM_STAT_SUM, BM_STAT_MAX, BM_STAT_FMIN, -1, 99, 1 << 30};
  for (int s : bad_stats)
    expect(bm_reduce_keep(s, p, F32, 2, 8, 1, 8, p, F32, p, &kept, nullptr, 0, nullptr), BM_E_ARG, "stat", "stat");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, F32, 2, 8, 1, 8, p, I32, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "not a float dtype", "integer out_dtype");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, F32, 2, 8, 1, 8, p, -5, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "not a float dtype", "bad out_dtype");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, 99, 2, 8, 1, 8, p, F32, p, &kept, nullptr, 0, nullptr), BM_E_ARG, "dtype",
         "bad in_dtype");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, F32, 2, 8, 1, 7, p, F32, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "row_pitch", "pitch < R");
  expect(bm_reduce_keep(BM_STAT_VAR, p, F32, 2, 8, 4, 16, p, F64, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "row_pitch", "pitch with I > 1");
  expect(bm_reduce_keep(BM_STAT_VAR, p, F32, 2, 8, 1, -1, p, F64, p, &kept, nullptr, 0, nullptr), BM_E_ARG,
         "row_pitch", "negative pitch");
  const long long empty[][3] = {{0, 8, 1}, {2, 0, 1}, {2, 8, 0}, {-1, 8, 1}, {2, -8, 1}};
  for (auto &e : empty)
    expect(bm_reduce_keep(BM_STAT_STD, p, F32, e[0], e[1], e[2], e[1], p, F32, p, &kept, nullptr, 0, nullptr),
           BM_E_ARG, "empty reduction", "empty");
  if (kept != 7) {
    fprintf(stderr, "FAIL: kept written (%d) by a refused call\n", kept);
    ++fails;
  }
  // a chunked plan without its workspace: refused before any launch, nothing kept
  expect(bm_reduce_keep(BM_STAT_VAR, p, F32, 1, 200000, 1, 200000, p, F32, p, &kept, nullptr, 0, nullptr), BM_E_WS,
         "workspace too small", "chunked, no workspace");
  expect(bm_reduce_keep(BM_STAT_MEAN, p, F32, 1, 200000, 1, 200000, p, F32, p, &kept, p, 16, nullptr), BM_E_WS,
         "workspace too small", "chunked, short workspace");
  if (kept != 0) {
    fprintf(stderr, "FAIL: kept = %d after a chunked plan\n", kept);
    ++fails;
  }
  if (fails) return 1;
  puts("keep_args_asan ok");
  return 0;
}

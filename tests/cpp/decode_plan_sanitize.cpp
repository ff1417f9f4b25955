// Standalone sanitizer harness for the decode attention's host-only code
// (attn_decode_plan.h: argument checks and the split policy). Build with
//   c++ -std=c++17 -fsanitize=address,undefined decode_plan_sanitize.cpp
// and run; it sweeps shapes, CU counts and requested split counts and holds
// every plan to what the kernel relies on.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../../adapcc_amd/ops/csrc/attn_decode_plan.h"

using namespace adapcc;

static void require(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "decode_plan_sanitize: %s\n", what);
  std::exit(1);
}

static bool throws(long B, long H, long Hk, long Smax, long D) {
  try {
    decode_check_shapes("test", B, H, Hk, Smax, D);
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main() {
  long plans = 0;
  for (long B : {1L, 2L, 32L, 65535L})
    for (long Hk : {1L, 4L, 16L, 65535L})
      for (long Smax : {1L, 127L, 128L, 129L, 300L, 16384L, 1L << 30})
        for (int cu : {0, 1, 64, 256, 1 << 20})
          for (int req : {-1, 0, 1, 2, 3, 128, 129, 1 << 30}) {
            const DecodePlan p = decode_split_plan(B, Hk, Smax, cu, req);
            ++plans;
            require(p.n_splits >= 1, "n_splits >= 1");
            require(p.L >= kDecodeWgKeys && p.L % kDecodeWgKeys == 0,
                    "L a positive multiple of 128");
            // the splits cover the cache and none is wholly past it
            require((long)p.n_splits * p.L >= Smax, "splits cover Smax");
            require((long)(p.n_splits - 1) * p.L < Smax, "no split past Smax");
            require(req < 1 || p.n_splits <= req, "at most the count asked");
            require(req >= 1 || p.n_splits <= kDecodeMaxSplits, "policy cap");
            // asking for the count a plan gave returns that plan
            const DecodePlan again =
                decode_split_plan(B, Hk, Smax, cu, p.n_splits);
            require(again.n_splits == p.n_splits && again.L == p.L,
                    "a plan's count reproduces it");
          }
  require(!throws(2, 12, 1, 300, 64) && !throws(1, 32, 1, 1, 128),
          "valid shapes pass");
  require(throws(2, 12, 1, 300, 32), "head_dim 32 throws");
  require(throws(2, 64, 1, 300, 64), "G = 64 throws");
  require(throws(2, 12, 5, 300, 64), "H % Hk != 0 throws");
  require(throws(0, 12, 1, 300, 64) && throws(2, 12, 1, 0, 64),
          "empty shapes throw");
  require(throws(2, 12, 1, (1L << 30) + 1, 64), "Smax past 2^30 throws");
  std::printf("decode_plan_sanitize: %ld plans ok\n", plans);
  return 0;
}

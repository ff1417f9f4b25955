// Host-only part of the attention over a KV cache (attn_decode.hip,
// attn_extend.hip): the argument checks and the split policies. No device
// code and no HIP header, so tests/cpp/decode_plan_sanitize.cpp can build it
// with a host compiler under ASan + UBSan.
#pragma once

#include <stdexcept>
#include <string>

namespace adapcc {

// Keys one workgroup pass covers: 4 waves x one 32-key sub-tile each. A
// split is a multiple of it, so every split starts on a wave-0 sub-tile.
constexpr int kDecodeWgKeys = 128;
// Target: this many workgroups per CU over the whole launch, at most
// kDecodeMaxSplits splits of one (batch, K/V head), and no split shorter
// than kDecodeMinSplitKeys of capacity. Settled on the MI355X with
// benchmarks/attn_bench.py --shape decode --sweep
// (profiles/attn_decode_sweep.txt); the figures are in attn_decode.hip's
// header.
constexpr int kDecodeWgPerCu = 2;
constexpr int kDecodeMaxSplits = 16;
constexpr int kDecodeMinSplitKeys = 1024;
// Query heads per K/V head the kernel takes: the 32 columns of one MFMA tile.
constexpr int kDecodeMaxGroup = 32;

struct DecodePlan {
  int n_splits;  // workgroups along the keys of one (batch, K/V head)
  int L;         // keys per split, a multiple of kDecodeWgKeys
};

inline void decode_check_shapes(const char* name, long B, long H, long Hk,
                                long Smax, long head_dim) {
  const std::string n(name);
  if (B < 1 || H < 1 || Hk < 1 || Smax < 1)
    throw std::runtime_error(n + ": empty shape");
  if (head_dim != 64 && head_dim != 128)
    throw std::runtime_error(n + ": head_dim must be 64 or 128, got " +
                             std::to_string(head_dim));
  if (H % Hk != 0)
    throw std::runtime_error(n + ": n_kv_head must divide H, got H " +
                             std::to_string(H) + ", n_kv_head " +
                             std::to_string(Hk));
  if (H / Hk > kDecodeMaxGroup)
    throw std::runtime_error(n + ": at most 32 query heads per K/V head, "
                             "got " + std::to_string(H / Hk));
  // grid (n_splits, Hk, B), and int key indices up to Smax + L
  if (B > 65535 || Hk > 65535 || Smax > (1L << 30))
    throw std::runtime_error(n + ": shape too large");
}

// A paged cache: n_pages pages of page_size key rows, max_pages table entries
// per sequence. The kernels split a row index with a shift and a mask, so a
// page is a power of two, and at least the 16 rows of an MFMA operand
// fragment; the capacity max_pages * page_size obeys decode_check_shapes'
// bound on Smax. Returns log2(page_size).
inline int paged_check_shapes(const char* name, long n_pages, long page_size,
                              long max_pages) {
  const std::string n(name);
  if (page_size < 16 || (page_size & (page_size - 1)) != 0)
    throw std::runtime_error(n + ": the page size must be a power of two "
                             ">= 16, got " + std::to_string(page_size));
  if (n_pages < 1 || max_pages < 1)
    throw std::runtime_error(n + ": empty page pool or block table");
  if (page_size > (1L << 30) || max_pages > (1L << 30) / page_size ||
      n_pages > (1L << 30))
    throw std::runtime_error(n + ": paged shape too large");
  int lg = 4;
  while ((1L << lg) < page_size) ++lg;
  return lg;
}

// Splits of a cache of capacity Smax for a launch that has `groups`
// workgroups before any split. `requested` <= 0 is the policy: enough splits
// that groups * n_splits workgroups fill the chip wg_per_cu times over, at
// most max_splits of them and none under min_split_keys of capacity.
// `requested` >= 1 asks for that many. Either way a split is a multiple of
// 128 keys, so the count that comes back can be smaller than the one asked
// for. Shapes only: the lengths never enter, so nothing has to be read back
// from the device and a captured graph stays valid when the lengths change.
inline DecodePlan split_plan(long groups, long Smax, int n_cu, int requested,
                             int wg_per_cu, int max_splits,
                             int min_split_keys) {
  const long most = (Smax + kDecodeWgKeys - 1) / kDecodeWgKeys;
  long n = requested;
  if (n <= 0) {
    const long want = (long)wg_per_cu * (n_cu > 0 ? n_cu : 1);
    n = (want + groups - 1) / groups;
    if (n > max_splits) n = max_splits;
    if (n > Smax / min_split_keys) n = Smax / min_split_keys;
  }
  if (n > most) n = most;
  if (n < 1) n = 1;
  long L = (Smax + n - 1) / n;
  L = (L + kDecodeWgKeys - 1) / kDecodeWgKeys * kDecodeWgKeys;
  n = (Smax + L - 1) / L;
  return {(int)n, (int)L};
}

// Decode: one workgroup per (batch, K/V head) before the split.
inline DecodePlan decode_split_plan(long B, long Hk, long Smax, int n_cu,
                                    int requested) {
  return split_plan(B * Hk, Smax, n_cu, requested, kDecodeWgPerCu,
                    kDecodeMaxSplits, kDecodeMinSplitKeys);
}

// The multi-row kernel (attn_extend.hip): its launch has row_tiles =
// ceil(Sq * G / 128) independent workgroups per (batch, K/V head) before any
// split, which count to the policy as batch entries do. L, a multiple of
// 128, is a multiple of that kernel's 64-key tile. With decode's limits the
// policy was 13 to 39 % behind the best forced count wherever few workgroups
// meet a long cache (benchmarks/attn_bench.py --shape extend --sweep,
// profiles/attn_extend_split.txt; the figures are in attn_extend.hip's
// header): alone on its CU a workgroup of this kernel walks 1024 keys in 20
// to 30 us, several times the 6 us a second launch costs, so its splits go
// down to 256 keys and up to 32, the largest count measured. A cache under kExtendMinSmax keys is
// not split by the policy: the calls made before the split existed (Smax
// 1024 and under) keep their output bits, and the sweep has no shape with
// few workgroups there, so what they would gain is not measured.
constexpr int kExtendWgPerCu = 2;
constexpr int kExtendMaxSplits = 32;
constexpr int kExtendMinSplitKeys = 256;
constexpr int kExtendMinSmax = 2048;

inline DecodePlan extend_split_plan(long B, long Hk, long row_tiles,
                                    long Smax, int n_cu, int requested) {
  if (requested <= 0 && Smax < kExtendMinSmax) requested = 1;
  return split_plan(B * row_tiles * Hk, Smax, n_cu, requested,
                    kExtendWgPerCu, kExtendMaxSplits, kExtendMinSplitKeys);
}

}  // namespace adapcc

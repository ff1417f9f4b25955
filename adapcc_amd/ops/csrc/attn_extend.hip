// Multi-row attention over a KV cache (gfx950), bf16, head_dim 64 or 128: a
// block of Sq new query rows per sequence against that sequence's cached
// keys, grouped-query aware (chunked prefill, a second turn on a kept cache,
// a handful of drafted tokens, cross-attention). Forward only.
//
//   q        [B, H, Sq, D]       any batch/head/row strides, rows contiguous
//   k_cache  [B, Hk, Smax, D]    likewise
//   v_cache  [B, Hk, Smax, D]
//   seqlens  int32 [B] on the device: past_b = clamp(seqlens[b], 0, Smax)
//   q_lens   int32 [B] or null:       n_b = clamp(q_lens[b], 0, Sq), else Sq
//   out      [B, H, Sq, D]       any strides; lse fp32 [B, H, Sq] or null
//
// With new rows (k_new, v_new [B, Hk, Sq, D]) fa_cache_append_kernel first
// copies rows i < n_b into cache rows past_b + i (rows at or past Smax are
// dropped) and total_b = min(past_b + n_b, Smax); without, total_b = past_b.
// off_b = total_b - n_b. Causal: query row i < n_b sees keys 0 .. off_b + i
// (bottom-right aligned); non-causal: keys < total_b. A row i >= n_b, or one
// that sees no key, gives zeros and lse -inf, written by the kernel.
//
// The training forward (attn.hip) gives a workgroup 128 rows of one query
// head, so under GQA every K/V tile is staged once per query head, a prompt
// must be a multiple of 128 rows, and a chunk of 8 rows would leave three
// quarters of its MFMA columns empty. The decode kernel (attn_decode.hip)
// has one row per head. This kernel splits the work its own way:
//
//  * One workgroup serves one K/V head. The G = H / Hk query heads and the Sq
//    positions are flattened into group rows r = i * G + g, position-major,
//    so the causal limit off_b + r / G never falls as r grows. Grid
//    (ceil(Sq * G / 128), Hk, B); a workgroup takes 128 consecutive group
//    rows, 32 per wave: the 32 columns of S^T = K·Q^T
//    (v_mfma_f32_32x32x16_bf16, attn.hip's orientation). A lane owns one
//    (head, position) row; the online softmax in the exp2 domain is
//    lane-local. Every K/V tile that reaches LDS serves all G heads, so K/V
//    traffic and staging fall by G against the per-query-head forward, and 8
//    drafted tokens at G = 4 fill a wave. G need not divide 128 or 32: heads
//    of one position may sit in two waves or two workgroups; all that
//    follows uses r / G and r % G per lane and their extremes per wave.
//  * Q never touches LDS: a lane loads its row's 16-byte pieces from global
//    in operand order and keeps the D/16 fragments in registers. K and V go
//    through attn_frag.h's swizzled [32][64] row images (read_row_frag for K,
//    read_tr_frag for V^T, a 128-wide row as two images side by side), in
//    64-key tiles, double-buffered: the next tile's global loads are issued
//    before the current tile's MFMAs and written to the other buffer after
//    them, one barrier per tile. P returns to operand layout with pack_frag;
//    O^T = V^T·P^T sits in D/32 accumulators under one rescale.
//  * A workgroup whose positions are i0..i1 (cut at n_b - 1) walks tiles up
//    to key off_b + i1 when causal, total_b - 1 when not. Per wave and
//    32-key half, wave-uniformly: a half past the wave's largest limit is
//    skipped; a half that reaches past the wave's smallest limit (the
//    diagonal band, and the last, ragged tile) runs the masked code; every
//    other half runs the unmasked code. With a long cache nearly all do.
//  * Ragged: K/V rows are clamped to total_b - 1 and a padding lane repeats
//    the last valid group row of its sequence (loads, limit and all), so no
//    byte past a length is read and padding holds finite values; masked keys
//    are set to kNegBig before the running max. A wave that is all padding
//    skips MFMA and softmax but takes the barriers. A workgroup with no row
//    that sees a key writes its zeros and -inf and leaves before the first
//    barrier. All lengths are clamped on the device.
//  * Causal workgroups are issued heavy-first (blockIdx.x reversed): the
//    last rows walk the most tiles. The effect on the tail is not measured.
//  * A short chunk over a long cache would be a handful of workgroups, so
//    the keys are split as in decode: extend_split_plan (attn_decode_plan.h)
//    gives n_splits and L, a multiple of 128 keys, from the shapes alone,
//    never from the lengths (no host sync; a captured graph stays valid when
//    the lengths are refilled). n_splits == 1 is the launch above. Above 1
//    the grid is (row tiles * n_splits, Hk, B), the split the minor index;
//    the kSplit instantiation walks tiles of keys [split * L, (split + 1) * L)
//    cut at the workgroup's largest key. L is a multiple of the 64-key tile,
//    so the masking above, on absolute key indices, needs no new case. It
//    stores fp32 partials from the accumulators, 16 B per lane and store:
//    o_part[b, h, i, split, :], normalised by the split's own row sum, and
//    lse_part[b, h, i, split]. A row with no key in the split (its limit
//    under the split's start, padding, a dead row tile, a split past the
//    largest key) writes lse_part = -inf and no o_part; every lse_part entry
//    is written on every call, so the workspaces come uninitialised.
//    fa_extend_combine_kernel, one wave per output row, skips -inf splits,
//    weights the rest by exp(lse_s - lse_tot) in fp32, rounds once to bf16
//    through out's strides; a row with only -inf splits gets zeros and -inf.
//  * No atomics, no counters: deterministic.
//  * Paged cache (block_table != null; the kPaged instantiations): k_cache
//    and v_cache are pools [N, Hk, P, D], logical key row j of sequence b is
//    row j & (P - 1) of page table[b, j >> log2 P], and Smax = max_pages * P
//    feeds the clamps, the append's drop and the split plan. Paging changes
//    addresses only: the tile walk, masking, partials and combine are the
//    code above, so the output bits are those of the unpaged call on the
//    gathered slab. Every address goes through attn_cache.h's paged_offset,
//    after the row's clamp to total_b - 1 (no entry past a sequence's pages
//    is read) and with the entry clamped to [0, N - 1]. The staging threads
//    load rows srow and srow + 32 of a 64-key tile: with P >= 64 the tile
//    lies in one page and the lookup is one scalar load per tile, by the
//    tile's first key; with P 16 or 32 each thread looks up its two rows.
//    The lookup is a dependent load in front of the next tile's prefetch,
//    which the double buffer is left to hide: the entry for tile t + 2 is
//    not fetched ahead (not tried). Measured (profiles/attn_paged.txt,
//    contiguous / paged at P 16, 64, 256, us, two timings of one code within
//    0.3 %): B1 Sq 8 H16 Hk4 D128 over 16384 45.0 / 49.1, 47.8, 48.0; B8 Sq
//    512 H12 D64 over 3584 111 / 119, 116, 116. So the double buffer does
//    not hide all of it: 4 to 9 %, most at P 16 with its two vector lookups
//    a thread (reasoning, not a trace); against gathering the pages first (99 and 199 us) it is 1.7x
//    to 2x faster. The kPaged = false code is the parent's: its times
//    differ from a build of the parent by what two runs of one build do.
//
// Split policy, measured on one MI355X (256 CUs) with benchmarks/
// attn_bench.py --shape extend --sweep (profiles/attn_extend_split.txt: host
// clock over back-to-back calls ended by a synchronise, candidates
// alternating in one process, rounds within 1 % of each other but for two
// figures under 25 us at 6 %). Sq 8, causal, us per call at forced counts of 1
// / 2 / 4 / 8 / 16 / 32 (of which 11 and 26 are used over 4096 and 16384 keys):
//   B1  H16 Hk4  D128 over 16384   464 / 236 / 130 / 75.9 / 52.0 / 45.2
//   B1  H16 Hk1  D128 over 16384   492 / 245 / 126 / 74.4 / 50.8 / 44.4
//   B1  H12 Hk1  D64  over 16384   341 / 178 / 97.5 / 57.8 / 41.8 / 38.5
//   B1  H16 Hk4  D128 over 4096    112 / 65.2 / 40.0 / 28.5 / 24.2 / 25.0
//   B32 H16 Hk1  D128 over 16384   525 / 292 / 165 / 102 / 84.4 / 107
//   B32 H16 Hk4  D128 over 16384   569 / 316 / 189 / 212 / 240 / 261
//   B32 H16 Hk16 D128 over 16384   701 / 710 / 722 / 752 / 785 / 851
//   B8 Sq 512 H12 Hk12 D64 over 3584   119 / 111 / 121 / 150 / 231 / 512
// Under decode's constants (at most 16 splits, none under 1024 keys) the
// policy picked 4 splits over 4096 keys and 15 over 16384 and was 13 to 39 %
// behind the best forced count at B1 and at B32 Hk1 (B1 Hk4 D128 over 4096:
// 40.0 us against 24.2). Hence constants of its own: two workgroups per CU,
// at most 32 splits (the largest count measured), none under 256 keys. With
// them the policy is within 1.1 % of the best forced count at every shape of
// the sweep, which is also what two timings of the same launch differ by.
// The three shapes that lost to the composed SDPA route at one split (B1, 8
// rows over 16384 keys) now take 45.2 us against 450 (H16 Hk4 D128), 44.5
// against 411 (Hk1) and 38.3 against 269 (H12 Hk1 D64). Where the policy
// gives one split the time is the parent commit's to 0.5 %.
//
// Resources (gfx950; profiles/attn_extend_resources.txt): head_dim 64 126
// VGPRs, 32 KB LDS, 4 waves/SIMD by registers (three workgroups per CU
// asked for); head_dim 128 198 VGPRs, 64 KB LDS, 2 waves/SIMD; the split
// instantiations 120 and 196 VGPRs with the same LDS; the combine kernel 18
// and 19 VGPRs, no LDS; the paged instantiations 118 and 194 VGPRs, split
// 122 and 198, the same LDS and occupancy; the append kernel 18 VGPRs, paged
// 20; no scratch anywhere.
//
// Build: ops/build.py compiles this file with the packed fp32 VALU forms
// off (-packed-fp32-ops), the rule for new kernel files (STATUS.md, "Known
// limits").

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "attn_cache.h"
#include "attn_decode_plan.h"
#include "attn_frag.h"

namespace adapcc {

namespace {

constexpr int kRows = 128;          // group rows per workgroup, 32 per wave
constexpr int kHalfImg = 4096;      // attn_frag.h's [32][64] bf16 row image
constexpr int kImg = 2 * kHalfImg;  // 64 keys of one 64-column block

template <int kHD>
constexpr int kTileImg = (kHD / 64) * kImg;  // one 64-key tile, all blocks

struct ExtendParams {
  const __bf16* q;
  const __bf16 *k, *v;       // the caches
  const int* seqlens;        // [B]
  const int* q_lens;         // [B] or null
  long q_sb, q_sh, q_ss;     // element strides
  long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
  long o_sb, o_sh, o_ss;
  int H, G, Sq, Smax;
  int append;                // 1: the chunk's keys were appended at past_b
  int causal;
  float scale;
  __bf16* out;
  float* lse;                // [B, H, Sq], may be null
  int n_splits, L;           // key splits of a row tile, keys per split
  float* o_part;             // [B, H, Sq, n_splits, D]   n_splits > 1
  float* lse_part;           // [B, H, Sq, n_splits]      n_splits > 1
  PageMap pg;                // kPaged: k, v are pools, k_sb, v_sb page strides
};

// Staging: 256 threads copy a [64 keys][kHD] tile from global to LDS. Thread
// t moves the 16 B at column (t&7)*8 of every 64-column block of rows t>>3
// and (t>>3)+32: whole 128-B rows per eight lanes, held in registers across
// the current tile's compute.
template <int kHD>
struct RowTile {
  uint4 x[kHD / 32];  // per block: row srow, row srow + 32
};

template <int kHD>
__device__ __forceinline__ RowTile<kHD> ld_tile(const __bf16* g, long ss,
                                                int r0, int r1, int scol) {
  RowTile<kHD> t;
#pragma unroll
  for (int blk = 0; blk < kHD / 64; ++blk) {
    t.x[2 * blk] =
        *reinterpret_cast<const uint4*>(g + (long)r0 * ss + blk * 64 + scol);
    t.x[2 * blk + 1] =
        *reinterpret_cast<const uint4*>(g + (long)r1 * ss + blk * 64 + scol);
  }
  return t;
}

// kPaged: the same two rows of a tile whose first key is kt, found through
// the block table (attn_cache.h). r0 and r1 are clamped to the sequence's
// last key, which lies in the tile or past it, so they stay inside the tile:
// with 64 rows or more to a page the tile lies in one page and one
// wave-uniform (scalar) lookup by kt serves all lanes; with 16 or 32 each
// lane looks up its own two rows.
template <int kHD>
__device__ __forceinline__ RowTile<kHD> ld_tile_paged(
    const __bf16* g, const PageMap& pm, const int* trow, long sp, long ss,
    int kt, int r0, int r1, int scol) {
  long o0, o1;
  if (pm.lg >= 6) {
    o0 = paged_offset_in(pm, trow, kt, r0, sp, ss);
    o1 = paged_offset_in(pm, trow, kt, r1, sp, ss);
  } else {
    o0 = paged_offset(pm, trow, r0, sp, ss);
    o1 = paged_offset(pm, trow, r1, sp, ss);
  }
  RowTile<kHD> t;
#pragma unroll
  for (int blk = 0; blk < kHD / 64; ++blk) {
    t.x[2 * blk] = *reinterpret_cast<const uint4*>(g + o0 + blk * 64 + scol);
    t.x[2 * blk + 1] =
        *reinterpret_cast<const uint4*>(g + o1 + blk * 64 + scol);
  }
  return t;
}

template <int kHD>
__device__ __forceinline__ void st_tile(char* im, int srow, int scol,
                                        const RowTile<kHD>& t) {
  const int at = row_img_byte(srow, scol);
#pragma unroll
  for (int blk = 0; blk < kHD / 64; ++blk) {
    *reinterpret_cast<uint4*>(im + blk * kImg + at) = t.x[2 * blk];
    *reinterpret_cast<uint4*>(im + blk * kImg + kHalfImg + at) =
        t.x[2 * blk + 1];
  }
}

// ---------------------------------------------------------------------------
// Grid (ceil(Sq * G / 128), Hk, B), 256 threads = 4 waves; wave w owns group
// rows r0 + 32 w .. + 31 of K/V head blockIdx.y. kSplit: grid.x is row tile *
// n_splits + split, the workgroup walks keys [split * L, (split + 1) * L)
// only and stores fp32 partials; the arithmetic of a tile is the same.
// kPaged: K and V rows come from a page pool through the block table; only
// the two staging loads differ.
// ---------------------------------------------------------------------------
template <int kHD, bool kSplit, bool kPaged>
__global__ __launch_bounds__(256, kHD == 64 ? 3 : 2) void fa_extend_kernel(
    ExtendParams p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  constexpr int kNC = kHD / 16;  // 16-column chunks of a row
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  // 64-key tiles, double-buffered: K images, then V images
  __shared__ __attribute__((aligned(16))) char smem[4 * kTileImg<kHD>];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kTileImg<kHD>;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int G = p.G, H = p.H, Sq = p.Sq;
  // heavy-first: the last rows of a causal chunk walk the most tiles
  const int split = kSplit ? (int)(blockIdx.x % p.n_splits) : 0;
  const int tile = kSplit ? (int)(blockIdx.x / p.n_splits) : (int)blockIdx.x;
  const int ntiles = kSplit ? (int)(gridDim.x / p.n_splits) : (int)gridDim.x;
  const int bx = p.causal ? ntiles - 1 - tile : tile;
  const int k0 = kSplit ? split * p.L : 0;  // first key of this split

  const SeqLens sl = seq_lens(p.seqlens, p.q_lens, b, Sq, p.Smax, p.append);
  const int total = sl.total;
  const int off = total - sl.n;     // may be negative: an overfull cache
  const int nrows = sl.n * G;       // valid group rows of this sequence
  const int r0 = bx * kRows;
  const int rw = r0 + wave * 32;    // this wave's first group row

  // this lane's own row (where it stores) and the row it computes: padding
  // lanes repeat the sequence's last valid row
  const int r_own = rw + (lane & 31);
  const bool own = r_own < Sq * G;
  const int i_own = r_own / G;
  const int h_own = hk * G + (r_own - i_own * G);

  // largest key any row of this workgroup sees
  const int i1 = min((r0 + kRows - 1) / G, sl.n - 1);
  const int kmax = p.causal ? off + i1 : total - 1;
  // a split that starts past it has nothing to do, like a dead row tile
  const bool live = r0 < nrows && kmax >= k0;

  bool seen = false;                // does the computed row see a key
  float inv = 0.f, lse_v = -INFINITY;
  f32x16 acc0 = {}, acc1 = {};
  [[maybe_unused]] f32x16 acc2 = {}, acc3 = {};

  if (live) {  // workgroup-uniform: the barriers below are taken by all
    const int r = min(r_own, nrows - 1);
    const int i = r / G;
    const int h = hk * G + (r - i * G);
    const int lim = p.causal ? off + i : total - 1;  // last key this row sees
    // a row whose limit lies under the split sees none of its keys
    seen = r_own < nrows && lim >= k0;
    // the wave's extremes of lim: position-major rows make it monotone
    const bool wave_on = rw < nrows;
    const int wlo = p.causal ? off + rw / G : total - 1;
    const int whi =
        p.causal ? off + min(rw + 31, nrows - 1) / G : total - 1;

    // Q^T B-fragments, direct from global: lane l holds
    // Q[head h, position i][c*16 + 8*hi + e]
    const __bf16* qrow =
        p.q + (long)b * p.q_sb + (long)h * p.q_sh + (long)i * p.q_ss;
    bf16x8 qf[kNC];
#pragma unroll
    for (int c = 0; c < kNC; ++c)
      qf[c] = *reinterpret_cast<const bf16x8*>(qrow + c * 16 + hi * 8);

    // paged: the head's plane of the pool; the page comes per tile or row
    const __bf16* kg =
        p.k + (kPaged ? 0 : (long)b * p.k_sb) + (long)hk * p.k_sh;
    const __bf16* vg =
        p.v + (kPaged ? 0 : (long)b * p.v_sb) + (long)hk * p.v_sh;
    [[maybe_unused]] const int* trow =
        kPaged ? p.pg.table + (long)b * p.pg.max_pages : nullptr;
    const int klast = total - 1;    // >= 0 here; loads never go past it

    float m = kNegBig, ssum = 0.f;
    const float c1 = p.scale * kLog2e;
    float mc = m * c1;

    const int srow = threadIdx.x >> 3;       // staging: this thread's row
    const int scol = (threadIdx.x & 7) * 8;  // and column (bf16)
    // tiles t0 .. n64 - 1: L is a multiple of 64, so a split starts and
    // (unless kmax cuts it) ends on a tile boundary
    const int t0 = k0 / 64;
    const int n64 = (kSplit ? min(kmax, k0 + p.L - 1) : kmax) / 64 + 1;

    // prologue: stage the first tile
    if constexpr (kPaged) {
      const int kr0 = min(k0 + srow, klast);
      const int kr1 = min(k0 + srow + 32, klast);
      st_tile<kHD>(kimg, srow, scol,
                   ld_tile_paged<kHD>(kg, p.pg, trow, p.k_sb, p.k_ss, k0, kr0,
                                      kr1, scol));
      st_tile<kHD>(vimg, srow, scol,
                   ld_tile_paged<kHD>(vg, p.pg, trow, p.v_sb, p.v_ss, k0, kr0,
                                      kr1, scol));
    } else {
      st_tile<kHD>(kimg, srow, scol,
                   ld_tile<kHD>(kg, p.k_ss, min(k0 + srow, klast),
                                min(k0 + srow + 32, klast), scol));
      st_tile<kHD>(vimg, srow, scol,
                   ld_tile<kHD>(vg, p.v_ss, min(k0 + srow, klast),
                                min(k0 + srow + 32, klast), scol));
    }
    __syncthreads();

    int cur = 0;
    for (int t = t0; t < n64; ++t) {
      // the next tile's loads fly during this one's compute
      RowTile<kHD> nk, nv;
      const bool pref = t + 1 < n64;
      if (pref) {
        const int kr0 = min((t + 1) * 64 + srow, klast);
        const int kr1 = min((t + 1) * 64 + srow + 32, klast);
        if constexpr (kPaged) {
          nk = ld_tile_paged<kHD>(kg, p.pg, trow, p.k_sb, p.k_ss,
                                  (t + 1) * 64, kr0, kr1, scol);
          nv = ld_tile_paged<kHD>(vg, p.pg, trow, p.v_sb, p.v_ss,
                                  (t + 1) * 64, kr0, kr1, scol);
        } else {
          nk = ld_tile<kHD>(kg, p.k_ss, kr0, kr1, scol);
          nv = ld_tile<kHD>(vg, p.v_ss, kr0, kr1, scol);
        }
      }

#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int kbase = t * 64 + half * 32;
        // wave-uniform: all padding, or no row of the wave sees this half
        if (!wave_on || kbase > whi) break;
        const char* ki = kimg + cur * kTileImg<kHD> + half * kHalfImg;
        const char* vi = vimg + cur * kTileImg<kHD> + half * kHalfImg;

        // S^T tile: C[key][row] = sum_d K[key][d] * Q[row][d]
        f32x16 s = {};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < kNC; ++c)
          s = mfma(read_row_frag(ki + (c >> 2) * kImg, lane, c & 3), qf[c],
                   s);
        __builtin_amdgcn_s_setprio(0);

        // attn_cache.h's cache_tile_step plus the s_setprio pair, written
        // out: the call cost registers (128 / 208 VGPRs for 126 / 198) and
        // 1.2 % at one D 128 shape (profiles/README.md, "Shared header").
        float pv[16];
        float tmax = kNegBig;
        if (kbase + 31 > wlo) {
          // the band of this wave's limits, or the ragged last tile
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            pv[x] = kbase + crow(x, hi) > lim ? kNegBig : s[x];
            tmax = fmaxf(tmax, pv[x]);
          }
        } else {
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            pv[x] = s[x];
            tmax = fmaxf(tmax, pv[x]);
          }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        if (!__all(tmax <= m)) {
          const float mnew = fmaxf(m, tmax);
          const float alpha = __builtin_amdgcn_exp2f((m - mnew) * c1);
          m = mnew;
          mc = m * c1;
          ssum *= alpha;
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            acc0[x] *= alpha;
            acc1[x] *= alpha;
            if constexpr (kNB == 4) {
              acc2[x] *= alpha;
              acc3[x] *= alpha;
            }
          }
        }

        // P = exp2(S*c1 - mc). A row that has seen no key yet (negative
        // limit) holds m = kNegBig and gets P = 1 here: finite, lane-local,
        // and thrown away in the epilogue.
        float psum = 0.f;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
          pv[x] = __builtin_amdgcn_exp2f(__builtin_fmaf(pv[x], c1, -mc));
          psum += pv[x];
        }
        ssum += psum;

        // P to operand fragments (keys 0-15 / 16-31), then
        // O^T += V^T · P^T with V^T from hardware transpose reads
        const bf16x8 p0 = pack_frag(&pv[0]);
        const bf16x8 p1 = pack_frag(&pv[8]);
        __builtin_amdgcn_s_setprio(1);
        acc0 = mfma(read_tr_frag(vi, lane, 0, 0), p0, acc0);
        acc0 = mfma(read_tr_frag(vi, lane, 1, 0), p1, acc0);
        acc1 = mfma(read_tr_frag(vi, lane, 0, 1), p0, acc1);
        acc1 = mfma(read_tr_frag(vi, lane, 1, 1), p1, acc1);
        if constexpr (kNB == 4) {
          acc2 = mfma(read_tr_frag(vi + kImg, lane, 0, 0), p0, acc2);
          acc2 = mfma(read_tr_frag(vi + kImg, lane, 1, 0), p1, acc2);
          acc3 = mfma(read_tr_frag(vi + kImg, lane, 0, 1), p0, acc3);
          acc3 = mfma(read_tr_frag(vi + kImg, lane, 1, 1), p1, acc3);
        }
        __builtin_amdgcn_s_setprio(0);
      }

      if (pref) {
        st_tile<kHD>(kimg + (cur ^ 1) * kTileImg<kHD>, srow, scol, nk);
        st_tile<kHD>(vimg + (cur ^ 1) * kTileImg<kHD>, srow, scol, nv);
      }
      __syncthreads();
      cur ^= 1;
    }

    const float stot = ssum + __shfl_xor(ssum, 32, 64);
    if (seen) {
      inv = 1.f / stot;
      lse_v = p.scale * m + __builtin_amdgcn_logf(stot) * kLn2;
    }
  }

  // epilogue: stores only. Rows past n_b and rows that saw no key get
  // explicit zeros and -inf: the output was allocated uninitialised.
  if (!own) return;
  if constexpr (kSplit) {
    // fp32 partial, normalised by this split's row sum, straight from the
    // accumulators: a lane holds 4 consecutive d per (db, mq). A row without
    // a key in this split leaves -inf and its o_part row unwritten.
    const long at =
        (((long)b * H + h_own) * Sq + i_own) * p.n_splits + split;
    if (hi == 0) p.lse_part[at] = lse_v;
    if (!seen) return;
    float* orow = p.o_part + at * kHD;
#pragma unroll
    for (int db = 0; db < kNB; ++db) {
      const f32x16& a = db == 3 ? acc3 : db == 2 ? acc2 : db ? acc1 : acc0;
#pragma unroll
      for (int mq = 0; mq < 4; ++mq)
        *reinterpret_cast<float4*>(orow + db * 32 + 8 * mq + 4 * hi) =
            make_float4(a[4 * mq] * inv, a[4 * mq + 1] * inv,
                        a[4 * mq + 2] * inv, a[4 * mq + 3] * inv);
    }
    return;
  }
  if (hi == 0 && p.lse != nullptr)
    p.lse[((long)b * H + h_own) * Sq + i_own] = lse_v;
  __bf16* orow = p.out + (long)b * p.o_sb + (long)h_own * p.o_sh +
                 (long)i_own * p.o_ss;
#pragma unroll
  for (int db = 0; db < kNB; ++db) {
    const f32x16& a = db == 3 ? acc3 : db == 2 ? acc2 : db ? acc1 : acc0;
#pragma unroll
    for (int mq = 0; mq < 4; ++mq) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = seen ? a[4 * mq + e] * inv : 0.f;
      store4_bf16(orow + db * 32 + 8 * mq + 4 * hi, o[0], o[1], o[2], o[3]);
    }
  }
}

// ---------------------------------------------------------------------------
// Merge of the splits: one wave per output row (b, h, i), four rows per
// workgroup: blockIdx.x * 4 + wave runs over the B * H * Sq rows in
// lse_part's order. Lane l owns kHD/64 consecutive columns. A split with
// lse_part = -inf is skipped and its o_part never read; a row with only
// such splits gets zeros and lse -inf. Weights and sums in fp32, one
// rounding to bf16, written through out's (b, h, row) strides.
// ---------------------------------------------------------------------------
template <int kHD>
__global__ __launch_bounds__(256) void fa_extend_combine_kernel(
    const float* o_part, const float* lse_part, __bf16* out, float* lse,
    long rows, int H, int Sq, int n_splits, long o_sb, long o_sh, long o_ss) {
  constexpr int kPer = kHD / 64;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* lp = lse_part + row * n_splits;
  float mx = -INFINITY;
  for (int s = 0; s < n_splits; ++s) mx = fmaxf(mx, lp[s]);
  float acc[kPer] = {};
  float tot = -INFINITY;
  if (mx > -INFINITY) {
    float sum = 0.f;
    for (int s = 0; s < n_splits; ++s)
      if (lp[s] > -INFINITY) sum += expf(lp[s] - mx);
    tot = mx + logf(sum);
    for (int s = 0; s < n_splits; ++s) {
      if (!(lp[s] > -INFINITY)) continue;
      const float w = expf(lp[s] - tot);
      const float* op = o_part + (row * n_splits + s) * kHD + lane * kPer;
#pragma unroll
      for (int j = 0; j < kPer; ++j) acc[j] += w * op[j];
    }
  }
  const long bh = row / Sq;
  const long i = row - bh * Sq;
  const long b = bh / H;
  __bf16* dst = out + b * o_sb + (bh - b * H) * o_sh + i * o_ss + lane * kPer;
#pragma unroll
  for (int j = 0; j < kPer; ++j) dst[j] = (__bf16)acc[j];
  if (lane == 0 && lse != nullptr) lse[row] = tot;
}

template <int kHD, bool kPaged>
void launch_extend(const ExtendParams& p, long row_tiles, int Hk, int B,
                   hipStream_t stream) {
  if (p.n_splits == 1) {
    hipLaunchKernelGGL((fa_extend_kernel<kHD, false, kPaged>),
                       dim3((unsigned)row_tiles, Hk, B), dim3(256), 0, stream,
                       p);
    return;
  }
  hipLaunchKernelGGL((fa_extend_kernel<kHD, true, kPaged>),
                     dim3((unsigned)(row_tiles * p.n_splits), Hk, B),
                     dim3(256), 0, stream, p);
  const long rows = (long)B * p.H * p.Sq;
  hipLaunchKernelGGL(fa_extend_combine_kernel<kHD>,
                     dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream,
                     p.o_part, p.lse_part, p.out, p.lse, rows, p.H, p.Sq,
                     p.n_splits, p.o_sb, p.o_sh, p.o_ss);
}

// ---------------------------------------------------------------------------
// In-place cache update, for this file and (at Sq = 1) attn_decode.hip. Grid
// (ceil(Sq * D/4 / 256), Hk, B): thread e of a (batch, K/V head) moves 16 B;
// a row is D/8 pieces of k, then D/8 of v. Rows i >= n_b and rows that would
// land at or past Smax are left alone.
// ---------------------------------------------------------------------------
struct AppendParams {
  __bf16 *k, *v;
  const __bf16 *kn, *vn;
  const int *seqlens, *q_lens;
  long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
  long kn_sb, kn_sh, kn_ss, vn_sb, vn_sh, vn_ss;
  int Sq, Smax, D;
  PageMap pg;  // kPaged: k, v are pools, k_sb, v_sb their page strides
};

template <bool kPaged>
__global__ __launch_bounds__(256) void fa_cache_append_kernel(
    AppendParams p) {
  const int hk = blockIdx.y, b = blockIdx.z;
  const SeqLens sl = seq_lens(p.seqlens, p.q_lens, b, p.Sq, p.Smax, 1);
  const int per = p.D / 8;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int i = e / (2 * per);
  const int piece = e - i * 2 * per;
  const int row = sl.past + i;
  if (i >= sl.n || row >= p.Smax) return;
  if constexpr (kPaged) {
    // 0 <= row < max_pages * P: the entry is one of the table row's
    const int* trow = p.pg.table + (long)b * p.pg.max_pages;
    if (piece < per)
      *reinterpret_cast<uint4*>(
          p.k + (long)hk * p.k_sh +
          paged_offset(p.pg, trow, row, p.k_sb, p.k_ss) + piece * 8) =
          *reinterpret_cast<const uint4*>(p.kn + (long)b * p.kn_sb +
                                          (long)hk * p.kn_sh +
                                          (long)i * p.kn_ss + piece * 8);
    else
      *reinterpret_cast<uint4*>(
          p.v + (long)hk * p.v_sh +
          paged_offset(p.pg, trow, row, p.v_sb, p.v_ss) + (piece - per) * 8) =
          *reinterpret_cast<const uint4*>(p.vn + (long)b * p.vn_sb +
                                          (long)hk * p.vn_sh +
                                          (long)i * p.vn_ss +
                                          (piece - per) * 8);
    return;
  }
  if (piece < per)
    *reinterpret_cast<uint4*>(p.k + (long)b * p.k_sb + (long)hk * p.k_sh +
                              (long)row * p.k_ss + piece * 8) =
        *reinterpret_cast<const uint4*>(p.kn + (long)b * p.kn_sb +
                                        (long)hk * p.kn_sh +
                                        (long)i * p.kn_ss + piece * 8);
  else
    *reinterpret_cast<uint4*>(p.v + (long)b * p.v_sb + (long)hk * p.v_sh +
                              (long)row * p.v_ss + (piece - per) * 8) =
        *reinterpret_cast<const uint4*>(p.vn + (long)b * p.vn_sb +
                                        (long)hk * p.vn_sh +
                                        (long)i * p.vn_ss + (piece - per) * 8);
}

}  // namespace

// ---------------------------------------------------------------------------
// Host side. Nothing here reads the lengths. fa_cache_append: attn_cache.h
// describes the arguments.
// ---------------------------------------------------------------------------
void fa_cache_append(void* k_cache, void* v_cache, const void* k_new,
                     const void* v_new, const int* seqlens, const int* q_lens,
                     const long* cache_strides, const long* new_strides, int B,
                     int Hk, int Sq, int Smax, int head_dim,
                     const PageMap& pages, hipStream_t stream) {
  AppendParams a = {};
  a.k = (__bf16*)k_cache;
  a.v = (__bf16*)v_cache;
  a.kn = (const __bf16*)k_new;
  a.vn = (const __bf16*)v_new;
  a.seqlens = seqlens;
  a.q_lens = q_lens;
  a.k_sb = cache_strides[0], a.k_sh = cache_strides[1];
  a.k_ss = cache_strides[2];
  a.v_sb = cache_strides[3], a.v_sh = cache_strides[4];
  a.v_ss = cache_strides[5];
  a.kn_sb = new_strides[0], a.kn_sh = new_strides[1], a.kn_ss = new_strides[2];
  a.vn_sb = new_strides[3], a.vn_sh = new_strides[4], a.vn_ss = new_strides[5];
  a.Sq = Sq;
  a.Smax = Smax;
  a.D = head_dim;
  a.pg = pages;
  const long pieces = (long)Sq * (head_dim / 4);
  const dim3 grid((unsigned)((pieces + 255) / 256), Hk, B);
  if (pages.table != nullptr)
    hipLaunchKernelGGL(fa_cache_append_kernel<true>, grid, dim3(256), 0,
                       stream, a);
  else
    hipLaunchKernelGGL(fa_cache_append_kernel<false>, grid, dim3(256), 0,
                       stream, a);
}

// attn_cache.h describes the arguments: the launch of launch_extend's second
// step, for attn_extend_fp8.hip.
void fa_extend_combine(const float* o_part, const float* lse_part, void* out,
                       float* lse, int B, int H, int Sq, int n_splits,
                       int head_dim, long o_sb, long o_sh, long o_ss,
                       hipStream_t stream) {
  const long rows = (long)B * H * Sq;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (head_dim == 64)
    hipLaunchKernelGGL(fa_extend_combine_kernel<64>, grid, dim3(256), 0,
                       stream, o_part, lse_part, (__bf16*)out, lse, rows, H,
                       Sq, n_splits, o_sb, o_sh, o_ss);
  else
    hipLaunchKernelGGL(fa_extend_combine_kernel<128>, grid, dim3(256), 0,
                       stream, o_part, lse_part, (__bf16*)out, lse, rows, H,
                       Sq, n_splits, o_sb, o_sh, o_ss);
}

// The split count the policy (num_splits <= 0) or the caller (>= 1) gets for
// these shapes (G = H / Hk) on `device`, the tensors' device index: the size
// of the o_part / lse_part workspaces.
int fa_extend_splits(int B, int Hk, int Sq, int G, int Smax, int num_splits,
                     int device) {
  if (B < 1 || Hk < 1 || Sq < 1 || G < 1 || Smax < 1)
    throw std::runtime_error("fa_extend_splits: empty shape");
  const DeviceScope scope("fa_extend", device);
  return extend_split_plan(B, Hk, ((long)Sq * G + kRows - 1) / kRows, Smax,
                           device_cu_count("fa_extend"), num_splits)
      .n_splits;
}

// Bound in bindings.hip. strides (elements): q, k_cache, v_cache, out (b, h,
// row each), then k_new, v_new (b, h, row each): 18 values. lse: fp32
// [B, H, Sq] or null; q_lens: int32 [B] or null. k_new and v_new: both or
// neither; with them rows i < n_b are appended at seqlens[b] + i first and
// the attention counts them. n_splits: what fa_extend_splits answered; above
// 1, o_part is fp32 [B, H, Sq, n_splits, head_dim] and lse_part fp32
// [B, H, Sq, n_splits], neither initialised. device: the tensors' device
// index, made current for the call; `stream` is one of its streams.
// block_table: null, or int32 [B, max_pages] on the device; then k_cache and
// v_cache are pools of n_pages pages of page_size rows, their strides are
// (page, head, row) and Smax is max_pages * page_size.
void fa_extend(const void* q, void* k_cache, void* v_cache,
               const int* seqlens, const int* q_lens, const void* k_new,
               const void* v_new, void* out, float* lse, int B, int H, int Hk,
               int Sq, int Smax, int head_dim, const long* strides,
               float scale, bool causal, int n_splits, float* o_part,
               float* lse_part, const int* block_table, int n_pages,
               int page_size, int max_pages, int device, hipStream_t stream) {
  decode_check_shapes("fa_extend", B, H, Hk, Smax, head_dim);
  const PageMap pages = make_page_map("fa_extend", block_table, n_pages,
                                      page_size, max_pages, Smax);
  const long G = H / Hk;
  // group rows and the append's piece index stay inside int arithmetic
  if (Sq < 1 || (long)Sq * G > (1L << 30) ||
      (long)Sq * (head_dim / 4) > (1L << 30))
    throw std::runtime_error("fa_extend: Sq must be >= 1 and Sq * (H / Hk) "
                             "at most 2^30, got Sq " + std::to_string(Sq));
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr ||
      seqlens == nullptr || out == nullptr)
    throw std::runtime_error("fa_extend: null pointer");
  if ((k_new == nullptr) != (v_new == nullptr))
    throw std::runtime_error("fa_extend: k_new and v_new go together");
  const DeviceScope scope("fa_extend", device);
  const long row_tiles = ((long)Sq * G + kRows - 1) / kRows;
  const DecodePlan plan = extend_split_plan(
      B, Hk, row_tiles, Smax, device_cu_count("fa_extend"), n_splits);
  if (n_splits < 1 || plan.n_splits != n_splits)
    throw std::runtime_error("fa_extend: n_splits " +
                             std::to_string(n_splits) +
                             " is not a split count of this shape");
  if (n_splits > 1 && (o_part == nullptr || lse_part == nullptr))
    throw std::runtime_error("fa_extend: split workspaces missing");
  // grid.x of the split launch and of the combine (four rows a workgroup)
  if (n_splits > 1 && (row_tiles * n_splits > (1L << 30) ||
                       (long)B * H * Sq > (1L << 32)))
    throw std::runtime_error("fa_extend: shape too large to split");

  ExtendParams p = {};
  p.q = (const __bf16*)q;
  p.k = (const __bf16*)k_cache;
  p.v = (const __bf16*)v_cache;
  p.seqlens = seqlens;
  p.q_lens = q_lens;
  p.q_sb = strides[0], p.q_sh = strides[1], p.q_ss = strides[2];
  p.k_sb = strides[3], p.k_sh = strides[4], p.k_ss = strides[5];
  p.v_sb = strides[6], p.v_sh = strides[7], p.v_ss = strides[8];
  p.o_sb = strides[9], p.o_sh = strides[10], p.o_ss = strides[11];
  p.H = H;
  p.G = (int)G;
  p.Sq = Sq;
  p.Smax = Smax;
  p.append = k_new != nullptr;
  p.causal = causal;
  p.scale = scale;
  p.out = (__bf16*)out;
  p.lse = lse;
  p.n_splits = n_splits;
  p.L = plan.L;
  p.o_part = o_part;
  p.lse_part = lse_part;
  p.pg = pages;

  if (k_new != nullptr)
    fa_cache_append(k_cache, v_cache, k_new, v_new, seqlens, q_lens,
                    strides + 3, strides + 12, B, Hk, Sq, Smax, head_dim,
                    pages, stream);
  const bool paged = pages.table != nullptr;
  if (head_dim == 64)
    paged ? launch_extend<64, true>(p, row_tiles, Hk, B, stream)
          : launch_extend<64, false>(p, row_tiles, Hk, B, stream);
  else
    paged ? launch_extend<128, true>(p, row_tiles, Hk, B, stream)
          : launch_extend<128, false>(p, row_tiles, Hk, B, stream);
}

}  // namespace adapcc

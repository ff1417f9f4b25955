// Multi-row attention over an FP8 (e4m3, OCP) KV cache (gfx950), head_dim 64
// or 128: attn_extend.hip's call with the caches stored as in
// attn_decode_fp8.hip. Forward only.
//
//   q        [B, H, Sq, D] bf16   any batch/head/row strides, rows contiguous
//   k_cache  [B, Hk, Smax, D]     e4m3 bytes, any batch/head/row strides, rows
//   v_cache  [B, Hk, Smax, D]     contiguous and 16-B aligned (16 elements);
//                                 with a block table, pools [N, Hk, P, D]
//   k_scale  fp32 [Hk], v_scale fp32 [Hk], on the device, > 0: a stored byte
//            c of K/V head hk stands for float(c) * scale[hk]
//   seqlens, q_lens, out, lse: as in attn_extend.hip, and so are the
//            semantics (bottom-right causal or not, zeros and lse -inf for a
//            row past n_b or one that sees no key)
//
// With new rows (k_new, v_new, bf16) fa_cache_append_fp8 quantises and writes
// them first, and the chunk's own keys are attended as stored: a prompt gives
// the same attention inputs however it is cut into chunks. (A bf16 prefill
// followed by kv_cache_append differs: there the prompt attends over the
// unquantised keys.)
//
// The work split is attn_extend.hip's, unchanged: one workgroup per (row tile
// of 128 group rows r = i * G + g, K/V head, batch), 32 rows per wave, causal
// row tiles heavy-first; the per-wave skip / masked / unmasked choice for each
// 32-key half; extend_split_plan, the fp32 partials and the combine kernel
// (fa_extend_combine); Q straight from global into registers; K and V as
// swizzled bf16 [32][64] row images in LDS, 64-key tiles, double-buffered, one
// barrier a tile, read with read_row_frag / read_tr_frag; rows clamped to
// total_b - 1 before any address is formed, so no byte past a length and no
// table entry past a sequence's pages is read. e4m3 -> bf16 is exact, so the
// MFMAs see the stored code values and the roundings are the bf16 kernel's.
// What is new is how bytes reach LDS:
//
//  * Staging map. A [64 keys][D] tile is 64 * D bytes, and a thread's load is
//    one global_load_dwordx4: 16 codes, 16 columns of one key row. A row is
//    D/16 pieces, so the 256 threads cover 64 rows (D 64) or 32 (D 128) per
//    load: thread t takes piece t % (D/16) of row t / (D/16) + (4096/D) j,
//    j < D/64. That is one load of K and one of V a tile at D 64, two each at
//    D 128: D/32 dwords in flight for the next tile against the bf16
//    kernel's D/8.
//  * Conversion once per workgroup, at the store to LDS: the 16 codes become
//    two bf16x8 (attn_cache.h's cvt8, v_cvt_scalef32_pk_bf16_fp8 at scale
//    1.0) and go to two 16-B slots of the row image (row_img_byte at columns
//    c and c + 8). D/4 conversion instructions per thread and tile serve all
//    128 query rows; the four waves then read bf16 fragments as in
//    attn_extend.hip. Q keeps that kernel's load: K goes through LDS, so
//    decode-fp8's permuted contraction index has no use here.
//  * Scales cost nothing per element: k_scale[hk] rides on c1 = scale *
//    k_scale * log2(e) and on the scale * m term of the lse, v_scale[hk] on
//    the 1 / l of the epilogue, which normalises the direct bf16 store and
//    the fp32 partials alike, so the combine kernel is attn_extend.hip's.
//  * Paged (kPaged): a wave's 64 threads hold 64 / (D/16) = 16 or 8
//    consecutive rows of the tile per load, starting at a multiple of their
//    count, so (a page being a power of two >= 16 rows) they lie in one page,
//    and after the clamp to total_b - 1 still do: the clamped rows are either
//    all that last row or lie between the wave's first row and it. The lookup
//    is therefore always wave-uniform, one table entry a wave: with P >= 64
//    one per tile, by the tile's first key; with P 16 or 32 one per load j,
//    by the wave's own first row, clamped (the bf16 kernel's rows t>>3 and
//    t>>3 + 32 need a per-lane lookup there). By the ISA the prologue's is a
//    scalar load and the loop's a one-address vector load followed by
//    v_readfirstlane. Addresses are paged_offset_in
//    with the pool's byte strides. Every offset of a tile, K's and V's, is
//    formed before its first load is issued: an offset waits for its table
//    entry, and a wait placed between the loads would also wait for the
//    loads ahead of it (attn_decode_fp8.hip's ld_kv).
//  * The span from the score tile to the last PV MFMA is written out, as in
//    attn_extend.hip, not a call of attn_cache.h's cache_tile_step. The
//    compiler's report decided: with the call head_dim 64 took 129 to 132
//    VGPRs, 3 waves/SIMD where the bf16 kernel has 4 (head_dim 128: 205 to
//    207, 2 waves/SIMD either way); written out it is 116 to 122 and 4. The
//    two forms were not timed against each other.
//
// Not tried: e4m3 kept in LDS (half the LDS, twice the tiles in flight) with
// the conversion at fragment read; every wave would then convert the whole
// tile, four times the conversion instructions.
//
// Resources (gfx950, this build's flags, from the compiler's report;
// profiles/attn_extend_fp8.txt), one split / split, then the same paged:
// head_dim 64 121 / 116 and 122 / 118 VGPRs, 32 KB LDS, 4 waves/SIMD;
// head_dim 128 188 / 186 and 188 / 188 VGPRs, 64 KB LDS, 2 waves/SIMD; no
// scratch anywhere. LDS and occupancy are the bf16 kernel's (126 and 198
// VGPRs there): the images hold bf16 either way, and the halved prefetch
// gives back 5 to 10 registers.
//
// Measured on one MI355X (profiles/attn_extend_fp8.txt; benchmarks/
// attn_bench.py --shape extend --fp8: fp8 and bf16 alternating in one process,
// the bf16 call timed twice within 0.4 %, one run; causal, the policy's split
// counts, which are bf16's: whether halved bytes move the best count is not
// measured), fp8 against bf16, us:
//   B32 Sq 8   H16 Hk16 D128 over 16384   547 / 749  (0.73; byte-bound)
//   B1  Sq 8   H16 Hk4  D128 over 16384   41.6 / 43.6  (0.95; 32 splits)
//   B8  Sq 512 H12 Hk12 D64  over 3584    97.6 / 100.4  (0.97; compute-bound)
// The byte-bound shape gains 27 % but stays far from the byte ratio 0.5 (3.93
// TB/s of its own bytes against bf16's 5.74): one tile in flight per
// workgroup is half the bytes in flight per CU, at the same two workgroups a
// CU that the bf16 images in LDS allow, and the conversion sits between a
// tile's arrival and its barrier (reasoning, not a counter run). A prefetch
// two tiles deep is not tried. At the compute-bound shape the conversion was
// expected to cost time; it does not show (2.7 % faster, noise 0.4 %). Paged
// at P 16 costs 8 % at the first shape and 2 % at the others (bf16: 0.4 and
// 7 %).
//
// Build: as attn_extend.hip, with the packed fp32 VALU forms off
// (ops/build.py).

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

struct ExtendFp8Params {
  const __bf16* q;
  const uint8_t *k, *v;      // the caches, e4m3 bytes
  const float *k_scale, *v_scale;  // [Hk]
  const int* seqlens;        // [B]
  const int* q_lens;         // [B] or null
  long q_sb, q_sh, q_ss;     // element strides
  long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;  // bytes
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

// The staging map: thread t owns piece t % kPieces (16 columns) of tile rows
// t / kPieces + kStep * j, j < kLoads.
template <int kHD>
struct Stage {
  static constexpr int kPieces = kHD / 16;     // 16-B pieces of a row
  static constexpr int kStep = 256 / kPieces;  // rows one load covers
  static constexpr int kLoads = 64 / kStep;    // loads of K (and of V) a tile
  static constexpr int kWaveRows = 64 / kPieces;  // consecutive rows a wave
};

// A thread's raw bytes of one 64-key tile, K and V, held in registers across
// the current tile's compute.
template <int kHD>
struct RawTile {
  uint4 k[Stage<kHD>::kLoads], v[Stage<kHD>::kLoads];
};

// The loads of the tile whose first key is kt. Rows are clamped to klast, the
// sequence's last key, which lies in the tile or past it. kPaged: the page of
// a load's rows is found once per wave (see the header); urow, the row that
// names it, is wave-uniform. All offsets first, then all loads.
template <int kHD, bool kPaged>
__device__ __forceinline__ void ld_kv(RawTile<kHD>& t, const uint8_t* kg,
                                      const uint8_t* vg, const PageMap& pm,
                                      const int* trow, long k_sp, long k_ss,
                                      long v_sp, long v_ss, int kt, int klast,
                                      int tid, int wave) {
  using S = Stage<kHD>;
  const int srow = tid / S::kPieces;
  const int sbyte = (tid % S::kPieces) * 16;
  long ko[S::kLoads], vo[S::kLoads];
#pragma unroll
  for (int j = 0; j < S::kLoads; ++j) {
    const int row = min(kt + srow + S::kStep * j, klast);
    if constexpr (kPaged) {
      const int urow = __builtin_amdgcn_readfirstlane(
          pm.lg >= 6
              ? kt
              : min(kt + wave * S::kWaveRows + S::kStep * j, klast));
      ko[j] = paged_offset_in(pm, trow, urow, row, k_sp, k_ss) + sbyte;
      vo[j] = paged_offset_in(pm, trow, urow, row, v_sp, v_ss) + sbyte;
    } else {
      ko[j] = (long)row * k_ss + sbyte;
      vo[j] = (long)row * v_ss + sbyte;
    }
  }
#pragma unroll
  for (int j = 0; j < S::kLoads; ++j)
    t.k[j] = *reinterpret_cast<const uint4*>(kg + ko[j]);
#pragma unroll
  for (int j = 0; j < S::kLoads; ++j)
    t.v[j] = *reinterpret_cast<const uint4*>(vg + vo[j]);
}

// One 16-B piece, dequantised, into the tile's images: row 0..63 of the tile
// is row & 31 of half image row >> 5 of the 64-column block of its columns.
__device__ __forceinline__ void st_piece(char* im, int row, int col,
                                         const uint4& x) {
  char* const at = im + (col >> 6) * kImg + (row >> 5) * kHalfImg;
  *reinterpret_cast<bf16x8*>(at + row_img_byte(row & 31, col & 63)) =
      cvt8(x.x, x.y);
  *reinterpret_cast<bf16x8*>(at + row_img_byte(row & 31, (col & 63) + 8)) =
      cvt8(x.z, x.w);
}

template <int kHD>
__device__ __forceinline__ void st_kv(char* kim, char* vim,
                                      const RawTile<kHD>& t, int tid) {
  using S = Stage<kHD>;
  const int srow = tid / S::kPieces;
  const int scol = (tid % S::kPieces) * 16;
#pragma unroll
  for (int j = 0; j < S::kLoads; ++j) {
    st_piece(kim, srow + S::kStep * j, scol, t.k[j]);
    st_piece(vim, srow + S::kStep * j, scol, t.v[j]);
  }
}

// ---------------------------------------------------------------------------
// Grid (ceil(Sq * G / 128), Hk, B), 256 threads = 4 waves; wave w owns group
// rows r0 + 32 w .. + 31 of K/V head blockIdx.y. kSplit: grid.x is row tile *
// n_splits + split, the workgroup walks keys [split * L, (split + 1) * L)
// only and stores fp32 partials. attn_extend.hip's fa_extend_kernel with
// other staging and the scales folded in.
// ---------------------------------------------------------------------------
template <int kHD, bool kSplit, bool kPaged>
__global__ __launch_bounds__(256, kHD == 64 ? 3 : 2) void fa_extend_fp8_kernel(
    ExtendFp8Params p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  constexpr int kNC = kHD / 16;  // 16-column chunks of a row
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  // 64-key tiles as bf16, double-buffered: K images, then V images
  __shared__ __attribute__((aligned(16))) char smem[4 * kTileImg<kHD>];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kTileImg<kHD>;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

    // paged: the head's plane of the pool; the page comes per tile or load
    const uint8_t* kg =
        p.k + (kPaged ? 0 : (long)b * p.k_sb) + (long)hk * p.k_sh;
    const uint8_t* vg =
        p.v + (kPaged ? 0 : (long)b * p.v_sb) + (long)hk * p.v_sh;
    const int* trow =
        kPaged ? p.pg.table + (long)b * p.pg.max_pages : nullptr;
    const int klast = total - 1;    // >= 0 here; loads never go past it

    float m = kNegBig, ssum = 0.f;
    // scores are q · codes: the key scale rides on the softmax scale
    const float qk_scale = p.scale * p.k_scale[hk];
    const float c1 = qk_scale * kLog2e;
    float mc = m * c1;

    // tiles t0 .. n64 - 1: L is a multiple of 64, so a split starts and
    // (unless kmax cuts it) ends on a tile boundary
    const int t0 = k0 / 64;
    const int n64 = (kSplit ? min(kmax, k0 + p.L - 1) : kmax) / 64 + 1;

    // prologue: stage the first tile
    RawTile<kHD> nx;
    ld_kv<kHD, kPaged>(nx, kg, vg, p.pg, trow, p.k_sb, p.k_ss, p.v_sb, p.v_ss,
                       k0, klast, tid, wave);
    st_kv<kHD>(kimg, vimg, nx, tid);
    __syncthreads();

    int cur = 0;
    for (int t = t0; t < n64; ++t) {
      // the next tile's bytes fly during this one's compute
      const bool pref = t + 1 < n64;
      if (pref)
        ld_kv<kHD, kPaged>(nx, kg, vg, p.pg, trow, p.k_sb, p.k_ss, p.v_sb,
                           p.v_ss, (t + 1) * 64, klast, tid, wave);

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
        // out as in attn_extend.hip (the header says why)
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

      // converted as they are written: once for the four waves
      if (pref)
        st_kv<kHD>(kimg + (cur ^ 1) * kTileImg<kHD>,
                   vimg + (cur ^ 1) * kTileImg<kHD>, nx, tid);
      __syncthreads();
      cur ^= 1;
    }

    const float stot = ssum + __shfl_xor(ssum, 32, 64);
    if (seen) {
      // O^T holds sums of V codes
      inv = p.v_scale[hk] / stot;
      lse_v = qk_scale * m + __builtin_amdgcn_logf(stot) * kLn2;
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

template <int kHD, bool kPaged>
void launch_extend_fp8(const ExtendFp8Params& p, long row_tiles, int Hk, int B,
                       hipStream_t stream) {
  if (p.n_splits == 1) {
    hipLaunchKernelGGL((fa_extend_fp8_kernel<kHD, false, kPaged>),
                       dim3((unsigned)row_tiles, Hk, B), dim3(256), 0, stream,
                       p);
    return;
  }
  hipLaunchKernelGGL((fa_extend_fp8_kernel<kHD, true, kPaged>),
                     dim3((unsigned)(row_tiles * p.n_splits), Hk, B),
                     dim3(256), 0, stream, p);
  fa_extend_combine(p.o_part, p.lse_part, p.out, p.lse, B, p.H, p.Sq,
                    p.n_splits, kHD, p.o_sb, p.o_sh, p.o_ss, stream);
}

}  // namespace

// ---------------------------------------------------------------------------
// Host side (bound in bindings.hip). Nothing here reads the lengths, the
// table or the scales. fa_extend (attn_extend.hip) over e4m3 caches: the same
// arguments, checks and workspaces, n_splits what fa_extend_splits answered,
// plus k_scale and v_scale, fp32 [Hk] on the device. Of the 18 strides those
// of the caches (3..8) count bytes. q, k_new, v_new and out are bf16; new
// rows are quantised as they are appended, and attended as stored.
// ---------------------------------------------------------------------------
void fa_extend_fp8(const void* q, void* k_cache, void* v_cache,
                   const int* seqlens, const int* q_lens, const void* k_new,
                   const void* v_new, const float* k_scale,
                   const float* v_scale, void* out, float* lse, int B, int H,
                   int Hk, int Sq, int Smax, int head_dim, const long* strides,
                   float scale, bool causal, int n_splits, float* o_part,
                   float* lse_part, const int* block_table, int n_pages,
                   int page_size, int max_pages, int device,
                   hipStream_t stream) {
  decode_check_shapes("fa_extend_fp8", B, H, Hk, Smax, head_dim);
  const PageMap pages = make_page_map("fa_extend_fp8", block_table, n_pages,
                                      page_size, max_pages, Smax);
  const long G = H / Hk;
  // group rows and the append's piece index stay inside int arithmetic
  if (Sq < 1 || (long)Sq * G > (1L << 30) ||
      (long)Sq * (head_dim / 4) > (1L << 30))
    throw std::runtime_error("fa_extend_fp8: Sq must be >= 1 and Sq * (H / "
                             "Hk) at most 2^30, got Sq " + std::to_string(Sq));
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr ||
      seqlens == nullptr || out == nullptr)
    throw std::runtime_error("fa_extend_fp8: null pointer");
  if (k_scale == nullptr || v_scale == nullptr)
    throw std::runtime_error("fa_extend_fp8: k_scale and v_scale are needed");
  if ((k_new == nullptr) != (v_new == nullptr))
    throw std::runtime_error("fa_extend_fp8: k_new and v_new go together");
  const DeviceScope scope("fa_extend_fp8", device);
  const long row_tiles = ((long)Sq * G + kRows - 1) / kRows;
  const DecodePlan plan = extend_split_plan(
      B, Hk, row_tiles, Smax, device_cu_count("fa_extend_fp8"), n_splits);
  if (n_splits < 1 || plan.n_splits != n_splits)
    throw std::runtime_error("fa_extend_fp8: n_splits " +
                             std::to_string(n_splits) +
                             " is not a split count of this shape");
  if (n_splits > 1 && (o_part == nullptr || lse_part == nullptr))
    throw std::runtime_error("fa_extend_fp8: split workspaces missing");
  // grid.x of the split launch and of the combine (four rows a workgroup)
  if (n_splits > 1 && (row_tiles * n_splits > (1L << 30) ||
                       (long)B * H * Sq > (1L << 32)))
    throw std::runtime_error("fa_extend_fp8: shape too large to split");

  ExtendFp8Params p = {};
  p.q = (const __bf16*)q;
  p.k = (const uint8_t*)k_cache;
  p.v = (const uint8_t*)v_cache;
  p.k_scale = k_scale;
  p.v_scale = v_scale;
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
    fa_cache_append_fp8(k_cache, v_cache, k_new, v_new, seqlens, q_lens,
                        k_scale, v_scale, strides + 3, strides + 12, B, Hk, Sq,
                        Smax, head_dim, pages, stream);
  const bool paged = pages.table != nullptr;
  if (head_dim == 64)
    paged ? launch_extend_fp8<64, true>(p, row_tiles, Hk, B, stream)
          : launch_extend_fp8<64, false>(p, row_tiles, Hk, B, stream);
  else
    paged ? launch_extend_fp8<128, true>(p, row_tiles, Hk, B, stream)
          : launch_extend_fp8<128, false>(p, row_tiles, Hk, B, stream);
}

}  // namespace adapcc

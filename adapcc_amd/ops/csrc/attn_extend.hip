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
//  * No atomics, no counters: deterministic.
//
// Resources (gfx950; profiles/attn_extend_resources.txt): head_dim 64 126
// VGPRs, 32 KB LDS, 4 waves/SIMD by registers (three workgroups per CU
// asked for); head_dim 128 198 VGPRs, 64 KB LDS, 2 waves/SIMD; no scratch.
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
// rows r0 + 32 w .. + 31 of K/V head blockIdx.y.
// ---------------------------------------------------------------------------
template <int kHD>
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
  const int bx = p.causal ? (int)(gridDim.x - 1 - blockIdx.x)
                          : (int)blockIdx.x;

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
  const bool live = r0 < nrows && kmax >= 0;

  bool seen = false;                // does the computed row see a key
  float inv = 0.f, lse_v = -INFINITY;
  f32x16 acc0 = {}, acc1 = {};
  [[maybe_unused]] f32x16 acc2 = {}, acc3 = {};

  if (live) {  // workgroup-uniform: the barriers below are taken by all
    const int r = min(r_own, nrows - 1);
    const int i = r / G;
    const int h = hk * G + (r - i * G);
    const int lim = p.causal ? off + i : total - 1;  // last key this row sees
    seen = r_own < nrows && lim >= 0;
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

    const __bf16* kg = p.k + (long)b * p.k_sb + (long)hk * p.k_sh;
    const __bf16* vg = p.v + (long)b * p.v_sb + (long)hk * p.v_sh;
    const int klast = total - 1;    // >= 0 here; loads never go past it

    float m = kNegBig, ssum = 0.f;
    const float c1 = p.scale * kLog2e;
    float mc = m * c1;

    const int srow = threadIdx.x >> 3;       // staging: this thread's row
    const int scol = (threadIdx.x & 7) * 8;  // and column (bf16)
    const int n64 = kmax / 64 + 1;

    // prologue: stage tile 0
    st_tile<kHD>(kimg, srow, scol,
                 ld_tile<kHD>(kg, p.k_ss, min(srow, klast),
                              min(srow + 32, klast), scol));
    st_tile<kHD>(vimg, srow, scol,
                 ld_tile<kHD>(vg, p.v_ss, min(srow, klast),
                              min(srow + 32, klast), scol));
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < n64; ++t) {
      // the next tile's loads fly during this one's compute
      RowTile<kHD> nk, nv;
      const bool pref = t + 1 < n64;
      if (pref) {
        const int kr0 = min((t + 1) * 64 + srow, klast);
        const int kr1 = min((t + 1) * 64 + srow + 32, klast);
        nk = ld_tile<kHD>(kg, p.k_ss, kr0, kr1, scol);
        nv = ld_tile<kHD>(vg, p.v_ss, kr0, kr1, scol);
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
};

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
                     hipStream_t stream) {
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
  const long pieces = (long)Sq * (head_dim / 4);
  hipLaunchKernelGGL(fa_cache_append_kernel,
                     dim3((unsigned)((pieces + 255) / 256), Hk, B), dim3(256),
                     0, stream, a);
}

// Bound in bindings.hip. strides (elements): q, k_cache, v_cache, out (b, h,
// row each), then k_new, v_new (b, h, row each): 18 values. lse: fp32
// [B, H, Sq] or null; q_lens: int32 [B] or null. k_new and v_new: both or
// neither; with them rows i < n_b are appended at seqlens[b] + i first and
// the attention counts them. device: the tensors' device index, made current
// for the call; `stream` is one of its streams.
void fa_extend(const void* q, void* k_cache, void* v_cache,
               const int* seqlens, const int* q_lens, const void* k_new,
               const void* v_new, void* out, float* lse, int B, int H, int Hk,
               int Sq, int Smax, int head_dim, const long* strides,
               float scale, bool causal, int device, hipStream_t stream) {
  decode_check_shapes("fa_extend", B, H, Hk, Smax, head_dim);
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

  if (k_new != nullptr)
    fa_cache_append(k_cache, v_cache, k_new, v_new, seqlens, q_lens,
                    strides + 3, strides + 12, B, Hk, Sq, Smax, head_dim,
                    stream);
  const dim3 grid((unsigned)(((long)Sq * G + kRows - 1) / kRows), Hk, B);
  if (head_dim == 64)
    hipLaunchKernelGGL(fa_extend_kernel<64>, grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(fa_extend_kernel<128>, grid, dim3(256), 0, stream, p);
}

}  // namespace adapcc

// Decode attention over an FP8 (e4m3, OCP) KV cache (gfx950), head_dim 64 or
// 128, and the quantising append that fills such a cache. Forward only.
//
//   q        [B, H, D]  bf16     the new token's queries
//   k_cache  [B, Hk, Smax, D]    e4m3 bytes, any batch/head/row strides, rows
//   v_cache  [B, Hk, Smax, D]    contiguous and 16-B aligned (16 elements)
//   k_scale  fp32 [Hk], v_scale fp32 [Hk], on the device, > 0: a stored byte
//            c of K/V head hk stands for float(c) * scale[hk]
//   seqlens  int32 [B] on the device: keys that count, clamped to [0, Smax]
//
// attn_decode.hip is bound by the K/V bytes; this kernel reads half of them.
// The work split is that file's, so decode_split_plan, the fp32 partials and
// the combine kernel (fa_decode_combine) are shared unchanged: grid
// (n_splits, Hk, B), four waves round-robin over 32-key sub-tiles, the G
// query heads as the 32 MFMA columns, no workgroup barrier in the main loop,
// attn_cache.h's cache_tile_step for softmax and PV, one __syncthreads ahead
// of the in-workgroup merge, no atomics. e4m3 -> bf16 is exact (3 mantissa
// bits, range inside bf16's), so the bf16 MFMAs see the stored code values
// and the only rounding this file adds is the append's. What is new is how
// bytes reach the operands:
//
//  * K, global to fragments. A key row is D bytes. The contraction index of
//    S^T = K·Q^T may be permuted as long as both operands agree, so a lane
//    owns 16 contiguous bytes of its key row: lane l loads bytes
//    [32 j + 16 (l>>5), +16) of row l&31, j < D/32, one global_load_dwordx4
//    each (D/32 a sub-tile; the bf16 column order would take D/16 strided
//    8-byte loads). Its low 8 bytes are the fragment of MFMA chunk 2j, its
//    high 8 that of chunk 2j + 1, so element e of chunk c = 2j + t is column
//    32 j + 16 (l>>5) + 8 t + e. Q is loaded once, from global, with the same
//    map: 32 contiguous bytes of bf16 per j and lane.
//  * V, 16-B pieces of whole rows: lane t takes piece t % (D/16) of row
//    t / (D/16) + (1024/D) i, so a load instruction covers 16 (D 64) or 8
//    (D 128) whole rows and a sub-tile is again D/32 loads. The 16 codes are
//    converted in registers and written as two 16-B slots of the wave's
//    [32][64] bf16 row image(s) (attn_frag.h), so ds_read_b64_tr_b16, the
//    PV MFMAs and the LDS budget are the bf16 kernel's.
//  * Conversion (attn_cache.h's cvt8): v_cvt_scalef32_pk_bf16_fp8 with
//    scale 1.0, one instruction per two codes straight to a packed bf16 pair
//    (8 per 16-B load). The
//    alternative, v_cvt_pk_f32_fp8 then v_cvt_pk_bf16_f32, is two per pair;
//    chosen by that count, the alternative was not timed.
//  * Prefetch as in the bf16 kernel: the next sub-tile's raw bytes (D/4
//    dwords of K and V together, half of bf16's) wait in registers while the
//    current one is computed.
//  * The scales cost nothing per element: the MFMAs run on raw codes
//    (|x| <= 448, fp32 accumulation), k_scale[hk] is folded into
//    c1 = scale * k_scale * log2(e) and into the scale * M term of the lse,
//    v_scale[hk] into the 1 / l of the merge. lse is the logsumexp of the
//    scaled scores of the dequantised keys.
//  * Ragged and paged handling is the bf16 kernel's: rows are clamped to the
//    split's last key before any load (no byte at a row >= len is read),
//    keys past it are masked to kNegBig, pages are found with
//    paged_sub_offset and the pool's strides.
//
// Not tried: PV on fp8 MFMA with ds_read_b64_tr_b8. It would round P to fp8
// and change the numerics contract.
//
// fa_cache_append_fp8 is fa_cache_append (attn_extend.hip) with the rounding:
// thread e of a (batch, K/V head) reads 16 B (8 bf16) of a new row, divides
// by the head's scale in fp32 (correctly rounded division), clamps to +-448
// (the hardware conversion does not saturate), packs with v_cvt_pk_fp8_f32
// (round to nearest even) and stores 8 B. Rows i >= n_b and rows that would
// land at or past Smax are left alone.
//
// Resources (gfx950, this build's flags, from the compiler's report): decode
// head_dim 64 131 VGPRs (paged 135), 33 KB LDS, 3 waves/SIMD; head_dim 128
// 213 VGPRs (paged 213), 65 KB LDS, 2 waves/SIMD; the append 23 VGPRs (paged
// 22), no LDS, 8 waves/SIMD; no scratch anywhere. Against the bf16 kernel
// that is 28 fewer registers at either width (the halved prefetch) and the
// same occupancy, which the LDS of the merge sets. Timings:
// profiles/attn_decode_fp8.txt.
//
// Build: as attn_decode.hip, with the packed fp32 VALU forms off
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

constexpr int kBlkImg = 4096;  // attn_frag.h's [32][64] bf16 row image

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct DecodeFp8Params {
  const __bf16* q;
  const uint8_t *k, *v;     // the caches, e4m3 bytes
  const float *k_scale, *v_scale;  // [Hk]
  const int* seqlens;       // [B]
  long q_sb, q_sh;          // element strides
  long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;  // bytes
  int H, G, Smax, n_splits, L;
  int append;               // 1: attention covers seqlens[b] + 1 keys
  float scale;
  float* o_part;            // [B, H, n_splits, D]   n_splits > 1
  float* lse_part;          // [B, H, n_splits]      n_splits > 1
  __bf16* out;              // [B, H, D] contiguous
  float* lse;               // [B, H], may be null
  PageMap pg;               // kPaged: k, v are pools, k_sb, v_sb page strides
};

// A lane's raw bytes of one sub-tile of K or of V: kHD/32 loads of 16 B.
template <int kHD>
struct Raw {
  u32x4 x[kHD / 32];
};

// Byte offset of key row `row` (clamped by the caller) in the head's plane.
template <bool kPaged>
__device__ __forceinline__ long row_offset(const PageMap& pm, const int* trow,
                                           long sp, long ss, int kb, int row) {
  if constexpr (kPaged)
    return paged_sub_offset(pm, trow, kb, row, sp, ss);
  else
    return (long)row * ss;
}

// A sub-tile's loads. K: lane l, bytes [32 j + 16 (l>>5), +16) of key row
// kb + (l&31). V: lane t, piece t % (kHD/16) of key rows kb + t / (kHD/16) +
// (1024/kHD) j. Every offset is formed before the first load is issued: a
// paged offset waits for its table entry, and a wait placed between the
// loads would also wait for the loads ahead of it.
template <int kHD, bool kPaged>
__device__ __forceinline__ void ld_kv(Raw<kHD>& tk, Raw<kHD>& tv,
                                      const uint8_t* kg, const uint8_t* vg,
                                      const PageMap& pm, const int* trow,
                                      long k_sp, long k_ss, long v_sp,
                                      long v_ss, int kb, int klast, int lane) {
  constexpr int kNL = kHD / 32, kPieces = kHD / 16, kRows = 64 / kPieces;
  const long koff =
      row_offset<kPaged>(pm, trow, k_sp, k_ss, kb,
                         min(kb + (lane & 31), klast)) + (lane >> 5) * 16;
  long voff[kNL];
#pragma unroll
  for (int j = 0; j < kNL; ++j)
    voff[j] = row_offset<kPaged>(
                  pm, trow, v_sp, v_ss, kb,
                  min(kb + lane / kPieces + kRows * j, klast)) +
              (lane % kPieces) * 16;
#pragma unroll
  for (int j = 0; j < kNL; ++j)
    tk.x[j] = *reinterpret_cast<const u32x4*>(kg + koff + 32 * j);
#pragma unroll
  for (int j = 0; j < kNL; ++j)
    tv.x[j] = *reinterpret_cast<const u32x4*>(vg + voff[j]);
}

// The wave's V share, dequantised, into its row image(s): a piece is 16
// columns, two 16-B slots of one image row.
template <int kHD>
__device__ __forceinline__ void st_v(char* im, const Raw<kHD>& t, int lane) {
  constexpr int kPieces = kHD / 16, kRows = 64 / kPieces;
  const int col = (lane % kPieces) * 16;
  char* const blk = im + (col >> 6) * kBlkImg;
#pragma unroll
  for (int j = 0; j < kHD / 32; ++j) {
    const int row = lane / kPieces + kRows * j;
    *reinterpret_cast<bf16x8*>(blk + row_img_byte(row, col & 63)) =
        cvt8(t.x[j][0], t.x[j][1]);
    *reinterpret_cast<bf16x8*>(blk + row_img_byte(row, (col & 63) + 8)) =
        cvt8(t.x[j][2], t.x[j][3]);
  }
}

// ---------------------------------------------------------------------------
// Partial attention of one (batch, K/V head, key split).
// Grid (n_splits, Hk, B), 256 threads = 4 waves; attn_decode.hip's
// fa_decode_kernel with other loads and the scales folded in.
// ---------------------------------------------------------------------------
template <int kHD, bool kPaged>
__global__ __launch_bounds__(256, 2) void fa_decode_fp8_kernel(
    DecodeFp8Params p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  constexpr int kNL = kHD / 32;  // 16-B loads of a lane per sub-tile
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  constexpr int kWaveBytes = kHD * 32 * 4;  // a wave's O^T [kHD][32] fp32,
                                            // laid over its V image
  constexpr int kPer = kHD / 8;  // output columns per thread in the merge
  __shared__ __attribute__((aligned(16))) char smem[4 * kWaveBytes];
  __shared__ float2 ml[4][32];   // (running max, row sum) per wave, column

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hi = lane >> 5;
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = p.G, H = p.H;

  // the keys that count, the appended one among them; clamped to [0, Smax]
  const int len = seq_lens(p.seqlens, nullptr, b, 1, p.Smax, p.append).total;
  const int k0 = split * p.L;
  const int kend = min(k0 + p.L, len);

  if (k0 >= kend) {
    // no mass; nothing below this point is reached, so no barrier is missed
    if (p.n_splits > 1) {
      if (tid < G)
        p.lse_part[((long)b * H + hk * G + tid) * p.n_splits + split] =
            -INFINITY;
    } else {
      // the one split is empty only at len == 0: zero row, lse -inf
      const uint4 z = {0u, 0u, 0u, 0u};
      for (int i = tid; i < G * (kHD / 8); i += 256)
        *reinterpret_cast<uint4*>(p.out + ((long)b * H + hk * G) * kHD +
                                  (long)i * 8) = z;
      if (tid < G && p.lse != nullptr)
        p.lse[(long)b * H + hk * G + tid] = -INFINITY;
    }
    return;
  }
  const int klast = kend - 1;  // >= 0; loads never go past it

  // Q^T B-fragments straight from global in K's permuted column order:
  // chunk 2j + t of lane l holds Q[head g][32 j + 16 hi + 8 t + e].
  const int g = min(lane & 31, G - 1);
  const __bf16* qrow =
      p.q + (long)b * p.q_sb + (long)(hk * G + g) * p.q_sh + hi * 16;
  bf16x8 qf[2 * kNL];
#pragma unroll
  for (int c = 0; c < 2 * kNL; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(qrow + (c >> 1) * 32 +
                                             (c & 1) * 8);

  // paged: the head's plane of the pool; the page comes per sub-tile or row
  const uint8_t* kg = p.k + (kPaged ? 0 : (long)b * p.k_sb) + (long)hk * p.k_sh;
  const uint8_t* vg = p.v + (kPaged ? 0 : (long)b * p.v_sb) + (long)hk * p.v_sh;
  const int* trow = kPaged ? p.pg.table + (long)b * p.pg.max_pages : nullptr;
  char* const vim = smem + wave * kWaveBytes;

  // O^T, one accumulator per 32 columns; acc2, acc3 (columns 64..127) are
  // dead at head_dim 64. Named, not an array: an array went to scratch.
  f32x16 acc0 = {}, acc1 = {};
  [[maybe_unused]] f32x16 acc2 = {}, acc3 = {};
  float m = kNegBig, ssum = 0.f;
  // scores are q · codes: the key scale rides on the softmax scale
  const float qk_scale = p.scale * p.k_scale[hk];
  const float c1 = qk_scale * kLog2e;
  float mc = m * c1;

  // this wave's sub-tiles: k0 + 32*wave, then every 128 keys
  int kb = k0 + wave * 32;
  Raw<kHD> nk, nv;
  if (kb < kend)
    ld_kv<kHD, kPaged>(nk, nv, kg, vg, p.pg, trow, p.k_sb, p.k_ss, p.v_sb,
                       p.v_ss, kb, klast, lane);

  for (; kb < kend; kb += 128) {
    // the sub-tile loaded last time round: V goes into the image as bf16
    const Raw<kHD> kr = nk;
    st_v<kHD>(vim, nv, lane);
    wave_lds_fence();

    // the next one's loads fly during this one's compute
    const int kn = kb + 128;
    if (kn < kend)
      ld_kv<kHD, kPaged>(nk, nv, kg, vg, p.pg, trow, p.k_sb, p.k_ss, p.v_sb,
                         p.v_ss, kn, klast, lane);

    // S^T tile: C[key][head] = sum_d K[key][d] * Q[head][d], d permuted
    f32x16 s = {};
#pragma unroll
    for (int j = 0; j < kNL; ++j) {
      s = mfma(cvt8(kr.x[j][0], kr.x[j][1]), qf[2 * j], s);
      s = mfma(cvt8(kr.x[j][2], kr.x[j][3]), qf[2 * j + 1], s);
    }

    // softmax and PV; the sub-tile with the split's last key masks the rest
    cache_tile_step<kHD>(s, kb + 31 > klast, kb, klast, vim, kBlkImg, lane,
                         m, mc, ssum, c1, acc0, acc1, acc2, acc3);
    wave_lds_fence();
  }

  // The wave's state into LDS: O^T[d][column] over its own image (its reads
  // of it are done, in order), (m, l) beside it. A wave that had no
  // sub-tile hands over l = 0 and zeros.
  const float stot = ssum + __shfl_xor(ssum, 32, 64);
  float* const ow = reinterpret_cast<float*>(smem + wave * kWaveBytes);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* const at = ow + crow(r, hi) * 32 + (lane & 31);
    at[0] = acc0[r];
    at[32 * 32] = acc1[r];
    if constexpr (kNB == 4) {
      at[64 * 32] = acc2[r];
      at[96 * 32] = acc3[r];
    }
  }
  if (hi == 0) ml[wave][lane] = make_float2(m, stot);
  __syncthreads();

  // Merge: thread t takes column t&31 and kPer consecutive d.
  const int gc = tid & 31, dg = tid >> 5;
  float wgt[4];
  float M = kNegBig;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (ml[w][gc].y > 0.f) M = fmaxf(M, ml[w][gc].x);
  float ltot = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float2 x = ml[w][gc];
    wgt[w] = x.y > 0.f ? __builtin_amdgcn_exp2f((x.x - M) * c1) : 0.f;
    ltot += wgt[w] * x.y;
  }
  // wave 0 always has a key: ltot > 0. O^T holds sums of V codes.
  const float inv = p.v_scale[hk] / ltot;
  float o[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int d = dg * kPer + j;
    float x = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      x += wgt[w] *
           reinterpret_cast<const float*>(smem + w * kWaveBytes)[d * 32 + gc];
    o[j] = x * inv;
  }
  if (gc >= G) return;  // padding columns store nothing
  const long bh = (long)b * H + hk * G + gc;
  const float lse = qk_scale * M + __builtin_amdgcn_logf(ltot) * kLn2;
  if (p.n_splits > 1) {
    float* dst = p.o_part + (bh * p.n_splits + split) * kHD + dg * kPer;
#pragma unroll
    for (int j = 0; j < kPer; j += 4)
      *reinterpret_cast<float4*>(dst + j) =
          make_float4(o[j], o[j + 1], o[j + 2], o[j + 3]);
    if (dg == 0) p.lse_part[bh * p.n_splits + split] = lse;
  } else {
    __bf16* dst = p.out + bh * kHD + dg * kPer;
#pragma unroll
    for (int j = 0; j < kPer; j += 4)
      store4_bf16(dst + j, o[j], o[j + 1], o[j + 2], o[j + 3]);
    if (dg == 0 && p.lse != nullptr) p.lse[bh] = lse;
  }
}

template <int kHD>
void launch_decode_fp8(const DecodeFp8Params& p, dim3 grid,
                       hipStream_t stream) {
  if (p.pg.table != nullptr)
    hipLaunchKernelGGL((fa_decode_fp8_kernel<kHD, true>), grid, dim3(256), 0,
                       stream, p);
  else
    hipLaunchKernelGGL((fa_decode_fp8_kernel<kHD, false>), grid, dim3(256), 0,
                       stream, p);
}

// ---------------------------------------------------------------------------
// Quantising cache update. Grid (ceil(Sq * D/4 / 256), Hk, B): thread e of a
// (batch, K/V head) turns 8 bf16 into 8 B; a row is D/8 pieces of k, then
// D/8 of v.
// ---------------------------------------------------------------------------
struct AppendFp8Params {
  uint8_t *k, *v;
  const __bf16 *kn, *vn;
  const float *k_scale, *v_scale;
  const int *seqlens, *q_lens;
  long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;  // bytes
  long kn_sb, kn_sh, kn_ss, vn_sb, vn_sh, vn_ss;
  int Sq, Smax, D;
  PageMap pg;  // kPaged: k, v are pools, k_sb, v_sb their page strides
};

// q8 of eight values: fp32 division, clamp, round to nearest even.
__device__ __forceinline__ uint2 quantize8(bf16x8 x, float s) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    f[i] = fminf(fmaxf(__fdiv_rn((float)x[i], s), -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return make_uint2((unsigned)lo, (unsigned)hi);
}

template <bool kPaged>
__global__ __launch_bounds__(256) void fa_cache_append_fp8_kernel(
    AppendFp8Params p) {
  const int hk = blockIdx.y, b = blockIdx.z;
  const SeqLens sl = seq_lens(p.seqlens, p.q_lens, b, p.Sq, p.Smax, 1);
  const int per = p.D / 8;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int i = e / (2 * per);
  const int piece = e - i * 2 * per;
  const int row = sl.past + i;
  if (i >= sl.n || row >= p.Smax) return;
  const bool is_k = piece < per;
  const int col = (is_k ? piece : piece - per) * 8;
  const bf16x8 x = *reinterpret_cast<const bf16x8*>(
      is_k ? p.kn + (long)b * p.kn_sb + (long)hk * p.kn_sh +
                 (long)i * p.kn_ss + col
           : p.vn + (long)b * p.vn_sb + (long)hk * p.vn_sh +
                 (long)i * p.vn_ss + col);
  const long sp = is_k ? p.k_sb : p.v_sb, ss = is_k ? p.k_ss : p.v_ss;
  long off;
  if constexpr (kPaged) {
    // 0 <= row < max_pages * P: the entry is one of the table row's
    off = paged_offset(p.pg, p.pg.table + (long)b * p.pg.max_pages, row, sp,
                       ss);
  } else {
    off = (long)b * sp + (long)row * ss;
  }
  uint8_t* dst = (is_k ? p.k + (long)hk * p.k_sh : p.v + (long)hk * p.v_sh) +
                 off + col;
  *reinterpret_cast<uint2*>(dst) =
      quantize8(x, is_k ? p.k_scale[hk] : p.v_scale[hk]);
}

}  // namespace

// attn_cache.h describes the arguments.
void fa_cache_append_fp8(void* k_cache, void* v_cache, const void* k_new,
                         const void* v_new, const int* seqlens,
                         const int* q_lens, const float* k_scale,
                         const float* v_scale, const long* cache_strides,
                         const long* new_strides, int B, int Hk, int Sq,
                         int Smax, int head_dim, const PageMap& pages,
                         hipStream_t stream) {
  AppendFp8Params a = {};
  a.k = (uint8_t*)k_cache;
  a.v = (uint8_t*)v_cache;
  a.kn = (const __bf16*)k_new;
  a.vn = (const __bf16*)v_new;
  a.k_scale = k_scale;
  a.v_scale = v_scale;
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
    hipLaunchKernelGGL(fa_cache_append_fp8_kernel<true>, grid, dim3(256), 0,
                       stream, a);
  else
    hipLaunchKernelGGL(fa_cache_append_fp8_kernel<false>, grid, dim3(256), 0,
                       stream, a);
}

// ---------------------------------------------------------------------------
// Host side (bound in bindings.hip). Nothing here reads the lengths, the
// table or the scales.
// ---------------------------------------------------------------------------

// The append step alone: rows i < n_b of k_new, v_new [B, Hk, Sq, head_dim]
// (bf16) to cache rows seqlens[b] + i. k_scale, v_scale (fp32 [Hk]) both
// given: e4m3 caches through fa_cache_append_fp8; both null: bf16 caches
// through fa_cache_append. cache_strides and new_strides (elements): k then
// v, (b, h, row) each, (page, h, row) with a block_table.
void fa_kv_append(void* k_cache, void* v_cache, const void* k_new,
                  const void* v_new, const int* seqlens, const int* q_lens,
                  const float* k_scale, const float* v_scale,
                  const long* cache_strides, const long* new_strides, int B,
                  int Hk, int Sq, int Smax, int head_dim,
                  const int* block_table, int n_pages, int page_size,
                  int max_pages, int device, hipStream_t stream) {
  decode_check_shapes("fa_kv_append", B, Hk, Hk, Smax, head_dim);
  if (Sq < 1 || Sq > (1 << 24))
    throw std::runtime_error("fa_kv_append: Sq out of range");
  const PageMap pages = make_page_map("fa_kv_append", block_table, n_pages,
                                      page_size, max_pages, Smax);
  if (k_cache == nullptr || v_cache == nullptr || k_new == nullptr ||
      v_new == nullptr || seqlens == nullptr)
    throw std::runtime_error("fa_kv_append: null pointer");
  if ((k_scale == nullptr) != (v_scale == nullptr))
    throw std::runtime_error("fa_kv_append: k_scale and v_scale go together");
  const DeviceScope scope("fa_kv_append", device);
  if (k_scale != nullptr)
    fa_cache_append_fp8(k_cache, v_cache, k_new, v_new, seqlens, q_lens,
                        k_scale, v_scale, cache_strides, new_strides, B, Hk,
                        Sq, Smax, head_dim, pages, stream);
  else
    fa_cache_append(k_cache, v_cache, k_new, v_new, seqlens, q_lens,
                    cache_strides, new_strides, B, Hk, Sq, Smax, head_dim,
                    pages, stream);
}

// fa_decode (attn_decode.hip) over e4m3 caches: the same arguments and
// workspaces, n_splits what fa_decode_splits answered, plus k_scale and
// v_scale, fp32 [Hk] on the device. The cache strides count bytes. q, k_new,
// v_new and out are bf16; new rows are quantised as they are appended.
void fa_decode_fp8(const void* q, void* k_cache, void* v_cache,
                   const int* seqlens, const void* k_new, const void* v_new,
                   const float* k_scale, const float* v_scale, void* out,
                   float* lse, float* o_part, float* lse_part, int B, int H,
                   int Hk, int Smax, int head_dim, const long* strides,
                   float scale, int n_splits, const int* block_table,
                   int n_pages, int page_size, int max_pages, int device,
                   hipStream_t stream) {
  decode_check_shapes("fa_decode_fp8", B, H, Hk, Smax, head_dim);
  const PageMap pages = make_page_map("fa_decode_fp8", block_table, n_pages,
                                      page_size, max_pages, Smax);
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr ||
      seqlens == nullptr || out == nullptr)
    throw std::runtime_error("fa_decode_fp8: null pointer");
  if (k_scale == nullptr || v_scale == nullptr)
    throw std::runtime_error("fa_decode_fp8: k_scale and v_scale are needed");
  if ((k_new == nullptr) != (v_new == nullptr))
    throw std::runtime_error("fa_decode_fp8: k_new and v_new go together");
  const DeviceScope scope("fa_decode_fp8", device);
  const DecodePlan plan = decode_split_plan(
      B, Hk, Smax, device_cu_count("fa_decode_fp8"), n_splits);
  if (n_splits < 1 || plan.n_splits != n_splits)
    throw std::runtime_error("fa_decode_fp8: n_splits " +
                             std::to_string(n_splits) +
                             " is not a split count of this shape");
  if (n_splits > 1 && (o_part == nullptr || lse_part == nullptr))
    throw std::runtime_error("fa_decode_fp8: split workspaces missing");

  DecodeFp8Params p = {};
  p.q = (const __bf16*)q;
  p.k = (const uint8_t*)k_cache;
  p.v = (const uint8_t*)v_cache;
  p.k_scale = k_scale;
  p.v_scale = v_scale;
  p.seqlens = seqlens;
  p.q_sb = strides[0];
  p.q_sh = strides[1];
  p.k_sb = strides[2];
  p.k_sh = strides[3];
  p.k_ss = strides[4];
  p.v_sb = strides[5];
  p.v_sh = strides[6];
  p.v_ss = strides[7];
  p.H = H;
  p.G = H / Hk;
  p.Smax = Smax;
  p.n_splits = n_splits;
  p.L = plan.L;
  p.append = k_new != nullptr;
  p.scale = scale;
  p.o_part = o_part;
  p.lse_part = lse_part;
  p.out = (__bf16*)out;
  p.lse = lse;
  p.pg = pages;

  if (k_new != nullptr) {
    // one new row per sequence: Sq = 1, no q_lens, row strides 0
    const long new_strides[6] = {strides[8],  strides[9],  0,
                                 strides[10], strides[11], 0};
    fa_cache_append_fp8(k_cache, v_cache, k_new, v_new, seqlens, nullptr,
                        k_scale, v_scale, strides + 2, new_strides, B, Hk, 1,
                        Smax, head_dim, pages, stream);
  }
  const dim3 grid(n_splits, Hk, B);
  if (head_dim == 64)
    launch_decode_fp8<64>(p, grid, stream);
  else
    launch_decode_fp8<128>(p, grid, stream);
  if (n_splits > 1)
    fa_decode_combine(o_part, lse_part, out, lse, n_splits, (long)B * H,
                      head_dim, stream);
}

}  // namespace adapcc

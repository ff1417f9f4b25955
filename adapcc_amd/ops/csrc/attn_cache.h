// What the two attention kernels over a KV cache share (gfx950, bf16):
// attn_decode.hip (one query row per sequence, split over the keys) and
// attn_extend.hip (a block of rows): the clamped lengths of a sequence, the
// map from a logical key row to its place in a paged cache (PageMap,
// paged_offset: every K, V and append address of the kPaged instantiations),
// the cache append's interface (one kernel, in attn_extend.hip), the host
// helpers that make the tensors' device current, and cache_tile_step, the
// span from the finished score tile to the last PV MFMA. Decode calls it;
// extend holds the same span written out (with an s_setprio pair), since as
// a function call it got another register allocation and lost time at one
// shape (profiles/README.md, "Shared header ..."). attn_decode_fp8.hip, decode
// over an e4m3 cache, is a third user: the lengths, the page map, the tile
// step, and decode's combine kernel through a host launcher.
// attn_extend_fp8.hip, extend over an e4m3 cache, is a fourth: all of that
// with extend's combine kernel, and cvt8, the e4m3 -> bf16 conversion both
// fp8 files use. Compiled only through these files, so with their flags
// (ops/build.py: packed fp32 VALU forms off).
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "attn_decode_plan.h"
#include "attn_frag.h"

namespace adapcc {

constexpr float kNegBig = -3.0e38f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// The lengths of sequence b: past_b = clamp(seqlens[b], 0, Smax) cached keys,
// n_b = clamp(q_lens[b], 0, Sq) new rows (Sq without q_lens), total_b the
// keys that count, with the new rows where they were appended. The clamps
// bound every address the kernels form: a malformed length cannot send a
// load or store outside the tensors.
struct SeqLens {
  int past, n, total;
};

__device__ __forceinline__ SeqLens seq_lens(const int* seqlens,
                                            const int* q_lens, int b, int Sq,
                                            int Smax, int append) {
  SeqLens s;
  s.past = min(max(seqlens[b], 0), Smax);
  s.n = q_lens != nullptr ? min(max(q_lens[b], 0), Sq) : Sq;
  s.total = append ? min(s.past + s.n, Smax) : s.past;
  return s;
}

// A paged cache (the kPaged instantiations): k and v are pools [N, Hk, P, D]
// of N pages of P = 1 << lg key rows, and logical key row j of sequence b is
// row j & (P - 1) of page table[b * max_pages + (j >> lg)]. The pool's
// (page, head, row) strides travel where a slab's (batch, head, row) strides
// do, and Smax = max_pages * P. table == nullptr: not paged.
struct PageMap {
  const int* table;  // int32 [B, max_pages], rows contiguous
  int max_pages, n_pages, lg;
};

// The one place a table entry becomes an address. page_base: the element
// offset of the page that holds logical row `row` of the sequence whose
// table row is `trow`; the entry is clamped to [0, N - 1] first, so a
// malformed table gives unspecified values but no access outside the pool
// (what seq_lens does for lengths). The caller has clamped `row` to
// [0, total_b - 1], so row >> lg < max_pages and no entry past the
// sequence's pages is read. With a wave-uniform `row` the load is scalar.
__device__ __forceinline__ long page_base(const PageMap& pm, const int* trow,
                                          int row, long page_stride) {
  const int page = min(max(trow[row >> pm.lg], 0), pm.n_pages - 1);
  return (long)page * page_stride;
}

// Logical row -> element offset inside one head's plane of the pool.
__device__ __forceinline__ long paged_offset(const PageMap& pm,
                                             const int* trow, int row,
                                             long page_stride,
                                             long row_stride) {
  return page_base(pm, trow, row, page_stride) +
         (long)(row & ((1 << pm.lg) - 1)) * row_stride;
}

// The same for a row known to lie in the page of `urow` (a tile that does
// not straddle a page: one lookup, by the wave-uniform urow, for all lanes).
__device__ __forceinline__ long paged_offset_in(const PageMap& pm,
                                                const int* trow, int urow,
                                                int row, long page_stride,
                                                long row_stride) {
  return page_base(pm, trow, urow, page_stride) +
         (long)(row & ((1 << pm.lg) - 1)) * row_stride;
}

// The decode kernels' lookup (attn_decode.hip, attn_decode_fp8.hip): where a
// wave's loads find key row `row` (clamped to the split's last key, so
// inside the sub-tile that starts at kb) of a page pool. kb is a multiple of
// 32: with 32 rows or more to a page the sub-tile lies in one page and one
// wave-uniform (scalar) lookup serves every lane; at 16 it lies in two and
// each lane looks up its own row.
__device__ __forceinline__ long paged_sub_offset(const PageMap& pm,
                                                 const int* trow, int kb,
                                                 int row, long sp, long ss) {
  if (pm.lg >= 5)
    return paged_offset_in(pm, trow, __builtin_amdgcn_readfirstlane(kb), row,
                           sp, ss);
  return paged_offset(pm, trow, row, sp, ss);
}

// Orders this wave's LDS writes and reads for the compiler; the hardware
// serves one wave's LDS instructions in order.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Four f32 -> four bf16 (round to nearest even), one 8-byte store.
__device__ __forceinline__ void store4_bf16(__bf16* dst, float a, float b,
                                            float c, float d) {
  unsigned lo, hi;
  asm("v_cvt_pk_bf16_f32 %0, %2, %3\n\t"
      "v_cvt_pk_bf16_f32 %1, %4, %5"
      : "=&v"(lo), "=&v"(hi)
      : "v"(a), "v"(b), "v"(c), "v"(d));
  uint2 st = {lo, hi};
  *reinterpret_cast<uint2*>(dst) = st;
}

// Eight e4m3 codes (two dwords, byte 0 first) -> eight bf16, exactly:
// v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, one instruction per two codes.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

__device__ __forceinline__ bf16x8 cvt8(unsigned a, unsigned b) {
  union {
    bf16x2 h[4];
    bf16x8 f;
  } r;
  r.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false);
  r.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true);
  r.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false);
  r.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true);
  return r.f;
}

// One 32-key tile of the online softmax and of O^T += V^T · P^T. `s` is the
// finished S^T tile (this lane: keys kbase + crow(r, lane >> 5) of its own
// row). `masked` is wave-uniform: the tile reaches past some lane's `lim`,
// the last key that lane sees, and keys past it go to kNegBig before the
// running max. `vimg` is the tile's V as attn_frag.h row images, one per 64
// columns, `vblk` bytes apart. m, mc = m * c1, ssum: the lane's running max
// and row sum, c1 = scale * log2(e). acc0..acc3 are O^T, one per 32 columns
// (acc2, acc3 dead at head_dim 64); named, not an array: an array went to
// scratch.
//
// A row that has seen no key yet holds m = kNegBig and gets P = 1 here:
// finite, lane-local, and for its caller to throw away.
template <int kHD>
__device__ __forceinline__ void cache_tile_step(
    const f32x16& s, bool masked, int kbase, int lim, const char* vimg,
    int vblk, int lane, float& m, float& mc, float& ssum, float c1,
    f32x16& acc0, f32x16& acc1, f32x16& acc2, f32x16& acc3) {
  const int hi = lane >> 5;
  float pv[16];
  float tmax = kNegBig;
  if (masked) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pv[r] = kbase + crow(r, hi) > lim ? kNegBig : s[r];
      tmax = fmaxf(tmax, pv[r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pv[r] = s[r];
      tmax = fmaxf(tmax, pv[r]);
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
    for (int r = 0; r < 16; ++r) {
      acc0[r] *= alpha;
      acc1[r] *= alpha;
      if constexpr (kHD == 128) {
        acc2[r] *= alpha;
        acc3[r] *= alpha;
      }
    }
  }

  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    pv[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(pv[r], c1, -mc));
    psum += pv[r];
  }
  ssum += psum;

  // P to operand fragments (keys 0-15 / 16-31), then
  // O^T += V^T · P^T with V^T from hardware transpose reads
  const bf16x8 p0 = pack_frag(&pv[0]);
  const bf16x8 p1 = pack_frag(&pv[8]);
  acc0 = mfma(read_tr_frag(vimg, lane, 0, 0), p0, acc0);
  acc0 = mfma(read_tr_frag(vimg, lane, 1, 0), p1, acc0);
  acc1 = mfma(read_tr_frag(vimg, lane, 0, 1), p0, acc1);
  acc1 = mfma(read_tr_frag(vimg, lane, 1, 1), p1, acc1);
  if constexpr (kHD == 128) {
    acc2 = mfma(read_tr_frag(vimg + vblk, lane, 0, 0), p0, acc2);
    acc2 = mfma(read_tr_frag(vimg + vblk, lane, 1, 0), p1, acc2);
    acc3 = mfma(read_tr_frag(vimg + vblk, lane, 0, 1), p0, acc3);
    acc3 = mfma(read_tr_frag(vimg + vblk, lane, 1, 1), p1, acc3);
  }
}

// In-place cache update ahead of the attention kernel, on its stream (defined
// in attn_extend.hip): rows i < n_b of k_new, v_new [B, Hk, Sq, head_dim] go
// to cache rows past_b + i; rows that would land at or past Smax are dropped,
// so a full cache is left alone. cache_strides: k_cache, then v_cache, (b, h,
// row) each; new_strides: k_new, then v_new, likewise. q_lens may be null.
// The caller has checked the shapes and made the device current. With
// pages.table the caches are pools, cache_strides their (page, head, row)
// strides and Smax = max_pages * P: cache row past_b + i is found through
// paged_offset.
void fa_cache_append(void* k_cache, void* v_cache, const void* k_new,
                     const void* v_new, const int* seqlens, const int* q_lens,
                     const long* cache_strides, const long* new_strides, int B,
                     int Hk, int Sq, int Smax, int head_dim,
                     const PageMap& pages, hipStream_t stream);

// The same for e4m3 caches (attn_decode_fp8.hip): the bf16 rows are written
// as q8(x, s) = rne_e4m3(clamp(float(x) / s, -448, 448)) with s = k_scale[hk]
// or v_scale[hk] (fp32 [Hk] on the device), and the cache strides count
// bytes.
void fa_cache_append_fp8(void* k_cache, void* v_cache, const void* k_new,
                         const void* v_new, const int* seqlens,
                         const int* q_lens, const float* k_scale,
                         const float* v_scale, const long* cache_strides,
                         const long* new_strides, int B, int Hk, int Sq,
                         int Smax, int head_dim, const PageMap& pages,
                         hipStream_t stream);

// Decode's merge of the key splits (attn_decode.hip's combine kernel): o_part
// fp32 [BH, n_splits, head_dim] normalised partials and lse_part fp32
// [BH, n_splits] to out bf16 [BH, head_dim] and lse fp32 [BH] (or null).
void fa_decode_combine(const float* o_part, const float* lse_part, void* out,
                       float* lse, int n_splits, long BH, int head_dim,
                       hipStream_t stream);

// Extend's merge of the key splits (attn_extend.hip's combine kernel): o_part
// fp32 [B, H, Sq, n_splits, head_dim] normalised partials and lse_part fp32
// [B, H, Sq, n_splits] to out bf16 through its (b, h, row) element strides
// and lse fp32 [B, H, Sq] (or null).
void fa_extend_combine(const float* o_part, const float* lse_part, void* out,
                       float* lse, int B, int H, int Sq, int n_splits,
                       int head_dim, long o_sb, long o_sh, long o_ss,
                       hipStream_t stream);

// The PageMap of a host call, checked (attn_decode_plan.h): block_table null
// is the unpaged call and gives table == nullptr; else Smax must be
// max_pages * page_size.
inline PageMap make_page_map(const char* name, const int* block_table,
                             int n_pages, int page_size, int max_pages,
                             int Smax) {
  PageMap pm = {};
  if (block_table == nullptr) return pm;
  pm.lg = paged_check_shapes(name, n_pages, page_size, max_pages);
  if ((long)max_pages * page_size != Smax)
    throw std::runtime_error(std::string(name) +
                             ": Smax must be max_pages * page_size");
  pm.table = block_table;
  pm.max_pages = max_pages;
  pm.n_pages = n_pages;
  return pm;
}

// Makes `device` HIP's current device for the scope of a host call, so the
// launches (and decode's CU count) belong to the device the tensors and the
// stream are on; puts the caller's device back afterwards. `name` opens the
// error messages.
class DeviceScope {
 public:
  DeviceScope(const char* name, int device) {
    if (hipGetDevice(&prev_) != hipSuccess)
      throw std::runtime_error(std::string(name) +
                               ": cannot read the current device");
    if (device != prev_) {
      if (hipSetDevice(device) != hipSuccess)
        throw std::runtime_error(std::string(name) +
                                 ": cannot select device " +
                                 std::to_string(device));
      changed_ = true;
    }
  }
  ~DeviceScope() {
    if (changed_) (void)hipSetDevice(prev_);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;

 private:
  int prev_ = 0;
  bool changed_ = false;
};

// CUs of the current device, asked each time (no process-wide cache: hosts
// can hold different devices).
inline int device_cu_count(const char* name) {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess || n < 1)
    throw std::runtime_error(std::string(name) +
                             ": cannot read the CU count");
  return n;
}

}  // namespace adapcc

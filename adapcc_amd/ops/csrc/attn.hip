// Hand-written CDNA4 flash attention (gfx950), bf16, head_dim=64, in two
// modes: causal with S % 128 == 0 (GPT-2), and non-causal self-attention
// over any S >= 1 (ViT: S = 197).
//
// Replaces the stock SDPA path for the GPT-2 flagship workload, where the
// aotriton kernels ran at ~2% of the MFMA roof (rocprof round-1 evidence:
// attention was 27.7% of the training step). Design per the MI355X HIP
// guide's attention recipe: per-wave 32-row Q blocks, K/V tiles staged in
// LDS (XOR-swizzled K rows for conflict-free ds_read_b128; a custom
// interleaved V image consumed with ds_read_b64_tr_b16 hardware transpose
// reads), softmax kept lane-local by computing S^T = K·Q^T with
// v_mfma_f32_32x32x16_bf16 so each lane owns one Q row's scores, online
// softmax in the exp2 domain, and P redistributed to MFMA operand layout
// with v_cvt_pk_bf16_f32 + v_permlane32_swap_b32 (no LDS round trip).
// The MFMA fragment maps and the LDS row image are in attn_frag.h.
//
// Forward computes O^T = V^T · P^T per 32-wide KV tile so the online-max
// state and the O accumulator stay indexed by the SAME lane-local q; the
// backward splits FA2-style into a dq kernel (q-tile outer) and a dkv
// kernel (kv-tile outer), both recomputing P from the saved logsumexp.
//
// The three kernels are templates on <kCausal, kRagged>. <true,false> is
// the GPT-2 case. The non-causal mode loops over all ceil(S/64) tiles;
// its kRagged form (S % 128 != 0) clamps the row index of every load to
// S-1 (so no byte at a row >= S is read and whatever lands in a padding
// position is finite), masks keys >= S to kNegBig before the running max
// (P forced to 0 in the backward), predicates every store on row < S, and
// skips the MFMA/softmax work of 32-row half-tiles and of waves that are
// all padding (those waves still stage and take every barrier).
//
// Reference parity note: the reference (JoeyYoung/adapcc) has no attention
// kernels (models used stock torch); this op exists to meet BASELINE.json's
// "hot ops as hand-written MFMA/LDS kernels" requirement.

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "attn_frag.h"

namespace adapcc {

namespace {

constexpr int kQT = 128;    // q rows per workgroup (32 per wave)
constexpr float kNegBig = -3.0e38f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Strides for one tensor: plane = b*sb + h*sh, row stride ss (elements).
struct TStride {
  long sb, sh, ss;
};

// Base of the (b, h) plane of a tensor.
template <typename T>
__device__ __forceinline__ T* plane(T* x, const TStride& s, int b, int h) {
  return x + (long)b * s.sb + (long)h * s.sh;
}

// One parameter block for all three kernels; the forward fills and reads
// only the first part.
struct FaParams {
  const __bf16 *q, *k, *v;
  __bf16* o;           // written by the forward, read by the dq kernel
  float* lse;          // [B,H,S] natural-log row logsumexp
  TStride qs, ks, vs, os;
  int H, S;
  float scale;
  // backward only
  const __bf16* dout;
  float* delta;        // [B,H,S] rowsum(dO*O): written by the dq kernel,
                       // read by the dkv kernel launched after it
  __bf16 *dq, *dk, *dv;
  TStride dos_, dqs, dks, dvs;
};

// Row index used for a load: in the ragged mode rows >= S do not exist, so
// they read row S-1 instead (real data, hence finite).
// Two spellings, chosen per kernel by what the register allocator makes of
// them: the forward keeps 64-bit row arithmetic (its causal code is then
// instruction for instruction the earlier one), the backward kernels index
// in 32 bits, which keeps all their instantiations free of scratch.
template <bool kRagged>
__device__ __forceinline__ long ld_row(long row, int S) {
  return kRagged ? (long)min((int)row, S - 1) : row;
}
template <bool kRagged>
__device__ __forceinline__ int ld_row32(int row, int S) {
  return kRagged ? min(row, S - 1) : row;
}

// ---------------------------------------------------------------------------
// Staging: 256 threads cooperatively copy a [64][64] bf16 tile (8 KB) from
// global (row stride `ss` elements) into an LDS image of two 32-row halves
// (row_img_byte addresses within each half). Thread t moves the 16 B at
// column scol = (t&7)*8 of rows srow = t>>3 and srow+32: two 16-B loads, held
// in registers across the tile's compute, then two 16-B ds_writes.
// ---------------------------------------------------------------------------
constexpr int kHalfImg = 4096;       // one 32-row half
constexpr int kImg = 2 * kHalfImg;   // one 64-row image

// Image `buf` (0/1) of a double-buffered pair that starts at `base`.
__device__ __forceinline__ char* img(char* base, int buf) {
  return base + buf * kImg;
}

struct RowPair {
  uint4 a, b;  // this thread's 16 B of rows srow and srow+32
};

// r0, r1: the (clamped) global rows that land in image rows srow, srow+32.
__device__ __forceinline__ RowPair ld_pair(const __bf16* g, long ss, long r0,
                                           long r1, int scol) {
  return {*reinterpret_cast<const uint4*>(g + r0 * ss + scol),
          *reinterpret_cast<const uint4*>(g + r1 * ss + scol)};
}

__device__ __forceinline__ void st_pair(char* im, int srow, int scol,
                                        const RowPair& x) {
  *reinterpret_cast<uint4*>(im + row_img_byte(srow, scol)) = x.a;
  *reinterpret_cast<uint4*>(im + kHalfImg + row_img_byte(srow, scol)) = x.b;
}

// The dkv kernel's side tile: lse*log2e and delta of a q tile's 64 rows, as
// two double-buffered float[64] pairs (lse2 at [0,128), delta at [128,256)),
// staged by threads 0..63 alongside the row images.
constexpr int kSideDelta = 128;

struct SideVal {
  float lse2, delta;
};

__device__ __forceinline__ SideVal ld_side(const float* lseg,
                                           const float* deltag, int row) {
  return {lseg[row] * kLog2e, deltag[row]};
}

// Buffer `buf` of the lse2 tile; its delta twin is kSideDelta floats on.
__device__ __forceinline__ float* side_buf(float* side, int buf) {
  return side + (buf ? 64 : 0);
}

// Two stores off two bases with one unsigned index: spelled as one base
// plus a constant, the dkv kernel takes one more VGPR.
__device__ __forceinline__ void st_side(float* side, int buf, unsigned i,
                                        const SideVal& x) {
  side[(buf ? 64 : 0) + i] = x.lse2;
  (side + kSideDelta)[(buf ? 64 : 0) + i] = x.delta;
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

// exp2(s*c1 - off): P against the running max (forward, off = m*c1) or the
// saved logsumexp (backward, off = lse*log2e).
__device__ __forceinline__ float p_elem(float s, float c1, float off) {
  return __builtin_amdgcn_exp2f(__builtin_fmaf(s, c1, -off));
}

// dS = P * (dP - D) * scale
__device__ __forceinline__ float ds_elem(float pe, float dp, float delta,
                                         float scale) {
  return pe * (dp - delta) * scale;
}

// ---------------------------------------------------------------------------
// Forward.
// Grid: (ceil(S/128), B*H); block 256 = 4 waves, wave w owns q rows
// qt*128 + w*32 .. +31.
// ---------------------------------------------------------------------------
template <bool kCausal, bool kRagged>
__global__ __launch_bounds__(256, 3) void fa_fwd_kernel(FaParams p) {
  static_assert(!(kCausal && kRagged), "causal needs S % 128 == 0");
  // 64-row KV tiles, double-buffered: K images, then V images.
  __shared__ __attribute__((aligned(16))) char smem[4 * kImg];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kImg;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int qt = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;

  const __bf16* qg = plane(p.q, p.qs, b, h);
  const __bf16* kg = plane(p.k, p.ks, b, h);
  const __bf16* vg = plane(p.v, p.vs, b, h);
  __bf16* og = plane(p.o, p.os, b, h);
  float* lseg = p.lse + (long)bh * p.S;

  const int qb = qt * kQT + wave * 32;      // this wave's first q row
  const int qrow = qb + (lane & 31);        // this lane's q row
  const long qld = ld_row<kRagged>((long)qrow, p.S);

  // Q^T B-fragments, direct from global: lane l holds
  // Q[qrow][chunk*16 + 8*hi + e].
  bf16x8 qf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(
        qg + qld * p.qs.ss + c * 16 + hi * 8);

  f32x16 acc0 = {}, acc1 = {};
  float m = kNegBig, ssum = 0.f;
  const float c1 = p.scale * kLog2e;
  float mc = m * c1;
  // defer-max threshold (guide T13): skip the O/ssum rescale while the
  // tile max grows by <= 8 natural-log units; P is then bounded by e^8,
  // which f32 row sums and the bf16 P quantization tolerate (~3x max-abs
  // error vs always-rescale; covered by the spiked-key GPU test).
  const float thr = 8.0f / p.scale;

  const int srow = threadIdx.x >> 3;        // staging: this thread's row
  const int scol = (threadIdx.x & 7) * 8;   // and column (bf16)
  // 64-row tiles: up to the diagonal (causal) or all of them
  const int n64 = kCausal ? (qt + 1) * (kQT / 64) : (p.S + 63) / 64;

  // prologue: stage tile 0
  {
    const long r0 = ld_row<kRagged>((long)srow, p.S);
    const long r1 = ld_row<kRagged>((long)(srow + 32), p.S);
    st_pair(img(kimg, 0), srow, scol, ld_pair(kg, p.ks.ss, r0, r1, scol));
    st_pair(img(vimg, 0), srow, scol, ld_pair(vg, p.vs.ss, r0, r1, scol));
  }
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < n64; ++t) {
    // issue next tile's staging loads early; writes land after compute
    RowPair nk, nv;
    const bool pref = t + 1 < n64;
    if (pref) {
      const long kb = (long)(t + 1) * 64 + srow;
      const long kb0 = ld_row<kRagged>(kb, p.S);
      const long kb1 = ld_row<kRagged>(kb + 32, p.S);
      nk = ld_pair(kg, p.ks.ss, kb0, kb1, scol);
      nv = ld_pair(vg, p.vs.ss, kb0, kb1, scol);
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kbase = t * 64 + half * 32;
      if (kCausal) {
        if (kbase > qb + 31) break;  // wave-uniform causal cut
      } else if (kRagged) {
        // wave-uniform: a half-tile or a wave that is all padding
        if (kbase >= p.S || qb >= p.S) break;
      }
      const char* ki = img(kimg, cur) + half * kHalfImg;
      const char* vi = img(vimg, cur) + half * kHalfImg;

      // S^T tile: C[k][q] = sum_d K[k][d] * Q[q][d]
      f32x16 s = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        s = mfma(read_row_frag(ki, lane, c), qf[c], s);
      __builtin_amdgcn_s_setprio(0);

      float pv[16];
      float tmax = kNegBig;
      if (kCausal ? kbase + 31 > qb : kRagged && kbase + 31 >= p.S) {
        // diagonal tile for this wave: apply the causal mask; ragged: the
        // tile that holds key S-1, mask the keys past it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kglob = kbase + crow(r, hi);
          pv[r] = (kCausal ? kglob > qrow : kglob >= p.S) ? kNegBig : s[r];
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
      if (!__all(tmax <= m + thr)) {
        const float mnew = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f((m - mnew) * c1);
        m = mnew;
        mc = m * c1;
        ssum *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc0[r] *= alpha;
          acc1[r] *= alpha;
        }
      }

      // P = exp2(S*c1 - mc) in place; accumulate lane-partial row sum
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pv[r] = p_elem(pv[r], c1, mc);
        psum += pv[r];
      }
      ssum += psum;

      // redistribute P to operand fragments (k blocks 0-15 / 16-31)
      const bf16x8 p0 = pack_frag(&pv[0]);
      const bf16x8 p1 = pack_frag(&pv[8]);

      // O^T += V^T · P^T  (A = V^T via hardware transpose reads)
      __builtin_amdgcn_s_setprio(1);
      acc0 = mfma(read_tr_frag(vi, lane, 0, 0), p0, acc0);
      acc0 = mfma(read_tr_frag(vi, lane, 1, 0), p1, acc0);
      acc1 = mfma(read_tr_frag(vi, lane, 0, 1), p0, acc1);
      acc1 = mfma(read_tr_frag(vi, lane, 1, 1), p1, acc1);
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_pair(img(kimg, cur ^ 1), srow, scol, nk);
      st_pair(img(vimg, cur ^ 1), srow, scol, nv);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: combine row-sum halves, normalize, store O and lse
  const float stot = ssum + __shfl_xor(ssum, 32, 64);
  const float inv = 1.f / stot;
  if (kRagged && qrow >= p.S) return;  // stores only; no barrier follows
  if ((lane >> 5) == 0)
    lseg[qrow] = p.scale * m + __builtin_amdgcn_logf(stot) * kLn2;

  __bf16* orow = og + (long)qrow * p.os.ss;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const f32x16& a = db ? acc1 : acc0;
#pragma unroll
    for (int mq = 0; mq < 4; ++mq)
      store4_bf16(orow + db * 32 + 8 * mq + 4 * hi, a[4 * mq] * inv,
                  a[4 * mq + 1] * inv, a[4 * mq + 2] * inv,
                  a[4 * mq + 3] * inv);
  }
}

// ---------------------------------------------------------------------------
// Backward dQ. Grid (ceil(S/128), B*H). Per q-tile, loop kv tiles:
//   S^T = K·Q^T           (A=K row frags, B=Q^T frags)      lane-q local
//   P^T = exp2(S*c1 - lse*log2e), masked (causal, or keys >= S)
//   dP^T = V·dO^T         (A=V row frags, B=dO^T frags)
//   dS^T = P^T * (dP^T - D[q]) * scale
//   dQ^T += K^T·dS^T      (A=K^T tr frags, B=packed dS^T)
//
// The prologue also forms D[q] = rowsum(dO*O) from the dO fragments it holds
// anyway plus one read of O, and stores it to p.delta for the dkv kernel.
// ---------------------------------------------------------------------------
// Sum of the 8 bf16 products a[e]*b[e] in f32 (each product is exact),
// added as a balanced tree over adjacent elements:
// ((p0+p1)+(p2+p3)) + ((p4+p5)+(p6+p7)). The row sum is kept in this fixed
// pairwise order end to end (see the dq prologue): it is the order of the
// fp32 row reduction this replaces, so delta, and with it every gradient,
// keeps its bits.
__device__ __forceinline__ float dot8_tree(bf16x8 a, bf16x8 b) {
  union {
    bf16x8 f;
    unsigned u[4];
  } x, y;
  x.f = a;
  y.f = b;
  float pr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // (+0 + p_even) + p_odd, one rounding: the element pair of word i
    const float ev = __builtin_fmaf(__uint_as_float(x.u[i] << 16),
                                    __uint_as_float(y.u[i] << 16), 0.f);
    pr[i] = __builtin_fmaf(__uint_as_float(x.u[i] & 0xffff0000u),
                           __uint_as_float(y.u[i] & 0xffff0000u), ev);
  }
  return (pr[0] + pr[1]) + (pr[2] + pr[3]);
}

template <bool kCausal, bool kRagged>
__global__ __launch_bounds__(256, 3) void fa_bwd_dq_kernel(FaParams p) {
  static_assert(!(kCausal && kRagged), "causal needs S % 128 == 0");
  // 64-row KV tiles, double-buffered: K images, then V images.
  __shared__ __attribute__((aligned(16))) char smem[4 * kImg];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kImg;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int qt = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;

  const __bf16* qg = plane(p.q, p.qs, b, h);
  const __bf16* kg = plane(p.k, p.ks, b, h);
  const __bf16* vg = plane(p.v, p.vs, b, h);
  const __bf16* dog = plane(p.dout, p.dos_, b, h);
  const __bf16* og = plane(p.o, p.os, b, h);
  __bf16* dqg = plane(p.dq, p.dqs, b, h);

  const int qb = qt * kQT + wave * 32;
  const int qrow = qb + (lane & 31);
  const long qld = ld_row32<kRagged>(qrow, p.S);

  // this lane holds 32 of its q row's 64 dO (and O) elements as four runs
  // of 8 (columns c*16 + hi*8 ..); lane^32 holds the runs in between. n16[c]
  // joins each run with its neighbour from the partner lane, so both lanes
  // walk the same adjacent-pair tree over the whole row.
  bf16x8 qf[4], dof[4];
  float n16[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    dof[c] = *reinterpret_cast<const bf16x8*>(
        dog + qld * p.dos_.ss + c * 16 + hi * 8);
    const float n8 = dot8_tree(
        dof[c], *reinterpret_cast<const bf16x8*>(
                    og + qld * p.os.ss + c * 16 + hi * 8));
    n16[c] = n8 + __shfl_xor(n8, 32, 64);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(
        qg + qld * p.qs.ss + c * 16 + hi * 8);
  const float lse2 = p.lse[(long)bh * p.S + qld] * kLog2e;
  const float dvq = (n16[0] + n16[1]) + (n16[2] + n16[3]);
  if (hi == 0 && (!kRagged || qrow < p.S))
    p.delta[(long)bh * p.S + qrow] = dvq;
  const float c1 = p.scale * kLog2e;

  f32x16 dacc0 = {}, dacc1 = {};

  const int srow = threadIdx.x >> 3;
  const int scol = (threadIdx.x & 7) * 8;
  const int n64 = kCausal ? (qt + 1) * (kQT / 64) : (p.S + 63) / 64;
  {
    const long r0 = ld_row32<kRagged>(srow, p.S);
    const long r1 = ld_row32<kRagged>(srow + 32, p.S);
    st_pair(img(kimg, 0), srow, scol, ld_pair(kg, p.ks.ss, r0, r1, scol));
    st_pair(img(vimg, 0), srow, scol, ld_pair(vg, p.vs.ss, r0, r1, scol));
  }
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < n64; ++t) {
    RowPair nk, nv;
    const bool pref = t + 1 < n64;
    if (pref) {
      const long kb0 = ld_row32<kRagged>((t + 1) * 64 + srow, p.S);
      const long kb1 = ld_row32<kRagged>((t + 1) * 64 + srow + 32, p.S);
      nk = ld_pair(kg, p.ks.ss, kb0, kb1, scol);
      nv = ld_pair(vg, p.vs.ss, kb0, kb1, scol);
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kbase = t * 64 + half * 32;
      if (kCausal) {
        if (kbase > qb + 31) break;
      } else if (kRagged) {
        if (kbase >= p.S || qb >= p.S) break;  // all padding
      }
      const char* ki = img(kimg, cur) + half * kHalfImg;
      const char* vi = img(vimg, cur) + half * kHalfImg;

      f32x16 s = {}, dp = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s = mfma(read_row_frag(ki, lane, c), qf[c], s);
        dp = mfma(read_row_frag(vi, lane, c), dof[c], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // two loops on purpose: the unmasked one carries no compare
      float ds[16];
      if (kCausal ? kbase + 31 > qb : kRagged && kbase + 31 >= p.S) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kglob = kbase + crow(r, hi);
          const float pe = (kCausal ? kglob > qrow : kglob >= p.S)
                               ? 0.f
                               : p_elem(s[r], c1, lse2);
          ds[r] = ds_elem(pe, dp[r], dvq, p.scale);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ds[r] = ds_elem(p_elem(s[r], c1, lse2), dp[r], dvq, p.scale);
      }
      const bf16x8 d0 = pack_frag(&ds[0]);
      const bf16x8 d1 = pack_frag(&ds[8]);
      __builtin_amdgcn_s_setprio(1);
      dacc0 = mfma(read_tr_frag(ki, lane, 0, 0), d0, dacc0);
      dacc0 = mfma(read_tr_frag(ki, lane, 1, 0), d1, dacc0);
      dacc1 = mfma(read_tr_frag(ki, lane, 0, 1), d0, dacc1);
      dacc1 = mfma(read_tr_frag(ki, lane, 1, 1), d1, dacc1);
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_pair(img(kimg, cur ^ 1), srow, scol, nk);
      st_pair(img(vimg, cur ^ 1), srow, scol, nv);
    }
    __syncthreads();
    cur ^= 1;
  }

  if (kRagged && qrow >= p.S) return;  // stores only; no barrier follows
  __bf16* drow = dqg + (long)qrow * p.dqs.ss;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const f32x16& a = db ? dacc1 : dacc0;
#pragma unroll
    for (int mq = 0; mq < 4; ++mq)
      store4_bf16(drow + db * 32 + 8 * mq + 4 * hi, a[4 * mq], a[4 * mq + 1],
                  a[4 * mq + 2], a[4 * mq + 3]);
  }
}

// ---------------------------------------------------------------------------
// Backward dK/dV. Grid (ceil(S/128), B*H); wave owns kv rows kt*128+w*32..+31,
// loops q tiles >= the diagonal (causal) or all q tiles:
//   S = Q·K^T   as C[q][k]: A=Q row frags (LDS), B=K direct (registers)
//   P^T[k][q] = exp2(S*c1 - lse[q]*log2e) masked            lane-k local
//   dP[q][k]: A=dO row frags, B=V^T direct (registers)
//   dV += P^T·dO   (A=packed P^T, B=dO^T tr frags)
//   dS^T = P^T*(dP-D[q])*scale;  dK += dS^T·Q (A=packed dS^T, B=Q^T tr)
// ---------------------------------------------------------------------------
template <bool kCausal, bool kRagged>
__global__ __launch_bounds__(256, 2) void fa_bwd_dkv_kernel(FaParams p) {
  static_assert(!(kCausal && kRagged), "causal needs S % 128 == 0");
  // 64-row q tiles, double-buffered: Q images, then dO images, then the
  // lse2/delta side tile; the epilogue reuses [0,32K) as per-wave f32
  // scratch for the coalesced dV/dK stores.
  __shared__ __attribute__((aligned(16))) char smem[4 * kImg + 1024];
  char* const qimg = smem;
  char* const doimg = smem + 2 * kImg;
  float* const side = reinterpret_cast<float*>(smem + 4 * kImg);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int kt = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;

  const __bf16* qg = plane(p.q, p.qs, b, h);
  const __bf16* kg = plane(p.k, p.ks, b, h);
  const __bf16* vg = plane(p.v, p.vs, b, h);
  const __bf16* dog = plane(p.dout, p.dos_, b, h);
  __bf16* dkg = plane(p.dk, p.dks, b, h);
  __bf16* dvg = plane(p.dv, p.dvs, b, h);
  const float* lseg = p.lse + (long)bh * p.S;
  const float* deltag = p.delta + (long)bh * p.S;

  const int kbb = kt * kQT + wave * 32;     // this wave's first k row
  const int krow = kbb + (lane & 31);       // this lane's k row
  const long kld = ld_row32<kRagged>(krow, p.S);

  // K and V^T B-fragments direct from global: lane holds
  // K[krow][chunk*16+8*hi+e] / V[krow][...]
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    kf[c] = *reinterpret_cast<const bf16x8*>(
        kg + kld * p.ks.ss + c * 16 + hi * 8);
    vf[c] = *reinterpret_cast<const bf16x8*>(
        vg + kld * p.vs.ss + c * 16 + hi * 8);
  }

  const float c1 = p.scale * kLog2e;
  f32x16 dvacc0 = {}, dvacc1 = {}, dkacc0 = {}, dkacc1 = {};

  const int srow = threadIdx.x >> 3;
  const int scol = (threadIdx.x & 7) * 8;
  const int t0 = kCausal ? kt : 0;          // first 64-row q tile
  const int n64 = (p.S + 63) / 64;

  // stage q/dO tile t0 and its side tile
  {
    const int qb0 = t0 * 64;
    const long r0 = ld_row32<kRagged>(qb0 + srow, p.S);
    const long r1 = ld_row32<kRagged>(qb0 + srow + 32, p.S);
    st_pair(img(qimg, 0), srow, scol, ld_pair(qg, p.qs.ss, r0, r1, scol));
    st_pair(img(doimg, 0), srow, scol, ld_pair(dog, p.dos_.ss, r0, r1, scol));
    if (threadIdx.x < 64) {
      const int rq = ld_row32<kRagged>(qb0 + (int)threadIdx.x, p.S);
      st_side(side, 0, threadIdx.x, ld_side(lseg, deltag, rq));
    }
  }
  __syncthreads();

  int cur = 0;
  for (int t = t0; t < n64; ++t) {
    RowPair nq, nd;
    SideVal ns = {0.f, 0.f};
    const bool pref = t + 1 < n64;
    if (pref) {
      const int qb1 = (t + 1) * 64;
      const long r0 = ld_row32<kRagged>(qb1 + srow, p.S);
      const long r1 = ld_row32<kRagged>(qb1 + srow + 32, p.S);
      nq = ld_pair(qg, p.qs.ss, r0, r1, scol);
      nd = ld_pair(dog, p.dos_.ss, r0, r1, scol);
      if (threadIdx.x < 64) {
        const int rq = ld_row32<kRagged>(qb1 + (int)threadIdx.x, p.S);
        ns = ld_side(lseg, deltag, rq);
      }
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int qbase = t * 64 + half * 32;
      if (kCausal) {
        if (qbase + 31 < kbb) continue;     // wave-uniform causal cut
      } else if (kRagged) {
        // wave-uniform: a q half-tile or a k-row wave that is all padding
        if (qbase >= p.S || kbb >= p.S) break;
      }
      const char* qi = img(qimg, cur) + half * kHalfImg;
      const char* di = img(doimg, cur) + half * kHalfImg;
      const float* lsec = side_buf(side, cur) + half * 32;
      const float* dc = lsec + kSideDelta;

      f32x16 sacc = {}, dp = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sacc = mfma(read_row_frag(qi, lane, c), kf[c], sacc);
        dp = mfma(read_row_frag(di, lane, c), vf[c], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // two loops on purpose: the unmasked one carries no compare
      float pv[16], ds[16];
      if (kCausal ? qbase < kbb + 31 : kRagged && qbase + 31 >= p.S) {
        // diagonal: mask q < k; ragged: mask the q rows past S-1
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qglob = qbase + crow(r, hi);
          pv[r] = (kCausal ? qglob < krow : qglob >= p.S)
                      ? 0.f
                      : p_elem(sacc[r], c1, lsec[crow(r, hi)]);
          ds[r] = ds_elem(pv[r], dp[r], dc[crow(r, hi)], p.scale);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pv[r] = p_elem(sacc[r], c1, lsec[crow(r, hi)]);
          ds[r] = ds_elem(pv[r], dp[r], dc[crow(r, hi)], p.scale);
        }
      }
      const bf16x8 p0 = pack_frag(&pv[0]);
      const bf16x8 p1 = pack_frag(&pv[8]);
      __builtin_amdgcn_s_setprio(1);
      dvacc0 = mfma(p0, read_tr_frag(di, lane, 0, 0), dvacc0);
      dvacc0 = mfma(p1, read_tr_frag(di, lane, 1, 0), dvacc0);
      dvacc1 = mfma(p0, read_tr_frag(di, lane, 0, 1), dvacc1);
      dvacc1 = mfma(p1, read_tr_frag(di, lane, 1, 1), dvacc1);
      __builtin_amdgcn_s_setprio(0);
      const bf16x8 e0 = pack_frag(&ds[0]);
      const bf16x8 e1 = pack_frag(&ds[8]);
      __builtin_amdgcn_s_setprio(1);
      dkacc0 = mfma(e0, read_tr_frag(qi, lane, 0, 0), dkacc0);
      dkacc0 = mfma(e1, read_tr_frag(qi, lane, 1, 0), dkacc0);
      dkacc1 = mfma(e0, read_tr_frag(qi, lane, 0, 1), dkacc1);
      dkacc1 = mfma(e1, read_tr_frag(qi, lane, 1, 1), dkacc1);
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_pair(img(qimg, cur ^ 1), srow, scol, nq);
      st_pair(img(doimg, cur ^ 1), srow, scol, nd);
      if (threadIdx.x < 64) st_side(side, cur ^ 1, threadIdx.x, ns);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: C[k-rows][d=lane&31] per accumulator pair -> round-trip
  // through this wave's 8 KB LDS scratch for coalesced row-major stores.
  __syncthreads();
  float* scratch = reinterpret_cast<float*>(smem) + wave * 2048;  // 8 KB
#pragma unroll
  for (int t = 0; t < 2; ++t) {  // 0: dV, 1: dK
    const f32x16& a0 = t ? dkacc0 : dvacc0;
    const f32x16& a1 = t ? dkacc1 : dvacc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      scratch[crow(r, hi) * 64 + (lane & 31)] = a0[r];
      scratch[crow(r, hi) * 64 + 32 + (lane & 31)] = a1[r];
    }
    __builtin_amdgcn_s_waitcnt(0);  // drain LDS writes (wave-local reuse)
    __bf16* outg = (t ? dkg : dvg);
    const TStride& os = t ? p.dks : p.dvs;
    const int row = lane >> 1;           // 2 lanes per k row
    const int dhalf = (lane & 1) * 32;
#pragma unroll
    for (int mq = 0; mq < 8; ++mq) {
      const float* src = scratch + row * 64 + dhalf + mq * 4;
      if (!kRagged || kbb + row < p.S)
        store4_bf16(outg + (long)(kbb + row) * os.ss + dhalf + mq * 4, src[0],
                    src[1], src[2], src[3]);
    }
    __syncthreads();  // scratch reused for dK after dV drains
  }
}

// ---------------------------------------------------------------------------
// Host side.
// ---------------------------------------------------------------------------
TStride stride_at(const long* s, int i) {
  return {s[3 * i], s[3 * i + 1], s[3 * i + 2]};
}

void check_len(const char* name, int S, bool causal) {
  if (S < 1) throw std::runtime_error(std::string(name) + ": S < 1");
  if (causal && S % kQT != 0)
    throw std::runtime_error(std::string(name) +
                             ": causal needs S % 128 == 0");
}

// Calls f(kCausal, kRagged) with the mode as two std::bool_constant values.
template <typename F>
void with_mode(bool causal, int S, F&& f) {
  if (causal)
    f(std::true_type{}, std::false_type{});
  else if (S % kQT == 0)
    f(std::false_type{}, std::false_type{});
  else
    f(std::false_type{}, std::true_type{});
}

// The part of the parameter block that both directions fill. strides: 3 per
// tensor, q, k, v, o first.
FaParams fwd_params(const void* q, const void* k, const void* v, void* o,
                    float* lse, int H, int S, const long* strides,
                    float scale) {
  FaParams p = {};
  p.q = (const __bf16*)q;
  p.k = (const __bf16*)k;
  p.v = (const __bf16*)v;
  p.o = (__bf16*)o;
  p.lse = lse;
  p.qs = stride_at(strides, 0);
  p.ks = stride_at(strides, 1);
  p.vs = stride_at(strides, 2);
  p.os = stride_at(strides, 3);
  p.H = H;
  p.S = S;
  p.scale = scale;
  return p;
}

}  // namespace

// ---------------------------------------------------------------------------
// Host launchers (bound in bindings.hip).
// ---------------------------------------------------------------------------
void fa_forward(const void* q, const void* k, const void* v, void* o,
                float* lse, int B, int H, int S, const long* strides,
                float scale, hipStream_t stream, bool causal) {
  check_len("fa_forward", S, causal);
  const FaParams p = fwd_params(q, k, v, o, lse, H, S, strides, scale);
  const dim3 grid((S + kQT - 1) / kQT, B * H);
  with_mode(causal, S, [&](auto c, auto r) {
    constexpr bool kC = decltype(c)::value, kR = decltype(r)::value;
    hipLaunchKernelGGL((fa_fwd_kernel<kC, kR>), grid, dim3(256), 0, stream, p);
  });
}

// strides: q, k, v, o, dO, dq, dk, dv. delta is a [B,H,S] f32 workspace the
// dq kernel fills and the dkv kernel consumes; o and lse are only read.
void fa_backward(const void* q, const void* k, const void* v, const void* o,
                 const void* do_, const float* lse, float* delta, void* dq,
                 void* dk, void* dv, int B, int H, int S, const long* strides,
                 float scale, hipStream_t stream, bool causal) {
  check_len("fa_backward", S, causal);
  FaParams p = fwd_params(q, k, v, const_cast<void*>(o),
                          const_cast<float*>(lse), H, S, strides, scale);
  p.dout = (const __bf16*)do_;
  p.delta = delta;
  p.dq = (__bf16*)dq;
  p.dk = (__bf16*)dk;
  p.dv = (__bf16*)dv;
  p.dos_ = stride_at(strides, 4);
  p.dqs = stride_at(strides, 5);
  p.dks = stride_at(strides, 6);
  p.dvs = stride_at(strides, 7);
  const dim3 grid((S + kQT - 1) / kQT, B * H);
  with_mode(causal, S, [&](auto c, auto r) {
    constexpr bool kC = decltype(c)::value, kR = decltype(r)::value;
    hipLaunchKernelGGL((fa_bwd_dq_kernel<kC, kR>), grid, dim3(256), 0, stream,
                       p);
    hipLaunchKernelGGL((fa_bwd_dkv_kernel<kC, kR>), grid, dim3(256), 0, stream,
                       p);
  });
}

}  // namespace adapcc

// Hand-written CDNA4 flash attention (gfx950), bf16, head_dim 64 or 128, in
// three modes: causal with S % 128 == 0 (GPT-2), non-causal self-attention
// over any S >= 1 (ViT: S = 197), and variable-length, causal or not, over
// sequences of any lengths packed back to back in [total, H, head_dim]
// tensors with cu_seqlens (GPT-2 on documents).
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
// The three kernels are templates on <kHD, kCausal, kRagged, kDrop, kVarlen,
// kGqa>.
// <64,true,false,false,false> is the GPT-2 case.
// kHD is the head dimension, 64 or 128. A 128-wide row is two blocks of 64
// columns and a 64-row tile two of attn_frag.h's row images side by side,
// each with its own 128-byte-row swizzle, so every fragment read is the
// 64-wide one at a block offset: S^T accumulates over kHD/16 chunks in
// column order, O^T (dQ^T, dV, dK) is kHD/32 accumulators that share one P
// (dS) and, in the forward, one rescale factor, and delta = rowsum(dO*O)
// adds the two blocks' pairwise trees, lower block first. Staging moves
// twice the bytes per tile (four 16-B loads per thread and tensor), LDS is
// 64 KB per workgroup (65 KB in the dkv kernel, plus the dropout parts), and
// the launch bounds follow: forward and dq 2 workgroups per CU (up to 256
// VGPRs), dkv 1, since its two K/V operand sets and eight accumulators need
// the AGPRs as well (no instantiation uses scratch). Mask, tile map, plan
// and the causal, ragged, dropout and varlen logic do not depend on kHD,
// and the kHD = 64 instantiations are instruction for instruction the
// kernels from before the parameter: where a loop over blocks would do,
// the blocks are spelled out under `if constexpr` for that reason.
// kDrop adds attention dropout
// on P (mask function in attn_drop.h): the forward zeroes dropped P after
// the row sum, so the normaliser and lse are those of the undropped scores,
// and folds 1/(1-p) into the epilogue's 1/rowsum; delta = rowsum(dO*O) needs no
// change since O carries the dropout; the backward regenerates the mask and
// forms dS = P * (keep * dP/(1-p) - delta) * scale and
// dV = (P*keep)^T dO / (1-p), the last factor on the fp32 accumulator. The
// seed is read from device memory by the kernels, so a captured graph sees
// the value of each replay. The kDrop=false instantiations are instruction
// for instruction the kernels without the parameter.
// The non-causal mode loops over all ceil(S/64) tiles;
// its kRagged form (S % 128 != 0) clamps the row index of every load to
// S-1 (so no byte at a row >= S is read and whatever lands in a padding
// position is finite), masks keys >= S to kNegBig before the running max
// (P forced to 0 in the backward), predicates every store on row < S, and
// skips the MFMA/softmax work of 32-row half-tiles and of waves that are
// all padding (those waves still stage and take every barrier).
// kVarlen (always with kRagged) is that ragged code run per sequence: a
// plan kernel turns cu_seqlens into a (seq, tile, start, len) map on the
// device, the launch has total/128 + n_seqs workgroups in x and the heads
// in y, and a workgroup takes its tile, its length S = len and its first
// row from the map (an unused entry leaves before the first barrier); every
// row index is local to the sequence, lse and delta are [H, total], the
// dropout plane is seq*H + h. Its causal form is the one place where
// kCausal and kRagged meet: the tile loop stops at the diagonal or at
// ceil(S/64), whichever comes first, a row sees keys <= min(q, S-1), and
// in the dkv kernel q rows >= S get P = dS = 0. A valid row then computes
// bit for bit what the fixed-length causal kernel computes for it on the
// sequence zero-padded to a multiple of 128.
// kGqa is grouped-query (multi-query) attention: k, v, dk, dv have Hk =
// H / G heads, G a runtime integer > 1 (G == 1 launches the kGqa=false
// instantiations, which are instruction for instruction the kernels without
// the parameter), and query head h reads K/V head h / G. In the forward and
// the dq kernel that is the whole change: grid, q, o, dO, dq, lse, delta
// and the dropout plane b*H + h stay by query head. The dkv kernel's grid
// counts K/V heads; a workgroup loads the K/V fragments of its k tile once
// and walks the q tiles of the group's G query heads in turn, one flattened
// (head, tile) loop whose last tile of a head prefetches the first of the
// next, so the double buffer runs through. dV and dK accumulate over all of
// them in fp32 and one epilogue rounds the group sum once: no atomics, no
// second pass, deterministic. What moves from head to head is wave-uniform:
// the q, dO, lse and delta planes, the mask plane of the staged q parts,
// and (per lane, recomputed at each head) the k part of the mask word.
//
// Reference parity note: the reference (JoeyYoung/adapcc) has no attention
// kernels (models used stock torch); this op exists to meet BASELINE.json's
// "hot ops as hand-written MFMA/LDS kernels" requirement.

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "attn_drop.h"
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
  // dropout, kDrop instantiations only (both directions)
  const long* seed;    // device memory: a graph replay sees a fresh value
  unsigned drop_thr;   // keep iff word >= drop_thr
  float drop_rp;       // 1/(1-p)
  // variable-length mode, kVarlen instantiations only (both directions)
  const int4* tmap;    // [gridDim.x] (seq, tile, start, len), seq < 0: unused
  int total;           // packed rows; lse and delta are [H, total]
  // grouped-query mode, kGqa instantiations only (both directions)
  int G;               // query heads per K/V head: k, v, dk, dv have H/G heads
};

// Variable-length mode: q, k, v, ... are [total, H, kHD] views that hold the
// sequences back to back, and workgroup x of the launch owns the 128-row
// tile `tile` of sequence `seq`, rows start .. start+len-1 of the packed
// buffer, as the plan kernel (below) wrote it into tmap[x]. The kernels take
// start and len from the map alone, never from cu_seqlens, so the plan's
// clamping bounds every address. Inside the sequence the code is the ragged
// one with S = len and all row indices local; the mask plane is seq*H + h.
struct VarlenTile {
  int seq, tile, start, len;
};

__device__ __forceinline__ VarlenTile varlen_tile(const FaParams& p) {
  const int4 e = p.tmap[blockIdx.x];
  return {e.x, e.y, e.z, e.w};
}

// Base of a kernel's rows in x: the (b, h) plane, or in the variable-length
// mode head h from packed row row0 on.
template <bool kVarlen, typename T>
__device__ __forceinline__ T* seq_plane(T* x, const TStride& s, int b, int h,
                                        long row0) {
  if constexpr (kVarlen)
    return x + (long)h * s.sh + row0 * s.ss;
  else
    return plane(x, s, b, h);
}

// K/V head of query head h: h itself, or in the grouped-query mode h / G.
template <bool kGqa>
__device__ __forceinline__ int kv_head(int h, int G) {
  if constexpr (kGqa)
    return h / G;
  else
    return h;
}

// An entry the plan left unused (or, should the map ever be stale, a tile
// past its sequence): the workgroup leaves before its first barrier.
__device__ __forceinline__ bool varlen_idle(const VarlenTile& t) {
  return t.seq < 0 || (long)t.tile * kQT >= t.len;
}

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

// 64-row KV tiles that q tile qt walks (forward, dq): up to the diagonal
// when causal, to the last key when not; causal and ragged (the
// variable-length mode) stops at whichever comes first.
template <bool kCausal, bool kRagged>
__device__ __forceinline__ int tile_count(int qt, int S) {
  if (kCausal && kRagged) return min((qt + 1) * (kQT / 64), (S + 63) / 64);
  return kCausal ? (qt + 1) * (kQT / 64) : (S + 63) / 64;
}

// Is key kglob hidden from q row qrow? qlim = min(qrow, S-1), used by the
// causal ragged form alone.
template <bool kCausal, bool kRagged>
__device__ __forceinline__ bool key_masked(int kglob, int qrow, int qlim,
                                           int S) {
  if (kCausal && kRagged) return kglob > qlim;
  return kCausal ? kglob > qrow : kglob >= S;
}

// ---------------------------------------------------------------------------
// Staging: 256 threads cooperatively copy a [64][kHD] bf16 tile (8 KB at
// head_dim 64, 16 KB at 128) from global (row stride `ss` elements) into LDS.
// A row is kHD/64 blocks of 64 columns, and each block of the tile is one
// image of two 32-row halves (row_img_byte addresses within each half), the
// blocks' images side by side: attn_frag.h's [32][64] row image and its
// swizzle serve both widths. Thread t moves the 16 B at column scol =
// (t&7)*8 of every block of rows srow = t>>3 and srow+32: two 16-B loads per
// block, held in registers across the tile's compute, then as many 16-B
// ds_writes.
// ---------------------------------------------------------------------------
constexpr int kHalfImg = 4096;       // one 32-row half of one column block
constexpr int kImg = 2 * kHalfImg;   // one 64-row image of one column block

template <int kHD>
constexpr int kTileImg = (kHD / 64) * kImg;  // one 64-row tile, all blocks

// Tile image `buf` (0/1) of a double-buffered pair that starts at `base`.
template <int kHD>
__device__ __forceinline__ char* img(char* base, int buf) {
  return base + buf * kTileImg<kHD>;
}

// Fragment reads off a tile image (`im`: its 32-row half): 16-column chunk c
// of the row, and 32-column block db of the transpose, each inside the
// 64-column block that holds it. At head_dim 64 these are attn_frag.h's
// reads themselves.
template <int kHD>
__device__ __forceinline__ bf16x8 read_row_chunk(const char* im, int lane,
                                                 int c) {
  if constexpr (kHD == 64)
    return read_row_frag(im, lane, c);
  else
    return read_row_frag(im + (c >> 2) * kImg, lane, c & 3);
}

template <int kHD>
__device__ __forceinline__ bf16x8 read_tr_blk(const char* im, int lane,
                                              int kb, int db) {
  if constexpr (kHD == 64)
    return read_tr_frag(im, lane, kb, db);
  else
    return read_tr_frag(im + (db >> 1) * kImg, lane, kb, db & 1);
}

struct RowPair {
  uint4 a, b;  // this thread's 16 B of rows srow and srow+32, one block
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

// The same for all kHD/64 column blocks of the rows. Spelled out per block,
// not looped: the head_dim 64 kernels then compile to what they were before
// the width became a parameter.
template <int kHD>
struct RowTile {
  RowPair blk[kHD / 64];
};

template <int kHD>
__device__ __forceinline__ RowTile<kHD> ld_tile(const __bf16* g, long ss,
                                                long r0, long r1, int scol) {
  RowTile<kHD> x;
  x.blk[0] = ld_pair(g, ss, r0, r1, scol);
  if constexpr (kHD == 128) x.blk[1] = ld_pair(g + 64, ss, r0, r1, scol);
  return x;
}

template <int kHD>
__device__ __forceinline__ void st_tile(char* im, int srow, int scol,
                                        const RowTile<kHD>& x) {
  st_pair(im, srow, scol, x.blk[0]);
  if constexpr (kHD == 128) st_pair(im + kImg, srow, scol, x.blk[1]);
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

// Dropout (kDrop instantiations): the mask word of attn_drop.h splits into
// a per-q and a per-k part. Each kernel computes the part of the axis its
// lanes own once per lane; the part of the tile's 64 rows of the other axis
// is computed by threads 0..63 into a double-buffered unsigned[64] pair
// behind the kernel's other LDS, one tile ahead like the row images. Being
// computed, not loaded, it is written straight into the buffer the next
// iteration reads: the barrier that ended the previous iteration retired
// that buffer's readers.
template <bool kDrop>
constexpr int kPartBytes = kDrop ? 2 * 64 * 4 : 0;

__device__ __forceinline__ unsigned* part_buf(unsigned* part, int buf) {
  return part + (buf ? 64 : 0);
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
// qt*128 + w*32 .. +31. kGqa: k and v are read at head h / G.
// ---------------------------------------------------------------------------
template <int kHD, bool kCausal, bool kRagged, bool kDrop,
          bool kVarlen = false, bool kGqa = false>
__global__ __launch_bounds__(256, kHD == 64 ? 3 : 2) void fa_fwd_kernel(
    FaParams p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  static_assert(kVarlen ? kRagged : !(kCausal && kRagged),
                "fixed-length causal needs S % 128 == 0; varlen is ragged");
  constexpr int kNC = kHD / 16;  // 16-column chunks of a row
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  // 64-row KV tiles, double-buffered: K images, then V images (then the
  // tiles' dropout k parts).
  __shared__ __attribute__((aligned(16))) char
      smem[4 * kTileImg<kHD> + kPartBytes<kDrop>];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kTileImg<kHD>;
  [[maybe_unused]] unsigned* const kpart =
      reinterpret_cast<unsigned*>(smem + 4 * kTileImg<kHD>);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  // tile, mask plane, (b, h) of the tensor plane, length, and (varlen) the
  // sequence's first packed row
  int qt = blockIdx.x, bh = blockIdx.y, b, h, S = p.S;
  long row0 = 0;
  if constexpr (kVarlen) {
    const VarlenTile vt = varlen_tile(p);
    if (varlen_idle(vt)) return;
    qt = vt.tile;
    b = 0;
    h = blockIdx.y;
    bh = vt.seq * p.H + h;
    S = vt.len;
    row0 = vt.start;
  } else {
    b = bh / p.H;
    h = bh % p.H;
  }

  const __bf16* qg = seq_plane<kVarlen>(p.q, p.qs, b, h, row0);
  const int hk = kv_head<kGqa>(h, p.G);
  const __bf16* kg = seq_plane<kVarlen>(p.k, p.ks, b, hk, row0);
  const __bf16* vg = seq_plane<kVarlen>(p.v, p.vs, b, hk, row0);
  __bf16* og = seq_plane<kVarlen>(p.o, p.os, b, h, row0);
  float* lseg =
      p.lse + (kVarlen ? (long)h * p.total + row0 : (long)bh * S);

  const int qb = qt * kQT + wave * 32;      // this wave's first q row
  const int qrow = qb + (lane & 31);        // this lane's q row
  const long qld = ld_row<kRagged>((long)qrow, S);
  // causal and ragged: a row sees keys <= min(qrow, S-1). Rows >= S of the
  // wave that holds row S-1 thereby repeat that row, loads and mask alike,
  // so they never decide the wave-wide rescale below differently from it.
  [[maybe_unused]] const int qlim = min(qrow, S - 1);

  // Q^T B-fragments, direct from global: lane l holds
  // Q[qrow][chunk*16 + 8*hi + e].
  bf16x8 qf[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(
        qg + qld * p.qs.ss + c * 16 + hi * 8);

  // O^T, one accumulator per 32 columns; acc2, acc3 (columns 64..127) are
  // dead at head_dim 64
  f32x16 acc0 = {}, acc1 = {};
  [[maybe_unused]] f32x16 acc2 = {}, acc3 = {};
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
  const int n64 = tile_count<kCausal, kRagged>(qt, S);

  // dropout: this lane's q part; seed_hi feeds the tiles' k parts
  [[maybe_unused]] unsigned dqa = 0, seed_hi = 0;
  if constexpr (kDrop) {
    const unsigned long sd = (unsigned long)*p.seed;
    dqa = drop_q_part((unsigned)sd, bh, qrow);
    seed_hi = (unsigned)(sd >> 32);
  }

  // prologue: stage tile 0
  {
    const long r0 = ld_row<kRagged>((long)srow, S);
    const long r1 = ld_row<kRagged>((long)(srow + 32), S);
    st_tile<kHD>(img<kHD>(kimg, 0), srow, scol,
                 ld_tile<kHD>(kg, p.ks.ss, r0, r1, scol));
    st_tile<kHD>(img<kHD>(vimg, 0), srow, scol,
                 ld_tile<kHD>(vg, p.vs.ss, r0, r1, scol));
    if constexpr (kDrop)
      if (threadIdx.x < 64)
        kpart[threadIdx.x] = drop_k_part(seed_hi, bh, threadIdx.x);
  }
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < n64; ++t) {
    // issue next tile's staging loads early; writes land after compute
    RowTile<kHD> nk, nv;
    const bool pref = t + 1 < n64;
    if (pref) {
      const long kb = (long)(t + 1) * 64 + srow;
      const long kb0 = ld_row<kRagged>(kb, S);
      const long kb1 = ld_row<kRagged>(kb + 32, S);
      nk = ld_tile<kHD>(kg, p.ks.ss, kb0, kb1, scol);
      nv = ld_tile<kHD>(vg, p.vs.ss, kb0, kb1, scol);
      if constexpr (kDrop)
        if (threadIdx.x < 64)
          part_buf(kpart, cur ^ 1)[threadIdx.x] =
              drop_k_part(seed_hi, bh, (t + 1) * 64 + threadIdx.x);
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kbase = t * 64 + half * 32;
      if (kCausal) {
        if (kbase > qb + 31) break;  // wave-uniform causal cut
      }
      if (kRagged) {
        // wave-uniform: a half-tile or a wave that is all padding
        if (kbase >= S || qb >= S) break;
      }
      const char* ki = img<kHD>(kimg, cur) + half * kHalfImg;
      const char* vi = img<kHD>(vimg, cur) + half * kHalfImg;

      // S^T tile: C[k][q] = sum_d K[k][d] * Q[q][d]
      f32x16 s = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < kNC; ++c)
        s = mfma(read_row_chunk<kHD>(ki, lane, c), qf[c], s);
      __builtin_amdgcn_s_setprio(0);

      float pv[16];
      float tmax = kNegBig;
      if ((kCausal && kbase + 31 > qb) || (kRagged && kbase + 31 >= S)) {
        // diagonal tile for this wave: apply the causal mask; ragged: the
        // tile that holds key S-1, mask the keys past it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kglob = kbase + crow(r, hi);
          pv[r] = key_masked<kCausal, kRagged>(kglob, qrow, qlim, S)
                      ? kNegBig
                      : s[r];
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
          if constexpr (kNB == 4) {
            acc2[r] *= alpha;
            acc3[r] *= alpha;
          }
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

      // dropout after the row sum: the normaliser and lse stay those of
      // the undropped scores; 1/(1-p) goes into the epilogue's inv
      if constexpr (kDrop) {
        const unsigned* kp = part_buf(kpart, cur) + half * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!drop_keep_parts(dqa, kp[crow(r, hi)], p.drop_thr))
            pv[r] = 0.f;
      }

      // redistribute P to operand fragments (k blocks 0-15 / 16-31)
      const bf16x8 p0 = pack_frag(&pv[0]);
      const bf16x8 p1 = pack_frag(&pv[8]);

      // O^T += V^T · P^T  (A = V^T via hardware transpose reads)
      __builtin_amdgcn_s_setprio(1);
      acc0 = mfma(read_tr_blk<kHD>(vi, lane, 0, 0), p0, acc0);
      acc0 = mfma(read_tr_blk<kHD>(vi, lane, 1, 0), p1, acc0);
      acc1 = mfma(read_tr_blk<kHD>(vi, lane, 0, 1), p0, acc1);
      acc1 = mfma(read_tr_blk<kHD>(vi, lane, 1, 1), p1, acc1);
      if constexpr (kNB == 4) {
        acc2 = mfma(read_tr_blk<kHD>(vi, lane, 0, 2), p0, acc2);
        acc2 = mfma(read_tr_blk<kHD>(vi, lane, 1, 2), p1, acc2);
        acc3 = mfma(read_tr_blk<kHD>(vi, lane, 0, 3), p0, acc3);
        acc3 = mfma(read_tr_blk<kHD>(vi, lane, 1, 3), p1, acc3);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_tile<kHD>(img<kHD>(kimg, cur ^ 1), srow, scol, nk);
      st_tile<kHD>(img<kHD>(vimg, cur ^ 1), srow, scol, nv);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: combine row-sum halves, normalize, store O and lse
  const float stot = ssum + __shfl_xor(ssum, 32, 64);
  float inv = 1.f / stot;
  if constexpr (kDrop) inv = p.drop_rp / stot;
  if (kRagged && qrow >= S) return;  // stores only; no barrier follows
  if ((lane >> 5) == 0)
    lseg[qrow] = p.scale * m + __builtin_amdgcn_logf(stot) * kLn2;

  __bf16* orow = og + (long)qrow * p.os.ss;
#pragma unroll
  for (int db = 0; db < kNB; ++db) {
    const f32x16& a = db == 3 ? acc3 : db == 2 ? acc2 : db ? acc1 : acc0;
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

template <int kHD, bool kCausal, bool kRagged, bool kDrop,
          bool kVarlen = false, bool kGqa = false>
__global__ __launch_bounds__(256, kHD == 64 ? 3 : 2) void fa_bwd_dq_kernel(
    FaParams p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  static_assert(kVarlen ? kRagged : !(kCausal && kRagged),
                "fixed-length causal needs S % 128 == 0; varlen is ragged");
  constexpr int kNC = kHD / 16;  // 16-column chunks of a row
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  // 64-row KV tiles, double-buffered: K images, then V images (then the
  // tiles' dropout k parts).
  __shared__ __attribute__((aligned(16))) char
      smem[4 * kTileImg<kHD> + kPartBytes<kDrop>];
  char* const kimg = smem;
  char* const vimg = smem + 2 * kTileImg<kHD>;
  [[maybe_unused]] unsigned* const kpart =
      reinterpret_cast<unsigned*>(smem + 4 * kTileImg<kHD>);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  int qt = blockIdx.x, bh = blockIdx.y, b, h, S = p.S;  // as in the forward
  long row0 = 0;
  if constexpr (kVarlen) {
    const VarlenTile vt = varlen_tile(p);
    if (varlen_idle(vt)) return;
    qt = vt.tile;
    b = 0;
    h = blockIdx.y;
    bh = vt.seq * p.H + h;
    S = vt.len;
    row0 = vt.start;
  } else {
    b = bh / p.H;
    h = bh % p.H;
  }

  const __bf16* qg = seq_plane<kVarlen>(p.q, p.qs, b, h, row0);
  const int hk = kv_head<kGqa>(h, p.G);
  const __bf16* kg = seq_plane<kVarlen>(p.k, p.ks, b, hk, row0);
  const __bf16* vg = seq_plane<kVarlen>(p.v, p.vs, b, hk, row0);
  const __bf16* dog = seq_plane<kVarlen>(p.dout, p.dos_, b, h, row0);
  const __bf16* og = seq_plane<kVarlen>(p.o, p.os, b, h, row0);
  __bf16* dqg = seq_plane<kVarlen>(p.dq, p.dqs, b, h, row0);
  // first element of this plane's (varlen: this sequence's) lse and delta
  const long lrow0 = kVarlen ? (long)h * p.total + row0 : (long)bh * S;

  const int qb = qt * kQT + wave * 32;
  const int qrow = qb + (lane & 31);
  const long qld = ld_row32<kRagged>(qrow, S);
  [[maybe_unused]] const int qlim = min(qrow, S - 1);  // see the forward

  // this lane holds half of its q row's kHD dO (and O) elements as kHD/16
  // runs of 8 (columns c*16 + hi*8 ..); lane^32 holds the runs in between.
  // n16[c] joins each run with its neighbour from the partner lane, so both
  // lanes walk the same adjacent-pair tree over the whole row.
  bf16x8 qf[kNC], dof[kNC];
  float n16[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    dof[c] = *reinterpret_cast<const bf16x8*>(
        dog + qld * p.dos_.ss + c * 16 + hi * 8);
    const float n8 = dot8_tree(
        dof[c], *reinterpret_cast<const bf16x8*>(
                    og + qld * p.os.ss + c * 16 + hi * 8));
    n16[c] = n8 + __shfl_xor(n8, 32, 64);
  }
#pragma unroll
  for (int c = 0; c < kNC; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(
        qg + qld * p.qs.ss + c * 16 + hi * 8);
  const float lse2 = p.lse[lrow0 + qld] * kLog2e;
  // the tree's top: 64-column blocks, then (head_dim 128) the two blocks
  float dvq = (n16[0] + n16[1]) + (n16[2] + n16[3]);
  if constexpr (kHD == 128)
    dvq = dvq + ((n16[4] + n16[5]) + (n16[6] + n16[7]));
  if (hi == 0 && (!kRagged || qrow < S))
    p.delta[lrow0 + qrow] = dvq;
  const float c1 = p.scale * kLog2e;

  // dQ^T, one accumulator per 32 columns (dacc2, dacc3: head_dim 128)
  f32x16 dacc0 = {}, dacc1 = {};
  [[maybe_unused]] f32x16 dacc2 = {}, dacc3 = {};

  const int srow = threadIdx.x >> 3;
  const int scol = (threadIdx.x & 7) * 8;
  const int n64 = tile_count<kCausal, kRagged>(qt, S);

  // dropout: this lane's q part; seed_hi feeds the tiles' k parts
  [[maybe_unused]] unsigned dqa = 0, seed_hi = 0;
  if constexpr (kDrop) {
    const unsigned long sd = (unsigned long)*p.seed;
    dqa = drop_q_part((unsigned)sd, bh, qrow);
    seed_hi = (unsigned)(sd >> 32);
  }
  {
    const long r0 = ld_row32<kRagged>(srow, S);
    const long r1 = ld_row32<kRagged>(srow + 32, S);
    st_tile<kHD>(img<kHD>(kimg, 0), srow, scol,
                 ld_tile<kHD>(kg, p.ks.ss, r0, r1, scol));
    st_tile<kHD>(img<kHD>(vimg, 0), srow, scol,
                 ld_tile<kHD>(vg, p.vs.ss, r0, r1, scol));
    if constexpr (kDrop)
      if (threadIdx.x < 64)
        kpart[threadIdx.x] = drop_k_part(seed_hi, bh, threadIdx.x);
  }
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < n64; ++t) {
    RowTile<kHD> nk, nv;
    const bool pref = t + 1 < n64;
    if (pref) {
      const long kb0 = ld_row32<kRagged>((t + 1) * 64 + srow, S);
      const long kb1 = ld_row32<kRagged>((t + 1) * 64 + srow + 32, S);
      nk = ld_tile<kHD>(kg, p.ks.ss, kb0, kb1, scol);
      nv = ld_tile<kHD>(vg, p.vs.ss, kb0, kb1, scol);
      if constexpr (kDrop)
        if (threadIdx.x < 64)
          part_buf(kpart, cur ^ 1)[threadIdx.x] =
              drop_k_part(seed_hi, bh, (t + 1) * 64 + threadIdx.x);
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kbase = t * 64 + half * 32;
      if (kCausal) {
        if (kbase > qb + 31) break;
      }
      if (kRagged) {
        if (kbase >= S || qb >= S) break;  // all padding
      }
      const char* ki = img<kHD>(kimg, cur) + half * kHalfImg;
      const char* vi = img<kHD>(vimg, cur) + half * kHalfImg;

      f32x16 s = {}, dp = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < kNC; ++c) {
        s = mfma(read_row_chunk<kHD>(ki, lane, c), qf[c], s);
        dp = mfma(read_row_chunk<kHD>(vi, lane, c), dof[c], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // two loops on purpose: the unmasked one carries no compare
      float ds[16];
      // dropout: the MFMA gave dP of the dropped, rescaled P; the dP that
      // dS wants is keep * that / (1-p)
      [[maybe_unused]] const unsigned* kp =
          part_buf(kpart, cur) + half * 32;
      auto dpk = [&](int r) {
        if constexpr (kDrop)
          return drop_keep_parts(dqa, kp[crow(r, hi)], p.drop_thr)
                     ? dp[r] * p.drop_rp
                     : 0.f;
        else
          return dp[r];
      };
      if (kDrop) {
        // one loop: beside the mask word the compare is cheap, and the
        // second copy of the loop costs registers (scratch at 3 waves/SIMD)
        const int lim = kCausal ? (kRagged ? qlim : qrow)
                        : kRagged ? S - 1
                                  : 0x7fffffff;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kglob = kbase + crow(r, hi);
          const float pe = kglob > lim ? 0.f : p_elem(s[r], c1, lse2);
          ds[r] = ds_elem(pe, dpk(r), dvq, p.scale);
        }
      } else if ((kCausal && kbase + 31 > qb) ||
                 (kRagged && kbase + 31 >= S)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kglob = kbase + crow(r, hi);
          const float pe = key_masked<kCausal, kRagged>(kglob, qrow, qlim, S)
                               ? 0.f
                               : p_elem(s[r], c1, lse2);
          ds[r] = ds_elem(pe, dpk(r), dvq, p.scale);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ds[r] = ds_elem(p_elem(s[r], c1, lse2), dpk(r), dvq, p.scale);
      }
      const bf16x8 d0 = pack_frag(&ds[0]);
      const bf16x8 d1 = pack_frag(&ds[8]);
      __builtin_amdgcn_s_setprio(1);
      dacc0 = mfma(read_tr_blk<kHD>(ki, lane, 0, 0), d0, dacc0);
      dacc0 = mfma(read_tr_blk<kHD>(ki, lane, 1, 0), d1, dacc0);
      dacc1 = mfma(read_tr_blk<kHD>(ki, lane, 0, 1), d0, dacc1);
      dacc1 = mfma(read_tr_blk<kHD>(ki, lane, 1, 1), d1, dacc1);
      if constexpr (kNB == 4) {
        dacc2 = mfma(read_tr_blk<kHD>(ki, lane, 0, 2), d0, dacc2);
        dacc2 = mfma(read_tr_blk<kHD>(ki, lane, 1, 2), d1, dacc2);
        dacc3 = mfma(read_tr_blk<kHD>(ki, lane, 0, 3), d0, dacc3);
        dacc3 = mfma(read_tr_blk<kHD>(ki, lane, 1, 3), d1, dacc3);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_tile<kHD>(img<kHD>(kimg, cur ^ 1), srow, scol, nk);
      st_tile<kHD>(img<kHD>(vimg, cur ^ 1), srow, scol, nv);
    }
    __syncthreads();
    cur ^= 1;
  }

  if (kRagged && qrow >= S) return;  // stores only; no barrier follows
  __bf16* drow = dqg + (long)qrow * p.dqs.ss;
#pragma unroll
  for (int db = 0; db < kNB; ++db) {
    const f32x16& a = db == 3 ? dacc3 : db == 2 ? dacc2 : db ? dacc1 : dacc0;
#pragma unroll
    for (int mq = 0; mq < 4; ++mq)
      store4_bf16(drow + db * 32 + 8 * mq + 4 * hi, a[4 * mq], a[4 * mq + 1],
                  a[4 * mq + 2], a[4 * mq + 3]);
  }
}

// ---------------------------------------------------------------------------
// Backward dK/dV. Grid (ceil(S/128), B*H), kGqa: B*Hk; wave owns kv rows
// kt*128+w*32..+31, loops q tiles >= the diagonal (causal) or all q tiles
// (kGqa: of each of the group's G query heads in turn):
//   S = Q·K^T   as C[q][k]: A=Q row frags (LDS), B=K direct (registers)
//   P^T[k][q] = exp2(S*c1 - lse[q]*log2e) masked            lane-k local
//   dP[q][k]: A=dO row frags, B=V^T direct (registers)
//   dV += P^T·dO   (A=packed P^T, B=dO^T tr frags)
//   dS^T = P^T*(dP-D[q])*scale;  dK += dS^T·Q (A=packed dS^T, B=Q^T tr)
// ---------------------------------------------------------------------------
template <int kHD, bool kCausal, bool kRagged, bool kDrop,
          bool kVarlen = false, bool kGqa = false>
__global__ __launch_bounds__(256, kHD == 64 ? 2 : 1) void fa_bwd_dkv_kernel(
    FaParams p) {
  static_assert(kHD == 64 || kHD == 128, "head_dim 64 or 128");
  static_assert(kVarlen ? kRagged : !(kCausal && kRagged),
                "fixed-length causal needs S % 128 == 0; varlen is ragged");
  constexpr int kNC = kHD / 16;  // 16-column chunks of a row
  constexpr int kNB = kHD / 32;  // 32-column blocks: one accumulator each
  // 64-row q tiles, double-buffered: Q images, then dO images, then the
  // lse2/delta side tile (then the tiles' dropout q parts); the epilogue
  // reuses the images as per-wave f32 scratch for the coalesced dV/dK stores.
  __shared__ __attribute__((aligned(16))) char
      smem[4 * kTileImg<kHD> + 1024 + kPartBytes<kDrop>];
  char* const qimg = smem;
  char* const doimg = smem + 2 * kTileImg<kHD>;
  float* const side =
      reinterpret_cast<float*>(smem + 4 * kTileImg<kHD>);
  [[maybe_unused]] unsigned* const qpart =
      reinterpret_cast<unsigned*>(smem + 4 * kTileImg<kHD> + 1024);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  int kt = blockIdx.x, bh = blockIdx.y, b, h, S = p.S;  // as in the forward
  // grouped-query mode: y counts K/V heads, hk is this workgroup's, and h,
  // bh start at the first of its G query heads, hk*G .. hk*G + G-1
  int hk;
  long row0 = 0;
  if constexpr (kVarlen) {
    const VarlenTile vt = varlen_tile(p);
    if (varlen_idle(vt)) return;
    kt = vt.tile;
    b = 0;
    hk = blockIdx.y;
    h = kGqa ? hk * p.G : hk;
    bh = vt.seq * p.H + h;
    S = vt.len;
    row0 = vt.start;
  } else if constexpr (kGqa) {
    const int Hk = p.H / p.G;
    b = bh / Hk;
    hk = bh % Hk;
    h = hk * p.G;
    bh = b * p.H + h;
  } else {
    b = bh / p.H;
    h = bh % p.H;
    hk = h;
  }

  // kGqa: qg, dog, lseg, deltag (and bh) are those of the head the staging
  // is at; they move on to the group's next query head when the prefetch
  // does (below)
  const __bf16* qg = seq_plane<kVarlen>(p.q, p.qs, b, h, row0);
  const __bf16* kg = seq_plane<kVarlen>(p.k, p.ks, b, hk, row0);
  const __bf16* vg = seq_plane<kVarlen>(p.v, p.vs, b, hk, row0);
  const __bf16* dog = seq_plane<kVarlen>(p.dout, p.dos_, b, h, row0);
  __bf16* dkg = seq_plane<kVarlen>(p.dk, p.dks, b, hk, row0);
  __bf16* dvg = seq_plane<kVarlen>(p.dv, p.dvs, b, hk, row0);
  const long lrow0 = kVarlen ? (long)h * p.total + row0 : (long)bh * S;
  const float* lseg = p.lse + lrow0;
  const float* deltag = p.delta + lrow0;

  const int kbb = kt * kQT + wave * 32;     // this wave's first k row
  const int krow = kbb + (lane & 31);       // this lane's k row
  const long kld = ld_row32<kRagged>(krow, S);

  // K and V^T B-fragments direct from global: lane holds
  // K[krow][chunk*16+8*hi+e] / V[krow][...]
  bf16x8 kf[kNC], vf[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    kf[c] = *reinterpret_cast<const bf16x8*>(
        kg + kld * p.ks.ss + c * 16 + hi * 8);
    vf[c] = *reinterpret_cast<const bf16x8*>(
        vg + kld * p.vs.ss + c * 16 + hi * 8);
  }

  const float c1 = p.scale * kLog2e;
  // dV and dK, one accumulator per 32 columns (2, 3: head_dim 128)
  f32x16 dvacc0 = {}, dvacc1 = {}, dkacc0 = {}, dkacc1 = {};
  [[maybe_unused]] f32x16 dvacc2 = {}, dvacc3 = {}, dkacc2 = {}, dkacc3 = {};

  const int srow = threadIdx.x >> 3;
  const int scol = (threadIdx.x & 7) * 8;
  // first 64-row q tile: the diagonal's. The workgroup's keys start at row
  // kt * kQT, and the causal cut below skips every earlier tile whole.
  const int t0 = kCausal ? kt * (kQT / 64) : 0;
  const int n64 = (S + 63) / 64;

  // dropout: this lane's k part; seed_lo feeds the tiles' q parts
  [[maybe_unused]] unsigned dkb = 0, seed_lo = 0;
  // kGqa: the k part belongs to the plane, so each head of the group gets
  // its own when the tile loop reaches it; bhc is the plane the loop is at
  [[maybe_unused]] unsigned seed_hi = 0;
  [[maybe_unused]] int bhc = bh;
  if constexpr (kDrop) {
    const unsigned long sd = (unsigned long)*p.seed;
    seed_lo = (unsigned)sd;
    dkb = drop_k_part((unsigned)(sd >> 32), bh, krow);
    if constexpr (kGqa) seed_hi = (unsigned)(sd >> 32);
  }
  // kGqa: heads of the group still to be staged / still to be walked after
  // the current one. The tile loop below is the flattened (head, tile)
  // iteration: the last tile of a head prefetches tile t0 of the next, so
  // the double buffer never drains inside a workgroup.
  [[maybe_unused]] int stage_left = 0, walk_left = 0;
  if constexpr (kGqa) stage_left = walk_left = p.G - 1;

  // stage q/dO tile t0 and its side tile
  {
    const int qb0 = t0 * 64;
    const long r0 = ld_row32<kRagged>(qb0 + srow, S);
    const long r1 = ld_row32<kRagged>(qb0 + srow + 32, S);
    st_tile<kHD>(img<kHD>(qimg, 0), srow, scol,
                 ld_tile<kHD>(qg, p.qs.ss, r0, r1, scol));
    st_tile<kHD>(img<kHD>(doimg, 0), srow, scol,
                 ld_tile<kHD>(dog, p.dos_.ss, r0, r1, scol));
    if (threadIdx.x < 64) {
      const int rq = ld_row32<kRagged>(qb0 + (int)threadIdx.x, S);
      st_side(side, 0, threadIdx.x, ld_side(lseg, deltag, rq));
      if constexpr (kDrop)
        qpart[threadIdx.x] = drop_q_part(seed_lo, bh, qb0 + threadIdx.x);
    }
  }
  __syncthreads();

  int cur = 0;
  for (int t = t0; t < n64; ++t) {
    RowTile<kHD> nq, nd;
    SideVal ns = {0.f, 0.f};
    bool pref = t + 1 < n64;
    int tn = t + 1;  // the tile to prefetch
    if constexpr (kGqa) {
      if (!pref && stage_left > 0) {
        // last tile of a head: go on to tile t0 of the group's next head,
        // one plane on in q, dO, lse, delta and the mask (wave-uniform)
        --stage_left;
        pref = true;
        tn = t0;
        qg += p.qs.sh;
        dog += p.dos_.sh;
        lseg += kVarlen ? p.total : S;
        deltag += kVarlen ? p.total : S;
        ++bh;
      }
    }
    if (pref) {
      const int qb1 = tn * 64;
      const long r0 = ld_row32<kRagged>(qb1 + srow, S);
      const long r1 = ld_row32<kRagged>(qb1 + srow + 32, S);
      nq = ld_tile<kHD>(qg, p.qs.ss, r0, r1, scol);
      nd = ld_tile<kHD>(dog, p.dos_.ss, r0, r1, scol);
      if (threadIdx.x < 64) {
        const int rq = ld_row32<kRagged>(qb1 + (int)threadIdx.x, S);
        ns = ld_side(lseg, deltag, rq);
        if constexpr (kDrop)
          part_buf(qpart, cur ^ 1)[threadIdx.x] =
              drop_q_part(seed_lo, bh, qb1 + threadIdx.x);
      }
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int qbase = t * 64 + half * 32;
      if (kCausal) {
        if (qbase + 31 < kbb) continue;     // wave-uniform causal cut
      }
      if (kRagged) {
        // wave-uniform: a q half-tile or a k-row wave that is all padding
        if (qbase >= S || kbb >= S) break;
      }
      const char* qi = img<kHD>(qimg, cur) + half * kHalfImg;
      const char* di = img<kHD>(doimg, cur) + half * kHalfImg;
      const float* lsec = side_buf(side, cur) + half * 32;
      const float* dc = lsec + kSideDelta;

      f32x16 sacc = {}, dp = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < kNC; ++c) {
        sacc = mfma(read_row_chunk<kHD>(qi, lane, c), kf[c], sacc);
        dp = mfma(read_row_chunk<kHD>(di, lane, c), vf[c], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // two loops on purpose: the unmasked one carries no compare
      float pv[16], ds[16];
      // dropout: dS takes the undropped P and keep * dP / (1-p)
      [[maybe_unused]] bool keep[16];
      if constexpr (kDrop) {
        const unsigned* qp = part_buf(qpart, cur) + half * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          keep[r] = drop_keep_parts(qp[crow(r, hi)], dkb, p.drop_thr);
          dp[r] = keep[r] ? dp[r] * p.drop_rp : 0.f;
        }
      }
      if ((kCausal && qbase < kbb + 31) || (kRagged && qbase + 31 >= S)) {
        // diagonal: mask q < k; ragged: mask the q rows past S-1, which
        // then add exact zeros to dK and dV (their P and dS are 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qglob = qbase + crow(r, hi);
          pv[r] = ((kCausal && qglob < krow) || (kRagged && qglob >= S))
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
      // dV takes the dropped P; its 1/(1-p) goes onto the accumulator in
      // the epilogue
      if constexpr (kDrop) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!keep[r]) pv[r] = 0.f;
      }
      const bf16x8 p0 = pack_frag(&pv[0]);
      const bf16x8 p1 = pack_frag(&pv[8]);
      __builtin_amdgcn_s_setprio(1);
      dvacc0 = mfma(p0, read_tr_blk<kHD>(di, lane, 0, 0), dvacc0);
      dvacc0 = mfma(p1, read_tr_blk<kHD>(di, lane, 1, 0), dvacc0);
      dvacc1 = mfma(p0, read_tr_blk<kHD>(di, lane, 0, 1), dvacc1);
      dvacc1 = mfma(p1, read_tr_blk<kHD>(di, lane, 1, 1), dvacc1);
      if constexpr (kNB == 4) {
        dvacc2 = mfma(p0, read_tr_blk<kHD>(di, lane, 0, 2), dvacc2);
        dvacc2 = mfma(p1, read_tr_blk<kHD>(di, lane, 1, 2), dvacc2);
        dvacc3 = mfma(p0, read_tr_blk<kHD>(di, lane, 0, 3), dvacc3);
        dvacc3 = mfma(p1, read_tr_blk<kHD>(di, lane, 1, 3), dvacc3);
      }
      __builtin_amdgcn_s_setprio(0);
      const bf16x8 e0 = pack_frag(&ds[0]);
      const bf16x8 e1 = pack_frag(&ds[8]);
      __builtin_amdgcn_s_setprio(1);
      dkacc0 = mfma(e0, read_tr_blk<kHD>(qi, lane, 0, 0), dkacc0);
      dkacc0 = mfma(e1, read_tr_blk<kHD>(qi, lane, 1, 0), dkacc0);
      dkacc1 = mfma(e0, read_tr_blk<kHD>(qi, lane, 0, 1), dkacc1);
      dkacc1 = mfma(e1, read_tr_blk<kHD>(qi, lane, 1, 1), dkacc1);
      if constexpr (kNB == 4) {
        dkacc2 = mfma(e0, read_tr_blk<kHD>(qi, lane, 0, 2), dkacc2);
        dkacc2 = mfma(e1, read_tr_blk<kHD>(qi, lane, 1, 2), dkacc2);
        dkacc3 = mfma(e0, read_tr_blk<kHD>(qi, lane, 0, 3), dkacc3);
        dkacc3 = mfma(e1, read_tr_blk<kHD>(qi, lane, 1, 3), dkacc3);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (pref) {
      st_tile<kHD>(img<kHD>(qimg, cur ^ 1), srow, scol, nq);
      st_tile<kHD>(img<kHD>(doimg, cur ^ 1), srow, scol, nd);
      if (threadIdx.x < 64) st_side(side, cur ^ 1, threadIdx.x, ns);
    }
    __syncthreads();
    cur ^= 1;
    if constexpr (kGqa) {
      if (t + 1 == n64 && walk_left > 0) {
        // the next head's tile t0 is staged: walk it with that plane's
        // k part; dvacc*/dkacc* carry on, which forms the group sum
        --walk_left;
        t = t0 - 1;
        if constexpr (kDrop) dkb = drop_k_part(seed_hi, ++bhc, krow);
      }
    }
  }

  // epilogue: C[k-rows][d=lane&31] per accumulator -> round-trip through
  // this wave's [32][kHD] f32 LDS scratch (8 KB, 16 KB at head_dim 128) for
  // coalesced row-major stores.
  __syncthreads();
  float* scratch = reinterpret_cast<float*>(smem) + wave * (32 * kHD);
#pragma unroll
  for (int t = 0; t < 2; ++t) {  // 0: dV, 1: dK
    const f32x16& a0 = t ? dkacc0 : dvacc0;
    const f32x16& a1 = t ? dkacc1 : dvacc1;
    [[maybe_unused]] const f32x16& a2 = t ? dkacc2 : dvacc2;
    [[maybe_unused]] const f32x16& a3 = t ? dkacc3 : dvacc3;
    if (kDrop && t == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        scratch[crow(r, hi) * kHD + (lane & 31)] = a0[r] * p.drop_rp;
        scratch[crow(r, hi) * kHD + 32 + (lane & 31)] = a1[r] * p.drop_rp;
        if constexpr (kNB == 4) {
          scratch[crow(r, hi) * kHD + 64 + (lane & 31)] = a2[r] * p.drop_rp;
          scratch[crow(r, hi) * kHD + 96 + (lane & 31)] = a3[r] * p.drop_rp;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        scratch[crow(r, hi) * kHD + (lane & 31)] = a0[r];
        scratch[crow(r, hi) * kHD + 32 + (lane & 31)] = a1[r];
        if constexpr (kNB == 4) {
          scratch[crow(r, hi) * kHD + 64 + (lane & 31)] = a2[r];
          scratch[crow(r, hi) * kHD + 96 + (lane & 31)] = a3[r];
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0);  // drain LDS writes (wave-local reuse)
    __bf16* outg = (t ? dkg : dvg);
    const TStride& os = t ? p.dks : p.dvs;
    const int row = lane >> 1;           // 2 lanes per k row
    const int dhalf = (lane & 1) * (kHD / 2);
#pragma unroll
    for (int mq = 0; mq < kHD / 8; ++mq) {
      const float* src = scratch + row * kHD + dhalf + mq * 4;
      if (!kRagged || kbb + row < S)
        store4_bf16(outg + (long)(kbb + row) * os.ss + dhalf + mq * 4, src[0],
                    src[1], src[2], src[3]);
    }
    __syncthreads();  // scratch reused for dK after dV drains
  }
}

// ---------------------------------------------------------------------------
// The dropout mask itself, keep(seed, bh, q, k) as [B*H][S][S] bytes: the
// bridge between the three kernels above and the torch replica.
// Grid (ceil(S*S/256), B*H).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fa_dropout_mask_kernel(
    uint8_t* out, const long* seed, int S, unsigned thr) {
  const long n = (long)S * S;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned bh = blockIdx.y;
  out[bh * n + i] =
      drop_keep(*seed, bh, (unsigned)(i / S), (unsigned)(i % S), thr);
}

// ---------------------------------------------------------------------------
// The variable-length plan: cu_seqlens (n_seqs + 1 row offsets) -> the tile
// map of FaParams::tmap, on the device, so a launch never waits for the
// host to read the offsets. One workgroup.
//
// Sequence i is rows [e_i, e_{i+1}) with e_i = clamp(max(cu[0..i]), 0,
// total). For a well-formed vector (non-decreasing, cu[0] = 0, cu[n] =
// total) that is cu itself. For any other it is still a non-decreasing
// chain inside [0, total]: the sequences are disjoint, in range, and their
// lengths sum to at most total, so they have at most total/128 + n_seqs
// tiles, the size of the map and of the launches that index it. A sequence
// that comes out empty gets no tile. Entries past the last tile are -1.
//
// Thread t owns a run of consecutive sequences; two block scans carry the
// running maximum and the tile count across the runs.
// ---------------------------------------------------------------------------
constexpr int kIntMin = -2147483647 - 1;

// Exclusive scan of x over the block's 256 threads, max or sum; *all gets
// the reduction over all of them.
template <bool kMax>
__device__ __forceinline__ int plan_scan(int* buf, int x, int* all) {
  const int t = threadIdx.x;
  constexpr int kId = kMax ? kIntMin : 0;
  buf[t] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int y = t >= d ? buf[t - d] : kId;
    __syncthreads();
    buf[t] = kMax ? max(buf[t], y) : buf[t] + y;
    __syncthreads();
  }
  const int excl = t ? buf[t - 1] : kId;
  *all = buf[255];
  __syncthreads();
  return excl;
}

__device__ __forceinline__ int clamp_row(int x, int total) {
  return min(max(x, 0), total);
}

__global__ __launch_bounds__(256) void fa_varlen_plan_kernel(
    const int* cu, int n_seqs, int total, int max_tiles, int4* tmap) {
  __shared__ int buf[256];
  const int t = threadIdx.x;
  const int per = (n_seqs + 255) / 256;
  const int i0 = min(t * per, n_seqs), i1 = min(i0 + per, n_seqs);

  // running maximum in front of this thread's first sequence
  int mx = kIntMin;
  for (int i = i0; i < i1; ++i) mx = max(mx, cu[i + 1]);
  int unused;
  const int m0 = max(cu[0], plan_scan<true>(buf, mx, &unused));

  int tiles = 0;
  for (int i = i0, m = m0; i < i1; ++i) {
    const int e = clamp_row(m, total);
    m = max(m, cu[i + 1]);
    tiles += (clamp_row(m, total) - e + kQT - 1) / kQT;
  }
  int n_tiles;
  int at = plan_scan<false>(buf, tiles, &n_tiles);

  for (int i = i0, m = m0; i < i1; ++i) {
    const int e = clamp_row(m, total);
    m = max(m, cu[i + 1]);
    const int len = clamp_row(m, total) - e;
    for (int j = 0; j * kQT < len; ++j, ++at)
      if (at < max_tiles) tmap[at] = make_int4(i, j, e, len);
  }
  for (int x = n_tiles + t; x < max_tiles; x += 256)
    tmap[x] = make_int4(-1, -1, -1, -1);
}

// ---------------------------------------------------------------------------
// Host side.
// ---------------------------------------------------------------------------
TStride stride_at(const long* s, int i) {
  return {s[3 * i], s[3 * i + 1], s[3 * i + 2]};
}

// thr = clamp(round(p * 2^32), 1, 2^32 - 1), ties to even like Python's
// round(): the replica computes the same number.
unsigned drop_threshold(double p) {
  const double t = std::nearbyint(p * 4294967296.0);
  return (unsigned)std::min(std::max(t, 1.0), 4294967295.0);
}

void check_drop(const char* name, double p, const long* seed) {
  if (!(p >= 0.0 && p < 1.0))
    throw std::runtime_error(std::string(name) + ": need 0 <= dropout_p < 1");
  if (p > 0.0 && seed == nullptr)
    throw std::runtime_error(std::string(name) +
                             ": dropout needs a device seed");
}

void set_drop(FaParams& p, double dropout_p, const long* seed) {
  p.seed = seed;
  p.drop_thr = drop_threshold(dropout_p);
  p.drop_rp = (float)(1.0 / (1.0 - dropout_p));
}

void check_len(const char* name, int S, bool causal) {
  if (S < 1) throw std::runtime_error(std::string(name) + ": S < 1");
  if (causal && S % kQT != 0)
    throw std::runtime_error(std::string(name) +
                             ": causal needs S % 128 == 0");
}

void check_varlen(const char* name, int total, int n_seqs, int H) {
  if (total < 1) throw std::runtime_error(std::string(name) + ": total < 1");
  if (n_seqs < 1)
    throw std::runtime_error(std::string(name) + ": n_seqs < 1");
  if (H < 1) throw std::runtime_error(std::string(name) + ": H < 1");
  if ((long)total / kQT + n_seqs > 0x7fffffffL - kQT || total > 0x7fffff00)
    throw std::runtime_error(std::string(name) + ": too many tiles");
}

// Entries of the tile map, and workgroups in x of a variable-length launch.
int varlen_max_tiles(int total, int n_seqs) { return total / kQT + n_seqs; }

// Checks the lengths of a launch in either mode and returns the grid of the
// q-tile kernels, query heads in y. With a tile map S is `total` and there is
// one batch.
dim3 q_grid(const char* name, int B, int H, int S, bool causal,
            const int* tmap, int n_seqs) {
  if (tmap == nullptr) {
    check_len(name, S, causal);
    return dim3((S + kQT - 1) / kQT, B * H);
  }
  if (B != 1)
    throw std::runtime_error(std::string(name) +
                             ": a tile map needs B == 1, got " +
                             std::to_string(B));
  check_varlen(name, S, n_seqs, H);
  return dim3(varlen_max_tiles(S, n_seqs), H);
}

// Calls f(kCausal, kRagged, kDrop, kVarlen) with the mode as four
// std::bool_constant values. The variable-length mode is always ragged, and
// S means nothing to it.
template <typename F>
void with_mode(bool causal, int S, bool drop, bool varlen, F&& f) {
  auto g = [&](auto d) {
    if (varlen) {
      if (causal)
        f(std::true_type{}, std::true_type{}, d, std::true_type{});
      else
        f(std::false_type{}, std::true_type{}, d, std::true_type{});
    } else if (causal) {
      f(std::true_type{}, std::false_type{}, d, std::false_type{});
    } else if (S % kQT == 0) {
      f(std::false_type{}, std::false_type{}, d, std::false_type{});
    } else {
      f(std::false_type{}, std::true_type{}, d, std::false_type{});
    }
  };
  if (drop)
    g(std::true_type{});
  else
    g(std::false_type{});
}

// The part of the parameter block that both directions fill. strides: 3 per
// tensor, q, k, v, o first.
FaParams fwd_params(const char* name, const void* q, const void* k,
                    const void* v, void* o, float* lse, int H, int n_kv_head,
                    int S, const long* strides, float scale) {
  const int Hk = n_kv_head == 0 ? H : n_kv_head;
  if (H < 1 || Hk < 1 || H % Hk != 0)
    throw std::runtime_error(std::string(name) + ": need n_kv_head >= 1 that "
                             "divides H, got H " + std::to_string(H) +
                             ", n_kv_head " + std::to_string(n_kv_head));
  FaParams p = {};
  p.G = H / Hk;
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

// The backward's part. strides 4..7: dO, dq, dk, dv.
void bwd_params(FaParams& p, const void* do_, float* delta, void* dq,
                void* dk, void* dv, const long* strides) {
  p.dout = (const __bf16*)do_;
  p.delta = delta;
  p.dq = (__bf16*)dq;
  p.dk = (__bf16*)dk;
  p.dv = (__bf16*)dv;
  p.dos_ = stride_at(strides, 4);
  p.dqs = stride_at(strides, 5);
  p.dks = stride_at(strides, 6);
  p.dvs = stride_at(strides, 7);
}

// With a tile map the launch is variable-length: the kernels take every
// length from the map, so S moves to total and p.S is 0.
void set_varlen(FaParams& p, const int* tmap) {
  if (tmap == nullptr) return;
  p.tmap = reinterpret_cast<const int4*>(tmap);
  p.total = p.S;
  p.S = 0;
}

// Calls f(kHD) with the head dimension as a std::integral_constant.
template <typename F>
void with_head_dim(const char* name, int head_dim, F&& f) {
  if (head_dim == 64)
    f(std::integral_constant<int, 64>{});
  else if (head_dim == 128)
    f(std::integral_constant<int, 128>{});
  else
    throw std::runtime_error(std::string(name) +
                             ": head_dim must be 64 or 128, got " +
                             std::to_string(head_dim));
}

// Calls f(kGqa): G == 1 runs the instantiations without the flag, which are
// the kernels from before it.
template <typename F>
void with_gqa(int G, F&& f) {
  if (G > 1)
    f(std::true_type{});
  else
    f(std::false_type{});
}

void launch_fwd(const FaParams& p, dim3 grid, int head_dim, bool causal,
                bool drop, bool varlen, hipStream_t stream) {
  with_head_dim("fa_forward", head_dim, [&](auto hd) {
    with_mode(causal, p.S, drop, varlen, [&](auto c, auto r, auto d, auto vl) {
      with_gqa(p.G, [&](auto gq) {
        constexpr int kHD = decltype(hd)::value;
        constexpr bool kC = decltype(c)::value, kR = decltype(r)::value,
                       kD = decltype(d)::value, kV = decltype(vl)::value,
                       kG = decltype(gq)::value;
        hipLaunchKernelGGL((fa_fwd_kernel<kHD, kC, kR, kD, kV, kG>), grid,
                           dim3(256), 0, stream, p);
      });
    });
  });
}

// grid: that of the dq kernel, heads in y; the dkv kernel's y counts K/V
// heads, each workgroup walking the G query heads of its group.
void launch_bwd(const FaParams& p, dim3 grid, int head_dim, bool causal,
                bool drop, bool varlen, hipStream_t stream) {
  const dim3 kv_grid(grid.x, grid.y / p.G);
  with_head_dim("fa_backward", head_dim, [&](auto hd) {
    with_mode(causal, p.S, drop, varlen, [&](auto c, auto r, auto d, auto vl) {
      with_gqa(p.G, [&](auto gq) {
        constexpr int kHD = decltype(hd)::value;
        constexpr bool kC = decltype(c)::value, kR = decltype(r)::value,
                       kD = decltype(d)::value, kV = decltype(vl)::value,
                       kG = decltype(gq)::value;
        hipLaunchKernelGGL((fa_bwd_dq_kernel<kHD, kC, kR, kD, kV, kG>), grid,
                           dim3(256), 0, stream, p);
        hipLaunchKernelGGL((fa_bwd_dkv_kernel<kHD, kC, kR, kD, kV, kG>),
                           kv_grid, dim3(256), 0, stream, p);
      });
    });
  });
}

}  // namespace

// drop_threshold for the other users of attn_drop.h's mask (lnorm.hip).
unsigned fa_drop_threshold(double p) { return drop_threshold(p); }

// ---------------------------------------------------------------------------
// Host launchers (bound in bindings.hip). head_dim, the width of a q, k, v,
// o row, is 64 or 128; anything else throws. dropout_p == 0 launches the
// kDrop=false instantiations, which are the kernels without dropout, and
// never touches seed; dropout_p > 0 reads the 64-bit seed at `seed` (device
// memory) when the kernel runs. n_kv_head is the number of heads of k, v
// (and dk, dv); 0 means H. It must divide H, and query head h then reads
// K/V head h / (H / n_kv_head).
//
// tmap == nullptr is the fixed-length mode: tensors [B, H, S, head_dim], lse
// and delta fp32 [B, H, S]. With a tile map the same call is the
// variable-length mode: B must be 1 and S is `total`, the rows of the
// [total, H, head_dim] tensors handed over as [1, H, total, head_dim] views
// (batch stride unused), lse and delta fp32 [H, total], and tmap the int32
// [total/128 + n_seqs, 4] map that fa_varlen_plan filled on the same stream.
// Nothing here reads cu_seqlens or the map on the host.
// ---------------------------------------------------------------------------
void fa_forward(const void* q, const void* k, const void* v, void* o,
                float* lse, int B, int H, int S, const long* strides,
                float scale, hipStream_t stream, bool causal,
                double dropout_p, const long* seed, int head_dim,
                int n_kv_head, const int* tmap, int n_seqs) {
  const dim3 grid = q_grid("fa_forward", B, H, S, causal, tmap, n_seqs);
  check_drop("fa_forward", dropout_p, seed);
  FaParams p = fwd_params("fa_forward", q, k, v, o, lse, H, n_kv_head, S,
                          strides, scale);
  set_drop(p, dropout_p, seed);
  set_varlen(p, tmap);
  launch_fwd(p, grid, head_dim, causal, dropout_p > 0.0, tmap != nullptr,
             stream);
}

// strides: q, k, v, o, dO, dq, dk, dv. delta is an f32 workspace of lse's
// shape the dq kernel fills and the dkv kernel consumes; o and lse are only
// read.
void fa_backward(const void* q, const void* k, const void* v, const void* o,
                 const void* do_, const float* lse, float* delta, void* dq,
                 void* dk, void* dv, int B, int H, int S, const long* strides,
                 float scale, hipStream_t stream, bool causal,
                 double dropout_p, const long* seed, int head_dim,
                 int n_kv_head, const int* tmap, int n_seqs) {
  const dim3 grid = q_grid("fa_backward", B, H, S, causal, tmap, n_seqs);
  check_drop("fa_backward", dropout_p, seed);
  FaParams p = fwd_params("fa_backward", q, k, v, const_cast<void*>(o),
                          const_cast<float*>(lse), H, n_kv_head, S, strides,
                          scale);
  set_drop(p, dropout_p, seed);
  set_varlen(p, tmap);
  bwd_params(p, do_, delta, dq, dk, dv, strides);
  launch_bwd(p, grid, head_dim, causal, dropout_p > 0.0, tmap != nullptr,
             stream);
}

// cu_seqlens: int32 [n_seqs + 1] on the device; fills the tile map that the
// variable-length launches after it on this stream read.
void fa_varlen_plan(const int* cu_seqlens, int n_seqs, int total, int* tmap,
                    hipStream_t stream) {
  check_varlen("fa_varlen_plan", total, n_seqs, 1);
  if (cu_seqlens == nullptr || tmap == nullptr)
    throw std::runtime_error("fa_varlen_plan: null pointer");
  hipLaunchKernelGGL(fa_varlen_plan_kernel, dim3(1), dim3(256), 0, stream,
                     cu_seqlens, n_seqs, total,
                     varlen_max_tiles(total, n_seqs),
                     reinterpret_cast<int4*>(tmap));
}

// out: [B,H,S,S] bytes, 1 where the element is kept.
void fa_dropout_mask(uint8_t* out, const long* seed, int B, int H, int S,
                     double dropout_p, hipStream_t stream) {
  if (S < 1 || B < 1 || H < 1)
    throw std::runtime_error("fa_dropout_mask: empty shape");
  if (seed == nullptr)
    throw std::runtime_error("fa_dropout_mask: needs a device seed");
  check_drop("fa_dropout_mask", dropout_p, seed);
  const long n = (long)S * S;
  const dim3 grid((unsigned)((n + 255) / 256), B * H);
  hipLaunchKernelGGL(fa_dropout_mask_kernel, grid, dim3(256), 0, stream, out,
                     seed, S, drop_threshold(dropout_p));
}

}  // namespace adapcc


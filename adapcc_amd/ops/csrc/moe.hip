// Top-1 and top-2 MoE routing, dispatch and combine (CDNA4 / gfx950).
//
// Everything between the gate GEMM and the expert GEMMs, and between the
// experts and the residual add, without a host sync, a one-hot, a memset or
// an atomic that decides an order:
//   moe_route      logits [T,E] -> gate_p, expert, slot, src
//                  three launches: (1) per-token online softmax + first-max
//                  argmax and per-block per-expert counts, (2) one workgroup
//                  scans the counts over blocks, (3) ballot/popcount rank
//                  inside each wave + LDS wave offsets give the stable slot.
//   moe_route_bwd  dlogits = dgate_p * p_max * ((j == expert) - p_j)
//   moe_gather     out[r] = in[map[r]] (* fp32 scale), zeros where map < 0;
//                  serves dispatch fwd/bwd and combine fwd/bwd(dback)
//   moe_rowdot     out[r] = dot(a[r >> a_shift], b[map[r]]) in fp32 (dgate_p)
// Top-2 (GShard priority: every first choice before any second choice):
//   moe_route_topk      the same three launches over the 2T (choice, token)
//                       pairs in choice-major order, plus per-block partial
//                       sums of the softmax probabilities and one workgroup
//                       that folds them into load[E] and the Switch/GShard
//                       balance loss in a fixed order (no float atomics)
//   moe_route_topk_bwd  gate and balance-loss terms of dlogits in one pass
//   moe_gather2         out[r] = sum over two mapped rows (* fp32 scales),
//                       fp32 sum, one rounding: combine fwd, dispatch bwd
// Row kernels move 16 B per lane; rows are d elements with
// d * sizeof(T) % 16 == 0 and 16-B aligned bases. Row offsets are 64-bit.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>

#include "common.h"

namespace adapcc {

namespace {

constexpr int kMaxExperts = 256;
constexpr int kTokBlock = 256;   // tokens per routing workgroup
constexpr int kScanThreads = 1024;
constexpr int kScanGroups = 64;  // most block-chunks the scan splits into

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(__half x) { return __half2float(x); }
__device__ __forceinline__ float to_f(__hip_bfloat16 x) {
  return __bfloat162float(x);
}
template <typename T>
__device__ __forceinline__ T from_f(float x);
template <>
__device__ __forceinline__ float from_f<float>(float x) { return x; }
template <>
__device__ __forceinline__ __half from_f<__half>(float x) {
  return __float2half(x);
}
template <>
__device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float x) {
  return __float2bfloat16(x);
}

template <typename T>
struct alignas(16) Pk {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

// exp(x - m) with x <= m; equal values (also two infinities) give 1.
__device__ __forceinline__ float exp_rel(float x, float m) {
  return x == m ? 1.f : __expf(x - m);
}

// ---------------------------------------------------------------- routing

// One thread per token: online softmax over the E logits, strict '>' so the
// lowest index wins a tie. The block's per-expert histogram only needs
// totals, so LDS integer atomics are order-independent here.
template <typename T>
__global__ __launch_bounds__(kTokBlock) void route_top1_kernel(
    const T* __restrict__ logits, float* __restrict__ gate_p,
    int* __restrict__ expert, int* __restrict__ counts, long ntok, int E) {
  __shared__ int hist[kMaxExperts];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const long t = (long)blockIdx.x * kTokBlock + tid;
  if (t < ntok) {
    const T* x = logits + t * E;
    float m = to_f(x[0]), s = 1.f;
    int arg = 0;
    for (int j = 1; j < E; ++j) {
      const float v = to_f(x[j]);
      if (v > m) {
        s = s * exp_rel(m, v) + 1.f;
        m = v;
        arg = j;
      } else {
        s += exp_rel(v, m);
      }
    }
    gate_p[t] = 1.f / s;
    expert[t] = arg;
    atomicAdd(&hist[arg], 1);
  }
  __syncthreads();
  if (tid < E) counts[(long)blockIdx.x * E + tid] = hist[tid];
}

// Single workgroup: exclusive scan of counts[nb][E] over the block axis into
// offs[nb][E], and totals[E]. Thread (g, j) owns expert j in block-chunk g.
__global__ __launch_bounds__(kScanThreads) void route_scan_kernel(
    const int* __restrict__ counts, int* __restrict__ offs,
    int* __restrict__ totals, int nb, int E, int ep_log2) {
  __shared__ int part[kScanThreads];
  const int tid = threadIdx.x;
  const int ep = 1 << ep_log2;
  const int G = min(kScanGroups, kScanThreads >> ep_log2);
  const int j = tid & (ep - 1);
  const int g = tid >> ep_log2;
  const bool live = g < G && j < E;
  const int chunk = (nb + G - 1) / G;
  const int b0 = min(nb, g * chunk);
  const int b1 = min(nb, b0 + chunk);
  int sum = 0;
  if (live)
    for (int b = b0; b < b1; ++b) sum += counts[(long)b * E + j];
  part[tid] = sum;
  __syncthreads();
  if (!live) return;
  int run = 0;
  for (int g2 = 0; g2 < g; ++g2) run += part[(g2 << ep_log2) + j];
  if (g == G - 1) totals[j] = run + sum;
  for (int b = b0; b < b1; ++b) {
    offs[(long)b * E + j] = run;
    run += counts[(long)b * E + j];
  }
}

// Rank of this lane among the lower lanes of its wave that hold the same
// expert (ballot/popcount, one round per distinct expert in the wave); the
// first lane of each expert leaves the wave's count in wcount[e].
__device__ __forceinline__ int wave_rank(int e, bool active, int lane,
                                         int* __restrict__ wcount) {
  int rank = 0;
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int e0 = __shfl(e, leader, 64);
    const bool mine = active && e == e0;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      rank = __popcll(m & ((1ull << lane) - 1ull));
      if (rank == 0) wcount[e0] = __popcll(m);
    }
    todo &= ~m;
  }
  return rank;
}

// Stable position = tokens of the same expert in earlier blocks (offs) +
// in earlier waves of this block (LDS) + in lower lanes of this wave
// (ballot/popcount). Also writes -1 into every slot no token fills.
__global__ __launch_bounds__(kTokBlock) void route_rank_kernel(
    const int* __restrict__ expert, const int* __restrict__ offs,
    const int* __restrict__ totals, int* __restrict__ slot,
    int* __restrict__ src, long ntok, int E, int cap) {
  __shared__ int wcount[kTokBlock / 64][kMaxExperts];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int w = 0; w < kTokBlock / 64; ++w) wcount[w][tid] = 0;
  __syncthreads();

  const long t = (long)blockIdx.x * kTokBlock + tid;
  const bool active = t < ntok;
  const int e = active ? expert[t] : -1;
  const int rank = wave_rank(e, active, lane, wcount[wave]);
  __syncthreads();
  if (active) {
    int pos = offs[(long)blockIdx.x * E + e] + rank;
    for (int w = 0; w < wave; ++w) pos += wcount[w][e];
    const int s = pos < cap ? e * cap + pos : -1;
    slot[t] = s;
    if (s >= 0) src[s] = (int)t;
  }
  // empty slots: positions [min(total, cap), cap) of every expert
  const long nslot = (long)E * cap;
  for (long i = (long)blockIdx.x * kTokBlock + tid; i < nslot;
       i += (long)gridDim.x * kTokBlock) {
    const int j = (int)(i / cap);
    const int p = (int)(i - (long)j * cap);
    if (p >= totals[j]) src[i] = -1;
  }
}

// dlogits[t, j] = dgate[t] * p_max * ((j == e) - p_j), p recomputed from the
// logits and the saved p_max; dropped tokens get an exact zero row.
template <typename T>
__global__ __launch_bounds__(kTokBlock) void route_bwd_kernel(
    const T* __restrict__ logits, const float* __restrict__ gate_p,
    const int* __restrict__ expert, const int* __restrict__ slot,
    const float* __restrict__ dgate, T* __restrict__ dlogits, long ntok,
    int E) {
  const long t = (long)blockIdx.x * kTokBlock + threadIdx.x;
  if (t >= ntok) return;
  const T* x = logits + t * E;
  T* dx = dlogits + t * E;
  if (slot[t] < 0) {
    for (int j = 0; j < E; ++j) dx[j] = from_f<T>(0.f);
    return;
  }
  const int e = expert[t];
  const float pm = gate_p[t];
  const float c = dgate[t] * pm;
  const float xe = to_f(x[e]);
  for (int j = 0; j < E; ++j) {
    const float pj = exp_rel(to_f(x[j]), xe) * pm;
    dx[j] = from_f<T>(c * ((j == e ? 1.f : 0.f) - pj));
  }
}

// ------------------------------------------------------------ top-k routing

// One thread per token, one pass over its logits: the online softmax of
// route_top1_kernel (same operations in the same order, so 1/s is the same
// bits) plus the runner-up. Strict '>' everywhere: the lowest index wins a
// tie for the first choice and, among the rest, for the second. A demoted
// leader always precedes an equal runner-up, so it takes the second place.
// A second pass turns the logits into probabilities and sums them per expert
// over the block: xor shuffles inside each wave, then the four wave sums in
// wave order. counts is [K][nb][E] (choice-major), psum is [nb][E].
template <typename T, int K>
__global__ __launch_bounds__(kTokBlock) void route_topk_kernel(
    const T* __restrict__ logits, float* __restrict__ gate,
    float* __restrict__ pmax, int* __restrict__ expert,
    int* __restrict__ counts, float* __restrict__ psum, long ntok, int E,
    int normalize) {
  __shared__ int hist[K][kMaxExperts];
  __shared__ float wsum[kTokBlock / 64][kMaxExperts];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int c = 0; c < K; ++c) hist[c][tid] = 0;
  __syncthreads();
  const long t = (long)blockIdx.x * kTokBlock + tid;
  const bool active = t < ntok;
  const T* x = logits + (active ? t : 0) * E;
  float m = 0.f, inv_s = 0.f;
  if (active) {
    m = to_f(x[0]);
    float s = 1.f, m2 = 0.f;
    int arg = 0, arg2 = -1;
    for (int j = 1; j < E; ++j) {
      const float v = to_f(x[j]);
      if (v > m) {
        s = s * exp_rel(m, v) + 1.f;
        m2 = m;
        arg2 = arg;
        m = v;
        arg = j;
      } else {
        s += exp_rel(v, m);
        if (K == 2 && (arg2 < 0 || v > m2)) {
          m2 = v;
          arg2 = j;
        }
      }
    }
    inv_s = 1.f / s;
    pmax[t] = inv_s;
    expert[t * K] = arg;
    atomicAdd(&hist[0][arg], 1);
    if (K == 1) {
      gate[t] = inv_s;
    } else {
      expert[t * K + 1] = arg2;
      atomicAdd(&hist[K - 1][arg2], 1);
      const float r = exp_rel(m2, m);  // exp(x1 - x0) <= 1
      if (normalize) {
        const float g0 = 1.f / (1.f + r);
        gate[t * K] = g0;
        gate[t * K + 1] = r * g0;
      } else {
        gate[t * K] = inv_s;
        gate[t * K + 1] = r * inv_s;
      }
    }
  }
  for (int j = 0; j < E; ++j) {
    float p = active ? exp_rel(to_f(x[j]), m) * inv_s : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
    if (lane == 0) wsum[wave][j] = p;
  }
  __syncthreads();
  if (tid < E) {
    const long nb = gridDim.x;
#pragma unroll
    for (int c = 0; c < K; ++c)
      counts[(c * nb + blockIdx.x) * E + tid] = hist[c][tid];
    float acc = wsum[0][tid];
#pragma unroll
    for (int w = 1; w < kTokBlock / 64; ++w) acc += wsum[w][tid];
    psum[(long)blockIdx.x * E + tid] = acc;
  }
}

// route_rank_kernel over the K*T (choice, token) pairs: block c*nb + b ranks
// choice c of the tokens of block b, and offs (scanned over all K*nb blocks)
// already holds every first choice in front of any second choice. Writes
// slot[T,K], and token and choice per slot, -1 where no pair lands.
__global__ __launch_bounds__(kTokBlock) void route_rank_topk_kernel(
    const int* __restrict__ expert, const int* __restrict__ offs,
    const int* __restrict__ totals, int* __restrict__ slot,
    int* __restrict__ src, int* __restrict__ src_choice, long ntok, int nb,
    int K, int E, int cap) {
  __shared__ int wcount[kTokBlock / 64][kMaxExperts];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int w = 0; w < kTokBlock / 64; ++w) wcount[w][tid] = 0;
  __syncthreads();

  const int c = blockIdx.x / nb;
  const long t = (long)(blockIdx.x - c * nb) * kTokBlock + tid;
  const bool active = t < ntok;
  const int e = active ? expert[t * K + c] : -1;
  const int rank = wave_rank(e, active, lane, wcount[wave]);
  __syncthreads();
  if (active) {
    int pos = offs[(long)blockIdx.x * E + e] + rank;
    for (int w = 0; w < wave; ++w) pos += wcount[w][e];
    const int s = pos < cap ? e * cap + pos : -1;
    slot[t * K + c] = s;
    if (s >= 0) {
      src[s] = (int)t;
      src_choice[s] = c;
    }
  }
  const long nslot = (long)E * cap;
  for (long i = (long)blockIdx.x * kTokBlock + tid; i < nslot;
       i += (long)gridDim.x * kTokBlock) {
    const int j = (int)(i / cap);
    const int p = (int)(i - (long)j * cap);
    if (p >= totals[j]) {
      src[i] = -1;
      src_choice[i] = -1;
    }
  }
}

// Single workgroup: load[e] = first choices of e (first_total) and
// aux = E * sum_e (load[e] / T) * (sum_b psum[b][e] / T). Thread (g, j) adds
// expert j's block sums of quarter g in block order; the quarters, then the
// experts (shuffles, then the four wave sums), fold in a fixed order.
__global__ __launch_bounds__(kScanThreads) void route_aux_kernel(
    const float* __restrict__ psum, const int* __restrict__ first_total,
    int* __restrict__ load, float* __restrict__ aux, int nb, int E,
    long ntok) {
  constexpr int G = kScanThreads / kMaxExperts;
  __shared__ float part[G][kMaxExperts];
  __shared__ float wsum[kMaxExperts / 64];
  const int tid = threadIdx.x;
  const int j = tid & (kMaxExperts - 1);
  const int g = tid / kMaxExperts;
  const int chunk = (nb + G - 1) / G;
  const int b0 = min(nb, g * chunk);
  const int b1 = min(nb, b0 + chunk);
  float sum = 0.f;
  if (j < E)
    for (int b = b0; b < b1; ++b) sum += psum[(long)b * E + j];
  part[g][j] = sum;
  __syncthreads();
  const float inv_t = 1.f / (float)ntok;
  if (tid < kMaxExperts) {
    float term = 0.f;
    if (j < E) {
      float pm = part[0][j];
#pragma unroll
      for (int g2 = 1; g2 < G; ++g2) pm += part[g2][j];
      const int ld = first_total[j];
      load[j] = ld;
      term = ((float)ld * inv_t) * (pm * inv_t);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = term;
  }
  __syncthreads();
  if (tid == 0) {
    float total = wsum[0];
#pragma unroll
    for (int w = 1; w < kMaxExperts / 64; ++w) total += wsum[w];
    aux[0] = (float)E * total;
  }
}

// dlogits of the gate weights and of the balance loss together, p recomputed
// from the logits and the saved p_max. With c_k = kept_k * dgate_k:
//   raw         c_0 p_0 ((j == e0) - p_j) + c_1 p_1 ((j == e1) - p_j)
//   normalized  +-(c_0 - c_1) g0 g1 at e0 / e1
//   aux         daux (E / T) p_j (load_j / T - sum_e (load_e / T) p_e),
//               for every token, dropped or not; skipped when daux is null.
template <typename T, int K>
__global__ __launch_bounds__(kTokBlock) void route_topk_bwd_kernel(
    const T* __restrict__ logits, const float* __restrict__ pmax,
    const float* __restrict__ gate, const int* __restrict__ expert,
    const int* __restrict__ slot, const float* __restrict__ dgate,
    const int* __restrict__ load, const float* __restrict__ daux,
    T* __restrict__ dlogits, long ntok, int E, int normalize) {
  __shared__ float lw[kMaxExperts];
  const bool has_aux = daux != nullptr;
  const float inv_t = 1.f / (float)ntok;
  if (has_aux) {
    lw[threadIdx.x] = (int)threadIdx.x < E ? (float)load[threadIdx.x] * inv_t
                                           : 0.f;
    __syncthreads();
  }
  const long t = (long)blockIdx.x * kTokBlock + threadIdx.x;
  if (t >= ntok) return;
  const T* x = logits + t * E;
  T* dx = dlogits + t * E;
  const int e0 = expert[t * K];
  const int e1 = K == 2 ? expert[t * K + 1] : -1;
  const float pm = pmax[t];
  const float xe = to_f(x[e0]);
  float ca = 0.f, a = 0.f;
  if (has_aux) {
    ca = daux[0] * (float)E * inv_t;
    for (int j = 0; j < E; ++j) a += lw[j] * (exp_rel(to_f(x[j]), xe) * pm);
  }
  const float c0 = slot[t * K] >= 0 ? dgate[t * K] : 0.f;
  const float c1 = (K == 2 && slot[t * K + 1] >= 0) ? dgate[t * K + 1] : 0.f;
  float w0, w1, wsum;  // dx[j] = (j==e0) w0 + (j==e1) w1 - wsum p_j + aux
  if (K == 2 && normalize) {
    w0 = (c0 - c1) * gate[t * K] * gate[t * K + 1];
    w1 = -w0;
    wsum = 0.f;
  } else {
    w0 = c0 * pm;
    w1 = K == 2 ? c1 * gate[t * K + 1] : 0.f;
    wsum = w0 + w1;
  }
  for (int j = 0; j < E; ++j) {
    const float pj = exp_rel(to_f(x[j]), xe) * pm;
    float v = (j == e0 ? w0 : 0.f) + (j == e1 ? w1 : 0.f) - wsum * pj;
    if (has_aux) v += ca * pj * (lw[j] - a);
    dx[j] = from_f<T>(v);
  }
}

// ------------------------------------------------------------ row movement

// A workgroup covers 256/tpr rows at a time with tpr (a power of two) lanes
// per row, U such row groups per iteration so U row loads are in flight per
// lane behind the dependent map load.
template <typename T, bool SCALED, bool CHOICE, int U>
__global__ __launch_bounds__(256) void gather_rows_kernel(
    const T* __restrict__ in, long in_rows, const int* __restrict__ map,
    const float* __restrict__ scale, int scale_by_src,
    const int* __restrict__ choice, int nchoice, T* __restrict__ out,
    long rows, int vpr, int tpr_log2) {
  constexpr int PK = Pk<T>::N;
  const Pk<T>* inv = reinterpret_cast<const Pk<T>*>(in);
  Pk<T>* outv = reinterpret_cast<Pk<T>*>(out);
  const int tpr = 1 << tpr_log2;
  const int rpb = 256 >> tpr_log2;
  const int sub = threadIdx.x >> tpr_log2;
  const int v0 = threadIdx.x & (tpr - 1);
  const long group = (long)rpb * U;
  for (long base = (long)blockIdx.x * group; base < rows;
       base += (long)gridDim.x * group) {
    long r[U];
    long m[U];
    float s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      r[k] = base + (long)k * rpb + sub;
      const int mk = r[k] < rows ? map[r[k]] : -1;
      m[k] = (mk >= 0 && mk < in_rows) ? mk : -1;
      if (SCALED) {
        long si = scale_by_src ? m[k] : r[k];
        if (CHOICE && m[k] >= 0)  // scale is [in_rows, nchoice]
          si = si * nchoice + min(max(choice[r[k]], 0), nchoice - 1);
        s[k] = m[k] >= 0 ? scale[si] : 0.f;
      }
    }
    for (int v = v0; v < vpr; v += tpr) {
      Pk<T> a[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (m[k] >= 0) {
          a[k] = inv[m[k] * vpr + v];
        } else {
#pragma unroll
          for (int i = 0; i < PK; ++i) a[k].v[i] = from_f<T>(0.f);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (SCALED && m[k] >= 0) {
#pragma unroll
          for (int i = 0; i < PK; ++i)
            a[k].v[i] = from_f<T>(to_f(a[k].v[i]) * s[k]);
        }
        if (r[k] < rows) outv[r[k] * vpr + v] = a[k];
      }
    }
  }
}

// out[r] = in[map[r][0]] (* scale[r][0]) + in[map[r][1]] (* scale[r][1]),
// skipping entries with map < 0: the sum is taken in fp32 and rounded once,
// a single source is copied (or scaled) as gather_rows_kernel does, and a row
// with no source is zeros. Same lane layout as gather_rows_kernel.
template <typename T, bool SCALED, int U>
__global__ __launch_bounds__(256) void gather2_rows_kernel(
    const T* __restrict__ in, long in_rows, const int* __restrict__ map,
    const float* __restrict__ scale, T* __restrict__ out, long rows, int vpr,
    int tpr_log2) {
  constexpr int PK = Pk<T>::N;
  const Pk<T>* inv = reinterpret_cast<const Pk<T>*>(in);
  Pk<T>* outv = reinterpret_cast<Pk<T>*>(out);
  const int tpr = 1 << tpr_log2;
  const int rpb = 256 >> tpr_log2;
  const int sub = threadIdx.x >> tpr_log2;
  const int v0 = threadIdx.x & (tpr - 1);
  const long group = (long)rpb * U;
  for (long base = (long)blockIdx.x * group; base < rows;
       base += (long)gridDim.x * group) {
    long r[U];
    long m[U][2];
    float s[U][2];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      r[k] = base + (long)k * rpb + sub;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int mk = r[k] < rows ? map[r[k] * 2 + c] : -1;
        m[k][c] = (mk >= 0 && mk < in_rows) ? mk : -1;
        if (SCALED) s[k][c] = m[k][c] >= 0 ? scale[r[k] * 2 + c] : 0.f;
      }
    }
    for (int v = v0; v < vpr; v += tpr) {
      Pk<T> a[U][2];
#pragma unroll
      for (int k = 0; k < U; ++k) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (m[k][c] >= 0) {
            a[k][c] = inv[m[k][c] * vpr + v];
          } else {
#pragma unroll
            for (int i = 0; i < PK; ++i) a[k][c].v[i] = from_f<T>(0.f);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        Pk<T> o;
#pragma unroll
        for (int i = 0; i < PK; ++i) {
          float x0 = to_f(a[k][0].v[i]), x1 = to_f(a[k][1].v[i]);
          if (SCALED) {
            x0 *= s[k][0];
            x1 *= s[k][1];
          }
          const float both = x0 + x1;
          o.v[i] = from_f<T>(m[k][0] < 0 ? x1 : (m[k][1] < 0 ? x0 : both));
        }
        if (r[k] < rows) outv[r[k] * vpr + v] = o;
      }
    }
  }
}

// out[r] = dot(a[r >> a_shift], b[map[r]]) in fp32, 0 where map < 0 (a_shift
// 1: two map entries per row of a). tpr <= 64 lanes of one wave share a row
// and fold with xor shuffles, so the sum order is fixed.
template <typename T, int U>
__global__ __launch_bounds__(256) void rowdot_kernel(
    const T* __restrict__ a, const T* __restrict__ b, long b_rows,
    const int* __restrict__ map, float* __restrict__ out, long rows, int vpr,
    int tpr_log2, int a_shift) {
  constexpr int PK = Pk<T>::N;
  const Pk<T>* av = reinterpret_cast<const Pk<T>*>(a);
  const Pk<T>* bv = reinterpret_cast<const Pk<T>*>(b);
  const int tpr = 1 << tpr_log2;
  const int rpb = 256 >> tpr_log2;
  const int sub = threadIdx.x >> tpr_log2;
  const int v0 = threadIdx.x & (tpr - 1);
  const long group = (long)rpb * U;
  for (long base = (long)blockIdx.x * group; base < rows;
       base += (long)gridDim.x * group) {
    long r[U];
    long m[U];
    float acc[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      r[k] = base + (long)k * rpb + sub;
      const int mk = r[k] < rows ? map[r[k]] : -1;
      m[k] = (mk >= 0 && mk < b_rows) ? mk : -1;
      acc[k] = 0.f;
    }
    for (int v = v0; v < vpr; v += tpr) {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (m[k] >= 0) {
          const Pk<T> x = av[(r[k] >> a_shift) * vpr + v];
          const Pk<T> y = bv[m[k] * vpr + v];
#pragma unroll
          for (int i = 0; i < PK; ++i)
            acc[k] = __builtin_fmaf(to_f(x.v[i]), to_f(y.v[i]), acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      for (int off = tpr >> 1; off > 0; off >>= 1)
        acc[k] += __shfl_xor(acc[k], off, 64);
      if (v0 == 0 && r[k] < rows) out[r[k]] = acc[k];
    }
  }
}

int ceil_log2(long n) {
  int l = 0;
  while ((1L << l) < n) ++l;
  return l;
}

unsigned row_grid(long rows, long group) {
  long blocks = (rows + group - 1) / group;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

long check_rows(const char* what, int dtype, long rows, long d,
                std::initializer_list<const void*> ptrs) {
  if (dtype < 0 || dtype > (int)Dtype::BF16)
    throw std::runtime_error(std::string(what) + ": bad dtype " +
                             std::to_string(dtype));
  const long row_bytes = d * dtype_size((Dtype)dtype);
  if (rows < 1 || d < 1 || row_bytes % 16 != 0)
    throw std::runtime_error(std::string(what) +
                             ": need rows >= 1 and a row size that is a "
                             "multiple of 16 bytes");
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0)
      throw std::runtime_error(std::string(what) +
                               ": row buffers must be 16-byte aligned");
  return row_bytes / 16;
}

void check_route(const char* what, int dtype, long ntok, long E, long cap) {
  if (dtype < 0 || dtype > (int)Dtype::BF16)
    throw std::runtime_error(std::string(what) + ": bad dtype " +
                             std::to_string(dtype));
  if (ntok < 1 || E < 1 || E > kMaxExperts || cap < 1 ||
      E * cap >= (1L << 31) ||
      (ntok + kTokBlock - 1) / kTokBlock >= (1L << 31) / kMaxExperts)
    throw std::runtime_error(std::string(what) +
                             ": need T >= 1, 1 <= E <= 256, cap >= 1 and "
                             "E*cap < 2^31");
}

template <typename T>
void gather_launch(const void* in, long in_rows, const int* map,
                   const float* scale, int scale_by_src, const int* choice,
                   int nchoice, void* out, long rows, int vpr,
                   hipStream_t stream) {
  constexpr int U = 4;
  const int tl = ceil_log2(vpr < 256 ? vpr : 256);
  const dim3 grid(row_grid(rows, (long)(256 >> tl) * U));
  if (scale && choice)
    hipLaunchKernelGGL((gather_rows_kernel<T, true, true, U>), grid,
                       dim3(256), 0, stream, (const T*)in, in_rows, map,
                       scale, scale_by_src, choice, nchoice, (T*)out, rows,
                       vpr, tl);
  else if (scale)
    hipLaunchKernelGGL((gather_rows_kernel<T, true, false, U>), grid,
                       dim3(256), 0, stream, (const T*)in, in_rows, map,
                       scale, scale_by_src, choice, nchoice, (T*)out, rows,
                       vpr, tl);
  else
    hipLaunchKernelGGL((gather_rows_kernel<T, false, false, U>), grid,
                       dim3(256), 0, stream, (const T*)in, in_rows, map,
                       scale, scale_by_src, choice, nchoice, (T*)out, rows,
                       vpr, tl);
}

template <typename T>
void rowdot_launch(const void* a, const void* b, long b_rows, const int* map,
                   float* out, long rows, int vpr, int a_shift,
                   hipStream_t stream) {
  constexpr int U = 2;
  const int tl = ceil_log2(vpr < 64 ? vpr : 64);
  const dim3 grid(row_grid(rows, (long)(256 >> tl) * U));
  hipLaunchKernelGGL((rowdot_kernel<T, U>), grid, dim3(256), 0, stream,
                     (const T*)a, (const T*)b, b_rows, map, out, rows, vpr,
                     tl, a_shift);
}

}  // namespace

// Workspace ints: counts and offs are [ceil(T/256) * E], totals is [E].
void moe_route(int dtype, const void* logits, float* gate_p, int* expert,
               int* slot, int* src, int* counts, int* offs, int* totals,
               long ntok, long E, long cap, hipStream_t stream) {
  check_route("moe_route", dtype, ntok, E, cap);
  const int nb = (int)((ntok + kTokBlock - 1) / kTokBlock);
  const dim3 grid((unsigned)nb), block(kTokBlock);
  switch ((Dtype)dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((route_top1_kernel<float>), grid, block, 0, stream,
                         (const float*)logits, gate_p, expert, counts, ntok,
                         (int)E);
      break;
    case Dtype::F16:
      hipLaunchKernelGGL((route_top1_kernel<__half>), grid, block, 0, stream,
                         (const __half*)logits, gate_p, expert, counts, ntok,
                         (int)E);
      break;
    case Dtype::BF16:
      hipLaunchKernelGGL((route_top1_kernel<__hip_bfloat16>), grid, block, 0,
                         stream, (const __hip_bfloat16*)logits, gate_p,
                         expert, counts, ntok, (int)E);
      break;
  }
  hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kScanThreads), 0,
                     stream, counts, offs, totals, nb, (int)E,
                     ceil_log2(E));
  hipLaunchKernelGGL(route_rank_kernel, grid, block, 0, stream, expert, offs,
                     totals, slot, src, ntok, (int)E, (int)cap);
}

void moe_route_bwd(int dtype, const void* logits, const float* gate_p,
                   const int* expert, const int* slot, const float* dgate,
                   void* dlogits, long ntok, long E, hipStream_t stream) {
  check_route("moe_route_bwd", dtype, ntok, E, 1);
  const dim3 grid((unsigned)((ntok + kTokBlock - 1) / kTokBlock));
  const dim3 block(kTokBlock);
  switch ((Dtype)dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((route_bwd_kernel<float>), grid, block, 0, stream,
                         (const float*)logits, gate_p, expert, slot, dgate,
                         (float*)dlogits, ntok, (int)E);
      return;
    case Dtype::F16:
      hipLaunchKernelGGL((route_bwd_kernel<__half>), grid, block, 0, stream,
                         (const __half*)logits, gate_p, expert, slot, dgate,
                         (__half*)dlogits, ntok, (int)E);
      return;
    case Dtype::BF16:
      hipLaunchKernelGGL((route_bwd_kernel<__hip_bfloat16>), grid, block, 0,
                         stream, (const __hip_bfloat16*)logits, gate_p,
                         expert, slot, dgate, (__hip_bfloat16*)dlogits, ntok,
                         (int)E);
      return;
  }
}

// Top-k routing, k in {1, 2}. expert, slot and gate are [T, k]; src and
// src_choice are [E*cap]; pmax is [T]; load is [E]; aux is one float.
// Workspaces: counts and offs are [k * ceil(T/256) * E] ints, totals is [E]
// ints, psum is [ceil(T/256) * E] floats.
void moe_route_topk(int dtype, const void* logits, int k, int normalize,
                    float* gate, float* pmax, int* expert, int* slot,
                    int* src, int* src_choice, int* load, float* aux,
                    int* counts, int* offs, int* totals, float* psum,
                    long ntok, long E, long cap, hipStream_t stream) {
  check_route("moe_route_topk", dtype, ntok, E, cap);
  if (k < 1 || k > 2 || E < k)
    throw std::runtime_error("moe_route_topk: need k in {1, 2} and E >= k");
  const int nb = (int)((ntok + kTokBlock - 1) / kTokBlock);
  if ((long)k * nb >= (1L << 31) / kMaxExperts)
    throw std::runtime_error("moe_route_topk: too many tokens");
  const dim3 grid((unsigned)nb), block(kTokBlock);
#define ADAPCC_ROUTE_TOPK(T, K)                                              \
  hipLaunchKernelGGL((route_topk_kernel<T, K>), grid, block, 0, stream,      \
                     (const T*)logits, gate, pmax, expert, counts, psum,     \
                     ntok, (int)E, normalize)
  switch ((Dtype)dtype) {
    case Dtype::F32:
      if (k == 1) ADAPCC_ROUTE_TOPK(float, 1);
      else ADAPCC_ROUTE_TOPK(float, 2);
      break;
    case Dtype::F16:
      if (k == 1) ADAPCC_ROUTE_TOPK(__half, 1);
      else ADAPCC_ROUTE_TOPK(__half, 2);
      break;
    case Dtype::BF16:
      if (k == 1) ADAPCC_ROUTE_TOPK(__hip_bfloat16, 1);
      else ADAPCC_ROUTE_TOPK(__hip_bfloat16, 2);
      break;
  }
#undef ADAPCC_ROUTE_TOPK
  hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kScanThreads), 0,
                     stream, counts, offs, totals, k * nb, (int)E,
                     ceil_log2(E));
  // first choices per expert: where the second choices start, or everything
  const int* first_total = k == 2 ? offs + (long)nb * E : totals;
  hipLaunchKernelGGL(route_aux_kernel, dim3(1), dim3(kScanThreads), 0, stream,
                     psum, first_total, load, aux, nb, (int)E, ntok);
  hipLaunchKernelGGL(route_rank_topk_kernel, dim3((unsigned)(k * nb)), block,
                     0, stream, expert, offs, totals, slot, src, src_choice,
                     ntok, nb, k, (int)E, (int)cap);
}

// daux may be null: the balance loss got no gradient.
void moe_route_topk_bwd(int dtype, const void* logits, int k, int normalize,
                        const float* pmax, const float* gate,
                        const int* expert, const int* slot,
                        const float* dgate, const int* load,
                        const float* daux, void* dlogits, long ntok, long E,
                        hipStream_t stream) {
  check_route("moe_route_topk_bwd", dtype, ntok, E, 1);
  if (k < 1 || k > 2 || E < k)
    throw std::runtime_error(
        "moe_route_topk_bwd: need k in {1, 2} and E >= k");
  const dim3 grid((unsigned)((ntok + kTokBlock - 1) / kTokBlock));
  const dim3 block(kTokBlock);
#define ADAPCC_ROUTE_TOPK_BWD(T, K)                                          \
  hipLaunchKernelGGL((route_topk_bwd_kernel<T, K>), grid, block, 0, stream,  \
                     (const T*)logits, pmax, gate, expert, slot, dgate,      \
                     load, daux, (T*)dlogits, ntok, (int)E, normalize)
  switch ((Dtype)dtype) {
    case Dtype::F32:
      if (k == 1) ADAPCC_ROUTE_TOPK_BWD(float, 1);
      else ADAPCC_ROUTE_TOPK_BWD(float, 2);
      return;
    case Dtype::F16:
      if (k == 1) ADAPCC_ROUTE_TOPK_BWD(__half, 1);
      else ADAPCC_ROUTE_TOPK_BWD(__half, 2);
      return;
    case Dtype::BF16:
      if (k == 1) ADAPCC_ROUTE_TOPK_BWD(__hip_bfloat16, 1);
      else ADAPCC_ROUTE_TOPK_BWD(__hip_bfloat16, 2);
      return;
  }
#undef ADAPCC_ROUTE_TOPK_BWD
}

// out[r] = in[map[r]] for r < rows, times scale[r] (or scale[map[r]] when
// scale_by_src) if scale is given; zeros where map[r] is not in [0, in_rows).
// With choice (and scale_by_src), scale is [in_rows, nchoice] and row r takes
// scale[map[r]][choice[r]].
void moe_gather(int dtype, const void* in, long in_rows, const int* map,
                const float* scale, int scale_by_src, const int* choice,
                int nchoice, void* out, long rows, long d,
                hipStream_t stream) {
  const long vpr = check_rows("moe_gather", dtype, rows, d, {in, out});
  if (in_rows < 1 || vpr >= (1L << 31))
    throw std::runtime_error("moe_gather: bad source rows or row width");
  if (choice && (!scale || !scale_by_src || nchoice < 1))
    throw std::runtime_error(
        "moe_gather: choice needs a by-source scale and nchoice >= 1");
  switch ((Dtype)dtype) {
    case Dtype::F32:
      gather_launch<float>(in, in_rows, map, scale, scale_by_src, choice,
                           nchoice, out, rows, (int)vpr, stream);
      return;
    case Dtype::F16:
      gather_launch<__half>(in, in_rows, map, scale, scale_by_src, choice,
                            nchoice, out, rows, (int)vpr, stream);
      return;
    case Dtype::BF16:
      gather_launch<__hip_bfloat16>(in, in_rows, map, scale, scale_by_src,
                                    choice, nchoice, out, rows, (int)vpr,
                                    stream);
      return;
  }
}

// out[r] = in[map[r][0]] + in[map[r][1]] for r < rows, each term times
// scale[r][c] if scale is given and skipped where map[r][c] is not in
// [0, in_rows): fp32 sum, one rounding, zeros where both are skipped.
void moe_gather2(int dtype, const void* in, long in_rows, const int* map,
                 const float* scale, void* out, long rows, long d,
                 hipStream_t stream) {
  const long vpr = check_rows("moe_gather2", dtype, rows, d, {in, out});
  if (in_rows < 1 || vpr >= (1L << 31))
    throw std::runtime_error("moe_gather2: bad source rows or row width");
  constexpr int U = 2;
  const int tl = ceil_log2(vpr < 256 ? vpr : 256);
  const dim3 grid(row_grid(rows, (long)(256 >> tl) * U));
#define ADAPCC_GATHER2(T)                                                    \
  if (scale)                                                                 \
    hipLaunchKernelGGL((gather2_rows_kernel<T, true, U>), grid, dim3(256),   \
                       0, stream, (const T*)in, in_rows, map, scale,         \
                       (T*)out, rows, (int)vpr, tl);                         \
  else                                                                       \
    hipLaunchKernelGGL((gather2_rows_kernel<T, false, U>), grid, dim3(256),  \
                       0, stream, (const T*)in, in_rows, map, scale,         \
                       (T*)out, rows, (int)vpr, tl)
  switch ((Dtype)dtype) {
    case Dtype::F32:
      ADAPCC_GATHER2(float);
      return;
    case Dtype::F16:
      ADAPCC_GATHER2(__half);
      return;
    case Dtype::BF16:
      ADAPCC_GATHER2(__hip_bfloat16);
      return;
  }
#undef ADAPCC_GATHER2
}

// out[r] = dot(a[r >> a_shift], b[map[r]]) for r < rows; 0 where map[r] is
// not in [0, b_rows). a has rows >> a_shift rows.
void moe_rowdot(int dtype, const void* a, const void* b, long b_rows,
                const int* map, float* out, long rows, long d, int a_shift,
                hipStream_t stream) {
  const long vpr = check_rows("moe_rowdot", dtype, rows, d, {a, b});
  if (b_rows < 1 || vpr >= (1L << 31) || a_shift < 0 || a_shift > 1)
    throw std::runtime_error("moe_rowdot: bad source rows or row width");
  switch ((Dtype)dtype) {
    case Dtype::F32:
      rowdot_launch<float>(a, b, b_rows, map, out, rows, (int)vpr, a_shift,
                           stream);
      return;
    case Dtype::F16:
      rowdot_launch<__half>(a, b, b_rows, map, out, rows, (int)vpr, a_shift,
                            stream);
      return;
    case Dtype::BF16:
      rowdot_launch<__hip_bfloat16>(a, b, b_rows, map, out, rows, (int)vpr,
                                    a_shift, stream);
      return;
  }
}

}  // namespace adapcc

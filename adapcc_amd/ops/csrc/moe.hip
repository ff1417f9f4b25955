// Top-1 MoE routing, dispatch and combine (CDNA4 / gfx950).
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
//   moe_rowdot     out[r] = dot(a[r], b[map[r]]) in fp32 (dgate_p)
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
  int rank = 0;
  unsigned long long todo = __ballot(active);
  while (todo) {  // one round per distinct expert in the wave
    const int leader = __ffsll((long long)todo) - 1;
    const int e0 = __shfl(e, leader, 64);
    const bool mine = active && e == e0;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      rank = __popcll(m & ((1ull << lane) - 1ull));
      if (rank == 0) wcount[wave][e0] = __popcll(m);
    }
    todo &= ~m;
  }
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

// ------------------------------------------------------------ row movement

// A workgroup covers 256/tpr rows at a time with tpr (a power of two) lanes
// per row, U such row groups per iteration so U row loads are in flight per
// lane behind the dependent map load.
template <typename T, bool SCALED, int U>
__global__ __launch_bounds__(256) void gather_rows_kernel(
    const T* __restrict__ in, long in_rows, const int* __restrict__ map,
    const float* __restrict__ scale, int scale_by_src, T* __restrict__ out,
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
      if (SCALED)
        s[k] = m[k] >= 0 ? scale[scale_by_src ? m[k] : r[k]] : 0.f;
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

// out[r] = dot(a[r], b[map[r]]) in fp32, 0 where map < 0. tpr <= 64 lanes of
// one wave share a row and fold with xor shuffles, so the sum order is fixed.
template <typename T, int U>
__global__ __launch_bounds__(256) void rowdot_kernel(
    const T* __restrict__ a, const T* __restrict__ b, long b_rows,
    const int* __restrict__ map, float* __restrict__ out, long rows, int vpr,
    int tpr_log2) {
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
          const Pk<T> x = av[r[k] * vpr + v];
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
                   const float* scale, int scale_by_src, void* out, long rows,
                   int vpr, hipStream_t stream) {
  constexpr int U = 4;
  const int tl = ceil_log2(vpr < 256 ? vpr : 256);
  const dim3 grid(row_grid(rows, (long)(256 >> tl) * U));
  if (scale)
    hipLaunchKernelGGL((gather_rows_kernel<T, true, U>), grid, dim3(256), 0,
                       stream, (const T*)in, in_rows, map, scale,
                       scale_by_src, (T*)out, rows, vpr, tl);
  else
    hipLaunchKernelGGL((gather_rows_kernel<T, false, U>), grid, dim3(256), 0,
                       stream, (const T*)in, in_rows, map, scale,
                       scale_by_src, (T*)out, rows, vpr, tl);
}

template <typename T>
void rowdot_launch(const void* a, const void* b, long b_rows, const int* map,
                   float* out, long rows, int vpr, hipStream_t stream) {
  constexpr int U = 2;
  const int tl = ceil_log2(vpr < 64 ? vpr : 64);
  const dim3 grid(row_grid(rows, (long)(256 >> tl) * U));
  hipLaunchKernelGGL((rowdot_kernel<T, U>), grid, dim3(256), 0, stream,
                     (const T*)a, (const T*)b, b_rows, map, out, rows, vpr,
                     tl);
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

// out[r] = in[map[r]] for r < rows, times scale[r] (or scale[map[r]] when
// scale_by_src) if scale is given; zeros where map[r] is not in [0, in_rows).
void moe_gather(int dtype, const void* in, long in_rows, const int* map,
                const float* scale, int scale_by_src, void* out, long rows,
                long d, hipStream_t stream) {
  const long vpr = check_rows("moe_gather", dtype, rows, d, {in, out});
  if (in_rows < 1 || vpr >= (1L << 31))
    throw std::runtime_error("moe_gather: bad source rows or row width");
  switch ((Dtype)dtype) {
    case Dtype::F32:
      gather_launch<float>(in, in_rows, map, scale, scale_by_src, out, rows,
                           (int)vpr, stream);
      return;
    case Dtype::F16:
      gather_launch<__half>(in, in_rows, map, scale, scale_by_src, out, rows,
                            (int)vpr, stream);
      return;
    case Dtype::BF16:
      gather_launch<__hip_bfloat16>(in, in_rows, map, scale, scale_by_src,
                                    out, rows, (int)vpr, stream);
      return;
  }
}

// out[r] = dot(a[r], b[map[r]]) for r < rows; 0 where map[r] is not in
// [0, b_rows).
void moe_rowdot(int dtype, const void* a, const void* b, long b_rows,
                const int* map, float* out, long rows, long d,
                hipStream_t stream) {
  const long vpr = check_rows("moe_rowdot", dtype, rows, d, {a, b});
  if (b_rows < 1 || vpr >= (1L << 31))
    throw std::runtime_error("moe_rowdot: bad source rows or row width");
  switch ((Dtype)dtype) {
    case Dtype::F32:
      rowdot_launch<float>(a, b, b_rows, map, out, rows, (int)vpr, stream);
      return;
    case Dtype::F16:
      rowdot_launch<__half>(a, b, b_rows, map, out, rows, (int)vpr, stream);
      return;
    case Dtype::BF16:
      rowdot_launch<__hip_bfloat16>(a, b, b_rows, map, out, rows, (int)vpr,
                                    stream);
      return;
  }
}

}  // namespace adapcc

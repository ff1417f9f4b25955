// Fused cross-entropy for large vocabularies (CDNA4 / gfx950).
//
// Replaces torch's log_softmax + nll_loss pair on the flagship GPT-2 path,
// where the [B*S, V] bf16 logits tensor is 6.6 GB: the stock path writes
// (and autograd re-reads) a full log-softmax tensor of the same size, so
// fwd+bwd move ~26 GB of HBM traffic. This fused version never
// materializes log-softmax:
//   forward:  ONE read pass per row (online max/sum-exp in fp32), writes
//             per-row loss and logsumexp (fp32, 4 B each).
//   backward: ONE read of logits + ONE write of dlogits:
//             d = gscale * (exp(x - lse) - [j == target]).
// Memory-bound target: fwd ~= bytes(logits)/6.3 TB/s.
//
// Training (ce_fwd_grad_kernel): a row of up to kCeMaxVecs * 256 16-byte
// vectors (50257 bf16 columns: 25 per thread) stays in registers between
// the lse pass and the gradient pass, so loss, lse and
//   dlogits = g0 * (exp(x - lse) - [j == target]),  g0 = 1 / n_valid
// leave ONE kernel after ONE read of the logits: the forward's own read
// pass is gone. The accumulation below is shared with ce_fwd_kernel and the
// gradient expression with ce_bwd_kernel, so the three outputs carry the
// bits the two-kernel path gives. The backward then hands the saved dlogits
// on: ce_bwd_kernel reads the upstream gradient from device memory and
// returns at once when it is exactly 1.0f; any other value recomputes
// dlogits from the logits as before, over the saved tensor. Wider rows keep
// the two kernels.
//
// The reference has no analog (its models use transformers' CE); this is a
// new MI355X-first op in the spirit of BASELINE.json's north star (fuse
// elementwise/normalization work into the producing pass, keep tensors
// from round-tripping HBM).

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "common.h"

namespace adapcc {

namespace {

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(__half x) { return __half2float(x); }
__device__ __forceinline__ float to_f32(__hip_bfloat16 x) {
  return __bfloat162float(x);
}

template <typename T>
__device__ __forceinline__ T from_f32(float x);
template <>
__device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <>
__device__ __forceinline__ __half from_f32<__half>(float x) {
  return __float2half(x);
}
template <>
__device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float x) {
  return __float2bfloat16(x);
}

constexpr float kNegInf = -3.0e38f;

// Online (max, sumexp) accumulator combine.
__device__ __forceinline__ void combine(float& m, float& s, float m2,
                                        float s2) {
  const float mn = fmaxf(m, m2);
  // exp(-inf - -inf) guards: if both -inf, s stays 0.
  s = (m == kNegInf ? 0.f : s * __expf(m - mn)) +
      (m2 == kNegInf ? 0.f : s2 * __expf(m2 - mn));
  m = mn;
}

// 16-byte vector pack of T.
template <typename T>
struct alignas(16) Pack {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

// Block-wide (256 threads) reduce of the online pair into lane-broadcast
// (m, s) via wave shuffles + 4-slot LDS.
__device__ __forceinline__ void block_reduce_ms(float& m, float& s,
                                                float* lds_m, float* lds_s) {
  // wave64 butterfly
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float s2 = __shfl_xor(s, off, 64);
    combine(m, s, m2, s2);
  }
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    lds_m[wave] = m;
    lds_s[wave] = s;
  }
  __syncthreads();
  // every thread folds the 4 wave results (cheap, avoids a second bcast)
  m = lds_m[0];
  s = lds_s[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) combine(m, s, lds_m[w], lds_s[w]);
}

// A row as scalar head [0, head), nvec aligned 16-byte vectors from there,
// and a scalar tail from tail_start; head and tail are under one vector
// long. The head stops at cols in a row shorter than its misalignment.
struct RowSplit {
  long head, nvec, tail_start;
};

template <typename T>
__device__ __forceinline__ RowSplit row_split(const T* x, long cols) {
  constexpr int PK = Pack<T>::N;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
  long head = ((16 - (addr & 15)) & 15) / sizeof(T);
  if (head > cols) head = cols;
  const long nvec = (cols - head) / PK;
  return {head, nvec, head + nvec * PK};
}

// One vector's fp32 values / one scalar into a thread's online (max, sumexp)
// pair. ce_fwd_kernel and ce_fwd_grad_kernel both accumulate through these,
// in the same element order, so their lse and loss agree bit for bit.
template <int PK>
__device__ __forceinline__ void accum_vals(float& m, float& s,
                                           const float (&xv)[PK]) {
  float lm = xv[0];
#pragma unroll
  for (int j = 1; j < PK; ++j) lm = fmaxf(lm, xv[j]);
  if (lm > m) {
    s *= __expf(m - lm);  // s==0 when m was -inf: fine
    m = lm;
  }
#pragma unroll
  for (int j = 0; j < PK; ++j) s += __expf(xv[j] - m);
}

__device__ __forceinline__ void accum_one(float& m, float& s, float xv) {
  if (xv > m) {
    s *= __expf(m - xv);
    m = xv;
  }
  s += __expf(xv - m);
}

// d = gscale * (softmax - onehot), in fp32: both gradient kernels' element.
__device__ __forceinline__ float grad_val(float x, float l, float gscale,
                                          bool is_target) {
  const float sm = __expf(x - l);
  return gscale * (sm - (is_target ? 1.f : 0.f));
}

template <typename T>
__device__ __forceinline__ T grad_elem(T x, float l, float gscale,
                                       bool is_target) {
  return from_f32<T>(grad_val(to_f32(x), l, gscale, is_target));
}

// A 16-byte vector as four raw dwords: to_f32 of its elements, and the
// dwords of from_f32 of eight (four) floats. ce_fwd_grad_kernel keeps its
// row in this form: an array of 16-bit elements held across the kernel
// ends up one element to a register.
template <typename T>
struct Words;
template <>
struct Words<float> {
  __device__ __forceinline__ static void unpack(const uint4& w, float* o) {
    o[0] = __uint_as_float(w.x);
    o[1] = __uint_as_float(w.y);
    o[2] = __uint_as_float(w.z);
    o[3] = __uint_as_float(w.w);
  }
  __device__ __forceinline__ static uint4 pack(const float* i) {
    return make_uint4(__float_as_uint(i[0]), __float_as_uint(i[1]),
                      __float_as_uint(i[2]), __float_as_uint(i[3]));
  }
};
template <>
struct Words<__hip_bfloat16> {
  __device__ __forceinline__ static void unpack(const uint4& w, float* o) {
    const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = __uint_as_float(d[i] << 16);  // bf16 is fp32's top half
      o[2 * i + 1] = __uint_as_float(d[i] & 0xffff0000u);
    }
  }
  __device__ __forceinline__ static unsigned bits(float x) {
    return __bfloat16_as_ushort(__float2bfloat16(x));
  }
  __device__ __forceinline__ static uint4 pack(const float* i) {
    return make_uint4(bits(i[0]) | (bits(i[1]) << 16),
                      bits(i[2]) | (bits(i[3]) << 16),
                      bits(i[4]) | (bits(i[5]) << 16),
                      bits(i[6]) | (bits(i[7]) << 16));
  }
};
template <>
struct Words<__half> {
  __device__ __forceinline__ static void unpack(const uint4& w, float* o) {
    const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = __half2float(__ushort_as_half((unsigned short)d[i]));
      o[2 * i + 1] =
          __half2float(__ushort_as_half((unsigned short)(d[i] >> 16)));
    }
  }
  __device__ __forceinline__ static unsigned bits(float x) {
    return __half_as_ushort(__float2half(x));
  }
  __device__ __forceinline__ static uint4 pack(const float* i) {
    return make_uint4(bits(i[0]) | (bits(i[1]) << 16),
                      bits(i[2]) | (bits(i[3]) << 16),
                      bits(i[4]) | (bits(i[5]) << 16),
                      bits(i[6]) | (bits(i[7]) << 16));
  }
};

// One workgroup per row. Row base may be misaligned when cols is odd
// (bf16 row stride 2*cols B), so each row does scalar head/tail around an
// aligned 16-B-vectorized body.
template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(
    const T* __restrict__ logits, const long* __restrict__ targets,
    float* __restrict__ loss, float* __restrict__ lse, long cols,
    long ignore_index) {
  constexpr int PK = Pack<T>::N;
  const long row = blockIdx.x;
  const T* x = logits + row * cols;
  const int tid = threadIdx.x;

  const RowSplit sp = row_split<T>(x, cols);

  float m = kNegInf, s = 0.f;
  if (tid < sp.head) {
    const float xv = to_f32(x[tid]);
    m = xv;
    s = 1.f;
  }
  const Pack<T>* xp = reinterpret_cast<const Pack<T>*>(x + sp.head);
  for (long p = tid; p < sp.nvec; p += 256) {
    const Pack<T> pk = xp[p];
    float xv[PK];
#pragma unroll
    for (int j = 0; j < PK; ++j) xv[j] = to_f32(pk.v[j]);
    accum_vals<PK>(m, s, xv);
  }
  for (long i = sp.tail_start + tid; i < cols; i += 256)
    accum_one(m, s, to_f32(x[i]));

  __shared__ float lds_m[4], lds_s[4];
  block_reduce_ms(m, s, lds_m, lds_s);

  if (tid == 0) {
    const float l = m + __logf(s);
    lse[row] = l;
    const long t = targets[row];
    loss[row] = (t == ignore_index) ? 0.f : (l - to_f32(x[t]));
  }
}

// upstream (null in the two-kernel path): the fp32 gradient that reaches the
// mean loss. The dlogits ce_fwd_grad_kernel saved are this kernel's result
// for 1.0f exactly, so that value returns without touching memory (a small
// grid then walks the rows, and the early exit costs next to nothing);
// any other value recomputes every row over the saved tensor.
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(
    const T* __restrict__ logits, const long* __restrict__ targets,
    const float* __restrict__ lse, const float* __restrict__ gscale_ptr,
    const float* __restrict__ upstream, T* __restrict__ dlogits, long rows,
    long cols, long ignore_index) {
  constexpr int PK = Pack<T>::N;
  if (upstream != nullptr && *upstream == 1.0f) return;
  const int tid = threadIdx.x;

  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* x = logits + row * cols;
    T* dx = dlogits + row * cols;

    const long t = targets[row];
    const float gscale = (t == ignore_index) ? 0.f : *gscale_ptr;
    const float l = lse[row];

    const RowSplit sp = row_split<T>(x, cols);

    if (tid < sp.head) dx[tid] = grad_elem(x[tid], l, gscale, tid == t);
    const Pack<T>* xp = reinterpret_cast<const Pack<T>*>(x + sp.head);
    Pack<T>* dxp = reinterpret_cast<Pack<T>*>(dx + sp.head);
    for (long p = tid; p < sp.nvec; p += 256) {
      const Pack<T> pk = xp[p];
      Pack<T> o;
      const long base = sp.head + p * PK;
#pragma unroll
      for (int j = 0; j < PK; ++j)
        o.v[j] = grad_elem(pk.v[j], l, gscale, base + j == t);
      dxp[p] = o;
    }
    for (long i = sp.tail_start + tid; i < cols; i += 256)
      dx[i] = grad_elem(x[i], l, gscale, i == t);
  }
}

// Loss, lse and dlogits of one row from one read. NV: the most 16-byte
// vectors a thread holds, so the row (at most NV * 256 vectors between the
// scalar head and tail, each under one vector long) sits in registers with
// static indexing. Every thread walks ce_fwd_kernel's elements in its order;
// the gradient is ce_bwd_kernel's with gscale = *g0_ptr (1 / n_valid: the
// upstream gradient taken as 1).
template <typename T, int NV>
__global__ __launch_bounds__(256, 3) void ce_fwd_grad_kernel(
    const T* __restrict__ logits, const long* __restrict__ targets,
    const float* __restrict__ g0_ptr, float* __restrict__ loss,
    float* __restrict__ lse, T* __restrict__ dlogits, long cols,
    long ignore_index) {
  constexpr int PK = Pack<T>::N;
  const long row = blockIdx.x;
  const T* x = logits + row * cols;
  T* dx = dlogits + row * cols;
  const int tid = threadIdx.x;

  const RowSplit sp = row_split<T>(x, cols);
  const bool has_head = tid < sp.head;
  const long ti = sp.tail_start + tid;
  const bool has_tail = ti < cols;  // the tail is shorter than one vector

  // The whole row first: NV independent loads in flight per thread, held as
  // raw dwords (four registers a vector whatever T is). Every load is
  // unconditional: a load inside a divergent branch waits for its data
  // there, one vector at a time. Lanes past the row's end re-read vector 0
  // (element 0) and never use it; a row with no whole vector reads the
  // aligned 16 bytes that hold its first element instead.
  const uint4* xp =
      sp.nvec > 0 ? reinterpret_cast<const uint4*>(x + sp.head)
                  : reinterpret_cast<const uint4*>(
                        reinterpret_cast<const char*>(x) -
                        (reinterpret_cast<uintptr_t>(x) & 15));
  uint4 r[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const long p = tid + k * 256;
    r[k] = xp[p < sp.nvec ? p : 0];
  }
  const T xh = x[has_head ? tid : 0];
  const T xt = x[has_tail ? ti : 0];

  float m = kNegInf, s = 0.f;
  if (has_head) {
    m = to_f32(xh);
    s = 1.f;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    // Empty fences (no instruction) keep the row as raw dwords until each
    // vector's turn: left alone, the compiler converts the whole row to
    // fp32 ahead of the serial (m, s) chain and keeps those copies for the
    // gradient pass, at over twice the registers. This one ties vector k to
    // the chain's m (and, outside the branch, has every wave wait for the
    // load here, once); the gradient pass' ties it to the store before it.
    asm volatile(""
                 : "+v"(r[k].x), "+v"(r[k].y), "+v"(r[k].z), "+v"(r[k].w),
                   "+v"(m));
    if (tid + k * 256 < sp.nvec) {
      float xv[PK];
      Words<T>::unpack(r[k], xv);
      accum_vals<PK>(m, s, xv);
    }
  }
  if (has_tail) accum_one(m, s, to_f32(xt));

  __shared__ float lds_m[4], lds_s[4];
  block_reduce_ms(m, s, lds_m, lds_s);

  const float l = m + __logf(s);
  const long t = targets[row];
  if (tid == 0) {
    lse[row] = l;
    loss[row] = (t == ignore_index) ? 0.f : (l - to_f32(x[t]));
  }

  const float gscale = (t == ignore_index) ? 0.f : *g0_ptr;
  if (has_head) dx[tid] = grad_elem(xh, l, gscale, tid == t);
  uint4* dxp = reinterpret_cast<uint4*>(dx + sp.head);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const long p = tid + k * 256;
    if (p < sp.nvec) {
      asm volatile(""
                   : "+v"(r[k].x), "+v"(r[k].y), "+v"(r[k].z), "+v"(r[k].w)
                   :
                   : "memory");
      float xv[PK];
      Words<T>::unpack(r[k], xv);
      const long base = sp.head + p * PK;
#pragma unroll
      for (int j = 0; j < PK; ++j)
        xv[j] = grad_val(xv[j], l, gscale, base + j == t);
      (dxp + k * 256)[tid] = Words<T>::pack(xv);
    }
  }
  if (has_tail) dx[ti] = grad_elem(xt, l, gscale, ti == t);
}

// The widest instantiation; narrower rows take a smaller one.
constexpr int kCeMaxVecs = 25;

template <typename T>
void ce_fwd_grad_launch(const void* logits, const void* targets,
                        const float* g0, float* loss, float* lse,
                        void* dlogits, long rows, long cols,
                        long ignore_index, hipStream_t stream) {
  const dim3 block(256);
  const dim3 grid((unsigned)rows);
  const long vecs = (cols / Pack<T>::N + 255) / 256;  // per thread, at most
  // the caller has checked cols <= ce_fused_max_cols: vecs <= kCeMaxVecs
#define CE_FG_LAUNCH(NV)                                                     \
  hipLaunchKernelGGL((ce_fwd_grad_kernel<T, NV>), grid, block, 0, stream,    \
                     (const T*)logits, (const long*)targets, g0, loss, lse,  \
                     (T*)dlogits, cols, ignore_index)
  if (vecs <= 4)
    CE_FG_LAUNCH(4);
  else if (vecs <= 13)
    CE_FG_LAUNCH(13);
  else
    CE_FG_LAUNCH(kCeMaxVecs);
#undef CE_FG_LAUNCH
}

template <typename T>
void ce_bwd_launch(const void* logits, const void* targets, const float* lse,
                   const float* gscale, const float* upstream, void* dlogits,
                   long rows, long cols, long ignore_index,
                   hipStream_t stream) {
  // With an upstream pointer the kernel usually returns at once (training's
  // upstream gradient is 1), so the grid is capped at 2048 workgroups that
  // walk the rows: few to launch for nothing, enough to fill the chip when
  // the gradient has to be recomputed.
  const long nb = (upstream != nullptr && rows > 2048) ? 2048 : rows;
  hipLaunchKernelGGL((ce_bwd_kernel<T>), dim3((unsigned)nb), dim3(256), 0,
                     stream, (const T*)logits, (const long*)targets, lse,
                     gscale, upstream, (T*)dlogits, rows, cols, ignore_index);
}

}  // namespace

void ce_forward(int dtype, const void* logits, const void* targets,
                float* loss, float* lse, long rows, long cols,
                long ignore_index, hipStream_t stream) {
  const dim3 block(256);
  const dim3 grid((unsigned)rows);
  switch ((Dtype)dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((ce_fwd_kernel<float>), grid, block, 0, stream,
                         (const float*)logits, (const long*)targets, loss,
                         lse, cols, ignore_index);
      return;
    case Dtype::F16:
      hipLaunchKernelGGL((ce_fwd_kernel<__half>), grid, block, 0, stream,
                         (const __half*)logits, (const long*)targets, loss,
                         lse, cols, ignore_index);
      return;
    case Dtype::BF16:
      hipLaunchKernelGGL((ce_fwd_kernel<__hip_bfloat16>), grid, block, 0,
                         stream, (const __hip_bfloat16*)logits,
                         (const long*)targets, loss, lse, cols, ignore_index);
      return;
  }
  throw std::runtime_error("ce_forward: bad dtype " + std::to_string(dtype));
}

// The widest row ce_forward_grad takes, in columns; 0 for an unknown dtype.
long ce_fused_max_cols(int dtype) {
  switch ((Dtype)dtype) {
    case Dtype::F32: return (long)kCeMaxVecs * 256 * Pack<float>::N;
    case Dtype::F16:
    case Dtype::BF16: return (long)kCeMaxVecs * 256 * Pack<__half>::N;
  }
  return 0;
}

// loss, lse and dlogits = *g0 * (softmax - onehot) (0 in ignored rows) from
// one read of the logits; cols <= ce_fused_max_cols(dtype).
void ce_forward_grad(int dtype, const void* logits, const void* targets,
                     const float* g0, float* loss, float* lse, void* dlogits,
                     long rows, long cols, long ignore_index,
                     hipStream_t stream) {
  if (cols < 1 || cols > ce_fused_max_cols(dtype))
    throw std::runtime_error("ce_forward_grad: cols=" + std::to_string(cols) +
                             " outside [1, ce_fused_max_cols]");
  switch ((Dtype)dtype) {
    case Dtype::F32:
      ce_fwd_grad_launch<float>(logits, targets, g0, loss, lse, dlogits, rows,
                                cols, ignore_index, stream);
      return;
    case Dtype::F16:
      ce_fwd_grad_launch<__half>(logits, targets, g0, loss, lse, dlogits,
                                 rows, cols, ignore_index, stream);
      return;
    case Dtype::BF16:
      ce_fwd_grad_launch<__hip_bfloat16>(logits, targets, g0, loss, lse,
                                         dlogits, rows, cols, ignore_index,
                                         stream);
      return;
  }
  throw std::runtime_error("ce_forward_grad: bad dtype " +
                           std::to_string(dtype));
}

// upstream: null, or the fp32 upstream gradient on the device; when it is
// exactly 1.0f dlogits (ce_forward_grad's) is left as it stands.
void ce_backward(int dtype, const void* logits, const void* targets,
                 const float* lse, const float* gscale, const float* upstream,
                 void* dlogits, long rows, long cols, long ignore_index,
                 hipStream_t stream) {
  switch ((Dtype)dtype) {
    case Dtype::F32:
      ce_bwd_launch<float>(logits, targets, lse, gscale, upstream, dlogits,
                           rows, cols, ignore_index, stream);
      return;
    case Dtype::F16:
      ce_bwd_launch<__half>(logits, targets, lse, gscale, upstream, dlogits,
                            rows, cols, ignore_index, stream);
      return;
    case Dtype::BF16:
      ce_bwd_launch<__hip_bfloat16>(logits, targets, lse, gscale, upstream,
                                    dlogits, rows, cols, ignore_index, stream);
      return;
  }
  throw std::runtime_error("ce_backward: bad dtype " + std::to_string(dtype));
}

}  // namespace adapcc

// Fused tanh-GeLU forward/backward (CDNA4 / gfx950).
//
// Computes tanh via one v_exp_f32 + one v_rcp_f32
// (tanh z = 1 - 2/(exp(2z)+1)) with 16-byte vectorized bf16 I/O.
// Measured vs torch's tanh-GeLU at the flagship MLP shape
// ([131072, 3072] bf16): ~10% faster fwd+bwd — both near memory-bound;
// the shorter VALU chain is the difference. Kept for the dependency-free
// hot path and the fwd/bwd symmetry with the other fused ops.
//
// gelu_bwd_bias_kernel: the backward over a [rows, cols] input that also
// sums dx down its columns, which is the gradient of the bias the linear in
// front of the GeLU added (GPT-2's c_fc). torch got it from a reduce kernel
// that re-read the whole dx this kernel had just written. One wave owns one
// row at a time, as in ln_bwd_kernel: each lane keeps the same columns for
// every row it meets, adds the dx values as rounded to T (what a sum over
// the stored dx would see) into fp32 registers. At the end a block's four
// waves add up in LDS and the block writes one partial row; colsum.hip folds
// those. dx carries gelu_bwd_kernel's bits: in bf16 both kernels compute an
// element with gelu_bwd1_pinned.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "ln_cols.h"

namespace adapcc {

namespace {

constexpr float kA = 0.7978845608028654f;   // sqrt(2/pi)
constexpr float kB = 0.044715f;
constexpr float k2Log2e = 2.885390081777927f;  // 2*log2(e)

__device__ __forceinline__ float tanh_fast(float z) {
  // tanh(z) = 1 - 2/(exp(2z)+1); exp via exp2 (v_exp_f32). |z| is modest
  // for GeLU inputs; exp2 saturates cleanly at the fp32 range bounds.
  const float e = __builtin_amdgcn_exp2f(z * k2Log2e);
  return 1.f - 2.f / (e + 1.f);
}

__device__ __forceinline__ float gelu_fwd1(float x) {
  const float u = kA * __builtin_fmaf(kB * x * x, x, x);
  return 0.5f * x * (1.f + tanh_fast(u));
}

__device__ __forceinline__ float gelu_bwd1(float x, float g) {
  const float x2 = x * x;
  const float u = kA * __builtin_fmaf(kB * x2, x, x);
  const float t = tanh_fast(u);
  const float sech2 = 1.f - t * t;
  const float du = kA * __builtin_fmaf(3.f * kB, x2, 1.f);
  return g * (0.5f * (1.f + t) + 0.5f * x * sech2 * du);
}

// gelu_bwd1 with its two fused multiply-adds (1 - t*t and the final sum)
// written out and no other fusing allowed: the arithmetic the compiler chose
// for gelu_bwd_kernel<bf16>'s vector body when that called gelu_bwd1. Which
// products it fuses in gelu_bwd1 depends on the code around the call, so two
// kernels that must give the same bits cannot leave it to the compiler. The
// bf16 vector bodies of gelu_bwd_kernel and gelu_bwd_bias_kernel both call
// this. Everything else (f32, f16, the scalar tail) keeps gelu_bwd1.
__device__ __forceinline__ float gelu_bwd1_pinned(float x, float g) {
#pragma clang fp contract(off)
  const float x2 = x * x;
  const float u = kA * __builtin_fmaf(kB * x2, x, x);
  const float t = tanh_fast(u);
  const float sech2 = __builtin_fmaf(-t, t, 1.f);
  const float du = kA * __builtin_fmaf(3.f * kB, x2, 1.f);
  return g * __builtin_fmaf(0.5f * x * sech2, du, 0.5f * (1.f + t));
}

template <typename T>
struct alignas(16) Pk {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

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

// An element of the backward's vector body.
template <typename T>
__device__ __forceinline__ float gelu_bwd_vec1(float x, float g) {
  if constexpr (std::is_same<T, __hip_bfloat16>::value)
    return gelu_bwd1_pinned(x, g);
  else
    return gelu_bwd1(x, g);
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, long n) {
  constexpr int PK = Pk<T>::N;
  const long nvec = n / PK;
  const Pk<T>* xv = reinterpret_cast<const Pk<T>*>(x);
  Pk<T>* yv = reinterpret_cast<Pk<T>*>(y);
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    Pk<T> a = xv[i], o;
#pragma unroll
    for (int k = 0; k < PK; ++k) o.v[k] = from_f<T>(gelu_fwd1(to_f(a.v[k])));
    yv[i] = o;
  }
  for (long i = nvec * PK + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    y[i] = from_f<T>(gelu_fwd1(to_f(x[i])));
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    long n) {
  constexpr int PK = Pk<T>::N;
  const long nvec = n / PK;
  const Pk<T>* xv = reinterpret_cast<const Pk<T>*>(x);
  const Pk<T>* gv = reinterpret_cast<const Pk<T>*>(dy);
  Pk<T>* dv = reinterpret_cast<Pk<T>*>(dx);
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    Pk<T> a = xv[i], g = gv[i], o;
#pragma unroll
    for (int k = 0; k < PK; ++k)
      o.v[k] = from_f<T>(gelu_bwd_vec1<T>(to_f(a.v[k]), to_f(g.v[k])));
    dv[i] = o;
  }
  for (long i = nvec * PK + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    dx[i] = from_f<T>(gelu_bwd1(to_f(x[i]), to_f(dy[i])));
}

// x, dy, dx: [rows, COLS]; ws: [gridDim.x, COLS] fp32, one partial row per
// block. In chunk s a lane holds vector s * 64 + lane of the row.
template <typename T, int COLS>
__global__ __launch_bounds__(256) void gelu_bwd_bias_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    float* __restrict__ ws, long rows) {
  constexpr int PK = Pk<T>::N;
  static_assert(COLS % PK == 0, "COLS must be vector-divisible");
  constexpr int kVecs = COLS / PK;
  constexpr int kChunks = (kVecs + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wave_stride = (long)gridDim.x * 4;

  float acc[kChunks * PK];
#pragma unroll
  for (int i = 0; i < kChunks * PK; ++i) acc[i] = 0.f;

  for (long row = (long)blockIdx.x * 4 + wave; row < rows;
       row += wave_stride) {
    const Pk<T>* xv = reinterpret_cast<const Pk<T>*>(x + row * COLS);
    const Pk<T>* gv = reinterpret_cast<const Pk<T>*>(dy + row * COLS);
    Pk<T>* dv = reinterpret_cast<Pk<T>*>(dx + row * COLS);
#pragma unroll
    for (int s = 0; s < kChunks; ++s) {
      const int vi = s * 64 + lane;
      if (vi < kVecs) {
        const Pk<T> a = xv[vi], g = gv[vi];
        Pk<T> o;
#pragma unroll
        for (int k = 0; k < PK; ++k) {
          o.v[k] = from_f<T>(gelu_bwd1_pinned(to_f(a.v[k]), to_f(g.v[k])));
          acc[s * PK + k] += to_f(o.v[k]);
        }
        dv[vi] = o;
      }
    }
  }

  // the block's four waves add up in LDS in wave order (a fixed order),
  // then the block writes its one partial row
  __shared__ __attribute__((aligned(16))) float red[COLS];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int s = 0; s < kChunks; ++s) {
        const int vi = s * 64 + lane;
        if (vi < kVecs) {
#pragma unroll
          for (int k = 0; k < PK; ++k)
            red[vi * PK + k] =
                w == 0 ? acc[s * PK + k] : red[vi * PK + k] + acc[s * PK + k];
        }
      }
    }
    __syncthreads();
  }
  float* wr = ws + (long)blockIdx.x * COLS;
  for (int i = threadIdx.x * 4; i < COLS; i += 1024)
    *reinterpret_cast<float4*>(wr + i) =
        *reinterpret_cast<const float4*>(red + i);
}

template <typename T>
void gelu_bwd_bias_dispatch(const void* x, const void* dy, void* dx,
                            float* ws, long rows, long cols, int nblocks,
                            hipStream_t stream) {
#define GELU_BIAS_CASE(C)                                                  \
  if (cols == C) {                                                         \
    hipLaunchKernelGGL((gelu_bwd_bias_kernel<T, C>), dim3(nblocks),        \
                       dim3(256), 0, stream, (const T*)x, (const T*)dy,    \
                       (T*)dx, ws, rows);                                  \
    return;                                                                \
  }
  LN_COLS_LIST(GELU_BIAS_CASE)
#undef GELU_BIAS_CASE
  throw std::runtime_error("gelu_backward_bias: unsupported cols=" +
                           std::to_string(cols) +
                           " (check gelu_bias_supported first)");
}

}  // namespace

static dim3 ew_grid(long n) {
  long blocks = (n / 8 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

void gelu_forward(int dtype, const void* x, void* y, long n,
                  hipStream_t stream) {
  switch ((Dtype)dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((gelu_fwd_kernel<float>), ew_grid(n), dim3(256), 0,
                         stream, (const float*)x, (float*)y, n);
      return;
    case Dtype::F16:
      hipLaunchKernelGGL((gelu_fwd_kernel<__half>), ew_grid(n), dim3(256), 0,
                         stream, (const __half*)x, (__half*)y, n);
      return;
    case Dtype::BF16:
      hipLaunchKernelGGL((gelu_fwd_kernel<__hip_bfloat16>), ew_grid(n),
                         dim3(256), 0, stream, (const __hip_bfloat16*)x,
                         (__hip_bfloat16*)y, n);
      return;
  }
  throw std::runtime_error("gelu_forward: bad dtype");
}

void gelu_backward(int dtype, const void* x, const void* dy, void* dx, long n,
                   hipStream_t stream) {
  switch ((Dtype)dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((gelu_bwd_kernel<float>), ew_grid(n), dim3(256), 0,
                         stream, (const float*)x, (const float*)dy,
                         (float*)dx, n);
      return;
    case Dtype::F16:
      hipLaunchKernelGGL((gelu_bwd_kernel<__half>), ew_grid(n), dim3(256), 0,
                         stream, (const __half*)x, (const __half*)dy,
                         (__half*)dx, n);
      return;
    case Dtype::BF16:
      hipLaunchKernelGGL((gelu_bwd_kernel<__hip_bfloat16>), ew_grid(n),
                         dim3(256), 0, stream, (const __hip_bfloat16*)x,
                         (const __hip_bfloat16*)dy, (__hip_bfloat16*)dx, n);
      return;
  }
  throw std::runtime_error("gelu_backward: bad dtype");
}

// What gelu_backward_bias takes: LayerNorm's widths in bf16. gelu_bwd1_pinned
// is gelu_bwd_kernel's arithmetic as compiled for bf16; the f32 and f16
// instantiations of that kernel fuse differently, so those dtypes keep the
// plain backward (and torch's column sum).
bool gelu_bias_supported(long cols, int dtype) {
  if ((Dtype)dtype != Dtype::BF16) return false;
#define GELU_BIAS_CHECK(C) if (cols == C) return true;
  LN_COLS_LIST(GELU_BIAS_CHECK)
#undef GELU_BIAS_CHECK
  return false;
}

// dx as gelu_backward's, plus ws [nblocks, cols] fp32: per-block column
// sums of dx as rounded to the dtype. rows >= 1, 1 <= nblocks <= ceil(rows/4).
void gelu_backward_bias(int dtype, const void* x, const void* dy, void* dx,
                        float* ws, long rows, long cols, int nblocks,
                        hipStream_t stream) {
  if (rows < 1 || nblocks < 1 || nblocks > (rows + 3) / 4)
    throw std::runtime_error("gelu_backward_bias: need rows >= 1 and "
                             "1 <= nblocks <= ceil(rows / 4)");
  if ((Dtype)dtype == Dtype::BF16) {
    gelu_bwd_bias_dispatch<__hip_bfloat16>(x, dy, dx, ws, rows, cols, nblocks,
                                           stream);
    return;
  }
  throw std::runtime_error("gelu_backward_bias: bf16 only");
}

}  // namespace adapcc

// Column sums of partial rows (CDNA4 / gfx950).
//
// ln_bwd_kernel leaves one fp32 partial row per wave, gelu_bwd_bias_kernel
// one per block, in a [nslots, cols] workspace; the parameter gradient is
// its column sum. torch took one reduce_kernel launch per workspace and a
// cast kernel after each: 100 small launches per GPT-2 step for the 25
// LayerNorms alone. One launch here folds up to three workspaces of one
// shape and writes the parameter dtype directly.
//
// A 1024-thread workgroup owns 32 columns of one workspace (128 B of each
// partial row) and splits the slots 128 ways: a thread sums every 128th slot
// of its four columns in slot order, then the 128 partial sums meet in an
// LDS tree. The order is fixed, so the result is the same on every run; no
// atomics.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace adapcc {

namespace {

constexpr int kFoldCols = 32;     // columns per workgroup
constexpr int kFoldLanes = 8;     // float4 lanes across them
constexpr int kFoldGroups = 128;  // slot groups per workgroup

struct FoldArgs {
  const float* in[3];
  void* out[3];
};

__device__ __forceinline__ void fold_store(float* o, float v) { *o = v; }
__device__ __forceinline__ void fold_store(__half* o, float v) {
  *o = __float2half(v);
}
__device__ __forceinline__ void fold_store(__hip_bfloat16* o, float v) {
  *o = __float2bfloat16(v);
}

// grid (ceil(cols / 32), arrays); cols % 4 == 0.
template <typename T>
__global__ __launch_bounds__(1024) void colsum_fold_kernel(FoldArgs a,
                                                           long nslots,
                                                           long cols) {
  const float* __restrict__ src = a.in[blockIdx.y];
  T* __restrict__ dst = static_cast<T*>(a.out[blockIdx.y]);
  const int cl = threadIdx.x % kFoldLanes;
  const int sg = threadIdx.x / kFoldLanes;
  const long c = (long)blockIdx.x * kFoldCols + cl * 4;
  const bool live = c < cols;  // then c + 3 < cols too

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
#pragma unroll 4
    for (long s = sg; s < nslots; s += kFoldGroups) {
      const float4 v = *reinterpret_cast<const float4*>(src + s * cols + c);
      acc.x += v.x;
      acc.y += v.y;
      acc.z += v.z;
      acc.w += v.w;
    }
  }

  __shared__ float4 part[kFoldGroups][kFoldLanes];
  part[sg][cl] = acc;
  __syncthreads();
#pragma unroll
  for (int h = kFoldGroups / 2; h > 0; h >>= 1) {
    if (sg < h) {
      const float4 o = part[sg + h][cl];
      float4 m = part[sg][cl];
      m.x += o.x;
      m.y += o.y;
      m.z += o.z;
      m.w += o.w;
      part[sg][cl] = m;
    }
    __syncthreads();
  }
  if (sg == 0 && live) {
    const float4 r = part[0][cl];
    fold_store(dst + c, r.x);
    fold_store(dst + c + 1, r.y);
    fold_store(dst + c + 2, r.z);
    fold_store(dst + c + 3, r.w);
  }
}

}  // namespace

// Sums each [nslots, cols] fp32 array a_i down its columns into the [cols]
// output o_i of out_dtype. a0/o0 are required; a1/o1 and a2/o2 may be null
// (in pairs). cols % 4 == 0.
void colsum_fold(int out_dtype, const float* a0, const float* a1,
                 const float* a2, void* o0, void* o1, void* o2, long nslots,
                 long cols, hipStream_t stream) {
  if (nslots < 1 || cols < 4 || cols % 4 != 0)
    throw std::runtime_error("colsum_fold: need nslots >= 1 and cols a "
                             "positive multiple of 4, got " +
                             std::to_string(nslots) + " x " +
                             std::to_string(cols));
  const float* in[3] = {a0, a1, a2};
  void* out[3] = {o0, o1, o2};
  FoldArgs args = {};
  unsigned n = 0;
  for (int i = 0; i < 3; ++i) {
    if ((in[i] == nullptr) != (out[i] == nullptr))
      throw std::runtime_error("colsum_fold: array without its output");
    if (in[i] == nullptr) continue;
    args.in[n] = in[i];
    args.out[n] = out[i];
    ++n;
  }
  if (n == 0) throw std::runtime_error("colsum_fold: no array");
  const dim3 grid((unsigned)((cols + kFoldCols - 1) / kFoldCols), n);
  const dim3 block(kFoldLanes * kFoldGroups);
  switch ((Dtype)out_dtype) {
    case Dtype::F32:
      hipLaunchKernelGGL((colsum_fold_kernel<float>), grid, block, 0, stream,
                         args, nslots, cols);
      return;
    case Dtype::F16:
      hipLaunchKernelGGL((colsum_fold_kernel<__half>), grid, block, 0, stream,
                         args, nslots, cols);
      return;
    case Dtype::BF16:
      hipLaunchKernelGGL((colsum_fold_kernel<__hip_bfloat16>), grid, block, 0,
                         stream, args, nslots, cols);
      return;
  }
  throw std::runtime_error("colsum_fold: bad dtype " +
                           std::to_string(out_dtype));
}

}  // namespace adapcc

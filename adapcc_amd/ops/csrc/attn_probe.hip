// Probe kernels for the hardware-layout layer in attn_frag.h: each runs one
// helper on a known pattern so a GPU test can verify the lane->element maps
// independently of the attention kernels.

#include "attn_frag.h"

namespace adapcc {

namespace {

// tr-read probe: fill a swizzled row image with X[k][d] = k*64+d (bf16),
// run read_tr_frag for (kb, db) and dump each lane's 8 fragment elements
// -> out[lane][e]; a test checks lane l elem e == X[kb*16+8*(l>>5)+e][db*32+(l&31)].
__global__ void tr_probe_kernel(float* out, int kb, int db) {
  __shared__ __attribute__((aligned(16))) char img[4096];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 2048; i += 64) {
    const int k = i / 64, d = i % 64;
    *reinterpret_cast<__bf16*>(img + row_img_byte(k, d)) =
        (__bf16)(float)(k * 64 + d);
  }
  __syncthreads();
  bf16x8 f = read_tr_frag(img, lane, kb, db);
  union {
    bf16x8 v;
    __bf16 e[8];
  } u;
  u.v = f;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[lane * 8 + e] = (float)u.e[e];
}

// pack probe: lane provides p[r] = lane*100 + r; dump the packed fragment.
__global__ void pack_probe_kernel(float* out) {
  const int lane = threadIdx.x & 63;
  float p[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) p[r] = (float)(lane * 100 + r);
  bf16x8 f = pack_frag(p);
  union {
    bf16x8 v;
    __bf16 e[8];
  } u;
  u.v = f;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[lane * 8 + e] = (float)u.e[e];
}

// MFMA layout probe: C = A·B for one 32x32x16 tile with the documented
// fragment mappings.
__global__ void mfma_probe_kernel(const __bf16* a, const __bf16* b, float* c) {
  const int lane = threadIdx.x & 63;
  union {
    __bf16 e[8];
    bf16x8 f;
  } af, bf;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    af.e[e] = a[(lane % 32) * 16 + 8 * (lane / 32) + e];   // A[i][k]
    bf.e[e] = b[(8 * (lane / 32) + e) * 32 + (lane % 32)]; // B[k][j]
  }
  f32x16 acc = {};
  acc = mfma(af.f, bf.f, acc);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    c[crow(r, lane >> 5) * 32 + (lane % 32)] = acc[r];
}

}  // namespace

// Host launchers (bound in bindings.hip).
void mfma_probe(const void* a, const void* b, float* c, hipStream_t stream) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
                     (const __bf16*)a, (const __bf16*)b, c);
}

void tr_probe(float* out, int kb, int db, hipStream_t stream) {
  hipLaunchKernelGGL(tr_probe_kernel, dim3(1), dim3(64), 0, stream, out, kb,
                     db);
}

void pack_probe(float* out, hipStream_t stream) {
  hipLaunchKernelGGL(pack_probe_kernel, dim3(1), dim3(64), 0, stream, out);
}

}  // namespace adapcc

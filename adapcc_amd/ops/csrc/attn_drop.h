// Attention-dropout mask of the CDNA4 flash attention: one pure function
// keep(seed, bh, q, k) that the forward, the dq kernel, the dkv kernel and
// the fa_dropout_mask kernel all call, so the mask never depends on tiling,
// lane layout or which kernel asks. ops/attention.py holds the same
// arithmetic in torch integer ops (dropout_keep_mask_reference).
//
// A 32-bit word per (seed, plane bh = b*H + h, query row q, key row k); the
// element is kept iff word >= thr, thr = clamp(round(p * 2^32), 1, 2^32-1).
// All arithmetic is mod 2^32:
//   fmix(x): x^=x>>16; x*=0x85EBCA6B; x^=x>>13; x*=0xC2B2AE35; x^=x>>16
//   a = fmix(seed_lo + bh*0x9E3779B1 + q*0x85EBCA77)          per-q part
//   b = fmix((seed_hi ^ (bh*0xC2B2AE3D)) + k*0x27D4EB2F)      per-k part
//   x = a + b; x*=0x2C1B3C6D; x^=x>>15; x*=0x297A2D39; x^=x>>15
// The split lets a kernel compute the part of its lane-fixed axis once per
// lane and stage the part of the moving axis once per tile row; only the
// last line runs per element.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace adapcc {

__host__ __device__ __forceinline__ uint32_t drop_fmix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// seed_lo / seed_hi: the low and high 32 bits of the 64-bit seed.
__host__ __device__ __forceinline__ uint32_t drop_q_part(uint32_t seed_lo,
                                                         uint32_t bh,
                                                         uint32_t q) {
  return drop_fmix(seed_lo + bh * 0x9E3779B1u + q * 0x85EBCA77u);
}

__host__ __device__ __forceinline__ uint32_t drop_k_part(uint32_t seed_hi,
                                                         uint32_t bh,
                                                         uint32_t k) {
  return drop_fmix((seed_hi ^ (bh * 0xC2B2AE3Du)) + k * 0x27D4EB2Fu);
}

// The per-element word from the two parts.
__host__ __device__ __forceinline__ uint32_t drop_word(uint32_t a,
                                                       uint32_t b) {
  uint32_t x = a + b;
  x *= 0x2C1B3C6Du;
  x ^= x >> 15;
  x *= 0x297A2D39u;
  x ^= x >> 15;
  return x;
}

__host__ __device__ __forceinline__ bool drop_keep_parts(uint32_t a,
                                                         uint32_t b,
                                                         uint32_t thr) {
  return drop_word(a, b) >= thr;
}

__host__ __device__ __forceinline__ bool drop_keep(long seed, uint32_t bh,
                                                   uint32_t q, uint32_t k,
                                                   uint32_t thr) {
  const uint64_t s = (uint64_t)seed;
  return drop_keep_parts(drop_q_part((uint32_t)s, bh, q),
                         drop_k_part((uint32_t)(s >> 32), bh, k), thr);
}

}  // namespace adapcc

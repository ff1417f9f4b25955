// Hardware-layout layer of the CDNA4 flash attention (gfx950): the MFMA
// fragment maps, the C-register -> operand redistribution, and the swizzled
// LDS row image with its direct and hardware-transpose fragment reads.
// attn.hip builds the kernels on it; attn_probe.hip holds the probe kernels
// with which the GPU tests verify exactly this set on hardware.
//
// Layout conventions for v_mfma_f32_32x32x16_bf16 (verified on hardware by
// the mfma_probe test):
//   A[32x16]: lane l holds A[i = l%32][k = 8*(l/32) + e], e = 0..7
//   B[16x32]: lane l holds B[k = 8*(l/32) + e][j = l%32]
//   C[32x32]: lane l holds C[(r&3) + 8*(r>>2) + 4*(l>>5)][l%32], r = 0..15
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace adapcc {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// C-tile row of accumulator register r for this lane-half (l>>5).
__device__ __forceinline__ constexpr int crow(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// Redistribute 8 C-register f32 values (rows crow(o..o+7)) into one MFMA
// operand fragment holding elements k = 8*(l>>5) + (0..7) of the SAME
// lane-column: cvt_pk pairs then permlane32_swap exchanges the mismatched
// quartets between lane halves (guide T12). The s_nop covers the
// VALU-write -> v_permlane hazard window.
__device__ __forceinline__ bf16x8 pack_frag(const float* p) {
  unsigned a0, a1, b0, b1;
  asm volatile(
      "v_cvt_pk_bf16_f32 %0, %4, %5\n\t"
      "v_cvt_pk_bf16_f32 %1, %6, %7\n\t"
      "v_cvt_pk_bf16_f32 %2, %8, %9\n\t"
      "v_cvt_pk_bf16_f32 %3, %10, %11\n\t"
      "s_nop 1\n\t"
      "v_permlane32_swap_b32 %0, %2\n\t"
      "v_permlane32_swap_b32 %1, %3"
      : "=&v"(a0), "=&v"(a1), "=&v"(b0), "=&v"(b1)
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]),
        "v"(p[6]), "v"(p[7]));
  union {
    unsigned u[4];
    bf16x8 f;
  } r;
  r.u[0] = a0;
  r.u[1] = a1;
  r.u[2] = b0;
  r.u[3] = b1;
  return r.f;
}

// ---------------------------------------------------------------------------
// LDS images.
//
// Row image (K / Q / dO as direct row-major fragments): [32][64] bf16 with
// byte ^= ((row&7)<<4) XOR swizzle, read as 16-B ds_read_b128.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int row_img_byte(int row, int col_bf16) {
  return (row * 128 + col_bf16 * 2) ^ ((row & 7) << 4);
}

// A-or-B fragment read from a row image: lane l takes row (l&31), 8
// consecutive bf16 at column chunk*16 + (l>>5)*8.
__device__ __forceinline__ bf16x8 read_row_frag(const char* img, int lane,
                                                int chunk) {
  const int byte = row_img_byte(lane & 31, chunk * 16 + (lane >> 5) * 8);
  return *reinterpret_cast<const bf16x8*>(img + byte);
}

// Transpose fragments come straight from the SAME swizzled row image via
// ds_read_b64_tr_b16. Measured instruction semantics (tr2 probe, gfx950):
// within each 16-lane group, writing lane ids as 16g+4t+m (t,m in 0..3),
// destination lane 16g+4t+m element j receives
//     lds[ addr_supplied_by_lane(16g+4j+t) + m elements ]
// (addresses 8-B aligned; each source lane names one 4-element chunk).
// So lane s supplies the address of X[8*(s>>5) + 4r + ((s>>2)&3)]
//                                   [db*32 + 16*((s>>4)&1) + 4*(s&3)]
// and every lane l ends up with X[kb*16 + 8*(l>>5) + 4r + j][db*32 + (l&31)]
// in element 4r+j -- exactly the MFMA operand fragment of X^T. The 4-elem
// chunk is 8 B inside one 16-B slot, so the row image's XOR swizzle keeps
// it contiguous and aligned.
__device__ __forceinline__ int tr_addr_byte(int lane, int kb, int db, int r) {
  const int row = kb * 16 + r * 4 + 8 * (lane >> 5) + ((lane >> 2) & 3);
  const int col = db * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  return row_img_byte(row, col);
}

// Two tr reads -> one 8-element fragment: lane l holds X[8*(l>>5)+e][l&31]
// for k in [kb*16,+16), d in [db*32,+32), X^T-fragment oriented.
__device__ __forceinline__ bf16x8 read_tr_frag(const char* img, int lane,
                                               int kb, int db) {
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  union {
    bf16x4 h[2];
    bf16x8 f;
  } r;
  r.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_v4*)(img + tr_addr_byte(lane, kb, db, 0)));
  r.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_v4*)(img + tr_addr_byte(lane, kb, db, 1)));
  return r.f;
}

}  // namespace adapcc

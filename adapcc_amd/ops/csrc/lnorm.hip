// Fused LayerNorm for CDNA4 (gfx950) — forward + single-pass backward.
//
// Motivation (rocprof, GPT-2 small bf16 step): torch's LayerNorm stack is
// ~8% of step time and its backward reads (dy, x) twice (GradInput +
// PartGradGammaBeta). Here one wave64 owns one row: the row lives in
// registers between the statistics and normalize passes (COLS is a
// template parameter so all register indexing is static), cross-lane sums
// use shfl_xor, and the backward fuses dx with per-block dgamma/dbeta
// partials (single read of dy/x) accumulated in registers — each lane owns
// a fixed column set — and flushed once per wave; a tiny second kernel
// (colsum.hip) folds the per-wave partials.
//
// bf16/f16/f32 activations, fp32 statistics; instantiated for the common
// transformer widths (128..4096, divisible by the 16-byte vector width).
//
// ln_dropadd_*: the pre-norm residual step x_new = residual + dropout(h),
// y = LN(x_new) in one pass each way, as further instantiations of the two
// LayerNorm kernels. The forward rounds x_new to T and normalizes the
// rounded row by the code ln_fwd runs, so y is ln_fwd(x_new) bit for bit;
// the backward adds the gradient that reaches x_new directly to the LN
// input gradient before the one rounding and writes it as dresidual and,
// masked and scaled, as dh. The mask is attn_drop.h's keep(seed, site, row,
// col), regenerated in the backward and never stored: the column part is
// fixed per lane, the row part per row. The p = 0 instantiations carry no
// mask code.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include "attn_drop.h"
#include "common.h"
#include "ln_cols.h"

#include <stdexcept>
#include <string>

namespace adapcc {

#define DEV_INLINE __device__ __forceinline__

// attn.hip: the threshold its launcher puts beside attn_drop.h's word
unsigned fa_drop_threshold(double p);

namespace {

template <typename T> struct LnIo;
template <> struct LnIo<float> {
  using Vec = float4;
  static constexpr int kPerVec = 4;
  DEV_INLINE static void unpack(const Vec& v, float* o) {
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  DEV_INLINE static Vec pack(const float* i) {
    return make_float4(i[0], i[1], i[2], i[3]);
  }
};
template <> struct LnIo<__hip_bfloat16> {
  struct Vec { uint4 raw; };
  static constexpr int kPerVec = 8;
  DEV_INLINE static void unpack(const Vec& v, float* o) {
    const unsigned* w = reinterpret_cast<const unsigned*>(&v.raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __hip_bfloat162 h = *reinterpret_cast<const __hip_bfloat162*>(&w[i]);
      o[2 * i] = __bfloat162float(h.x);
      o[2 * i + 1] = __bfloat162float(h.y);
    }
  }
  DEV_INLINE static Vec pack(const float* i) {
    Vec v; unsigned* w = reinterpret_cast<unsigned*>(&v.raw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      __hip_bfloat162 h{__float2bfloat16(i[2 * k]),
                        __float2bfloat16(i[2 * k + 1])};
      w[k] = *reinterpret_cast<const unsigned*>(&h);
    }
    return v;
  }
};
template <> struct LnIo<__half> {
  struct Vec { uint4 raw; };
  static constexpr int kPerVec = 8;
  DEV_INLINE static void unpack(const Vec& v, float* o) {
    const unsigned* w = reinterpret_cast<const unsigned*>(&v.raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __half2 h = *reinterpret_cast<const __half2*>(&w[i]);
      o[2 * i] = __half2float(__low2half(h));
      o[2 * i + 1] = __half2float(__high2half(h));
    }
  }
  DEV_INLINE static Vec pack(const float* i) {
    Vec v; unsigned* w = reinterpret_cast<unsigned*>(&v.raw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      __half2 h = __floats2half2_rn(i[2 * k], i[2 * k + 1]);
      w[k] = *reinterpret_cast<const unsigned*>(&h);
    }
    return v;
  }
};

DEV_INLINE float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace

// Per-lane vector chunks for a COLS-wide row: ceil(COLS / (64*PV)) chunks;
// in chunk s, lanes with s*64 + lane < COLS/PV are active.
template <typename T, int COLS>
struct RowShape {
  using IO = LnIo<T>;
  static constexpr int PV = IO::kPerVec;
  static_assert(COLS % PV == 0, "COLS must be vector-divisible");
  static constexpr int kVecs = COLS / PV;             // 16B vectors per row
  static constexpr int kChunks = (kVecs + 63) / 64;   // per-lane chunks
  static constexpr int kElems = kChunks * PV;         // per-lane fp32 regs
};

// Residual dropout of the ln_dropadd entry points, by value. seed: one int64
// in device memory, read when the kernel runs; keep iff word >= thr, kept h
// times scale = 1/(1-p). Not touched at p = 0.
struct LnDrop {
  const long* seed;
  unsigned site;
  unsigned thr;
  float scale;
};

// r + h * scale with the product rounded before the sum, as written.
DEV_INLINE float ln_scaled_add(float r, float h, float scale) {
#pragma clang fp contract(off)
  return r + h * scale;
}

// The forward of ln_fwd and ln_dropadd_fwd. <false, false> is plain
// LayerNorm of x, and h, x_new and drop are not touched. kAdd: x is the
// residual, the row becomes x_new = round_to_T(x + (keep ? h * scale : 0))
// (kDrop) or round_to_T(x + h), is written out, and is normalized as T
// holds it by the code every instantiation shares: y is ln_fwd(x_new) bit
// for bit.
template <typename T, int COLS, bool kAdd, bool kDrop>
__global__ void __launch_bounds__(256) ln_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ b,
    T* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, long rows, float eps,
    const T* __restrict__ h, T* __restrict__ x_new, LnDrop drop) {
  static_assert(kAdd || !kDrop, "dropout acts on the added h");
  using RS = RowShape<T, COLS>;
  using IO = typename RS::IO;
  using Vec = typename IO::Vec;
  constexpr int PV = RS::PV;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= rows) return;

  uint32_t seed_hi = 0, ra = 0;
  if constexpr (kDrop) {
    const uint64_t sd = (uint64_t)*drop.seed;
    seed_hi = (uint32_t)(sd >> 32);
    ra = drop_q_part((uint32_t)sd, drop.site, (uint32_t)row);
  }

  const T* xr = x + row * COLS;
  float vals[RS::kElems];
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < RS::kChunks; ++s) {
    const int vi = s * 64 + lane;
    if (vi < RS::kVecs) {
      Vec v = reinterpret_cast<const Vec*>(xr)[vi];
      IO::unpack(v, &vals[s * PV]);
      if constexpr (kAdd) {
        float hv[PV];
        Vec vh = reinterpret_cast<const Vec*>(h + row * COLS)[vi];
        IO::unpack(vh, hv);
#pragma unroll
        for (int k = 0; k < PV; ++k) {
          if constexpr (kDrop) {
            // one row per wave: each column part is used once, so it is
            // computed in place. A dropped element keeps the residual's bits.
            const uint32_t cb =
                drop_k_part(seed_hi, drop.site, (uint32_t)(vi * PV + k));
            if (drop_keep_parts(ra, cb, drop.thr))
              vals[s * PV + k] =
                  ln_scaled_add(vals[s * PV + k], hv[k], drop.scale);
          } else {
            vals[s * PV + k] += hv[k];
          }
        }
        // the statistics see x_new as T holds it
        v = IO::pack(&vals[s * PV]);
        reinterpret_cast<Vec*>(x_new + row * COLS)[vi] = v;
        IO::unpack(v, &vals[s * PV]);
      }
#pragma unroll
      for (int k = 0; k < PV; ++k) sum += vals[s * PV + k];
    } else {
#pragma unroll
      for (int k = 0; k < PV; ++k) vals[s * PV + k] = 0.f;
    }
  }
  sum = wave_sum(sum);
  const float mean = sum / COLS;
  float var = 0.f;
#pragma unroll
  for (int s = 0; s < RS::kChunks; ++s) {
    if (s * 64 + lane < RS::kVecs) {
#pragma unroll
      for (int k = 0; k < PV; ++k) {
        const float d = vals[s * PV + k] - mean;
        var += d * d;
      }
    }
  }
  var = wave_sum(var);
  const float rstd = rsqrtf(var / COLS + eps);
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }

  T* yr = y + row * COLS;
#pragma unroll
  for (int s = 0; s < RS::kChunks; ++s) {
    const int vi = s * 64 + lane;
    if (vi < RS::kVecs) {
      float wv[PV], bv[PV], out[PV];
      Vec a = reinterpret_cast<const Vec*>(w)[vi];
      Vec c = reinterpret_cast<const Vec*>(b)[vi];
      IO::unpack(a, wv);
      IO::unpack(c, bv);
#pragma unroll
      for (int k = 0; k < PV; ++k)
        out[k] = (vals[s * PV + k] - mean) * rstd * wv[k] + bv[k];
      reinterpret_cast<Vec*>(yr)[vi] = IO::pack(out);
    }
  }
}

// The backward of ln_bwd and ln_dropadd_bwd. <false, false> is plain
// LayerNorm: dx is the LN input gradient, and dx_in, dh and drop are not
// touched. kAdd adds dx_in (the gradient that reaches x_new besides the
// LN) in fp32 before dx, there dresidual, is rounded; kDrop also writes
// dh = keep ? g * scale : 0 from the same fp32 g (at p = 0 dh is dx and is
// not written a second time).
template <typename T, int COLS, bool kAdd, bool kDrop>
__global__ void __launch_bounds__(256) ln_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const T* __restrict__ w, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, T* __restrict__ dx,
    float* __restrict__ ws_gamma, float* __restrict__ ws_beta, long rows,
    const T* __restrict__ dx_in, T* __restrict__ dh, LnDrop drop) {
  using RS = RowShape<T, COLS>;
  using IO = typename RS::IO;
  using Vec = typename IO::Vec;
  constexpr int PV = RS::PV;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wave_stride = (long)gridDim.x * 4;

  // each lane owns the same column set for every row it touches ->
  // dgamma/dbeta partials accumulate in registers, flushed once per wave
  float dg[RS::kElems];
  float db[RS::kElems];
#pragma unroll
  for (int i = 0; i < RS::kElems; ++i) dg[i] = db[i] = 0.f;

  // weight is row-invariant: load it once
  float wv[RS::kElems];
#pragma unroll
  for (int s = 0; s < RS::kChunks; ++s) {
    const int vi = s * 64 + lane;
    if (vi < RS::kVecs) {
      Vec v = reinterpret_cast<const Vec*>(w)[vi];
      IO::unpack(v, &wv[s * PV]);
    }
  }

  // so are the mask's column parts (1 dummy slot without dropout). The
  // 4096-wide rows fill the register file before them: their dropout
  // instantiations spill some 30 dwords per lane, with or without these.
  uint32_t cb[kDrop ? RS::kElems : 1];
  uint32_t seed_lo = 0;
  if constexpr (kDrop) {
    const uint64_t sd = (uint64_t)*drop.seed;
    seed_lo = (uint32_t)sd;
#pragma unroll
    for (int s = 0; s < RS::kChunks; ++s)
#pragma unroll
      for (int k = 0; k < PV; ++k)
        cb[s * PV + k] =
            drop_k_part((uint32_t)(sd >> 32), drop.site,
                        (uint32_t)((s * 64 + lane) * PV + k));
  }

  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += wave_stride) {
    const T* dyr = dy + row * COLS;
    const T* xr = x + row * COLS;
    const float mean = mean_in[row];
    const float rstd = rstd_in[row];

    float dyv[RS::kElems], xh[RS::kElems];
    Vec vin[kAdd ? RS::kChunks : 1];  // dx_in, issued with the other loads
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int s = 0; s < RS::kChunks; ++s) {
      const int vi = s * 64 + lane;
      if (vi < RS::kVecs) {
        float d[PV], xx[PV];
        Vec vd = reinterpret_cast<const Vec*>(dyr)[vi];
        Vec vx = reinterpret_cast<const Vec*>(xr)[vi];
        if constexpr (kAdd)
          vin[s] = reinterpret_cast<const Vec*>(dx_in + row * COLS)[vi];
        IO::unpack(vd, d);
        IO::unpack(vx, xx);
#pragma unroll
        for (int k = 0; k < PV; ++k) {
          const float xhat = (xx[k] - mean) * rstd;
          const float a = d[k] * wv[s * PV + k];
          dyv[s * PV + k] = d[k];
          xh[s * PV + k] = xhat;
          s1 += a;
          s2 += a * xhat;
        }
      }
    }
    s1 = wave_sum(s1) / COLS;
    s2 = wave_sum(s2) / COLS;

    T* dxr = dx + row * COLS;
    uint32_t ra = 0;
    if constexpr (kDrop) ra = drop_q_part(seed_lo, drop.site, (uint32_t)row);
#pragma unroll
    for (int s = 0; s < RS::kChunks; ++s) {
      const int vi = s * 64 + lane;
      if (vi < RS::kVecs) {
        float out[PV];
#pragma unroll
        for (int k = 0; k < PV; ++k) {
          const float a = dyv[s * PV + k] * wv[s * PV + k];
          out[k] = (a - s1 - xh[s * PV + k] * s2) * rstd;
          dg[s * PV + k] += dyv[s * PV + k] * xh[s * PV + k];
          db[s * PV + k] += dyv[s * PV + k];
        }
        if constexpr (kAdd) {
          float gin[PV];
          IO::unpack(vin[s], gin);
#pragma unroll
          for (int k = 0; k < PV; ++k) out[k] += gin[k];
        }
        reinterpret_cast<Vec*>(dxr)[vi] = IO::pack(out);
        if constexpr (kDrop) {
#pragma unroll
          for (int k = 0; k < PV; ++k)
            out[k] = drop_keep_parts(ra, cb[s * PV + k], drop.thr)
                         ? out[k] * drop.scale
                         : 0.f;
          reinterpret_cast<Vec*>(dh + row * COLS)[vi] = IO::pack(out);
        }
      }
    }
  }

  // flush per-wave partials (one slot per wave, no atomics); each lane's
  // PV floats are contiguous -> vectorized float4 stores
  const long slot = (long)blockIdx.x * 4 + wave;
  float* wg = ws_gamma + slot * COLS;
  float* wb = ws_beta + slot * COLS;
#pragma unroll
  for (int s = 0; s < RS::kChunks; ++s) {
    const int vi = s * 64 + lane;
    if (vi < RS::kVecs) {
#pragma unroll
      for (int q = 0; q < PV / 4; ++q) {
        reinterpret_cast<float4*>(wg + vi * PV)[q] =
            make_float4(dg[s * PV + 4 * q], dg[s * PV + 4 * q + 1],
                        dg[s * PV + 4 * q + 2], dg[s * PV + 4 * q + 3]);
        reinterpret_cast<float4*>(wb + vi * PV)[q] =
            make_float4(db[s * PV + 4 * q], db[s * PV + 4 * q + 1],
                        db[s * PV + 4 * q + 2], db[s * PV + 4 * q + 3]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------

bool ln_supported_api(long cols, int dtype) {
  const int pv = dtype_size((Dtype)dtype) == 4 ? 4 : 8;
  if (cols % pv) return false;
#define LN_CHECK(C) if (cols == C) return true;
  LN_COLS_LIST(LN_CHECK)
#undef LN_CHECK
  return false;
}

namespace {

// The kernels' arguments; h, x_new, dx_in, dh and drop belong to the
// ln_dropadd entry points and stay null / empty for plain LayerNorm.
struct LnFwdArgs {
  const void *x, *w, *b;
  void* y;
  float *mean, *rstd;
  long rows, cols;
  float eps;
  const void* h;
  void* x_new;
  LnDrop drop;
};

struct LnBwdArgs {
  const void *dy, *x, *w;
  const float *mean, *rstd;
  void* dx;
  float *ws_gamma, *ws_beta;
  long rows, cols;
  int nblocks;
  const void* dx_in;
  void* dh;
  LnDrop drop;
};

template <typename T, bool kAdd, bool kDrop>
void ln_fwd_dispatch(const LnFwdArgs& a, hipStream_t s) {
  const dim3 block(256);
  const dim3 grid((a.rows + 3) / 4);
#define LN_FWD_CASE(C)                                                      \
  if (a.cols == C) {                                                        \
    hipLaunchKernelGGL((ln_fwd_kernel<T, C, kAdd, kDrop>), grid, block, 0,  \
                       s, (const T*)a.x, (const T*)a.w, (const T*)a.b,      \
                       (T*)a.y, a.mean, a.rstd, a.rows, a.eps,              \
                       (const T*)a.h, (T*)a.x_new, a.drop);                 \
    return;                                                                 \
  }
  LN_COLS_LIST(LN_FWD_CASE)
#undef LN_FWD_CASE
  throw std::runtime_error("ln_forward: unsupported cols=" +
                           std::to_string(a.cols) +
                           " (check ln_supported first)");
}

template <typename T, bool kAdd, bool kDrop>
void ln_bwd_dispatch(const LnBwdArgs& a, hipStream_t s) {
  const dim3 block(256);
#define LN_BWD_CASE(C)                                                      \
  if (a.cols == C) {                                                        \
    hipLaunchKernelGGL((ln_bwd_kernel<T, C, kAdd, kDrop>),                  \
                       dim3(a.nblocks), block, 0, s, (const T*)a.dy,        \
                       (const T*)a.x, (const T*)a.w, a.mean, a.rstd,        \
                       (T*)a.dx, a.ws_gamma, a.ws_beta, a.rows,             \
                       (const T*)a.dx_in, (T*)a.dh, a.drop);                \
    return;                                                                 \
  }
  LN_COLS_LIST(LN_BWD_CASE)
#undef LN_BWD_CASE
  throw std::runtime_error("ln_backward: unsupported cols=" +
                           std::to_string(a.cols) +
                           " (check ln_supported first)");
}

// drop: dropout_p > 0; the add is there when its operand is.
template <typename T>
void ln_fwd_typed(const LnFwdArgs& a, bool drop, hipStream_t s) {
  if (a.h == nullptr)
    ln_fwd_dispatch<T, false, false>(a, s);
  else if (drop)
    ln_fwd_dispatch<T, true, true>(a, s);
  else
    ln_fwd_dispatch<T, true, false>(a, s);
}

template <typename T>
void ln_bwd_typed(const LnBwdArgs& a, bool drop, hipStream_t s) {
  const bool add = a.dx_in != nullptr;
  if (drop && add)
    ln_bwd_dispatch<T, true, true>(a, s);
  else if (drop)
    ln_bwd_dispatch<T, false, true>(a, s);
  else if (add)
    ln_bwd_dispatch<T, true, false>(a, s);
  else
    ln_bwd_dispatch<T, false, false>(a, s);
}

void ln_fwd_any(int dtype, const LnFwdArgs& a, bool drop, hipStream_t s) {
  switch ((Dtype)dtype) {
    case Dtype::F32: ln_fwd_typed<float>(a, drop, s); break;
    case Dtype::BF16: ln_fwd_typed<__hip_bfloat16>(a, drop, s); break;
    case Dtype::F16: ln_fwd_typed<__half>(a, drop, s); break;
  }
}

void ln_bwd_any(int dtype, const LnBwdArgs& a, bool drop, hipStream_t s) {
  switch ((Dtype)dtype) {
    case Dtype::F32: ln_bwd_typed<float>(a, drop, s); break;
    case Dtype::BF16: ln_bwd_typed<__hip_bfloat16>(a, drop, s); break;
    case Dtype::F16: ln_bwd_typed<__half>(a, drop, s); break;
  }
}

// The mask's row word is 32 bits wide; thr as the attention launcher's.
LnDrop ln_drop_args(const char* name, long rows, double p, const long* seed,
                    unsigned site) {
  if (rows < 1 || rows >= (1L << 32))
    throw std::runtime_error(std::string(name) + ": need 1 <= rows < 2^32");
  if (!(p >= 0.0 && p < 1.0))
    throw std::runtime_error(std::string(name) + ": need 0 <= dropout_p < 1");
  if (p > 0.0 && seed == nullptr)
    throw std::runtime_error(std::string(name) +
                             ": dropout needs a device seed");
  return LnDrop{seed, site, fa_drop_threshold(p), (float)(1.0 / (1.0 - p))};
}

}  // namespace

void ln_forward(int dtype, const void* x, const void* w, const void* b,
                void* y, float* mean, float* rstd, long rows, long cols,
                float eps, hipStream_t stream) {
  ln_fwd_any(dtype,
             {x, w, b, y, mean, rstd, rows, cols, eps, nullptr, nullptr, {}},
             false, stream);
}

void ln_backward(int dtype, const void* dy, const void* x, const void* w,
                 const float* mean, const float* rstd, void* dx,
                 float* ws_gamma, float* ws_beta, long rows, long cols,
                 int nblocks, hipStream_t stream) {
  ln_bwd_any(dtype,
             {dy, x, w, mean, rstd, dx, ws_gamma, ws_beta, rows, cols, nblocks,
              nullptr, nullptr, {}},
             false, stream);
}

// x_new = round_to_T(res + dropout(h)), y = LN(x_new); dropout_p > 0 reads
// the 64-bit seed at `seed` (device memory) when the kernel runs.
void ln_dropadd_forward(int dtype, const void* h, const void* res,
                        const void* w, const void* b, void* x_new, void* y,
                        float* mean, float* rstd, long rows, long cols,
                        float eps, double dropout_p, const long* seed,
                        unsigned site, hipStream_t stream) {
  const LnDrop drop =
      ln_drop_args("ln_dropadd_forward", rows, dropout_p, seed, site);
  if (h == nullptr || x_new == nullptr)
    throw std::runtime_error("ln_dropadd_forward: null h or x_new");
  ln_fwd_any(dtype,
             {res, w, b, y, mean, rstd, rows, cols, eps, h, x_new, drop},
             dropout_p > 0.0, stream);
}

// dx_new may be null (no gradient reaches x_new but through the LN); dh is
// written only at dropout_p > 0, where it must not be null.
void ln_dropadd_backward(int dtype, const void* dy, const void* dx_new,
                         const void* x_new, const void* w, const float* mean,
                         const float* rstd, void* dres, void* dh,
                         float* ws_gamma, float* ws_beta, long rows,
                         long cols, int nblocks, double dropout_p,
                         const long* seed, unsigned site,
                         hipStream_t stream) {
  const LnDrop drop =
      ln_drop_args("ln_dropadd_backward", rows, dropout_p, seed, site);
  if (dropout_p > 0.0 && dh == nullptr)
    throw std::runtime_error("ln_dropadd_backward: dropout needs dh");
  if (nblocks < 1)
    throw std::runtime_error("ln_dropadd_backward: nblocks < 1");
  ln_bwd_any(dtype,
             {dy, x_new, w, mean, rstd, dres, ws_gamma, ws_beta, rows, cols,
              nblocks, dx_new, dh, drop},
             dropout_p > 0.0, stream);
}

}  // namespace adapcc


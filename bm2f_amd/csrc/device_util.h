// Device primitives shared by the HIP kernels: vector types, element traits, the 64-lane sum, the typed logit
// load, the hardware-exp2 pairwise-loss family and a few MFMA / LDS / scheduling one-liners.  Header-only, no
// state; every function is compiled under the including file's flags.
//
// Parity tests pin the rounding of these forms and the determinism claims of their callers rest on wave_sum's
// order, so a kernel file includes this header and does not restate them.  Deliberately NOT here:
//   - point_sample.hip's sigmoid / softplus (expf / log1pf with an IEEE divide: the mask criterion's own bars);
//   - decoder.hip's wave_sum16 / wave_max16 and window_attn.hip's wave_sum4 / wave_max4 (partial reductions on
//     the permlane-swap path, not the 64-lane sum);
//   - block_sum of gnorm.hip and msda_generic.hip: gnorm's barriers sit before the LDS write and before the read (fp64,
//     fixed 256 threads), msda's after the write and after the read (templated type and block size), so the two
//     make different promises about when `red` may be reused -- they are not one function.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bm2f.h"

namespace m2f {

// vector types (MFMA operands / accumulators and 16-byte accesses)
using f4 = float __attribute__((ext_vector_type(4)));
using f16v = float __attribute__((ext_vector_type(16)));
using s4 = short __attribute__((ext_vector_type(4)));
using s8 = short __attribute__((ext_vector_type(8)));
using h8 = _Float16 __attribute__((ext_vector_type(8)));
using bf8 = __bf16 __attribute__((ext_vector_type(8)));
using lds_s4 = __attribute__((address_space(3))) s4;

// element traits: fp32 <-> storage type (round-to-nearest-even on the way down); files build their MFMA
// selectors on top of it
template <typename T> struct Elt;
template <> struct Elt<float> {
  static constexpr bool k16 = false;
  __device__ __forceinline__ static float to_f(float x) { return x; }
  __device__ __forceinline__ static float from_f(float x) { return x; }
};
template <> struct Elt<__bf16> {
  static constexpr bool k16 = true;
  __device__ __forceinline__ static float to_f(__bf16 x) { return static_cast<float>(x); }
  __device__ __forceinline__ static __bf16 from_f(float x) { return static_cast<__bf16>(x); }
};
template <> struct Elt<_Float16> {
  static constexpr bool k16 = true;
  __device__ __forceinline__ static float to_f(_Float16 x) { return static_cast<float>(x); }
  __device__ __forceinline__ static _Float16 from_f(float x) { return static_cast<_Float16>(x); }
};

// element i of a fp32 / fp16 / bf16 buffer (dtype: M2F_F32 / M2F_F16 / M2F_BF16) as fp32, an exact conversion
__device__ __forceinline__ float load_logit(const void* __restrict__ p, int dtype, int64_t i) {
  switch (dtype) {
    case M2F_F16: return static_cast<float>(static_cast<const _Float16*>(p)[i]);
    case M2F_BF16: return static_cast<float>(static_cast<const __bf16*>(p)[i]);
    default: return static_cast<const float*>(p)[i];
  }
}

// Sum over the 64 lanes, the result in every lane.  The xor-butterfly order 32, 16, ... 1 is fixed: callers
// document bitwise repeatability that depends on it.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// v[j] for a run-time j in 0..3 as selects, so v stays in registers (a dynamic index would go through scratch)
__device__ __forceinline__ float pick4(const float (&v)[4], int j) {
  return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
}

// exact fp32 32x32x2 MFMA step
__device__ __forceinline__ f16v mfma32(float a, float b, f16v c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Transposed 4x16 read: lane 4q+p of each 16-lane group passes the address of row q, columns 4p..4p+3 of
// its block; lane i receives column i of the 4 rows (row q in element q).
__device__ __forceinline__ s4 tr_read(const void* lds_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(reinterpret_cast<uintptr_t>(lds_ptr)));
}

// bijective XCD-aware remap: consecutive logical ids land on the same XCD (blocks id, id+8, ... share one)
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = id % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + id / 8;
}

// pairwise-loss math on the hardware exp2 / log2, shared by the spatial (weaksup.hip) and temporal
// (video_pairs.hip) losses so that the two round alike
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// log(1 + exp(t)) for t <= 0 on the raw hardware exp2/log2 (one v_exp_f32 + one v_log_f32; 1 + e lies in
// [1, 2], so no denormal range fix-ups are needed)
__device__ __forceinline__ float softplus_neg(float t) {
  return kLn2 * __builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(t * kLog2e));
}

__device__ __forceinline__ float log_sigmoid(float x) {  // F.logsigmoid: min(x,0) - log1p(exp(-|x|))
  return fminf(x, 0.f) - softplus_neg(-fabsf(x));
}

// s(a,b) = -log(sig(a)sig(b) + sig(-a)sig(-b)) = -(logsig(a) + logsig(b) + softplus(-(a+b))): the
// reference's log-space form (criterion.py:175-179, with logsig(-x) = logsig(x) - x) reduced to one
// softplus per pair; fa = log_sigmoid(a), fb = log_sigmoid(b) come from the caller, which may have staged them.
__device__ __forceinline__ float pair_term(float a, float fa, float b, float fb) {
  const float z = a + b;
  return -(fa + fb + fmaxf(-z, 0.f) + softplus_neg(-fabsf(z)));
}

__device__ __forceinline__ float sigmoid_neg(float t) {  // sig(-t), accurate in both tails
  const float e = __builtin_amdgcn_exp2f(-fabsf(t) * kLog2e);
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return t >= 0.f ? e * r : r;
}

// d s(a, b) / d a = sig(-(a+b)) - sig(-a), sna = sigmoid_neg(a)
__device__ __forceinline__ float pair_grad(float a, float sna, float b) { return sigmoid_neg(a + b) - sna; }

}  // namespace m2f

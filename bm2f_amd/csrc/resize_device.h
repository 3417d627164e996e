// Device-side geometry of the inference heads' "full-resolution mask logit" (inference.hip).
//
// The value of query q at output pixel (y, x) of one image is defined by the reference's eval branch
// (maskformer_model.py:337-342, :355-357):
//   1. F.interpolate((h, w) -> (Hp, Wp), bilinear, align_corners=False)        the padded batch size
//   2. crop to the image's (Hc, Wc)                                             sem_seg_postprocess
//   3. F.interpolate((Hc, Wc) -> (Ho, Wo), bilinear, align_corners=False)       skipped when equal
// Each interpolate is torch's upsample_bilinear2d formula evaluated literally (contraction off, as
// attn_mask_bits_kernel in decoder.hip does): src = max(scale*(dst+0.5)-0.5, 0), i0 = (int)src,
// i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1, v = ly0*(lx0*a + lx1*b) + ly1*(lx0*c + lx1*d).
// With step 3 active the value is a 4-tap blend of four 4-tap values, each rounded to fp32 as torch
// stores the intermediate image.
//
// Logits may be fp32, fp16 or bf16: they are converted to fp32 on load and everything after is fp32.
// For 16-bit logits the definition of correct is therefore "the reference run on logits.float()",
// which is deliberately more accurate than the reference run in half precision.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bm2f.h"
#include "device_util.h"  // load_logit: the typed load behind every ld(row, col)

namespace m2f {

struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap bilinear_tap(int dst, float scale, int in) {
#pragma clang fp contract(off)
  float s = scale * (static_cast<float>(dst) + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  Tap t;
  t.i0 = min(static_cast<int>(s), in - 1);
  t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
  t.l1 = s - static_cast<float>(t.i0);
  t.l0 = 1.f - t.l1;
  return t;
}

__device__ __forceinline__ float blend4(float ly0, float ly1, float lx0, float lx1, float a, float b, float c,
                                        float d) {
#pragma clang fp contract(off)
  return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}

__device__ __forceinline__ float sigmoidf_literal(float v) {
#pragma clang fp contract(off)
  return 1.f / (1.f + expf(-v));
}

// One image's geometry, from the (B, 4) int32 device table [Hc, Wc, Ho, Wo] clamped to the buffers:
// a bad table can make an image empty (Ho or Wo <= 0) but never an out-of-bounds access.
struct Geo {
  int h, w, Hc, Wc, Ho, Wo;
  bool two;
  float rh1, rw1, rh2, rw2;
};

__device__ __forceinline__ Geo load_geo(const int32_t* __restrict__ sizes, int b, int h, int w, int Hp, int Wp,
                                        int out_h, int out_w) {
  Geo g;
  g.h = h;
  g.w = w;
  g.Hc = max(1, min(sizes[b * 4 + 0], Hp));
  g.Wc = max(1, min(sizes[b * 4 + 1], Wp));
  g.Ho = min(sizes[b * 4 + 2], out_h);
  g.Wo = min(sizes[b * 4 + 3], out_w);
  g.two = (g.Ho != g.Hc) || (g.Wo != g.Wc);
  g.rh1 = static_cast<float>(h) / static_cast<float>(Hp);
  g.rw1 = static_cast<float>(w) / static_cast<float>(Wp);
  g.rh2 = static_cast<float>(g.Hc) / static_cast<float>(g.Ho);
  g.rw2 = static_cast<float>(g.Wc) / static_cast<float>(g.Wo);
  return g;
}

// Source taps of one output coordinate along one axis: t2 blends the two stage-1 rows t1[0], t1[1]
// (single stage: only t1[0] is used).
struct AxisTaps {
  Tap t1[2];
  Tap t2;
};

__device__ __forceinline__ AxisTaps axis_taps(int dst, bool two, float r1, int in1, float r2, int in2) {
  AxisTaps a;
  if (two) {
    a.t2 = bilinear_tap(dst, r2, in2);
    a.t1[0] = bilinear_tap(a.t2.i0, r1, in1);
    a.t1[1] = bilinear_tap(a.t2.i1, r1, in1);
  } else {
    a.t1[0] = bilinear_tap(dst, r1, in1);
    a.t1[1] = a.t1[0];
    a.t2 = Tap{dst, dst, 1.f, 0.f};
  }
  return a;
}

// The full-resolution logit from taps; ld(row, col) returns the fp32 source texel.
template <typename Ld>
__device__ __forceinline__ float logit_at(bool two, const AxisTaps& ay, const AxisTaps& ax, Ld ld) {
  auto stage1 = [&](const Tap& ty, const Tap& tx) {
    return blend4(ty.l0, ty.l1, tx.l0, tx.l1, ld(ty.i0, tx.i0), ld(ty.i0, tx.i1), ld(ty.i1, tx.i0), ld(ty.i1, tx.i1));
  };
  if (!two) return stage1(ay.t1[0], ax.t1[0]);
  const float a = stage1(ay.t1[0], ax.t1[0]);
  const float b = stage1(ay.t1[0], ax.t1[1]);
  const float c = stage1(ay.t1[1], ax.t1[0]);
  const float d = stage1(ay.t1[1], ax.t1[1]);
  return blend4(ay.t2.l0, ay.t2.l1, ax.t2.l0, ax.t2.l1, a, b, c, d);
}

}  // namespace m2f

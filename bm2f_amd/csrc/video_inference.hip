// Video inference and clip target preparation (mask2former_video/video_maskformer_model.py).
//
//   video_mask_kernel   the eval branch (:372-393) and inference_video (:651-694): masks = logit > 0 of the selected
//                       queries over all T frames, from the decoder's LOW-resolution logits (Q, T, h, w).  The
//                       reference upsamples all Q queries to a (Q, T, Hp, Wp) fp32 tensor first; here the resize chain
//                       of resize_device.h is evaluated per output pixel and only the mask is written.
//                       Grid (output tile, frame, slot); a workgroup (4 waves) owns a 16 x 64 pixel tile of one
//                       (slot, frame), a lane 4 consecutive x of one row.  The taps are monotone in the destination
//                       index, so the tile's source box is spanned by the taps of its first and last pixel; the box
//                       is staged in LDS once, converted to fp32, when it fits the budget, and read from global
//                       memory by the same arithmetic when it does not (an output much smaller than the logits).
//                       The logits are read in place through the slot -> query table.  Byte form: the lane's four
//                       0/1 bytes go out as one 32-bit word where the address allows.  Packed form: bit x % 32 of
//                       int32 word x / 32, combined over 8 lanes with shuffles; tail bits are zero.
//   feat_resize_pad_kernel   the DINO feature resize of prepare_weaksup_targets (:506-517): bilinear resize of the
//                       features zero-padded to (Hp, Wp), without building the padded copy: taps are clamped to the
//                       padded size and a tap at or beyond the source size contributes 0.  The tap weights come
//                       from integer arithmetic (exact_tap), the blend is fp32.
#include "bm2f.h"
#include "common.h"
#include "resize_device.h"

#include <hip/hip_runtime.h>

namespace {

using m2f::AxisTaps;

constexpr int kTileH = 16, kTileW = 64;   // output pixels per workgroup: 256 lanes x 4 consecutive x
constexpr int kLanesX = kTileW / 4;
constexpr int kCapDefault = 1536;         // LDS budget in source texels (6 KB): identity and every upscale fit
constexpr int kCapMax = 12288;            // 48 KB

struct VideoGeo {
  int h, w, Hc, Wc, Ho, Wo;
  float rh1, rw1, rh2, rw2;
};

template <bool kPacked>
__global__ void __launch_bounds__(256) video_mask_kernel(const void* __restrict__ logits, int dtype,
                                                         const int32_t* __restrict__ slot_query,
                                                         const int32_t* __restrict__ num_sel, int Q, int T,
                                                         VideoGeo g, int tiles_x, int cap, void* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float s_win[];
  const int s = blockIdx.z, t = blockIdx.y;
  if (num_sel != nullptr && s >= *num_sel) return;   // uniform: before any barrier
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * kTileH, x0 = tx * kTileW;   // inside the output: the grid is sized from (Ho, Wo)
  const int tid = threadIdx.x;
  const bool two = (g.Ho != g.Hc) || (g.Wo != g.Wc);
  const int h = g.h, w = g.w;

  // source box of the tile
  const int ylast = min(y0 + kTileH, g.Ho) - 1, xlast = min(x0 + kTileW, g.Wo) - 1;
  const int wy0 = m2f::axis_taps(y0, two, g.rh1, h, g.rh2, g.Hc).t1[0].i0;
  const int wy1 = m2f::axis_taps(ylast, two, g.rh1, h, g.rh2, g.Hc).t1[1].i1;
  const int wx0 = m2f::axis_taps(x0, two, g.rw1, w, g.rw2, g.Wc).t1[0].i0;
  const int wx1 = m2f::axis_taps(xlast, two, g.rw1, w, g.rw2, g.Wc).t1[1].i1;
  const int wh = wy1 - wy0 + 1, ww = wx1 - wx0 + 1;
  const bool use_win = static_cast<int64_t>(wh) * ww <= cap;   // uniform over the workgroup

  const int q = max(0, min(slot_query[s], Q - 1));
  const int64_t base = (static_cast<int64_t>(q) * T + t) * h * w;
  if (use_win) {
    const int wsz = wh * ww;
    for (int i = tid; i < wsz; i += 256) {
      const int ry = i / ww, rx = i - ry * ww;
      s_win[i] = m2f::load_logit(logits, dtype, base + static_cast<int64_t>(wy0 + ry) * w + wx0 + rx);
    }
    __syncthreads();
  }

  const int y = y0 + tid / kLanesX, xb = x0 + (tid % kLanesX) * 4;
  unsigned bits = 0;   // bit j: pixel xb + j
  if (y < g.Ho && xb < g.Wo) {
    const AxisTaps ay = m2f::axis_taps(y, two, g.rh1, h, g.rh2, g.Hc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xb + j;
      if (x < g.Wo) {
        const AxisTaps ax = m2f::axis_taps(x, two, g.rw1, w, g.rw2, g.Wc);
        float v;
        if (use_win)
          v = m2f::logit_at(two, ay, ax, [&](int r, int c) { return s_win[(r - wy0) * ww + (c - wx0)]; });
        else
          v = m2f::logit_at(two, ay, ax, [&](int r, int c) {
            return m2f::load_logit(logits, dtype, base + static_cast<int64_t>(r) * w + c);
          });
        bits |= (v > 0.f ? 1u : 0u) << j;
      }
    }
  }

  const int64_t plane = static_cast<int64_t>(s) * T + t;
  if (kPacked) {
    // 8 lanes of one row = 32 pixels = one word; every lane of the wave takes part in the shuffles
    unsigned word = bits << (4 * (tid & 7));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    const int words = (g.Wo + 31) >> 5, wi = xb >> 5;
    if ((tid & 7) == 0 && y < g.Ho && wi < words)
      static_cast<int32_t*>(out)[(plane * g.Ho + y) * words + wi] = static_cast<int32_t>(word);
  } else if (y < g.Ho && xb < g.Wo) {
    uint8_t* dst = static_cast<uint8_t*>(out) + (plane * g.Ho + y) * g.Wo + xb;
    if (xb + 3 < g.Wo && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
      // bytes (b0, b1, b2, b3) of one little-endian word
      *reinterpret_cast<uint32_t*>(dst) = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
    } else {
      for (int j = 0; j < 4 && xb + j < g.Wo; ++j) dst[j] = (bits >> j) & 1u;
    }
  }
}

// The tap of destination index dst with the source coordinate in * (dst + 0.5) / out - 0.5 taken exactly, as the
// integer fraction (in * (2 dst + 1) - out) / (2 out) clamped at 0: torch's own fp32 evaluation of the coordinate
// is off by ~1e-7 * in, which costs 1e-5 of the feature range at a non-integer ratio.  At an integer ratio the
// weights are the same binary fractions either way and the result is torch's, bit for bit.
__device__ __forceinline__ m2f::Tap exact_tap(int dst, int in, int out) {
  int64_t num = static_cast<int64_t>(in) * (2 * dst + 1) - out;
  num = num < 0 ? 0 : num;
  const int64_t den = 2 * static_cast<int64_t>(out);
  const int64_t q = num / den;
  m2f::Tap t;
  t.i0 = static_cast<int>(q);   // <= in - 1: the coordinate is below in - 0.5
  t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
  t.l1 = static_cast<float>(static_cast<double>(num - q * den) / static_cast<double>(den));
  t.l0 = 1.f - t.l1;
  return t;
}

// out[n, y, x] = bilinear(zero-padded src)(y, x); one thread per output pixel, x fastest
__global__ void __launch_bounds__(256) feat_resize_pad_kernel(const void* __restrict__ src, int dtype, int64_t total,
                                                              int Hs, int Ws, int Hp, int Wp, int oh, int ow,
                                                              float* __restrict__ out) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i >= total) return;
  const int x = static_cast<int>(i % ow);
  const int64_t r = i / ow;
  const int y = static_cast<int>(r % oh);
  const int64_t n = r / oh;
  const m2f::Tap ty = exact_tap(y, Hp, oh);
  const m2f::Tap tx = exact_tap(x, Wp, ow);
  const int64_t base = n * Hs * Ws;
  auto ld = [&](int yy, int xx) {
    return (yy < Hs && xx < Ws) ? m2f::load_logit(src, dtype, base + static_cast<int64_t>(yy) * Ws + xx) : 0.f;
  };
  out[i] = m2f::blend4(ty.l0, ty.l1, tx.l0, tx.l1, ld(ty.i0, tx.i0), ld(ty.i0, tx.i1), ld(ty.i1, tx.i0),
                       ld(ty.i1, tx.i1));
}

}  // namespace

extern "C" int m2f_infer_video(const void* logits, int dtype, const int32_t* slot_query, const int32_t* num_sel,
                               int num_queries, int num_slots, int num_frames, int in_h, int in_w, int pad_h,
                               int pad_w, int crop_h, int crop_w, int out_h, int out_w, int packed, void* out,
                               void* stream) {
  const char* fn = "m2f_infer_video";
  if (!logits || !slot_query || !out) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (!m2f::is_float_dtype(dtype)) return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, dtype);
  if (num_queries <= 0 || num_slots <= 0 || num_frames <= 0 || in_h <= 0 || in_w <= 0 || pad_h <= 0 || pad_w <= 0 ||
      crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (crop_h > pad_h || crop_w > pad_w)
    return m2f::fail(M2F_EINVAL, "%s: crop %d x %d exceeds the padded size %d x %d", fn, crop_h, crop_w, pad_h, pad_w);
  if (packed != 0 && packed != 1) return m2f::fail(M2F_EINVAL, "%s: packed must be 0 or 1", fn);
  if (!m2f::aligned(out, 4)) return m2f::fail(M2F_EINVAL, "%s: out must be 4-byte aligned", fn);
  const int64_t tiles_x = m2f::ceil_div(out_w, kTileW), tiles_y = m2f::ceil_div(out_h, kTileH);
  if (num_slots > 65535 || num_frames > 65535 || tiles_x * tiles_y > 0x7fffffff ||
      static_cast<int64_t>(in_h) * in_w > 0x7fffffff || static_cast<int64_t>(out_h) * out_w > 0x7fffffff)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  const int cap = min(m2f::option(m2f::kOptInferVideoCap, kCapDefault), kCapMax);
  VideoGeo g;
  g.h = in_h;
  g.w = in_w;
  g.Hc = crop_h;
  g.Wc = crop_w;
  g.Ho = out_h;
  g.Wo = out_w;
  g.rh1 = static_cast<float>(in_h) / static_cast<float>(pad_h);
  g.rw1 = static_cast<float>(in_w) / static_cast<float>(pad_w);
  g.rh2 = static_cast<float>(crop_h) / static_cast<float>(out_h);
  g.rw2 = static_cast<float>(crop_w) / static_cast<float>(out_w);
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y), num_frames, num_slots);
  const size_t lds = static_cast<size_t>(cap) * sizeof(float);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (packed)
    video_mask_kernel<true><<<grid, 256, lds, st>>>(logits, dtype, slot_query, num_sel, num_queries, num_frames, g,
                                                   static_cast<int>(tiles_x), cap, out);
  else
    video_mask_kernel<false><<<grid, 256, lds, st>>>(logits, dtype, slot_query, num_sel, num_queries, num_frames, g,
                                                    static_cast<int>(tiles_x), cap, out);
  return m2f::check_launch(fn);
}

extern "C" int m2f_feat_resize_pad(const void* feats, int dtype, int64_t planes, int src_h, int src_w, int pad_h,
                                   int pad_w, int out_h, int out_w, float* out, void* stream) {
  const char* fn = "m2f_feat_resize_pad";
  if (!feats || !out) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (!m2f::is_float_dtype(dtype)) return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, dtype);
  if (planes <= 0 || src_h <= 0 || src_w <= 0 || pad_h <= 0 || pad_w <= 0 || out_h <= 0 || out_w <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (src_h > pad_h || src_w > pad_w)
    return m2f::fail(M2F_EINVAL, "%s: source %d x %d exceeds the padded size %d x %d", fn, src_h, src_w, pad_h, pad_w);
  const int64_t total = planes * out_h * out_w;
  if (static_cast<int64_t>(src_h) * src_w > 0x7fffffff || static_cast<int64_t>(out_h) * out_w > 0x7fffffff ||
      planes > (INT64_MAX >> 31) || (total + 255) / 256 > 0x7fffffff)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  feat_resize_pad_kernel<<<m2f::ceil_div(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      feats, dtype, total, src_h, src_w, pad_h, pad_w, out_h, out_w, out);
  return m2f::check_launch(fn);
}

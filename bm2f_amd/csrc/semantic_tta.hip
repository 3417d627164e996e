// Semantic test-time augmentation: the loop of the reference's SemanticSegmentorWithTTA._inference_one_image
// (test_time_augmentation.py:71-98) over the V augmented views of ONE image, fused into one launch.  The reference
// runs the model per view, takes its (K, H, W) sem_seg, flips it back where the view was mirrored, adds it into a
// running sum and divides by V.  Here
//
//   out[k, y, x] = (sum_v sum_q probs_v[k, q] * s_{v,q}(y, x_v)) / V,      x_v = Wo - 1 - x if view v is flipped
//
// is semantic_kernel's GEMM (inference.hip) with its reduction dimension extended from Q to V * Q: the fp32 MFMA
// accumulators stay in registers across the views, and the (K, Ho, Wo) scores are written once, or never (labels).
// s follows the reference's two orders, selected per call:
//   before  (sem_seg_postprocess_before_inference): s = sigmoid(L), L the chained logit of resize_device.h built
//           from the view's own (h, w, Hp, Wp, Hc, Wc) onto (Ho, Wo);
//   after   (the default of the semantic configs): the scores are resized, not the logits, so
//           s = blend4 over the four stage-2 taps of sigmoid(stage-1 logit at that crop pixel).  The contraction
//           with probs is linear and commutes with the blend; the kernel contracts after blending.  This order
//           costs four sigmoids per (pixel, query) where `before` costs one.
// When (Ho, Wo) == (Hc, Wc) the second stage is the identity in both orders, as in load_geo.
//
// Tile, chunking and operand layout are semantic_kernel's: a workgroup (4 waves) owns 4 x 32 output pixels and all K
// classes (KT tiles of 32), per chunk of 32 queries it stages the view's probs chunk and the queries' source windows
// in LDS, forms the s tile [128 pix][32 q] in LDS and feeds the f32 MFMA.  The views loop outside the query chunks;
// the tap tables and the window are rebuilt per view.  A mirrored view reads the tile's columns in descending source
// order, so its source window is still one contiguous box; windows above kWinCap texels fall back to global loads.
//
// LDS budget (bytes), unchanged from semantic_kernel because a view's geometry lives in scalar registers:
// probs KT*32*36*4 (<= 36864), s tile 128*36*4 = 18432, windows 32*177*4 = 22656, tap tables 1440: 79392 at KT = 8,
// which lets two workgroups share a CU's 163840 B (65568 B at KT = 5, ADE20K's 150 classes).  Registers, not LDS,
// bound KT = 8: 141 VGPRs + 128 accumulator AGPRs admit one workgroup per CU, as in semantic_kernel (137 + 128); up to
// KT = 7 two fit.
//
// The sum runs in a fixed order (views ascending, queries ascending inside a view, no atomics): the result is
// bitwise repeatable.  The division by V and the labels' first-maximum scan are the epilogue; non-finite logits
// behave as in semantic_kernel (a pixel whose scores are all NaN gets label -1).
//
// A view's table row is clamped as load_geo clamps: Hc, Wc into [1, Hp], [1, Wp]; a row whose sizes are not
// positive, or whose logits would not lie inside the flat buffer, contributes nothing (the sum is still over V).
#include "bm2f.h"
#include "common.h"
#include "resize_device.h"

#include <hip/hip_runtime.h>

namespace {

using m2f::AxisTaps;
using m2f::f16v, m2f::f4;

constexpr int kMaxQ = 256, kMaxK = 256, kMaxV = 32;
constexpr int kTH = 4, kTW = 32, kPix = kTH * kTW;  // pixel tile: wave w owns row w
constexpr int kQC = 32;                             // queries per chunk
constexpr int kP = kQC + 4;                         // LDS pitch (floats): conflict-free ds_read_b128
constexpr int kWinCap = 176;                        // source texels per query staged in LDS, as semantic_kernel
constexpr int kWinPitch = kWinCap + 1;
constexpr int kFields = M2F_TTA_VIEW_FIELDS;

struct TapO {  // a Tap with its indices turned into offsets (window- or image-relative)
  int o0, o1;
  float l0, l1;
};

constexpr int tta_lds_bytes(int KT) {
  return (KT * 32 * kP + kPix * kP + kQC * kWinPitch) * 4 + (kTH * 2 + kTW * 2) * 16 + (kTH + kTW) * 8;
}

struct View {
  int64_t off;
  int h, w, Hc, Wc;
  float rh1, rw1, rh2, rw2;
  bool two, flip, ok;
};

// one row [offset, h, w, Hp, Wp, Hc, Wc, flip] of the device table, validated against the flat buffer
__device__ __forceinline__ View load_view(const int64_t* __restrict__ views, int v, int Q, int64_t numel, int Ho,
                                          int Wo) {
  const int64_t* r = views + static_cast<int64_t>(v) * kFields;
  const int64_t off = r[0], h = r[1], w = r[2], Hp = r[3], Wp = r[4];
  View s;
  s.ok = off >= 0 && off <= numel && h > 0 && w > 0 && Hp > 0 && Wp > 0 && h <= 0x7fffffff && w <= 0x7fffffff &&
         Hp <= 0x7fffffff && Wp <= 0x7fffffff && h * w <= 0x7fffffff && Q * h * w <= numel - off;
  s.off = off;
  s.h = static_cast<int>(h);
  s.w = static_cast<int>(w);
  s.Hc = static_cast<int>(max(int64_t{1}, min(r[5], Hp)));
  s.Wc = static_cast<int>(max(int64_t{1}, min(r[6], Wp)));
  s.flip = r[7] != 0;
  s.two = (Ho != s.Hc) || (Wo != s.Wc);
  s.rh1 = static_cast<float>(s.h) / static_cast<float>(static_cast<int>(Hp));
  s.rw1 = static_cast<float>(s.w) / static_cast<float>(static_cast<int>(Wp));
  s.rh2 = static_cast<float>(s.Hc) / static_cast<float>(Ho);
  s.rw2 = static_cast<float>(s.Wc) / static_cast<float>(Wo);
  return s;
}

// grid (ceil(Wo / 32), ceil(Ho / 4)), 256 threads
template <int KT>
__global__ void __launch_bounds__(256) semantic_tta_kernel(const void* __restrict__ logits, int dtype, int64_t numel,
                                                           const float* __restrict__ probs,
                                                           const int64_t* __restrict__ views, int V, int Q, int K,
                                                           int Ho, int Wo, int before, float* __restrict__ semseg,
                                                           int16_t* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                                               // [KT*32 classes][kP]
  float* sB = sA + KT * 32 * kP;                                  // [kPix][kP]
  float* sWin = sB + kPix * kP;                                   // [kQC][kWinPitch]
  TapO* sY = reinterpret_cast<TapO*>(sWin + kQC * kWinPitch);     // [kTH][2]
  TapO* sX = sY + kTH * 2;                                        // [kTW][2]
  float2* sY2 = reinterpret_cast<float2*>(sX + kTW * 2);          // [kTH] stage-2 (l0, l1)
  float2* sX2 = sY2 + kTH;                                        // [kTW]

  const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int ylast = min(y0 + kTH, Ho) - 1, xlast = min(x0 + kTW, Wo) - 1;
  const int ql = tid & 31, pg = tid >> 5;

  f16v acc[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  for (int v = 0; v < V; ++v) {
    const View g = load_view(views, v, Q, numel, Ho, Wo);
    if (!g.ok) continue;  // uniform
    const int h = g.h, w = g.w;
    // source columns of the tile: ascending x, or descending from Wo - 1 - x0 when the view is mirrored
    const int sxa = g.flip ? Wo - 1 - xlast : x0, sxb = g.flip ? Wo - 1 - x0 : xlast;
    const int wy0 = m2f::axis_taps(y0, g.two, g.rh1, h, g.rh2, g.Hc).t1[0].i0;
    const int wy1 = m2f::axis_taps(ylast, g.two, g.rh1, h, g.rh2, g.Hc).t1[1].i1;
    const int wx0 = m2f::axis_taps(sxa, g.two, g.rw1, w, g.rw2, g.Wc).t1[0].i0;
    const int wx1 = m2f::axis_taps(sxb, g.two, g.rw1, w, g.rw2, g.Wc).t1[1].i1;
    const int wh = wy1 - wy0 + 1, ww = wx1 - wx0 + 1, wsz = wh * ww;
    const bool use_win = wsz <= kWinCap;
    const int oy = use_win ? wy0 : 0, ox = use_win ? wx0 : 0, rs = use_win ? ww : w;

    // the previous view's last chunk ended with a barrier: its tables are no longer read
    if (tid < kTH) {
      const AxisTaps a = m2f::axis_taps(min(y0 + tid, Ho - 1), g.two, g.rh1, h, g.rh2, g.Hc);
      for (int t = 0; t < 2; ++t)
        sY[tid * 2 + t] = TapO{(a.t1[t].i0 - oy) * rs, (a.t1[t].i1 - oy) * rs, a.t1[t].l0, a.t1[t].l1};
      sY2[tid] = make_float2(a.t2.l0, a.t2.l1);
    } else if (tid >= 64 && tid < 64 + kTW) {
      const int c = tid - 64;
      const int x = min(x0 + c, Wo - 1);
      const AxisTaps a = m2f::axis_taps(g.flip ? Wo - 1 - x : x, g.two, g.rw1, w, g.rw2, g.Wc);
      for (int t = 0; t < 2; ++t) sX[c * 2 + t] = TapO{a.t1[t].i0 - ox, a.t1[t].i1 - ox, a.t1[t].l0, a.t1[t].l1};
      sX2[c] = make_float2(a.t2.l0, a.t2.l1);
    }

    const int64_t hw = static_cast<int64_t>(h) * w;
    const float* pv = probs + static_cast<int64_t>(v) * K * Q;
    for (int q0 = 0; q0 < Q; q0 += kQC) {
      // A chunk: probs[v, k, q0 + ql], zero padded in k and q
      for (int idx = tid; idx < KT * 32 * kQC; idx += 256) {
        const int k = idx >> 5, qq = q0 + (idx & 31);
        sA[k * kP + (idx & 31)] = (k < K && qq < Q) ? pv[static_cast<int64_t>(k) * Q + qq] : 0.f;
      }
      if (use_win) {
        for (int idx = tid; idx < kQC * wsz; idx += 256) {
          const int qi = idx / wsz, o = idx - qi * wsz;
          const int ry = o / ww, rx = o - ry * ww;
          const int qq = q0 + qi;
          sWin[qi * kWinPitch + o] =
              qq < Q ? m2f::load_logit(logits, dtype, g.off + qq * hw + (wy0 + ry) * w + wx0 + rx) : 0.f;
        }
      }
      __syncthreads();
      // B chunk: s of the view at the tile's pixels, [pixel][query]; lanes = queries
      {
        const int qq = q0 + ql;
        const int64_t qbase = g.off + min(qq, Q - 1) * hw;
        const float* win = sWin + ql * kWinPitch;
        auto ld = [&](int o) { return use_win ? win[o] : m2f::load_logit(logits, dtype, qbase + o); };
#pragma unroll 4
        for (int j = 0; j < kPix / 8; ++j) {
          const int p = pg + 8 * j, r = p >> 5, c = p & 31;
          float s = 0.f;
          if (qq < Q && y0 + r < Ho && x0 + c < Wo) {
            auto stage1 = [&](const TapO& ty, const TapO& tx) {
              return m2f::blend4(ty.l0, ty.l1, tx.l0, tx.l1, ld(ty.o0 + tx.o0), ld(ty.o0 + tx.o1), ld(ty.o1 + tx.o0),
                                 ld(ty.o1 + tx.o1));
            };
            if (!g.two) {
              s = m2f::sigmoidf_literal(stage1(sY[r * 2], sX[c * 2]));
            } else {
              float a = stage1(sY[r * 2], sX[c * 2]);
              float bb = stage1(sY[r * 2], sX[c * 2 + 1]);
              float cc = stage1(sY[r * 2 + 1], sX[c * 2]);
              float d = stage1(sY[r * 2 + 1], sX[c * 2 + 1]);
              const float2 ly = sY2[r], lx = sX2[c];
              if (before) {
                s = m2f::sigmoidf_literal(m2f::blend4(ly.x, ly.y, lx.x, lx.y, a, bb, cc, d));
              } else {
                a = m2f::sigmoidf_literal(a);
                bb = m2f::sigmoidf_literal(bb);
                cc = m2f::sigmoidf_literal(cc);
                d = m2f::sigmoidf_literal(d);
                s = m2f::blend4(ly.x, ly.y, lx.x, lx.y, a, bb, cc, d);
              }
            }
          }
          sB[p * kP + ql] = s;
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kQC / 8; ++kk) {
        const f4 fb = *reinterpret_cast<const f4*>(&sB[(wv * 32 + li) * kP + kk * 8 + lh * 4]);
#pragma unroll
        for (int i = 0; i < KT; ++i) {
          const f4 fa = *reinterpret_cast<const f4*>(&sA[(i * 32 + li) * kP + kk * 8 + lh * 4]);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[i] = m2f::mfma32(fa[s], fb[s], acc[i]);
        }
      }
      __syncthreads();
    }
  }

  // lane holds C[class = 32 i + (e & 3) + 8 (e >> 2) + 4 lh][pixel = (row wv, column li)]; the mean over the views
  // is the reference's division (test_time_augmentation.py:97)
  const float fv = static_cast<float>(V);
  const int y = y0 + wv, x = x0 + li;
  const bool inside = y < Ho && x < Wo;
  if (labels == nullptr) {
    if (!inside) return;
    const int64_t cs = static_cast<int64_t>(Ho) * Wo;
    float* dst = semseg + static_cast<int64_t>(y) * Wo + x;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (k < K) dst[k * cs] = acc[i][e] / fv;
      }
  } else {
    // first maximum over k, as semantic_kernel: ascending (i, e) is ascending k within a lane; then the two halves
    float best = -1.f;
    int bk = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        const float a = acc[i][e] / fv;
        if (k < K && (a > best || (a == best && k < bk))) {
          best = a;
          bk = k;
        }
      }
    const float ob = __shfl_xor(best, 32);
    const int ok = __shfl_xor(bk, 32);
    if (ob > best || (ob == best && ok < bk)) bk = ok;
    if (inside && lh == 0) labels[static_cast<int64_t>(y) * Wo + x] = static_cast<int16_t>(bk);
  }
}

template <int KT>
int launch_tta(const void* logits, int dtype, int64_t numel, const float* probs, const int64_t* views, int V, int Q,
               int K, int out_h, int out_w, int before, float* semseg, int16_t* labels, hipStream_t st) {
  const char* fn = "m2f_infer_semantic_tta";
  if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(&semantic_tta_kernel<KT>), tta_lds_bytes(KT), fn))
    return rc;
  const dim3 grid(m2f::ceil_div(out_w, kTW), m2f::ceil_div(out_h, kTH));
  semantic_tta_kernel<KT><<<grid, 256, tta_lds_bytes(KT), st>>>(logits, dtype, numel, probs, views, V, Q, K, out_h,
                                                               out_w, before, semseg, labels);
  return m2f::check_launch(fn);
}

}  // namespace

extern "C" int m2f_infer_semantic_tta(const void* logits, int dtype, int64_t logits_numel, const float* probs,
                                      const int64_t* views, int num_views, int num_queries, int num_classes, int out_h,
                                      int out_w, int before, float* semseg, int16_t* labels, void* stream) {
  const char* fn = "m2f_infer_semantic_tta";
  if (!logits || !probs || !views || (!semseg && !labels)) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (!m2f::is_float_dtype(dtype)) return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, dtype);
  if (num_views < 1 || num_views > kMaxV)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: num_views %d outside [1, %d]", fn, num_views, kMaxV);
  if (num_queries <= 0 || num_classes <= 0 || out_h <= 0 || out_w <= 0 || logits_numel <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (num_queries > kMaxQ) return m2f::fail(M2F_EUNSUPPORTED, "%s: num_queries %d > %d", fn, num_queries, kMaxQ);
  if (num_classes > kMaxK) return m2f::fail(M2F_EUNSUPPORTED, "%s: num_classes %d > %d", fn, num_classes, kMaxK);
  if (out_h > 65535 * 4 || static_cast<int64_t>(out_h) * out_w > 0x7fffffff)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = M2F_OK;
  if (!m2f::dispatch_one_of<1, 2, 3, 4, 5, 6, 7, 8>((num_classes + 31) / 32, [&](auto kt) {
        rc = launch_tta<kt.value>(logits, dtype, logits_numel, probs, views, num_views, num_queries, num_classes, out_h,
                                  out_w, before != 0, semseg, labels, st);
      }))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: num_classes %d", fn, num_classes);
  return rc;
}

// Fused inference heads: the eval branch of MaskFormer.forward (maskformer_model.py:333-377) and the three heads it
// calls -- semantic_inference (:509-513), panoptic_inference (:515-571), instance_inference (:573-624) -- computed
// from the decoder's LOW-resolution mask logits.  The reference upsamples the (Q, h, w) logits to (Q, Hp, Wp),
// writes their sigmoid and reads it again per head; here every head evaluates the resize chain per output pixel
// (resize_device.h holds the definition and the 16-bit rule) and writes only its result.
//
//   semantic_kernel   C[k, pix] = sum_q probs[k, q] * sigmoid(logit_q(pix)): a GEMM whose B operand is generated
//                     on the fly.  A workgroup (4 waves) owns a 4 x 32 pixel tile and all K classes (KT tiles of
//                     32, K <= 256).  Per chunk of 32 queries it stages the probs chunk [KT*32][32] and the
//                     queries' source windows in LDS, forms the sigmoid tile [128 pix][32 q] in LDS and feeds the
//                     f32 MFMA (gemm.hip's operand order: 4 contiguous k per lane and ds_read_b128).  The sigmoid
//                     tile never leaves the CU.  Epilogue: semseg rows straight from the accumulators (a wave's 32
//                     lanes = 128 contiguous bytes), or the per-pixel argmax as int16 (labels mode).
//   panoptic_kernel   one thread per output pixel loops over the kept queries: winner = argmax score*sigmoid
//                     (first maximum), the winner's own sigmoid >= 0.5 bit, and the three area counters of the
//                     reference's merge loop, counted with ballot/popcount and integer atomics (exact, so the
//                     result does not depend on scheduling).
//   instance_kernel   masks = logit > 0 as uint8 and per-tile fp32 partial sums of sigmoid*binary and binary,
//                     combined per query in tile order by instance_combine_kernel (fixed order).
//
// LDS budget of semantic_kernel (bytes): probs KT*32*36*4 (<= 36864), sigmoid tile 128*36*4 = 18432, windows
// 32*177*4 = 22656, tap tables 1440: 79392 at KT = 8, two workgroups per CU.
//
// Non-finite logits: the first-maximum scans compare with > as written, so a pixel whose scores are all NaN gets
// label -1 (labels mode) or keeps the first kept query (panoptic), where torch.argmax returns the NaN's index
// (the first one, so the panoptic head equals the CPU path and the labels differ from its 0).  The score planes
// are NaN at such a pixel.  The instance head leaves a NaN pixel out of the mask and of the score (`v > 0` is
// false), where the reference's mask score turns NaN.  +-inf logits give sigmoid exactly 1 / 0 in every head.
// test_inference_sweep_gpu.py pins all of this.
#include "bm2f.h"
#include "common.h"
#include "resize_device.h"

#include <hip/hip_runtime.h>

namespace {

using m2f::AxisTaps;
using m2f::Geo;
using m2f::Tap;
using m2f::f16v, m2f::f4, m2f::wave_sum;

constexpr int kMaxQ = 256, kMaxK = 256;
constexpr int kTH = 4, kTW = 32, kPix = kTH * kTW;  // semantic pixel tile: wave w owns row w
constexpr int kQC = 32;                             // queries per chunk
constexpr int kP = kQC + 4;                         // LDS pitch (floats): conflict-free ds_read_b128, as gemm.hip
// source texels per query staged in LDS; larger windows: global loads.  176 covers the 5 x 33 window of a tile at
// identity geometry (the compat functions) and every upscale
constexpr int kWinCap = 176;
constexpr int kWinPitch = kWinCap + 1;              // odd: lanes = queries read one offset without conflicts

struct TapO {  // a Tap with its indices turned into offsets (window- or image-relative)
  int o0, o1;
  float l0, l1;
};

constexpr int sem_lds_bytes(int KT) {
  return (KT * 32 * kP + kPix * kP + kQC * kWinPitch) * 4 + (kTH * 2 + kTW * 2) * 16 + (kTH + kTW) * 8;
}

template <int KT>
__global__ void __launch_bounds__(256) semantic_kernel(const void* __restrict__ logits, int dtype,
                                                       const float* __restrict__ probs,
                                                       const int32_t* __restrict__ sizes, int Q, int K, int h, int w,
                                                       int Hp, int Wp, int out_h, int out_w,
                                                       float* __restrict__ semseg, int16_t* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                                               // [KT*32 classes][kP]
  float* sB = sA + KT * 32 * kP;                                  // [kPix][kP]
  float* sWin = sB + kPix * kP;                                   // [kQC][kWinPitch]
  TapO* sY = reinterpret_cast<TapO*>(sWin + kQC * kWinPitch);     // [kTH][2]
  TapO* sX = sY + kTH * 2;                                        // [kTW][2]
  float2* sY2 = reinterpret_cast<float2*>(sX + kTW * 2);          // [kTH] stage-2 (l0, l1)
  float2* sX2 = sY2 + kTH;                                        // [kTW]

  const int b = blockIdx.z;
  const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
  const Geo g = m2f::load_geo(sizes, b, h, w, Hp, Wp, out_h, out_w);
  if (y0 >= g.Ho || x0 >= g.Wo) return;  // uniform: before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;

  // source window of the tile (the taps are monotone in the destination index)
  const int ylast = min(y0 + kTH, g.Ho) - 1, xlast = min(x0 + kTW, g.Wo) - 1;
  const int wy0 = m2f::axis_taps(y0, g.two, g.rh1, h, g.rh2, g.Hc).t1[0].i0;
  const int wy1 = m2f::axis_taps(ylast, g.two, g.rh1, h, g.rh2, g.Hc).t1[1].i1;
  const int wx0 = m2f::axis_taps(x0, g.two, g.rw1, w, g.rw2, g.Wc).t1[0].i0;
  const int wx1 = m2f::axis_taps(xlast, g.two, g.rw1, w, g.rw2, g.Wc).t1[1].i1;
  const int wh = wy1 - wy0 + 1, ww = wx1 - wx0 + 1, wsz = wh * ww;
  const bool use_win = wsz <= kWinCap;
  const int oy = use_win ? wy0 : 0, ox = use_win ? wx0 : 0, rs = use_win ? ww : w;

  if (tid < kTH) {
    const AxisTaps a = m2f::axis_taps(min(y0 + tid, g.Ho - 1), g.two, g.rh1, h, g.rh2, g.Hc);
    for (int t = 0; t < 2; ++t)
      sY[tid * 2 + t] = TapO{(a.t1[t].i0 - oy) * rs, (a.t1[t].i1 - oy) * rs, a.t1[t].l0, a.t1[t].l1};
    sY2[tid] = make_float2(a.t2.l0, a.t2.l1);
  } else if (tid >= 64 && tid < 64 + kTW) {
    const int c = tid - 64;
    const AxisTaps a = m2f::axis_taps(min(x0 + c, g.Wo - 1), g.two, g.rw1, w, g.rw2, g.Wc);
    for (int t = 0; t < 2; ++t) sX[c * 2 + t] = TapO{a.t1[t].i0 - ox, a.t1[t].i1 - ox, a.t1[t].l0, a.t1[t].l1};
    sX2[c] = make_float2(a.t2.l0, a.t2.l1);
  }

  f16v acc[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  const int64_t hw = static_cast<int64_t>(h) * w;
  const int ql = tid & 31, pg = tid >> 5;
  for (int q0 = 0; q0 < Q; q0 += kQC) {
    // A chunk: probs[b, k, q0 + ql], zero padded in k and q
    for (int idx = tid; idx < KT * 32 * kQC; idx += 256) {
      const int k = idx >> 5, qq = q0 + (idx & 31);
      sA[k * kP + (idx & 31)] = (k < K && qq < Q) ? probs[(static_cast<int64_t>(b) * K + k) * Q + qq] : 0.f;
    }
    if (use_win) {
      for (int idx = tid; idx < kQC * wsz; idx += 256) {
        const int qi = idx / wsz, o = idx - qi * wsz;
        const int ry = o / ww, rx = o - ry * ww;
        const int qq = q0 + qi;
        sWin[qi * kWinPitch + o] =
            qq < Q ? m2f::load_logit(logits, dtype, (static_cast<int64_t>(b) * Q + qq) * hw + (wy0 + ry) * w + wx0 + rx)
                   : 0.f;
      }
    }
    __syncthreads();
    // B chunk: sigmoid of the full-resolution logit, [pixel][query]; lanes = queries
    {
      const int qq = q0 + ql;
      const int64_t qbase = (static_cast<int64_t>(b) * Q + min(qq, Q - 1)) * hw;
      const float* win = sWin + ql * kWinPitch;
      auto ld = [&](int o) { return use_win ? win[o] : m2f::load_logit(logits, dtype, qbase + o); };
#pragma unroll 4
      for (int j = 0; j < kPix / 8; ++j) {
        const int p = pg + 8 * j, r = p >> 5, c = p & 31;
        float s = 0.f;
        if (qq < Q && y0 + r < g.Ho && x0 + c < g.Wo) {
          auto stage1 = [&](const TapO& ty, const TapO& tx) {
            return m2f::blend4(ty.l0, ty.l1, tx.l0, tx.l1, ld(ty.o0 + tx.o0), ld(ty.o0 + tx.o1), ld(ty.o1 + tx.o0),
                               ld(ty.o1 + tx.o1));
          };
          float v;
          if (!g.two) {
            v = stage1(sY[r * 2], sX[c * 2]);
          } else {
            const float a = stage1(sY[r * 2], sX[c * 2]);
            const float bb = stage1(sY[r * 2], sX[c * 2 + 1]);
            const float cc = stage1(sY[r * 2 + 1], sX[c * 2]);
            const float d = stage1(sY[r * 2 + 1], sX[c * 2 + 1]);
            const float2 ly = sY2[r], lx = sX2[c];
            v = m2f::blend4(ly.x, ly.y, lx.x, lx.y, a, bb, cc, d);
          }
          s = m2f::sigmoidf_literal(v);
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

  // lane holds C[class = 32 i + (e & 3) + 8 (e >> 2) + 4 lh][pixel = (row wv, column li)]
  const int y = y0 + wv, x = x0 + li;
  const bool inside = y < g.Ho && x < g.Wo;
  if (labels == nullptr) {
    if (!inside) return;
    float* dst = semseg + (static_cast<int64_t>(b) * K * out_h + y) * out_w + x;
    const int64_t cs = static_cast<int64_t>(out_h) * out_w;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (k < K) dst[k * cs] = acc[i][e];
      }
  } else {
    // first maximum over k: ascending (i, e) is ascending k within a lane; then the two lane halves
    float best = -1.f;
    int bk = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (k < K && (acc[i][e] > best || (acc[i][e] == best && k < bk))) {
          best = acc[i][e];
          bk = k;
        }
      }
    const float ob = __shfl_xor(best, 32);
    const int ok = __shfl_xor(bk, 32);
    if (ob > best || (ob == best && ok < bk)) bk = ok;
    if (inside && lh == 0) labels[(static_cast<int64_t>(b) * out_h + y) * out_w + x] = static_cast<int16_t>(bk);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// panoptic pass: grid (ceil(out_w / 64), ceil(out_h / 4), B), 256 threads, a wave = 64 consecutive x of one row
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) panoptic_kernel(const void* __restrict__ logits, int dtype,
                                                       const int32_t* __restrict__ keep_idx,
                                                       const float* __restrict__ keep_score,
                                                       const int32_t* __restrict__ num_keep,
                                                       const int32_t* __restrict__ sizes, int Q, int h, int w, int Hp,
                                                       int Wp, int out_h, int out_w, int16_t* __restrict__ winner,
                                                       uint8_t* __restrict__ inside_out,
                                                       int32_t* __restrict__ counters) {
  __shared__ int cnt[3][kMaxQ];  // mask_area, original_area, intersection
  const int b = blockIdx.z;
  const Geo g = m2f::load_geo(sizes, b, h, w, Hp, Wp, out_h, out_w);
  const int y0 = blockIdx.y * 4, x0 = blockIdx.x * 64;
  if (y0 >= g.Ho || x0 >= g.Wo) return;
  const int tid = threadIdx.x;
  const int nk = max(0, min(num_keep[b], Q));
  for (int i = tid; i < 3 * kMaxQ; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int y = y0 + (tid >> 6), x = x0 + (tid & 63);
  const bool valid = y < g.Ho && x < g.Wo;
  const AxisTaps ay = m2f::axis_taps(min(y, g.Ho - 1), g.two, g.rh1, h, g.rh2, g.Hc);
  const AxisTaps ax = m2f::axis_taps(min(x, g.Wo - 1), g.two, g.rw1, w, g.rw2, g.Wc);
  const int64_t hw = static_cast<int64_t>(h) * w;
  float best = 0.f;
  int win = -1;
  bool win_in = false;
  for (int k = 0; k < nk; ++k) {
    const int q = max(0, min(keep_idx[b * Q + k], Q - 1));
    const float score = keep_score[b * Q + k];
    const int64_t base = (static_cast<int64_t>(b) * Q + q) * hw;
    const float v = m2f::logit_at(g.two, ay, ax, [&](int r, int c) { return m2f::load_logit(logits, dtype, base + r * w + c); });
    const float s = m2f::sigmoidf_literal(v);
    const bool in = valid && s >= 0.5f;
    const unsigned long long bal = __ballot(in);
    if ((tid & 63) == 0 && bal != 0) atomicAdd(&cnt[1][k], __popcll(bal));
    const float p = score * s;
    if (win < 0 || p > best) {
      best = p;
      win = k;
      win_in = in;
    }
  }
  if (valid) {
    const int64_t o = (static_cast<int64_t>(b) * out_h + y) * out_w + x;
    winner[o] = static_cast<int16_t>(win);
    inside_out[o] = win_in ? 1 : 0;
    if (win >= 0) {
      atomicAdd(&cnt[0][win], 1);
      if (win_in) atomicAdd(&cnt[2][win], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * nk; i += 256) {
    const int k = i / 3, c = i - 3 * k;
    if (cnt[c][k] != 0) atomicAdd(&counters[(b * Q + k) * 3 + c], cnt[c][k]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// instance: grid (num_tiles, max_sel, B); a tile = 1024 consecutive pixels of the image's (Ho, Wo) raster
// ---------------------------------------------------------------------------------------------------------------
constexpr int kInstTile = 1024;

__global__ void __launch_bounds__(256) instance_kernel(const void* __restrict__ logits, int dtype,
                                                       const int32_t* __restrict__ sel_idx,
                                                       const int32_t* __restrict__ num_sel,
                                                       const int32_t* __restrict__ sizes, int Q, int S, int h, int w,
                                                       int Hp, int Wp, int out_h, int out_w, int num_tiles,
                                                       uint8_t* __restrict__ masks, float* __restrict__ partials) {
  __shared__ float red[2][4];
  const int b = blockIdx.z, s = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x;
  const Geo g = m2f::load_geo(sizes, b, h, w, Hp, Wp, out_h, out_w);
  float* part = partials + ((static_cast<int64_t>(b) * S + s) * num_tiles + tile) * 2;
  const int ns = max(0, min(num_sel[b], S));
  const int64_t npix = (g.Ho > 0 && g.Wo > 0) ? static_cast<int64_t>(g.Ho) * g.Wo : 0;
  if (s >= ns || static_cast<int64_t>(tile) * kInstTile >= npix) {
    if (tid == 0) part[0] = part[1] = 0.f;
    return;
  }
  const int q = max(0, min(sel_idx[b * S + s], Q - 1));
  const int64_t base = (static_cast<int64_t>(b) * Q + q) * h * w;
  float sum = 0.f, count = 0.f;
#pragma unroll
  for (int j = 0; j < kInstTile / 256; ++j) {
    const int64_t pix = static_cast<int64_t>(tile) * kInstTile + j * 256 + tid;
    if (pix < npix) {
      const int y = static_cast<int>(pix / g.Wo), x = static_cast<int>(pix - static_cast<int64_t>(y) * g.Wo);
      const AxisTaps ay = m2f::axis_taps(y, g.two, g.rh1, h, g.rh2, g.Hc);
      const AxisTaps ax = m2f::axis_taps(x, g.two, g.rw1, w, g.rw2, g.Wc);
      const float v = m2f::logit_at(g.two, ay, ax, [&](int r, int c) { return m2f::load_logit(logits, dtype, base + r * w + c); });
      const bool on = v > 0.f;
      masks[((static_cast<int64_t>(b) * S + s) * out_h + y) * out_w + x] = on ? 1 : 0;
      if (on) {
        sum += m2f::sigmoidf_literal(v);
        count += 1.f;
      }
    }
  }
  sum = wave_sum(sum);  // fixed butterfly order, then the fixed wave order below: bitwise repeatable partials
  count = wave_sum(count);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sum;
    red[1][tid >> 6] = count;
  }
  __syncthreads();
  if (tid == 0) {
    part[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    part[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// grid (max_sel, B), 64 threads: lane t adds tiles t, t + 64, ... in order, then a fixed butterfly
__global__ void __launch_bounds__(64) instance_combine_kernel(const float* __restrict__ partials, int S, int num_tiles,
                                                              float* __restrict__ sums) {
  const int64_t row = static_cast<int64_t>(blockIdx.y) * S + blockIdx.x;
  const float* part = partials + row * num_tiles * 2;
  float sum = 0.f, count = 0.f;
  for (int t = threadIdx.x; t < num_tiles; t += 64) {
    sum += part[t * 2];
    count += part[t * 2 + 1];
  }
  sum = wave_sum(sum);  // the fixed butterfly of the comment above: the order is part of the result
  count = wave_sum(count);
  if (threadIdx.x == 0) {
    sums[row * 2] = sum;
    sums[row * 2 + 1] = count;
  }
}

int check_common(const char* fn, const void* logits, int dtype, const int32_t* sizes, int batch, int Q, int h, int w,
                 int Hp, int Wp, int out_h, int out_w) {
  if (!logits || !sizes) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (!m2f::is_float_dtype(dtype)) return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, dtype);
  if (batch <= 0 || Q <= 0 || h <= 0 || w <= 0 || Hp <= 0 || Wp <= 0 || out_h <= 0 || out_w <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (Q > kMaxQ) return m2f::fail(M2F_EUNSUPPORTED, "%s: num_queries %d > %d", fn, Q, kMaxQ);
  if (batch > 65535 || out_h > 65535 * 4 || static_cast<int64_t>(h) * w > 0x7fffffff ||
      static_cast<int64_t>(out_h) * out_w > 0x7fffffff || static_cast<int64_t>(batch) * Q * 4 > 0x7fffffff)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  return M2F_OK;
}

template <int KT>
int launch_semantic(const void* logits, int dtype, const float* probs, const int32_t* sizes, int B, int Q, int K, int h,
                    int w, int Hp, int Wp, int out_h, int out_w, float* semseg, int16_t* labels, hipStream_t st) {
  const char* fn = "m2f_infer_semantic";
  if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(&semantic_kernel<KT>), sem_lds_bytes(KT), fn)) return rc;
  const dim3 grid(m2f::ceil_div(out_w, kTW), m2f::ceil_div(out_h, kTH), B);
  semantic_kernel<KT><<<grid, 256, sem_lds_bytes(KT), st>>>(logits, dtype, probs, sizes, Q, K, h, w, Hp, Wp, out_h,
                                                          out_w, semseg, labels);
  return m2f::check_launch(fn);
}

}  // namespace

extern "C" int m2f_infer_semantic(const void* logits, int dtype, const float* probs, const int32_t* sizes, int batch,
                                  int num_queries, int num_classes, int in_h, int in_w, int pad_h, int pad_w, int out_h,
                                  int out_w, float* semseg, int16_t* labels, void* stream) {
  const char* fn = "m2f_infer_semantic";
  if (!probs || (!semseg && !labels)) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (int rc = check_common(fn, logits, dtype, sizes, batch, num_queries, in_h, in_w, pad_h, pad_w, out_h, out_w)) return rc;
  if (num_classes <= 0) return m2f::fail(M2F_EINVAL, "%s: num_classes must be positive", fn);
  if (num_classes > kMaxK) return m2f::fail(M2F_EUNSUPPORTED, "%s: num_classes %d > %d", fn, num_classes, kMaxK);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = M2F_OK;
  if (!m2f::dispatch_one_of<1, 2, 3, 4, 5, 6, 7, 8>((num_classes + 31) / 32, [&](auto kt) {
        rc = launch_semantic<kt.value>(logits, dtype, probs, sizes, batch, num_queries, num_classes, in_h, in_w, pad_h,
                                       pad_w, out_h, out_w, semseg, labels, st);
      }))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: num_classes %d", fn, num_classes);
  return rc;
}

extern "C" int m2f_infer_panoptic_pass(const void* logits, int dtype, const int32_t* keep_idx, const float* keep_score,
                                       const int32_t* num_keep, const int32_t* sizes, int batch, int num_queries,
                                       int in_h, int in_w, int pad_h, int pad_w, int out_h, int out_w, int16_t* winner,
                                       uint8_t* inside, int32_t* counters, void* stream) {
  const char* fn = "m2f_infer_panoptic_pass";
  if (!keep_idx || !keep_score || !num_keep || !winner || !inside || !counters)
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (int rc = check_common(fn, logits, dtype, sizes, batch, num_queries, in_h, in_w, pad_h, pad_w, out_h, out_w)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipError_t e = m2f::zero_async(counters, static_cast<size_t>(batch) * num_queries * 3 * sizeof(int32_t), st);
      e != hipSuccess)
    return m2f::fail(M2F_ELAUNCH, "%s: %s", fn, hipGetErrorString(e));
  const dim3 grid(m2f::ceil_div(out_w, 64), m2f::ceil_div(out_h, 4), batch);
  panoptic_kernel<<<grid, 256, 0, st>>>(logits, dtype, keep_idx, keep_score, num_keep, sizes, num_queries, in_h, in_w,
                                        pad_h, pad_w, out_h, out_w, winner, inside, counters);
  return m2f::check_launch(fn);
}

extern "C" int m2f_infer_instance(const void* logits, int dtype, const int32_t* sel_idx, const int32_t* num_sel,
                                  const int32_t* sizes, int batch, int num_queries, int max_sel, int in_h, int in_w,
                                  int pad_h, int pad_w, int out_h, int out_w, int num_tiles, uint8_t* masks,
                                  float* partials, float* sums, void* stream) {
  const char* fn = "m2f_infer_instance";
  if (!sel_idx || !num_sel || !masks || !partials || !sums) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (int rc = check_common(fn, logits, dtype, sizes, batch, num_queries, in_h, in_w, pad_h, pad_w, out_h, out_w)) return rc;
  if (max_sel <= 0 || max_sel > 65535) return m2f::fail(M2F_EINVAL, "%s: max_sel %d outside [1, 65535]", fn, max_sel);
  const int64_t tiles = (static_cast<int64_t>(out_h) * out_w + kInstTile - 1) / kInstTile;
  if (static_cast<int64_t>(out_h) * out_w > (1 << 24))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: out_h * out_w > 2^24 (the fp32 pixel count of a mask would not be exact)", fn);
  if (num_tiles != tiles)
    return m2f::fail(M2F_EINVAL, "%s: num_tiles %d != ceil(out_h * out_w / %d) = %lld", fn, num_tiles, kInstTile,
                     static_cast<long long>(tiles));
  hipStream_t st = static_cast<hipStream_t>(stream);
  instance_kernel<<<dim3(num_tiles, max_sel, batch), 256, 0, st>>>(logits, dtype, sel_idx, num_sel, sizes, num_queries,
                                                                  max_sel, in_h, in_w, pad_h, pad_w, out_h, out_w,
                                                                  num_tiles, masks, partials);
  if (int rc = m2f::check_launch(fn)) return rc;
  instance_combine_kernel<<<dim3(max_sel, batch), 64, 0, st>>>(partials, max_sel, num_tiles, sums);
  return m2f::check_launch(fn);
}

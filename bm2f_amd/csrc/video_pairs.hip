// Temporal pairwise loss and temporal pair mining of the box-supervised video criterion.
//
// Reference (mask2former_video):
//   loss    modeling/criterion_proj_spatpair_temppair.py:25-69, :269-334: for every matched instance, every
//           frame pair (t, t+1) and every mined pixel pair, s = -log(sig(a)sig(b) + sig(-a)sig(-b)) of the
//           two mask logits, summed and divided by the pair count -- three nested Python loops with one
//           gather per (instance, frame pair);
//   mining  utils/weaksup_utils.py:64-165 + video_maskformer_model.py:523-558: per instance and frame pair,
//           a full cdist matrix between the features of the two box patches, only to take its arg-top-1.
//
// Here all pairs of all targets are packed once per criterion call into flat int32 arrays (target row,
// frame, linear pixel in frame t, linear pixel in frame t+1).  The forward kernel evaluates one pair per
// thread and reduces to per-block partials (fixed order: deterministic).  The backward kernel walks the
// endpoint list sorted by (target, frame, pixel): the thread that sits on the first endpoint of a segment
// sums the segment in stored order and writes the pixel's gradient once -- no atomics, bitwise repeatable.
// The mining kernel tiles the distance matrix 64 x 64 through LDS with a running arg-min per current pixel,
// so the matrix is never written.
#include "bm2f.h"
#include "common.h"
#include "device_util.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

constexpr int NT = 256;

// the pair term and its gradient are device_util.h's, the very functions of the spatial loss (weaksup.hip)
using m2f::log_sigmoid, m2f::pair_grad, m2f::pair_term, m2f::sigmoid_neg, m2f::wave_sum;

// Matched row n of pair i, or -1 when the pair is dead: a negative / out-of-range target row, frame or
// pixel (the packer marks invalid pairs with row -1) or a target that no query was matched to.
__device__ __forceinline__ int pair_row(int i, int N, int T, int64_t HW, const int* __restrict__ row_of_target,
                                        int n_targets, const int* __restrict__ prow, const int* __restrict__ pt,
                                        const int* __restrict__ p0, const int* __restrict__ p1) {
  const int g = prow[i], t = pt[i], a0 = p0[i], a1 = p1[i];
  if (g < 0 || g >= n_targets || t < 0 || t >= T - 1 || a0 < 0 || a0 >= HW || a1 < 0 || a1 >= HW) return -1;
  const int n = row_of_target[g];
  return (n >= 0 && n < N) ? n : -1;
}

__global__ void __launch_bounds__(NT) temporal_fwd_kernel(const float* __restrict__ src, int N, int T, int64_t HW,
                                                          const int* __restrict__ row_of_target, int n_targets,
                                                          const int* __restrict__ prow, const int* __restrict__ pt,
                                                          const int* __restrict__ p0, const int* __restrict__ p1, int P,
                                                          float* __restrict__ part_sum, int* __restrict__ part_cnt) {
  __shared__ float red_s[NT / 64];
  __shared__ int red_c[NT / 64];
  const int i = blockIdx.x * NT + threadIdx.x;
  float s = 0.f;
  int live = 0;
  if (i < P) {
    const int n = pair_row(i, N, T, HW, row_of_target, n_targets, prow, pt, p0, p1);
    if (n >= 0) {
      const float* base = src + (static_cast<int64_t>(n) * T + pt[i]) * HW;
      const float a = base[p0[i]], b = base[HW + p1[i]];
      s = pair_term(a, log_sigmoid(a), b, log_sigmoid(b));
      live = 1;
    }
  }
  s = wave_sum(s);
  const int c = __popcll(__ballot(live));
  if ((threadIdx.x & 63) == 0) {
    red_s[threadIdx.x >> 6] = s;
    red_c[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ts = 0.f;
    int tc = 0;
    for (int k = 0; k < NT / 64; ++k) {
      ts += red_s[k];
      tc += red_c[k];
    }
    part_sum[blockIdx.x] = ts;
    part_cnt[blockIdx.x] = tc;
  }
}

// Endpoint e (sorted by key = (target * T + frame) * HW + pixel, stable) is pair ep_code[e] >> 1, side
// ep_code[e] & 1 (0: the frame-t pixel, 1: the frame-(t+1) pixel).  The thread on the first endpoint of a
// run of equal keys owns the pixel.
__global__ void __launch_bounds__(NT) temporal_bwd_kernel(const float* __restrict__ src, int N, int T, int64_t HW,
                                                          const int* __restrict__ row_of_target, int n_targets,
                                                          const int* __restrict__ prow, const int* __restrict__ pt,
                                                          const int* __restrict__ p0, const int* __restrict__ p1, int P,
                                                          const int64_t* __restrict__ ep_key,
                                                          const int* __restrict__ ep_code, int64_t E,
                                                          const float* __restrict__ grad_scale,
                                                          float* __restrict__ grad) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
  if (e >= E) return;
  const int64_t key = ep_key[e];
  if (key < 0 || (e > 0 && ep_key[e - 1] == key)) return;
  const int64_t gf = key / HW;
  const int64_t pix = key - gf * HW;
  const int64_t g = gf / T;
  const int f = static_cast<int>(gf - g * T);
  if (g >= n_targets) return;
  const int n = row_of_target[g];
  if (n < 0 || n >= N) return;
  const float* inst = src + static_cast<int64_t>(n) * T * HW;
  const float a = inst[f * HW + pix];
  const float sna = sigmoid_neg(a);
  float acc = 0.f;
  for (int64_t j = e; j < E && ep_key[j] == key; ++j) {
    const int code = ep_code[j];
    const int i = code >> 1;
    if (i < 0 || i >= P) continue;
    if (pair_row(i, N, T, HW, row_of_target, n_targets, prow, pt, p0, p1) != n) continue;
    const float b = (code & 1) ? inst[pt[i] * HW + p0[i]] : inst[(pt[i] + 1) * HW + p1[i]];
    acc += pair_grad(a, sna, b);
  }
  grad[static_cast<int64_t>(n) * T * HW + f * HW + pix] = acc * grad_scale[0];
}

// ---------------------------------------------------------------------------------------------------------
// mining: for every pixel of the frame-t box (row-major), the frame-(t+1) box pixel at the smallest squared
// L2 feature distance (first minimum in row-major order).  Distances are summed as (a - b)^2 in fp32: no
// |a|^2 + |b|^2 - 2ab cancellation, so near-identical features keep their order.
// ---------------------------------------------------------------------------------------------------------
constexpr int MT = 64;   // pixels per tile side (current and next)
constexpr int DK = 16;   // feature channels per LDS stage
constexpr int MP = MT + 4;  // LDS row pitch: rows stay 16-byte aligned for the float4 reads
constexpr int kSegInts = 10;  // t, cx0, cy0, cw, nc, nx0, ny0, nw, nn, out_off

__global__ void __launch_bounds__(NT) temporal_mine_kernel(const float* __restrict__ feats, int T, int D, int h, int w,
                                                           const int* __restrict__ segs, int n_segs,
                                                           const int* __restrict__ blocks, int* __restrict__ out_p1,
                                                           int n_out) {
  __shared__ __attribute__((aligned(16))) float A[DK][MP];
  __shared__ __attribute__((aligned(16))) float Bn[DK][MP];
  const int sid = blocks[2 * blockIdx.x], c0 = blocks[2 * blockIdx.x + 1] * MT;
  if (sid < 0 || sid >= n_segs) return;
  const int* sg = segs + sid * kSegInts;
  const int t = sg[0], cx0 = sg[1], cy0 = sg[2], cw = sg[3], nc = sg[4];
  const int nx0 = sg[5], ny0 = sg[6], nw = sg[7], nn = sg[8], out_off = sg[9];
  // the host wrapper builds the table from boxes clipped to the frame; refuse anything else
  if (t < 0 || t >= T - 1 || cw <= 0 || nw <= 0 || nc <= 0 || nn <= 0 || cx0 < 0 || cy0 < 0 || nx0 < 0 || ny0 < 0 ||
      cx0 + cw > w || nx0 + nw > w || cy0 + (nc + cw - 1) / cw > h || ny0 + (nn + nw - 1) / nw > h || c0 >= nc)
    return;
  const int64_t plane = static_cast<int64_t>(h) * w;
  const float* fc = feats + static_cast<int64_t>(t) * D * plane;
  const float* fn = fc + static_cast<int64_t>(D) * plane;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  float best[4];
  int besti[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best[i] = INFINITY;
    besti[i] = 0;
  }
  for (int n0 = 0; n0 < nn; n0 += MT) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += DK) {
      for (int idx = threadIdx.x; idx < DK * MT; idx += NT) {
        const int k = idx / MT, j = idx % MT;
        float va = 0.f, vb = 0.f;
        if (d0 + k < D) {
          const int jc = c0 + j, jn = n0 + j;
          if (jc < nc) va = fc[(d0 + k) * plane + static_cast<int64_t>(cy0 + jc / cw) * w + cx0 + jc % cw];
          if (jn < nn) vb = fn[(d0 + k) * plane + static_cast<int64_t>(ny0 + jn / nw) * w + nx0 + jn % nw];
        }
        A[k][j] = va;
        Bn[k][j] = vb;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < DK; ++k) {
        const float4 a4 = *reinterpret_cast<const float4*>(&A[k][ty * 4]);
        const float4 b4 = *reinterpret_cast<const float4*>(&Bn[k][tx * 4]);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float df = av[i] - bv[j];
            acc[i][j] = fmaf(df, df, acc[i][j]);
          }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int jn = n0 + tx * 4 + j;
        if (jn < nn && acc[i][j] < best[i]) {  // strict: the first minimum wins
          best[i] = acc[i][j];
          besti[i] = jn;
        }
      }
  }
  // the 16 lanes tx = 0..15 of one ty are consecutive lanes of a wave
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    for (int off = 8; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best[i], off);
      const int oi = __shfl_xor(besti[i], off);
      if (ob < best[i] || (ob == best[i] && oi < besti[i])) {
        best[i] = ob;
        besti[i] = oi;
      }
    }
    const int jc = c0 + ty * 4 + i;
    if (tx == 0 && jc < nc && out_off >= 0 && out_off + jc < n_out)
      out_p1[out_off + jc] = (ny0 + besti[i] / nw) * w + nx0 + besti[i] % nw;
  }
}

int check_temporal(const char* fn, const void* src, int N, int T, int H, int W, int n_targets, int P) {
  if (N < 0 || T < 0 || H < 0 || W < 0 || n_targets < 0 || P < 0) return m2f::fail(M2F_EINVAL, "%s: negative size", fn);
  if (static_cast<int64_t>(H) * W > INT32_MAX) return m2f::fail(M2F_EUNSUPPORTED, "%s: H * W > 2^31 - 1", fn);
  if (N > 0 && T > 0 && H > 0 && W > 0 && !src) return m2f::fail(M2F_EINVAL, "%s: null src", fn);
  return M2F_OK;
}

}  // namespace

extern "C" int m2f_temporal_blocks(int P) { return P > 0 ? static_cast<int>(m2f::ceil_div(P, NT)) : 0; }

extern "C" int m2f_temporal_pairs_fwd(const float* src, int N, int T, int H, int W, const int* row_of_target,
                                      int n_targets, const int* pair_row, const int* pair_t, const int* pair_p0,
                                      const int* pair_p1, int P, float* part_sum, int* part_cnt, void* stream) {
  const char* fn = "m2f_temporal_pairs_fwd";
  if (int e = check_temporal(fn, src, N, T, H, W, n_targets, P)) return e;
  if (P == 0) return m2f::ok();
  if (!row_of_target || !pair_row || !pair_t || !pair_p0 || !pair_p1 || !part_sum || !part_cnt)
    return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  temporal_fwd_kernel<<<m2f::ceil_div(P, NT), NT, 0, static_cast<hipStream_t>(stream)>>>(
      src, N, T, static_cast<int64_t>(H) * W, row_of_target, n_targets, pair_row, pair_t, pair_p0, pair_p1, P, part_sum,
      part_cnt);
  return m2f::check_launch(fn);
}

extern "C" int m2f_temporal_pairs_bwd(const float* src, int N, int T, int H, int W, const int* row_of_target,
                                      int n_targets, const int* pair_row, const int* pair_t, const int* pair_p0,
                                      const int* pair_p1, int P, const int64_t* ep_key, const int* ep_code,
                                      const float* grad_scale, float* grad, void* stream) {
  const char* fn = "m2f_temporal_pairs_bwd";
  if (int e = check_temporal(fn, src, N, T, H, W, n_targets, P)) return e;
  if (P == 0 || N == 0) return m2f::ok();
  if (!row_of_target || !pair_row || !pair_t || !pair_p0 || !pair_p1 || !ep_key || !ep_code || !grad_scale || !grad)
    return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  const int64_t E = 2 * static_cast<int64_t>(P);
  temporal_bwd_kernel<<<m2f::ceil_div(E, NT), NT, 0, static_cast<hipStream_t>(stream)>>>(
      src, N, T, static_cast<int64_t>(H) * W, row_of_target, n_targets, pair_row, pair_t, pair_p0, pair_p1, P, ep_key,
      ep_code, E, grad_scale, grad);
  return m2f::check_launch(fn);
}

extern "C" int m2f_temporal_mine(const float* feats, int T, int D, int h, int w, const int* segs, int n_segs,
                                 const int* blocks, int n_blocks, int* out_p1, int n_out, void* stream) {
  const char* fn = "m2f_temporal_mine";
  if (T < 0 || D < 1 || h < 0 || w < 0 || n_segs < 0 || n_blocks < 0 || n_out < 0)
    return m2f::fail(M2F_EINVAL, "%s: bad sizes", fn);
  if (n_blocks == 0) return m2f::ok();
  if (!feats || !segs || !blocks || !out_p1) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  temporal_mine_kernel<<<n_blocks, NT, 0, static_cast<hipStream_t>(stream)>>>(feats, T, D, h, w, segs, n_segs, blocks,
                                                                              out_p1, n_out);
  return m2f::check_launch(fn);
}

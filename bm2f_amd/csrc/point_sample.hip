// Point sampling for the mask-supervised matcher and set criterion.
//
// Reference (mask2former / mask2former_video):
//   matcher    modeling/matcher.py:479-597 (video: :503-590): per image, K random points shared by all Q
//              predictions and G targets; point_sample (grid_sample, bilinear, zeros, align_corners=False) of both,
//              then (Q, K) x (K, G) contractions for the sigmoid-CE and dice costs, one image at a time.
//   criterion  modeling/criterion.py:827-882 (video: criterion.py:194-240): per matched mask, oversampled points ->
//              uncertainty -|x| -> top-k -> point_sample of logits and labels -> BCE and dice.
//
// point_sample(x, u) at normalised u = (ux, uy): pixel coordinate (ux * Wn - 0.5, uy * Hn - 0.5), the four
// neighbours weighted as torch's grid_sampler does ((x1 - px) * (y1 - py), ...), a corner outside the plane
// contributes 0.  (Hn, Wn) is the extent the coordinates are normalised over: the plane's own size, or, for the
// image criterion's targets, the batch's padded size (the pad itself is never materialised: a corner beyond the
// plane reads as the zero pad would).
//
// Logits are fp32 / fp16 / bf16 and evaluated in fp32; targets are uint8 (bool) or fp32 planes read in place through
// per-image / per-row pointer tables; prediction rows are addressed through a plane index table, never through a
// gathered copy.  Plane offsets are 64-bit; offsets inside a plane are 32-bit (H * W < 2^31 is checked).
//
// Label-map targets (the *_labels entry points): an image's G targets are one (Ht, Wt) map of uint8 / int16 / int32
// labels plus G int32 ids, target g being the set map == ids[g].  The kernels are the dense ones with another target
// reader (the TR template parameter): the value of a tap is (label == id) ? 1 : 0 where the dense reader converts a
// plane element, the taps are summed in the same order and a zero-weight tap is skipped alike, so every result is
// bitwise what the dense uint8 planes map[None] == ids[:, None, None] give.  The planes never exist.
//
// Match cost: a workgroup owns one (image, frame, 256-point tile).  Targets are sampled once per 32-target chunk
// into LDS, predictions per 32-query chunk and 64-point sub-tile; the (Q, G) partials of sum x t and sum sig(x) t
// are contracted from LDS with fp32 operands and fp64 accumulators, the row sums of softplus(x) / sig(x) and the
// column sums of t by wave reductions.  Per-tile partials go to a workspace; a second kernel sums them in tile order
// in fp64 and writes the weighted cost: no atomics, bitwise repeatable, and no (B, Q, K) tensor in memory.
#include "bm2f.h"
#include "common.h"
#include "device_util.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int PT = 64;            // points per sub-tile: one per lane
constexpr int SUB = 4;            // sub-tiles per workgroup
constexpr int TILE = PT * SUB;    // points per workgroup
constexpr int QC = 32, GC = 32;   // query / target chunk held in LDS
constexpr int LOSS_PER_THREAD = 4;
constexpr int LOSS_CHUNK = NT * LOSS_PER_THREAD;
constexpr int kTgtU8 = 0, kTgtF32 = 1;

using m2f::load_logit, m2f::wave_sum;

// Not device_util.h's exp2 forms: expf / log1pf with an IEEE divide, which the mask criterion's parity bars need.
__device__ __forceinline__ float sigmoid(float x) {  // accurate in both tails
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// The four bilinear taps of one point in an (H, W) plane; a tap outside the plane has weight 0 (offset 0).
struct Taps {
  int off[4];
  float w[4];
};

__device__ __forceinline__ Taps make_taps(float ux, float uy, int Hn, int Wn, int H, int W) {
  Taps t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    t.off[i] = 0;
    t.w[i] = 0.f;
  }
  const float px = fmaf(ux, static_cast<float>(Wn), -0.5f), py = fmaf(uy, static_cast<float>(Hn), -0.5f);
  // also false for NaN; px >= W or <= -1 has no corner in the plane
  if (!(px > -1.f && px < static_cast<float>(W) && py > -1.f && py < static_cast<float>(H))) return t;
  const float fx = floorf(px), fy = floorf(py);
  const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy);   // in [-1, W-1] x [-1, H-1]
  const float ax = px - fx, ay = py - fy, bx = (fx + 1.f) - px, by = (fy + 1.f) - py;
  const bool vx0 = x0 >= 0, vx1 = x0 + 1 < W, vy0 = y0 >= 0, vy1 = y0 + 1 < H;
  if (vy0 && vx0) { t.off[0] = y0 * W + x0; t.w[0] = bx * by; }
  if (vy0 && vx1) { t.off[1] = y0 * W + x0 + 1; t.w[1] = ax * by; }
  if (vy1 && vx0) { t.off[2] = (y0 + 1) * W + x0; t.w[2] = bx * ay; }
  if (vy1 && vx1) { t.off[3] = (y0 + 1) * W + x0 + 1; t.w[3] = ax * ay; }
  return t;
}

__device__ __forceinline__ float sample_logit(const void* __restrict__ base, int dtype, int64_t plane_off, const Taps& t) {
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (t.w[i] != 0.f) v += load_logit(base, dtype, plane_off + t.off[i]) * t.w[i];
  return v;
}

// Target readers.  Dense<TT>: one plane of TT (uint8 or float) per target.  Labels<LT>: one map of LT labels per image,
// a target is an id.  Table rows (int64):
//   match   Dense  [plane pointer, G, Ht, Wt]          Labels  [map pointer, G, Ht, Wt, pointer to G int32 ids]
//   rows    Dense  [plane pointer, Ht, Wt, Hn, Wn]     Labels  [map pointer, id, Ht, Wt, Hn, Wn]
template <typename TT>
struct Dense {
  using Elem = TT;
  static constexpr bool kLabels = false;
  static constexpr int kMatchFields = 4, kRowFields = 5;
};

template <typename LT>
struct Labels {
  using Elem = LT;
  static constexpr bool kLabels = true;
  static constexpr int kMatchFields = 5, kRowFields = 6;
};

// the value of one tap: the plane's element, or whether the map's label is the target's id
template <class TR>
__device__ __forceinline__ float tap_value(typename TR::Elem e, int id) {
  if constexpr (TR::kLabels) return static_cast<int>(e) == id ? 1.f : 0.f;
  else return static_cast<float>(e);
}

template <class TR>
__device__ __forceinline__ float sample_target(const typename TR::Elem* __restrict__ plane, int id, const Taps& t) {
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (t.w[i] != 0.f) v += tap_value<TR>(plane[t.off[i]], id) * t.w[i];
  return v;
}

// one row of the loss kernels' target table
template <class TR>
struct RowTarget {
  const typename TR::Elem* plane;
  int id, Ht, Wt, Hn, Wn;
  __device__ __forceinline__ explicit RowTarget(const int64_t* __restrict__ tb) {
    plane = reinterpret_cast<const typename TR::Elem*>(tb[0]);
    id = TR::kLabels ? static_cast<int>(tb[1]) : 0;
    const int64_t* s = tb + (TR::kLabels ? 2 : 1);
    Ht = static_cast<int>(s[0]), Wt = static_cast<int>(s[1]), Hn = static_cast<int>(s[2]), Wn = static_cast<int>(s[3]);
  }
  __device__ __forceinline__ bool ok() const { return plane != nullptr && Ht > 0 && Wt > 0; }
  __device__ __forceinline__ float sample(float ux, float uy) const {
    return sample_target<TR>(plane, id, make_taps(ux, uy, Hn, Wn, Ht, Wt));
  }
};

// ---------------------------------------------------------------------------------------------------------
// match cost, phase 1: per-tile partials.  Workspace record of (image b, frame t, tile):
//   [Q*Gm] sum x t | [Q*Gm] sum sig(x) t | [Q] sum softplus(x) | [Q] sum sig(x) | [Gm] sum t
// Only columns g < G_b are written (and read by phase 2).  tgt (B, TR::kMatchFields) int64, see the readers.
// Labels: thread tid reads the four corner labels and weights of point k0 + tid once into LDS (8 KiB), whatever G
// is; a chunk's ids are staged beside them and t[g][p] = sum_i w_i (label_i == id_g) is formed from registers.
// ---------------------------------------------------------------------------------------------------------
template <class TR>
__global__ void __launch_bounds__(NT) match_partial_kernel(const void* __restrict__ masks, int dtype, int Q, int T, int H,
                                                           int W, const float* __restrict__ coords, int K,
                                                           const int64_t* __restrict__ tgt, int Gm,
                                                           float* __restrict__ ws, int64_t rec, int ntiles) {
  __shared__ float tt[GC][TILE + 1];
  __shared__ float xs[QC][PT + 1], sg[QC][PT + 1];
  __shared__ float rsp[QC], rss[QC], cts[GC];
  constexpr int kStage = TR::kLabels ? TILE : 1;   // the label reader's per-point corners; unused by the dense one
  __shared__ float lw[4][kStage];
  __shared__ int ll[4][kStage], lid[TR::kLabels ? GC : 1];
  using TT = typename TR::Elem;
  const int tile = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t* tb = tgt + TR::kMatchFields * static_cast<int64_t>(b);
  const TT* tbase = reinterpret_cast<const TT*>(tb[0]);
  const int G = static_cast<int>(tb[1] < Gm ? tb[1] : Gm);
  const int Ht = static_cast<int>(tb[2]), Wt = static_cast<int>(tb[3]);
  if (G <= 0 || Ht <= 0 || Wt <= 0 || tbase == nullptr) return;
  const int32_t* ids = TR::kLabels ? reinterpret_cast<const int32_t*>(tb[TR::kMatchFields - 1]) : nullptr;
  if (TR::kLabels && ids == nullptr) return;
  float* out = ws + (static_cast<int64_t>(b) * T * ntiles + static_cast<int64_t>(t) * ntiles + tile) * rec;
  const int64_t qg = static_cast<int64_t>(Q) * Gm;
  float* o_xt = out;
  float* o_st = out + qg;
  float* o_sp = out + 2 * qg;
  float* o_ss = o_sp + Q;
  float* o_ts = o_ss + Q;
  const int64_t hw = static_cast<int64_t>(H) * W, thw = static_cast<int64_t>(Ht) * Wt;
  const float* cb = coords + static_cast<int64_t>(b) * K * 2;
  const int k0 = tile * TILE;
  const int qa = (tid >> 4) * 2, ga = tid & 15;   // this thread's 2 x 2 outputs: q in {qa, qa+1}, g in {ga, ga+16}

  if constexpr (TR::kLabels) {   // made visible by the barriers that open the chunk loop (G > 0)
    const int k = k0 + tid;
    const bool live = k < K;
    const Taps tp = make_taps(live ? cb[2 * k] : -4.f, live ? cb[2 * k + 1] : -4.f, Ht, Wt, Ht, Wt);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lw[i][tid] = tp.w[i];
      ll[i][tid] = tp.w[i] != 0.f ? static_cast<int>(tbase[tp.off[i]]) : 0;
    }
  }

  for (int g0 = 0; g0 < G; g0 += GC) {
    __syncthreads();   // the previous chunk's contraction has finished with tt
    if (tid < GC) {
      cts[tid] = 0.f;
      if constexpr (TR::kLabels) lid[tid] = g0 + tid < G ? ids[g0 + tid] : 0;
    }
    __syncthreads();
    for (int s = 0; s < SUB; ++s) {
      if constexpr (TR::kLabels) {
        int lab[4];
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lab[i] = ll[i][s * PT + lane];
          w[i] = lw[i][s * PT + lane];   // all 0 for a point beyond K
        }
        for (int gi = wv; gi < GC; gi += NT / 64) {
          float v = 0.f;
          if (g0 + gi < G) {
            const int id = lid[gi];
#pragma unroll
            for (int i = 0; i < 4; ++i)   // sample_target's order and its skip of zero-weight taps
              if (w[i] != 0.f) v += (lab[i] == id ? 1.f : 0.f) * w[i];
          }
          tt[gi][s * PT + lane] = v;
          const float sum = wave_sum(v);
          if (lane == 0) cts[gi] += sum;   // gi belongs to this wave alone
        }
      } else {
        const int k = k0 + s * PT + lane;
        const bool live = k < K;
        Taps tp = make_taps(live ? cb[2 * k] : -4.f, live ? cb[2 * k + 1] : -4.f, Ht, Wt, Ht, Wt);
        for (int gi = wv; gi < GC; gi += NT / 64) {
          const int g = g0 + gi;
          float v = 0.f;
          if (live && g < G) v = sample_target<TR>(tbase + (static_cast<int64_t>(g) * T + t) * thw, 0, tp);
          tt[gi][s * PT + lane] = v;
          const float sum = wave_sum(v);
          if (lane == 0) cts[gi] += sum;   // gi belongs to this wave alone
        }
      }
    }
    __syncthreads();
    if (tid < GC && g0 + tid < G) o_ts[g0 + tid] = cts[tid];

    for (int q0 = 0; q0 < Q; q0 += QC) {
      double axt[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, ast[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
      if (tid < QC) {
        rsp[tid] = 0.f;
        rss[tid] = 0.f;
      }
      for (int s = 0; s < SUB; ++s) {
        __syncthreads();   // the previous sub-tile's contraction has finished with xs / sg
        const int k = k0 + s * PT + lane;
        const bool live = k < K;
        Taps tp = make_taps(live ? cb[2 * k] : -4.f, live ? cb[2 * k + 1] : -4.f, H, W, H, W);
        for (int qi = wv; qi < QC; qi += NT / 64) {
          const int q = q0 + qi;
          float x = 0.f, sx = 0.f, sp = 0.f;
          if (live && q < Q) {
            x = sample_logit(masks, dtype, ((static_cast<int64_t>(b) * Q + q) * T + t) * hw, tp);
            sx = sigmoid(x);
            sp = softplus(x);
          }
          xs[qi][lane] = x;
          sg[qi][lane] = sx;
          if (g0 == 0) {
            const float a = wave_sum(sp), c = wave_sum(sx);
            if (lane == 0) {   // qi belongs to this wave alone
              rsp[qi] += a;
              rss[qi] += c;
            }
          }
        }
        __syncthreads();
#pragma unroll 4
        for (int p = 0; p < PT; ++p) {
          const float x0 = xs[qa][p], x1 = xs[qa + 1][p], s0 = sg[qa][p], s1 = sg[qa + 1][p];
          const float t0 = tt[ga][s * PT + p], t1 = tt[ga + 16][s * PT + p];
          axt[0][0] += static_cast<double>(x0) * t0;
          axt[0][1] += static_cast<double>(x0) * t1;
          axt[1][0] += static_cast<double>(x1) * t0;
          axt[1][1] += static_cast<double>(x1) * t1;
          ast[0][0] += static_cast<double>(s0) * t0;
          ast[0][1] += static_cast<double>(s0) * t1;
          ast[1][0] += static_cast<double>(s1) * t0;
          ast[1][1] += static_cast<double>(s1) * t1;
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int q = q0 + qa + i, g = g0 + ga + 16 * j;
          if (q < Q && g < G) {
            o_xt[static_cast<int64_t>(q) * Gm + g] = static_cast<float>(axt[i][j]);
            o_st[static_cast<int64_t>(q) * Gm + g] = static_cast<float>(ast[i][j]);
          }
        }
      if (g0 == 0 && tid < QC && q0 + tid < Q) {   // rsp / rss were last written before the final barrier above
        o_sp[q0 + tid] = rsp[tid];
        o_ss[q0 + tid] = rss[tid];
      }
    }
  }
}

// phase 2: sum the ntot = T * ntiles records of image b in order (fp64) and write the weighted cost.  tgt has
// `fields` int64 per image, of which the first four are read.
__global__ void __launch_bounds__(NT) match_reduce_kernel(const float* __restrict__ ws, int64_t rec, int ntot, int B, int Q,
                                                          int Gm, const int64_t* __restrict__ tgt, int fields,
                                                          const float* __restrict__ cost_class, float w_class, float w_mask,
                                                          float w_dice, double n_points, float* __restrict__ cost) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
  const int64_t qg = static_cast<int64_t>(Q) * Gm;
  if (idx >= B * qg) return;
  const int b = static_cast<int>(idx / qg);
  const int64_t r = idx - b * qg;
  const int q = static_cast<int>(r / Gm), g = static_cast<int>(r - static_cast<int64_t>(q) * Gm);
  const int64_t* tb = tgt + fields * static_cast<int64_t>(b);
  if (g >= tb[1] || tb[2] <= 0 || tb[3] <= 0 || tb[0] == 0) {
    cost[idx] = 0.f;
    return;
  }
  double xt = 0.0, st = 0.0, sp = 0.0, ss = 0.0, ts = 0.0;
  const float* base = ws + static_cast<int64_t>(b) * ntot * rec;
  for (int i = 0; i < ntot; ++i, base += rec) {
    xt += base[r];
    st += base[qg + r];
    sp += base[2 * qg + q];
    ss += base[2 * qg + Q + q];
    ts += base[2 * qg + 2 * Q + g];
  }
  const float c_mask = static_cast<float>((sp - xt) / n_points);
  const float c_dice = static_cast<float>(1.0 - (2.0 * st + 1.0) / (ss + ts + 1.0));
  const float c_class = cost_class ? cost_class[idx] : 0.f;
  cost[idx] = w_mask * c_mask + w_class * c_class + w_dice * c_dice;
}

// ---------------------------------------------------------------------------------------------------------
// per-row coordinates: uncertainty, loss forward, loss backward.  plane (R,) int64: the row's plane of masks
// (n_planes, H, W); a row whose plane is out of range is skipped (zero output).
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) uncertainty_kernel(const void* __restrict__ masks, int dtype, int64_t n_planes, int H,
                                                         int W, const int64_t* __restrict__ plane, int R,
                                                         const float* __restrict__ coords, int P,
                                                         float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
  if (idx >= static_cast<int64_t>(R) * P) return;
  const int r = static_cast<int>(idx / P);
  const int64_t pl = plane[r];
  float v = 0.f;
  if (pl >= 0 && pl < n_planes) {
    const Taps tp = make_taps(coords[2 * idx], coords[2 * idx + 1], H, W, H, W);
    v = -fabsf(sample_logit(masks, dtype, pl * (static_cast<int64_t>(H) * W), tp));
  }
  out[idx] = v;
}

// tgt (R, TR::kRowFields) int64: a RowTarget per row; (Hn, Wn) is the extent the row's coordinates are normalised
// over.  part (R, chunks, 4): sum BCE(x, t), sum sig(x) t, sum sig(x), sum t over the chunk's points.
template <class TR>
__global__ void __launch_bounds__(NT) loss_fwd_kernel(const void* __restrict__ masks, int dtype, int64_t n_planes, int H,
                                                      int W, const int64_t* __restrict__ plane,
                                                      const float* __restrict__ coords, int K,
                                                      const int64_t* __restrict__ tgt, float* __restrict__ part) {
  __shared__ float red[NT / 64][4];
  const int r = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  const int64_t pl = plane[r];
  const RowTarget<TR> row(tgt + TR::kRowFields * static_cast<int64_t>(r));
  const bool row_ok = pl >= 0 && pl < n_planes && row.ok();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (row_ok) {
    const float* cr = coords + static_cast<int64_t>(r) * K * 2;
#pragma unroll
    for (int j = 0; j < LOSS_PER_THREAD; ++j) {
      const int k = chunk * LOSS_CHUNK + j * NT + tid;
      if (k >= K) continue;
      const float ux = cr[2 * k], uy = cr[2 * k + 1];
      const float x = sample_logit(masks, dtype, pl * (static_cast<int64_t>(H) * W), make_taps(ux, uy, H, W, H, W));
      const float t = row.sample(ux, uy);
      const float s = sigmoid(x);
      acc[0] += softplus(x) - x * t;
      acc[1] += s * t;
      acc[2] += s;
      acc[3] += t;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = wave_sum(acc[i]);
    if ((tid & 63) == 0) red[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 4) {
    float v = 0.f;
    for (int w = 0; w < NT / 64; ++w) v += red[w][tid];
    part[(static_cast<int64_t>(r) * gridDim.y + chunk) * 4 + tid] = v;
  }
}

// grad (n_planes, H, W) fp32, zeroed by the caller, += d/dx of sum_r (g[r,0] BCE_r + g[r,1] A_r + g[r,2] S_r)
// (A = sum sig t, S = sum sig) through the bilinear weights: fp32 atomics.
template <class TR>
__global__ void __launch_bounds__(NT) loss_bwd_kernel(const void* __restrict__ masks, int dtype, int64_t n_planes, int H,
                                                      int W, const int64_t* __restrict__ plane, int R,
                                                      const float* __restrict__ coords, int K,
                                                      const int64_t* __restrict__ tgt, const float* __restrict__ g,
                                                      float* __restrict__ grad) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
  if (idx >= static_cast<int64_t>(R) * K) return;
  const int r = static_cast<int>(idx / K);
  const int64_t pl = plane[r];
  const RowTarget<TR> row(tgt + TR::kRowFields * static_cast<int64_t>(r));
  if (!(pl >= 0 && pl < n_planes && row.ok())) return;
  const float ux = coords[2 * idx], uy = coords[2 * idx + 1];
  const Taps tp = make_taps(ux, uy, H, W, H, W);
  const int64_t off = pl * (static_cast<int64_t>(H) * W);
  const float x = sample_logit(masks, dtype, off, tp);
  const float t = row.sample(ux, uy);
  const float s = sigmoid(x);
  const float dx = g[3 * r] * (s - t) + (g[3 * r + 1] * t + g[3 * r + 2]) * (s * (1.f - s));
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (tp.w[i] != 0.f) atomicAdd(grad + off + tp.off[i], dx * tp.w[i]);
}

int check_masks(const char* fn, const void* masks, int dtype, int64_t n_planes, int H, int W) {
  if (!m2f::is_float_dtype(dtype)) return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, dtype);
  if (n_planes < 0 || H < 1 || W < 1) return m2f::fail(M2F_EINVAL, "%s: bad sizes", fn);
  if (static_cast<int64_t>(H) * W > INT32_MAX) return m2f::fail(M2F_EUNSUPPORTED, "%s: H * W > 2^31 - 1", fn);
  if (n_planes > 0 && !masks) return m2f::fail(M2F_EINVAL, "%s: null masks", fn);
  return M2F_OK;
}

// Target code -> reader: f(Dense<uint8_t> / Dense<float>) for the dense entry points' tgt_dtype, f(Labels<...>) for
// the label entry points' bytes per label.  false (f not called) for any other code.
template <typename F>
bool dispatch_dense(int tgt_dtype, F&& f) {
  if (tgt_dtype == kTgtU8) f(Dense<uint8_t>{});
  else if (tgt_dtype == kTgtF32) f(Dense<float>{});
  else return false;
  return true;
}

template <typename F>
bool dispatch_labels(int label_bytes, F&& f) {
  if (label_bytes == 1) f(Labels<uint8_t>{});
  else if (label_bytes == 2) f(Labels<int16_t>{});
  else if (label_bytes == 4) f(Labels<int32_t>{});
  else return false;
  return true;
}

int bad_target(const char* fn, bool labels, int code) {
  return m2f::fail(M2F_EUNSUPPORTED, labels ? "%s: %d bytes per label (1, 2 or 4)" : "%s: target dtype %d", fn, code);
}

// code: tgt_dtype of the dense entry points, bytes per label of the label ones
template <typename F>
bool dispatch_target(bool labels, int code, F&& f) {
  return labels ? dispatch_labels(code, f) : dispatch_dense(code, f);
}

bool known_target(bool labels, int code) {
  return dispatch_target(labels, code, [](auto) {});
}

int64_t match_record(int Q, int Gm) { return 2 * static_cast<int64_t>(Q) * Gm + 2 * static_cast<int64_t>(Q) + Gm; }

}  // namespace

extern "C" int m2f_point_match_workspace(int B, int T, int Q, int Gm, int K, int64_t* floats) {
  const char* fn = "m2f_point_match_workspace";
  if (!floats) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  if (B < 0 || T < 0 || Q < 0 || Gm < 0 || K < 0) return m2f::fail(M2F_EINVAL, "%s: negative size", fn);
  *floats = static_cast<int64_t>(B) * T * m2f::ceil_div(K, TILE) * match_record(Q, Gm);
  return m2f::ok();
}

namespace {

int match_cost(const char* fn, bool labels, const void* masks, int dtype, int B, int Q, int T, int H, int W,
               const float* coords, int K, const int64_t* tgt, int code, int Gm, const float* cost_class, float w_class,
               float w_mask, float w_dice, float* workspace, int64_t ws_floats, float* cost, void* stream) {
  if (B < 0 || Q < 0 || T < 1 || K < 1 || Gm < 0) return m2f::fail(M2F_EINVAL, "%s: bad sizes", fn);
  if (int e = check_masks(fn, masks, dtype, static_cast<int64_t>(B) * Q * T, H, W)) return e;
  if (!known_target(labels, code)) return bad_target(fn, labels, code);
  if (B == 0 || Q == 0 || Gm == 0) return m2f::ok();
  if (!coords || !tgt || !workspace || !cost) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  if (B > 65535 || T > 65535) return m2f::fail(M2F_EUNSUPPORTED, "%s: B or T > 65535", fn);
  const int ntiles = static_cast<int>(m2f::ceil_div(K, TILE));
  const int64_t rec = match_record(Q, Gm);
  if (ws_floats < static_cast<int64_t>(B) * T * ntiles * rec) return m2f::fail(M2F_EINVAL, "%s: workspace too small", fn);
  if (static_cast<int64_t>(T) * ntiles > INT32_MAX || static_cast<int64_t>(B) * Q * Gm > (static_cast<int64_t>(INT32_MAX) - NT) * NT)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: problem too large", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(ntiles, T, B);
  int fields = 0;
  dispatch_target(labels, code, [&](auto tr) {
    using TR = decltype(tr);
    fields = TR::kMatchFields;
    match_partial_kernel<TR><<<grid, NT, 0, st>>>(masks, dtype, Q, T, H, W, coords, K, tgt, Gm, workspace, rec, ntiles);
  });
  if (int e = m2f::check_launch(fn)) return e;
  match_reduce_kernel<<<m2f::ceil_div(static_cast<int64_t>(B) * Q * Gm, NT), NT, 0, st>>>(
      workspace, rec, T * ntiles, B, Q, Gm, tgt, fields, cost_class, w_class, w_mask, w_dice, static_cast<double>(T) * K,
      cost);
  return m2f::check_launch(fn);
}

int loss_fwd(const char* fn, bool labels, const void* masks, int dtype, int64_t n_planes, int H, int W,
             const int64_t* plane, int R, const float* coords, int K, const int64_t* tgt, int code, float* part,
             void* stream) {
  if (R < 0 || K < 0) return m2f::fail(M2F_EINVAL, "%s: negative size", fn);
  if (int e = check_masks(fn, masks, dtype, n_planes, H, W)) return e;
  if (!known_target(labels, code)) return bad_target(fn, labels, code);
  if (R == 0 || K == 0) return m2f::ok();
  if (!plane || !coords || !tgt || !part) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  const int chunks = m2f_point_loss_chunks(K);
  if (chunks > 65535) return m2f::fail(M2F_EUNSUPPORTED, "%s: K too large", fn);
  const dim3 grid(R, chunks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_target(labels, code, [&](auto tr) {
    loss_fwd_kernel<decltype(tr)><<<grid, NT, 0, st>>>(masks, dtype, n_planes, H, W, plane, coords, K, tgt, part);
  });
  return m2f::check_launch(fn);
}

int loss_bwd(const char* fn, bool labels, const void* masks, int dtype, int64_t n_planes, int H, int W,
             const int64_t* plane, int R, const float* coords, int K, const int64_t* tgt, int code,
             const float* grad_rows, float* grad, void* stream) {
  if (R < 0 || K < 0) return m2f::fail(M2F_EINVAL, "%s: negative size", fn);
  if (int e = check_masks(fn, masks, dtype, n_planes, H, W)) return e;
  if (!known_target(labels, code)) return bad_target(fn, labels, code);
  if (R == 0 || K == 0) return m2f::ok();
  if (!plane || !coords || !tgt || !grad_rows || !grad) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  const int64_t n = static_cast<int64_t>(R) * K;
  if (n > (static_cast<int64_t>(INT32_MAX) - NT) * NT) return m2f::fail(M2F_EUNSUPPORTED, "%s: problem too large", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_target(labels, code, [&](auto tr) {
    loss_bwd_kernel<decltype(tr)><<<m2f::ceil_div(n, NT), NT, 0, st>>>(masks, dtype, n_planes, H, W, plane, R, coords, K,
                                                                       tgt, grad_rows, grad);
  });
  return m2f::check_launch(fn);
}

}  // namespace

extern "C" int m2f_point_match_cost(const void* masks, int dtype, int B, int Q, int T, int H, int W, const float* coords,
                                    int K, const int64_t* tgt, int tgt_dtype, int Gm, const float* cost_class,
                                    float w_class, float w_mask, float w_dice, float* workspace, int64_t ws_floats,
                                    float* cost, void* stream) {
  return match_cost("m2f_point_match_cost", false, masks, dtype, B, Q, T, H, W, coords, K, tgt, tgt_dtype, Gm, cost_class,
                    w_class, w_mask, w_dice, workspace, ws_floats, cost, stream);
}

extern "C" int m2f_point_match_cost_labels(const void* masks, int dtype, int B, int Q, int H, int W, const float* coords,
                                           int K, const int64_t* tgt, int label_bytes, int Gm, const float* cost_class,
                                           float w_class, float w_mask, float w_dice, float* workspace,
                                           int64_t ws_floats, float* cost, void* stream) {
  return match_cost("m2f_point_match_cost_labels", true, masks, dtype, B, Q, 1, H, W, coords, K, tgt, label_bytes, Gm,
                    cost_class, w_class, w_mask, w_dice, workspace, ws_floats, cost, stream);
}

extern "C" int m2f_point_uncertainty(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane,
                                     int R, const float* coords, int P, float* out, void* stream) {
  const char* fn = "m2f_point_uncertainty";
  if (R < 0 || P < 0) return m2f::fail(M2F_EINVAL, "%s: negative size", fn);
  if (int e = check_masks(fn, masks, dtype, n_planes, H, W)) return e;
  if (R == 0 || P == 0) return m2f::ok();
  if (!plane || !coords || !out) return m2f::fail(M2F_EINVAL, "%s: null argument", fn);
  const int64_t n = static_cast<int64_t>(R) * P;
  if (n > (static_cast<int64_t>(INT32_MAX) - NT) * NT) return m2f::fail(M2F_EUNSUPPORTED, "%s: problem too large", fn);
  uncertainty_kernel<<<m2f::ceil_div(n, NT), NT, 0, static_cast<hipStream_t>(stream)>>>(masks, dtype, n_planes, H, W, plane,
                                                                                       R, coords, P, out);
  return m2f::check_launch(fn);
}

extern "C" int m2f_point_loss_chunks(int K) { return K > 0 ? static_cast<int>(m2f::ceil_div(K, LOSS_CHUNK)) : 0; }

extern "C" int m2f_point_loss_fwd(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane, int R,
                                  const float* coords, int K, const int64_t* tgt, int tgt_dtype, float* part,
                                  void* stream) {
  return loss_fwd("m2f_point_loss_fwd", false, masks, dtype, n_planes, H, W, plane, R, coords, K, tgt, tgt_dtype, part,
                  stream);
}

extern "C" int m2f_point_loss_fwd_labels(const void* masks, int dtype, int64_t n_planes, int H, int W,
                                         const int64_t* plane, int R, const float* coords, int K, const int64_t* tgt,
                                         int label_bytes, float* part, void* stream) {
  return loss_fwd("m2f_point_loss_fwd_labels", true, masks, dtype, n_planes, H, W, plane, R, coords, K, tgt, label_bytes,
                  part, stream);
}

extern "C" int m2f_point_loss_bwd(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane, int R,
                                  const float* coords, int K, const int64_t* tgt, int tgt_dtype, const float* grad_rows,
                                  float* grad, void* stream) {
  return loss_bwd("m2f_point_loss_bwd", false, masks, dtype, n_planes, H, W, plane, R, coords, K, tgt, tgt_dtype,
                  grad_rows, grad, stream);
}

extern "C" int m2f_point_loss_bwd_labels(const void* masks, int dtype, int64_t n_planes, int H, int W,
                                         const int64_t* plane, int R, const float* coords, int K, const int64_t* tgt,
                                         int label_bytes, const float* grad_rows, float* grad, void* stream) {
  return loss_bwd("m2f_point_loss_bwd_labels", true, masks, dtype, n_planes, H, W, plane, R, coords, K, tgt, label_bytes,
                  grad_rows, grad, stream);
}

// MSDA forwards that gather every corner row from HBM: the fused 8-lane kernel and the quad kernels, fused and
// op-level (D = 32, P = 4).  The LDS-window forwards of msda_fwd_lds.hip run by default where they apply.
#include "msda_host.h"

#include <cmath>
#include <type_traits>

namespace {

using namespace m2f_msda;

// ------------------------------------------------------------------------------------------------
// Fused front end, forward: the MSDA forward reading the raw projection (offsets | logits) and the
// reference points instead of materialised sampling_locations / attention_weights.  Per pair the 8-lane
// group computes softmax over the L*P logits and loc = ref + offset / (W_l, H_l) exactly as the
// reference module does (ms_deform_attn.py:102-109), then samples as msda_fwd_f32_vec.
// ------------------------------------------------------------------------------------------------
//
// TILED: a workgroup takes one head of an 8 x 4 patch of queries of one level instead of 4 consecutive
// queries x 8 heads, with the head as the fastest block index: every XCD (blocks are dealt round-robin)
// then gathers one head's value rows (2.75 MB per 1024^2 image, L2-resident) and a block's 32 queries
// sample one compact neighbourhood of them (L1 reuse across the patch).  Needs Lq == S (encoder queries
// are the pixels).
// OFF32: every element offset of value / out fits 32 bits (checked on the host): 32-bit corner addressing.
template <int LT, bool TILED, bool OFF32>
__global__ void __launch_bounds__(256) msda_fused_fwd(const float* __restrict__ value, FrontEnd fe, TileGeom geo,
                                                      int64_t npairs, int S, int M, int Lq, float* __restrict__ out) {
  constexpr int D = 32, G = 8, P = 4, LP = LT * P;
  int64_t pair, n;
  int m, q;
  if constexpr (TILED) {
    const int g = threadIdx.x / G;
    int64_t b = blockIdx.x;
    m = static_cast<int>(b % M);
    b /= M;
    int T = 0;
#pragma unroll
    for (int l = 0; l < LT; ++l) T += ((geo.H[l] + 3) / 4) * ((geo.W[l] + 7) / 8);
    n = b / T;
    int t = static_cast<int>(b - n * T);
    int lv = 0;
#pragma unroll
    for (int l = 0; l < LT - 1; ++l) {
      const int nt = ((geo.H[l] + 3) / 4) * ((geo.W[l] + 7) / 8);
      if (lv == l && t >= nt) { t -= nt; lv = l + 1; }
    }
    const int H = geo.H[lv], W = geo.W[lv], tlx = (W + 7) / 8;
    const int y = (t / tlx) * 4 + (g >> 3), x = (t % tlx) * 8 + (g & 7);
    if (y >= H || x >= W) return;
    q = geo.start[lv] + y * W + x;
    pair = (n * Lq + q) * M + m;
  } else {
    pair = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
    if (pair >= npairs) return;
    m = static_cast<int>(pair % M);
    const int64_t nq0 = pair / M;
    n = nq0 / Lq;
    q = static_cast<int>(nq0 - n * Lq);
  }
  const int j = threadIdx.x % G;
  const int64_t nq = n * Lq + q;
  const int64_t rs = static_cast<int64_t>(M) * D;
  const float* prow = fe.proj + nq * fe.ld;
  const float* rrow = fe.ref + n * fe.ref_bs + static_cast<int64_t>(q) * LT * 2;
  const float* lg = prow + fe.lg0(m, M, LP);
  // softmax over the pair's L*P logits (ms_deform_attn.py:103-104), each exp computed once in the group:
  // lane j owns logits j and j + 8, the group max is a DPP reduction (exact), and every lane gathers the
  // twelve exps and sums them in logit order (the backward recomputes the same sum, msda_bwd_f32_tiled)
  static_assert(LP <= 16, "two logits per lane of the 8-lane group");
  const float l0 = j < LP ? lg[j] : -INFINITY, l1 = j + 8 < LP ? lg[j + 8] : -INFINITY;
  const float mx = max8_dpp(fmaxf(l0, l1));
  const float e0 = j < LP ? expf(l0 - mx) : 0.f, e1 = j + 8 < LP ? expf(l1 - mx) : 0.f;
  const int gb = (threadIdx.x & 63) & ~(G - 1);
  float a[LP];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < LP; ++k) {
    a[k] = __shfl(k < 8 ? e0 : e1, gb + (k & 7));
    sum += a[k];
  }
  const float inv = 1.f / sum;
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  f4 acc = z;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const int H = geo.H[l], W = geo.W[l];
    const int64_t lbase = ((n * S + geo.start[l]) * M + m) * D + 4 * j;
    const float2 rf = *reinterpret_cast<const float2*>(rrow + 2 * l);
    const float fW = static_cast<float>(W), fH = static_cast<float>(H);
    const float iW = 1.f / fW, iH = 1.f / fH;
    // the level's points; POW2 (W and H powers of two, wave-uniform): offsets scaled by the exact reciprocals
    auto points = [&](auto pow2) {
      constexpr bool POW2 = decltype(pow2)::value;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const float2 off = *reinterpret_cast<const float2*>(prow + fe.off0(m, LP) + (l * P + p) * 2);
        const float sx = rf.x + div_norm(off.x, fW, iW, POW2);
        const float sy = rf.y + div_norm(off.y, fH, iH, POW2);
        f4 val;
        bool ok;
        if constexpr (OFF32) {
          const Corners32 k = make_corners32(sx, sy, H, W, static_cast<int>(lbase), static_cast<int>(rs));
          const f4 v1 = ld4(value + k.o1), v2 = ld4(value + k.o2), v3 = ld4(value + k.o3), v4 = ld4(value + k.o4);
          // a corner outside the level of an in-range sample gets weight 0 instead of a zeroed row (one select,
          // not four): its clamped row is always another corner of the same sample, so the output is non-finite
          // in exactly the elements where the reference's is (only Inf may read as NaN); an out-of-range sample
          // (clamped onto the level's first pixel) is dropped by the select on its sum below
          const float w1 = k.c1 ? k.w1 : 0.f, w2 = k.c2 ? k.w2 : 0.f, w3 = k.c3 ? k.w3 : 0.f, w4 = k.c4 ? k.w4 : 0.f;
          val = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
          ok = k.ok;
        } else {
          const Corners k = make_corners(sx, sy, H, W, lbase, rs);
          f4 v1 = ld4(value + k.o1), v2 = ld4(value + k.o2), v3 = ld4(value + k.o3), v4 = ld4(value + k.o4);
          v1 = k.c1 ? v1 : z; v2 = k.c2 ? v2 : z; v3 = k.c3 ? v3 : z; v4 = k.c4 ? v4 : z;
          val = k.w1 * v1 + k.w2 * v2 + k.w3 * v3 + k.w4 * v4;
          ok = k.ok;
        }
        // a not-ok sample is dropped by one select on its sum, then one fma per channel
        const float wa = a[l * P + p] * inv;
        val = ok ? val : z;
        acc.x = fmaf(val.x, wa, acc.x); acc.y = fmaf(val.y, wa, acc.y);
        acc.z = fmaf(val.z, wa, acc.z); acc.w = fmaf(val.w, wa, acc.w);
      }
    };
    if (((W & (W - 1)) | (H & (H - 1))) == 0) points(std::true_type{});
    else points(std::false_type{});
  }
  *reinterpret_cast<f4*>(out + pair * D + 4 * j) = acc;
}

// ------------------------------------------------------------------------------------------------
// Fused forward, quad form (the default on the encoder layout).  The forward is VALU-issue bound, and in the
// 8-lane form above every lane of a pair re-derives every sample's geometry (about 45 VALU per sample) for a
// float4 of channels.  Here a QUAD of lanes serves one (query, head) pair, lane j owning channels 4j..4j+3 and
// 16+4j..16+4j+3 (two 64-byte halves of the 128-byte row, one load address per corner: the second half is the
// immediate offset).  Lane j derives the geometry of point j of each level ONCE; the quad then takes the four
// points in turn, each lane reading the owner's corner offsets and premultiplied corner weights by DPP quad
// broadcasts (a VALU operand modifier, no LDS), so a sample costs the quad one geometry plus 4 x (4 address
// adds + 4 weight moves + 16 packed FMAs) instead of 8 x (geometry + 16 FMAs + selects).  A sample outside
// (-1, H) x (-1, W) is skipped by the exec mask (as the reference, which skips it: non-finite values at its
// clamped rows never reach the output).  Workgroup = one head of an 8 x 8 patch of queries of one level, head
// the fastest block index (each XCD's L2 gathers one head's value rows).  32-bit offsets (checked on the host).
// ------------------------------------------------------------------------------------------------
// The four points of one level for the quad forward kernels: lane j holds point j's geometry (k) and attention
// weight (wa); the quad takes the points in turn, each lane gathering its 8 channels of the point's 4 corner rows
// (addresses and weights by DPP quad broadcast) into acc0 (channels 4j..4j+3) and acc1 (16+4j..16+4j+3).
template <int PB = 2>
__device__ __forceinline__ void quad_level_fwd(const char* __restrict__ vbytes, const QuadPoint& k, float wa,
                                               unsigned cjb, f4& acc0, f4& acc1) {
  // a corner outside the level weighs 0 (its clamped row is another corner of the same sample)
  const float w1 = k.w1 * wa, w2 = k.w2 * wa, w3 = k.w3 * wa, w4 = k.w4 * wa;
  const int okb = k.ok ? 1 : 0;
  // PB points per batch: their 8 * PB loads are issued (clamped, in-level addresses) before any of their math
  constexpr int kCtrl[4] = {0x00, 0x55, 0xAA, 0xFF};
  auto batch = [&](auto first) {
    constexpr int F = decltype(first)::value;
    f4 va[PB][8];
    const char* vhi = vbytes + 64;  // the row's second half (channels 16..31): an immediate offset
    auto load = [&](f4* v, unsigned o1, unsigned o2, unsigned o3, unsigned o4) {
      v[0] = ldb4(vbytes, o1); v[1] = ldb4(vhi, o1);
      v[2] = ldb4(vbytes, o2); v[3] = ldb4(vhi, o2);
      v[4] = ldb4(vbytes, o3); v[5] = ldb4(vhi, o3);
      v[6] = ldb4(vbytes, o4); v[7] = ldb4(vhi, o4);
    };
    auto load_pt = [&](auto pp) {
      constexpr int C = kCtrl[F + decltype(pp)::value];
      load(va[decltype(pp)::value], qpermi<C>(k.o1) + cjb, qpermi<C>(k.o2) + cjb, qpermi<C>(k.o3) + cjb,
           qpermi<C>(k.o4) + cjb);
    };
    load_pt(std::integral_constant<int, 0>{});
    if constexpr (PB > 1) load_pt(std::integral_constant<int, 1>{});
    if constexpr (PB > 2) { load_pt(std::integral_constant<int, 2>{}); load_pt(std::integral_constant<int, 3>{}); }
    // pin the loads here: otherwise each point's loads sink into its exec-masked block below and the points'
    // latencies are paid one after the other
#pragma unroll
    for (int pp = 0; pp < PB; ++pp)
#pragma unroll
      for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(va[pp][i]));
    auto fmas = [&](const f4* v, float u1, float u2, float u3, float u4) {
      acc0 += u1 * v[0]; acc1 += u1 * v[1];
      acc0 += u2 * v[2]; acc1 += u2 * v[3];
      acc0 += u3 * v[4]; acc1 += u3 * v[5];
      acc0 += u4 * v[6]; acc1 += u4 * v[7];
    };
    // a point outside (-1, H) x (-1, W) is skipped by the exec mask, as the reference skips it
    auto fma_pt = [&](auto pp) {
      constexpr int C = kCtrl[F + decltype(pp)::value];
      if (qpermi<C>(okb)) fmas(va[decltype(pp)::value], qpermf<C>(w1), qpermf<C>(w2), qpermf<C>(w3), qpermf<C>(w4));
    };
    fma_pt(std::integral_constant<int, 0>{});
    if constexpr (PB > 1) fma_pt(std::integral_constant<int, 1>{});
    if constexpr (PB > 2) { fma_pt(std::integral_constant<int, 2>{}); fma_pt(std::integral_constant<int, 3>{}); }
  };
  batch(std::integral_constant<int, 0>{});
  if constexpr (PB == 1) {
    batch(std::integral_constant<int, 1>{});
    batch(std::integral_constant<int, 2>{});
    batch(std::integral_constant<int, 3>{});
  } else if constexpr (PB == 2) {
    batch(std::integral_constant<int, 2>{});
  }
}

// Unfused forward, quad form (the reference op's interface: materialised sampling_loc / attention_weight, device
// spatial shapes; D = 32, P = 4, value bytes < 2^31): a quad per (n, q, m) pair, lane j reading point j of each
// level (the quad's four loc pairs / weights are contiguous).
__global__ void __launch_bounds__(256) msda_fwd_f32_q4(const float* __restrict__ value,
                                                       const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ lsi, const float* __restrict__ loc,
                                                       const float* __restrict__ attn, int64_t npairs, int S, int M,
                                                       int L, int Lq, float* __restrict__ out) {
  constexpr int D = 32, P = 4;
  __shared__ int sH[kMaxLevels], sW[kMaxLevels], sSt[kMaxLevels];
  if (threadIdx.x < L) {
    sH[threadIdx.x] = static_cast<int>(shapes[2 * threadIdx.x]);
    sW[threadIdx.x] = static_cast<int>(shapes[2 * threadIdx.x + 1]);
    sSt[threadIdx.x] = static_cast<int>(lsi[threadIdx.x]);
  }
  __syncthreads();
  const int64_t pair = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x >> 2);
  if (pair >= npairs) return;  // whole quads leave together
  const int j = threadIdx.x & 3;
  const int m = static_cast<int>(pair % M);
  const int n = static_cast<int>(pair / M / Lq);
  const int rsb = M * D * 4;
  const char* vbytes = reinterpret_cast<const char*>(value);
  const float* lp = loc + pair * L * P * 2;
  const float* ap = attn + pair * L * P;
  const unsigned cjb = 16u * j;
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
  for (int l = 0; l < L; ++l) {
    const int H = sH[l], W = sW[l];
    const int obase = ((n * S + sSt[l]) * M + m) * D * 4;
    const float2 xy = *reinterpret_cast<const float2*>(lp + 2 * (l * P + j));
    const QuadPoint k = quad_point(xy.y * H - 0.5f, xy.x * W - 0.5f, H, W, obase, rsb);
    quad_level_fwd(vbytes, k, ap[l * P + j], cjb, acc0, acc1);
  }
  float* o = out + pair * D + 4 * j;
  *reinterpret_cast<f4*>(o) = acc0;
  *reinterpret_cast<f4*>(o + 16) = acc1;
}

template <int LT, int PB = 2>
__global__ void __launch_bounds__(256) msda_fused_fwd_q4(const float* __restrict__ value, FrontEnd fe, TileGeom geo,
                                                         int S, int M, float* __restrict__ out) {
  constexpr int D = 32, P = 4, LP = LT * P;
  static_assert(P == 4, "one quad lane per point");
  const int qd = threadIdx.x >> 2, j = threadIdx.x & 3;
  int b = blockIdx.x;
  const int m = b % M;
  b /= M;
  int T = 0;
#pragma unroll
  for (int l = 0; l < LT; ++l) T += ((geo.H[l] + 7) >> 3) * ((geo.W[l] + 7) >> 3);
  const int n = b / T;
  int t = b - n * T, lv = 0;
#pragma unroll
  for (int l = 0; l < LT - 1; ++l) {
    const int nt = ((geo.H[l] + 7) >> 3) * ((geo.W[l] + 7) >> 3);
    if (lv == l && t >= nt) { t -= nt; lv = l + 1; }
  }
  const int Hq = geo.H[lv], Wq = geo.W[lv], tlx = (Wq + 7) >> 3;
  const int y = (t / tlx) * 8 + (qd >> 3), x = (t % tlx) * 8 + (qd & 7);
  if (y >= Hq || x >= Wq) return;  // whole quads leave together
  const int q = geo.start[lv] + y * Wq + x;
  const int64_t nq = static_cast<int64_t>(n) * S + q;
  const int rsb = M * D * 4;  // value row stride in bytes
  const char* vbytes = reinterpret_cast<const char*>(value);
  const float* prow = fe.proj + nq * fe.ld;
  const float* rrow = fe.ref + n * fe.ref_bs + static_cast<int64_t>(q) * LT * 2;
  // softmax over the pair's L*P logits (ms_deform_attn.py:103-104): lane j exps logit l*P + j of every level,
  // the quad max is exact, and every lane sums the exps in logit order (the sequential sum the backward
  // recomputes, msda_bwd_f32_tiled), so the attention weights are bit-identical to the other kernels'
  const float* lg = prow + fe.lg0(m, M, LP);
  float e[LT];
  float mx = -INFINITY;
#pragma unroll
  for (int l = 0; l < LT; ++l) { e[l] = lg[l * P + j]; mx = fmaxf(mx, e[l]); }
  mx = fmaxf(mx, qpermf<0xB1>(mx));
  mx = fmaxf(mx, qpermf<0x4E>(mx));
  float sum = 0.f;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    e[l] = expf(e[l] - mx);
    sum += qpermf<0x00>(e[l]);
    sum += qpermf<0x55>(e[l]);
    sum += qpermf<0xAA>(e[l]);
    sum += qpermf<0xFF>(e[l]);
  }
  const float inv = 1.f / sum;
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  f4 acc0 = z, acc1 = z;
  const unsigned cjb = 16u * j;  // this lane's channel bytes within a row half
  auto level = [&](int l, auto pow2) {
    constexpr bool POW2 = decltype(pow2)::value;
    const int H = geo.H[l], W = geo.W[l];
    const int obase = ((n * S + geo.start[l]) * M + m) * D * 4;
    const float2 rf = *reinterpret_cast<const float2*>(rrow + 2 * l);
    const float2 off = *reinterpret_cast<const float2*>(prow + fe.off0(m, LP) + (l * P + j) * 2);
    const float sx = rf.x + div_norm(off.x, static_cast<float>(W), geo.invW[l], POW2);
    const float sy = rf.y + div_norm(off.y, static_cast<float>(H), geo.invH[l], POW2);
    // this lane's point: corner byte offsets and weights (a corner outside the level weighted 0: its clamped row
    // is another corner of the same sample), times the attention weight
    const QuadPoint k = quad_point(sy * H - 0.5f, sx * W - 0.5f, H, W, obase, rsb);
    quad_level_fwd<PB>(vbytes, k, e[l] * inv, cjb, acc0, acc1);
  };
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    if (((geo.W[l] & (geo.W[l] - 1)) | (geo.H[l] & (geo.H[l] - 1))) == 0) level(l, std::true_type{});
    else level(l, std::false_type{});
  }
  float* o = out + (nq * M + m) * D + 4 * j;
  *reinterpret_cast<f4*>(o) = acc0;
  *reinterpret_cast<f4*>(o + 16) = acc1;
}

}  // namespace

namespace m2f_msda {

int launch_fwd_q4(const float* value, const int64_t* shapes, const int64_t* lsi, const float* loc, const float* attn,
                  const Dims& d, float* out, hipStream_t st) {
  msda_fwd_f32_q4<<<m2f::ceil_div(d.npairs(), 64), 256, 0, st>>>(value, shapes, lsi, loc, attn, d.npairs(), d.S,
                                                                  d.M, d.L, d.Lq, out);
  return M2F_OK;
}

int launch_fused_fwd_q4(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                        int pb, float* out, hipStream_t st) {
  int64_t T = 0;  // 8 x 8 patches of queries over the levels
  for (int l = 0; l < d.L; ++l) T += static_cast<int64_t>((geo.H[l] + 7) / 8) * ((geo.W[l] + 7) / 8);
  unsigned tg;
  if (int rc = m2f::grid_1d(T * d.M * d.N, fn, &tg)) return rc;
  m2f::dispatch_int<1, 4>(d.L, [&](auto lt) {
    m2f::dispatch_one_of<1, 2, 4>(pb, [&](auto pbt) {
      msda_fused_fwd_q4<lt.value, pbt.value><<<tg, 256, 0, st>>>(value, fe, geo, d.S, d.M, out);
    });
  });
  return M2F_OK;
}

int launch_fused_fwd(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                     bool tiled, bool off32, float* out, hipStream_t st) {
  unsigned tg;
  if (tiled) {
    int64_t T = 0;  // 4 x 8 patches of queries over the levels
    for (int l = 0; l < d.L; ++l) T += static_cast<int64_t>((geo.H[l] + 3) / 4) * ((geo.W[l] + 7) / 8);
    if (int rc = m2f::grid_1d(T * d.M * d.N, fn, &tg)) return rc;
  } else {
    tg = m2f::ceil_div(d.npairs(), 32);
  }
  m2f::dispatch_int<1, 4>(d.L, [&](auto lt) {
    m2f::dispatch_bool(tiled, [&](auto ti) {
      m2f::dispatch_bool(off32, [&](auto o32) {
        msda_fused_fwd<lt.value, ti.value, o32.value><<<tg, 256, 0, st>>>(value, fe, geo, d.npairs(), d.S, d.M, d.Lq,
                                                                          out);
      });
    });
  });
  return M2F_OK;
}

}  // namespace m2f_msda

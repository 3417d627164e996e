// The spatially tiled fp32 MSDA backward (encoder layout, D = 32, P = 4), fused and op-level, with the passes of
// its deterministic mode, its geometry builder and the stamped diagnostic entry point (M2F_DIAG builds).
#include "msda_host.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace {

using namespace m2f_msda;

// ------------------------------------------------------------------------------------------------
// fp32 backward, spatially tiled: encoder self-attention (Lq == S, query i = pyramid position i).
//
// Workgroup = (spatial tile, head m, image n), 512 threads (two per CU).  A tile is the same normalised rectangle on
// every level (level l's tile ty spans rows [ty*H_l/nty, (ty+1)*H_l/nty)), so its queries at every level
// sample the same neighbourhood of every level.
//
// grad_value is a scatter: every (query, sample, corner) adds w_c * a * g[query] (32 channels) to one
// pixel row.  Here it becomes a gather inside the workgroup:
//   phase 0  one lane per (query, level) derives that level's P samples ONCE (softmax and ref + offset /
//            (W, H) on the fused path, or the given loc / attn) into a 16-byte descriptor {ly, lx, a, floors}
//            per sample in LDS (h = loc_y * H - 0.5 = floor + ly ..., the two floors + 2 packed in 16 bits each;
//            floors -2 and fractions 0 when the sample lies outside (-1, H) x (-1, W): every corner outside),
//            stages the tile's grad_output rows (this head) in LDS and takes the bounding box of
//            the touched corners per level (every global load of the phase issued first).  The window = that
//            box clipped to the tile +- halo.
//   phase 1  counting sort of the samples by the window cell of their 2x2 corner block (the window grid
//            extended by one row / column up and left): an LDS counter per cell (returning adds give each
//            sample its rank), a block-wide exclusive scan, and one 32-bit slot per sample (its descriptor
//            index and its query's g-row offset).  Samples whose corners leave the window are flagged instead.
//   phase 2  a lane quad per query (8 channels per lane) gathers each sample's 4 corner rows (texture path),
//            forms the per-corner channel dots with g and writes grad_loc / grad_attn (or d offset / d logit)
//            once per point (quad transpose-reduce).  Flagged samples add their 4 corner rows with atomics.
//   phase 3  a 4-lane group per window pixel reads the 4 slot ranges whose cells cover it ((y,x) ->
//            corner 1 of cell (y,x), corner 2 of (y,x-1), corner 3 of (y-1,x), corner 4 of (y-1,x-1); the
//            row-major cell order makes them two contiguous ranges), accumulating w_c * a * g[query] in fp32 from the LDS descriptors and g rows (8 channels per
//            lane); the wave's 16 rows are transposed through LDS, 8 at a time, so that each atomic
//            instruction adds two whole 128-B rows to HBM.
//   Phases 2 and 3 read nothing the other writes: their units are dealt from one counter, interleaved
//   (OVERLAP), so the texture-bound gather and the LDS-bound walk run at once.
// Summation order (slot order, atomics across workgroups) is not fixed, as in the reference's atomics, except
// in the deterministic mode (DET, below).
// grad_loc / grad_attn (or d offset / d logit) are owned per (q, m) and written once.
//
// FUSED = true: the samples come from the raw projection (offsets | logits) and the reference points, and
// the outputs are the gradients w.r.t. that projection: d offset = d loc / (W, H) = sum_c dval/dloc * g * a
// in pixel units (the level scale cancels) and d logit = a * (d attn - sum_k a_k d attn_k) (softmax
// backward over the pair's L*P logits).
// ------------------------------------------------------------------------------------------------
#ifndef M2F_WALK_LANES
#define M2F_WALK_LANES 4        // phase-3 lanes per window pixel (2: an experiment build, tools/lib)
#endif
constexpr int kWalkLanes = M2F_WALK_LANES;   // phase-3 lanes per window pixel (32 / kWalkLanes channels each)
constexpr int kMaxBwdWaves = 16;
constexpr int kSortSamples = 6144;  // samples per workgroup the counting sort holds in registers (max_qt * L * P)
static_assert(kSortSamples < 65536, "phase 3's slots hold the sample index in 16 bits");
constexpr int kStageFloats = 8 * 32 + 8;  // per wave: 8 rows x 32 channels + 8 row offsets (a flush half)

struct TileState {
  int bb[kTileMaxL][4];  // min y, max y, min x, max x of touched corners (inclusive)
  int wy0[kTileMaxL], wx0[kTileMaxL], wh[kTileMaxL], ww[kTileMaxL];
  int roff[kTileMaxL + 1];   // window pixel offsets per level
  int coff[kTileMaxL + 1];   // extended-cell offsets per level ((wh+1) x (ww+1) cells)
  int qc[kTileMaxL + 1], qy0[kTileMaxL], qx0[kTileMaxL], qw[kTileMaxL];
  int wsum[kMaxBwdWaves];    // block scan
  float iww[kTileMaxL];      // 1 / ww (phase 3's row -> window coordinates)
  int H[kTileMaxL], W[kTileMaxL], start[kTileMaxL];  // the level shapes in LDS: a kernarg array indexed by a
  float invW[kTileMaxL], invH[kTileMaxL];            // per-lane level is a global load per use
  int next_batch;            // phase-3 row batches handed out dynamically
  int rbin[64];              // row sort: rows per record-count bin, then the bins' start positions
};
// the tiled backward's dynamic LDS (<= 156 KB, make_tile_geom) plus this static block within the CU's 160 KB, and
// within the 160 KB - 1 KB the launcher raises the dynamic limit to
static_assert(sizeof(TileState) <= 1024, "TileState must leave the dynamic LDS its 159 KB");

// g rows in LDS: query qi's 16-byte chunk c (float offset)
__device__ __forceinline__ int g_chunk_off(int qi, int c) { return qi * 32 + 4 * c; }

// pyramid position of the tile's query qi (levels in order, rows of the tile's rectangle on each level)
__device__ __forceinline__ int tile_query(const TileState& ts, int qi) {
  int lq = 0;
  while (qi >= ts.qc[lq + 1]) ++lq;
  const int r = qi - ts.qc[lq];
  return ts.start[lq] + (ts.qy0[lq] + r / ts.qw[lq]) * ts.W[lq] + ts.qx0[lq] + r % ts.qw[lq];
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    v += lane >= o ? t : 0;
  }
  return v;
}

// window cell of a sample whose top-left corner is (h0, w0), or -1 when a corner inside the level lies
// outside the window
__device__ __forceinline__ int window_cell(const TileState& ts, int l, int h0, int w0, int H, int W) {
  const int wy0 = ts.wy0[l], wx0 = ts.wx0[l], wh = ts.wh[l], ww = ts.ww[l];
  const bool ry = (h0 < 0 || (h0 >= wy0 && h0 < wy0 + wh)) && (h0 + 1 > H - 1 || (h0 + 1 >= wy0 && h0 + 1 < wy0 + wh));
  const bool rx = (w0 < 0 || (w0 >= wx0 && w0 < wx0 + ww)) && (w0 + 1 > W - 1 || (w0 + 1 >= wx0 && w0 + 1 < wx0 + ww));
  return (wh > 0 && ry && rx) ? ts.coff[l] + (h0 - wy0 + 1) * (ww + 1) + (w0 - wx0 + 1) : -1;
}

// STAMP (diagnostic builds only, M2F_DIAG): s_memtime at the phase barriers of each workgroup into `stamps`;
// NOFLUSH (diagnostic builds only): phase 3 without its HBM adds, to price them.
// TPB threads per workgroup: 512 (two workgroups per CU, 12x12 tiles; the default) or 1024 (one, 16x16 tiles).
// Fixed-point scale of the deterministic mode: 2^(61 - b - e) with max |grad_output| < 2^e and Lq < 2^b.  A
// grad_value element sums coef * g over samples whose coefficients (bilinear weight * attention weight, each
// <= 1; a query's attention weights per head sum to 1) total at most the image's Lq queries, so every partial
// and the total stay below 2^61; the resolution is max|g| * 2^-(61 - b) absolute (2^-46 at config 2's 21,504
// queries).
__device__ __forceinline__ float det_scale(unsigned maxbits, int Lq) {
  const float B = __uint_as_float(maxbits);
  int e = 0;
  if (B > 0.f) (void)frexpf(B, &e);
  const int b = 32 - __clz(Lq);
  return ldexpf(1.f, min(61 - b - e, 126));
}

// max |g| over finite entries (as the bits of a non-negative float: the unsigned order is the float order) and a
// flag for any non-finite entry: out[0], out[1] (zeroed by the caller)
__global__ void __launch_bounds__(256) msda_det_scale_kernel(const float4* __restrict__ g, int64_t n4,
                                                             unsigned* __restrict__ out) {
  unsigned mx = 0u, nf = 0u;
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * 256) {
    const float4 v = g[i];
    const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned b = __float_as_uint(fabsf(a[k]));
      if (b >= 0x7f800000u) nf = 1u;
      else mx = max(mx, b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = max(mx, __shfl_xor(mx, o)); nf |= __shfl_xor(nf, o); }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(out, mx);
    if (nf) atomicOr(out + 1, 1u);
  }
}

// grad_value = fixed-point sum * 2^-k, added to what the non-finite contributions left there in fp32 (zero almost
// everywhere); skipped when the non-finite flag sent the whole kernel down the fp32 atomics
__global__ void __launch_bounds__(256) msda_det_convert_kernel(const long long* __restrict__ acc, int64_t n, int Lq,
                                                               const unsigned* __restrict__ detscale,
                                                               float* __restrict__ gvalue) {
  if (detscale[1] != 0u) return;
  const double inv = 1.0 / static_cast<double>(det_scale(detscale[0], Lq));
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
    gvalue[i] += static_cast<float>(static_cast<double>(acc[i]) * inv);
}

// DET (deterministic mode, m2f_set_option msda_bwd_det): every grad_value contribution leaving a workgroup (the
// window rows, the out-of-window samples) is converted to 64-bit fixed point (scale 2^k from the launch's max
// |grad_output|, DetScale below) and added with integer atomics, whose sum does not depend on their order; the
// slots of each cell are sorted by sample, so a window row's fp32 partial is summed in a fixed order.  A
// conversion pass writes grad_value.  Non-finite grad_output falls back to the fp32 atomics (flag set by the scale
// pass), as the reference's kernel propagates them.
// Occupancy: four waves per SIMD (<= 128 VGPRs; a 1024-thread workgroup needs that) except for four levels, which
// run 512-thread workgroups only, at two waves per SIMD (<= 256 VGPRs): the L = 4 body (the reference module's
// default n_levels, ops/modules/ms_deform_attn.py:35) spilled 3-10 VGPRs at 128.
template <int LT, bool FUSED, int TPB, bool OVERLAP = true, bool DET = false, bool STAMP = false, bool NOFLUSH = false>
__global__ void __launch_bounds__(TPB, (LT == 4 && TPB == 512) ? 2 : 4) msda_bwd_f32_tiled(
    const float* __restrict__ value, const float* __restrict__ loc, const float* __restrict__ attn, FrontEnd fe,
    const float* __restrict__ gout, TileGeom geo, int S, int M, float* __restrict__ gvalue,
    float* __restrict__ gloc, float* __restrict__ gattn, unsigned long long* __restrict__ gacc = nullptr,
    const unsigned* __restrict__ detscale = nullptr, unsigned long long* __restrict__ stamps = nullptr) {
  constexpr int D = 32, P = 4, LP = LT * P;
  constexpr int kBwdThreads = TPB, kBwdWaves = TPB / 64, kSortPerThread = kSortSamples / TPB;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ TileState ts;
#define M2F_STAMP(k)                                                                                        \
  if constexpr (STAMP) {                                                                                    \
    if (threadIdx.x == 0)                                                                                   \
      stamps[static_cast<int64_t>(blockIdx.x) * 8 + (k)] = __builtin_amdgcn_s_memtime();                     \
  }

  // XCD-aware order: blocks are dealt round-robin over the 8 XCDs (b, b+8, ... share one); remap so each
  // XCD takes a contiguous run of (image, head) pairs, tile fastest, and its L2 holds one head's value
  // rows (2.75 MB per 1024^2 image) instead of several (speed only: any placement computes the same)
  const int ntiles = geo.nty * geo.ntx;
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tile = wg % ntiles, pm = wg / ntiles, m = pm % M, n = pm / M;
  const int ty = tile / geo.ntx, tx = tile - ty * geo.ntx;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int rs = M * D;  // value row stride (elements); N*S*M*D < 2^31 is checked on the host
  const int nsamp_max = geo.max_qt * LP;
  // LDS carve-up (16-byte aligned pieces): g rows [max_qt + 1][32] (the last a zero row: phase 3's padding records) |
  //   desc [max_qt * LP][4] | stage [waves][264] | cstart [max_cells + 1] i32 | oow [ceil(nsamp / 32)] u32
  //   | slots [max_qt * LP + 8] u32 | qmap [max_qt] i32
  float* gsh = reinterpret_cast<float*>(lds_raw);
  float* desc = gsh + (geo.max_qt + 1) * D;
  float* stage = desc + nsamp_max * 4;
  // cstart: the sort's counters, then the cells' slot ranges (values <= nsamp < 2^16).  The row sort below may put its
  // permutation into the high halves of these words: after it only 16-bit reads (cs16) are valid
  int* cstart = reinterpret_cast<int*>(stage + kBwdWaves * kStageFloats);
  unsigned* oow = reinterpret_cast<unsigned*>(cstart + ((geo.max_rows + 1 + 3) & ~3));
  unsigned* slots = reinterpret_cast<unsigned*>(oow + (((nsamp_max + 31) / 32 + 3) & ~3));
  int* qmap = reinterpret_cast<int*>(slots + nsamp_max + 8);  // pyramid position of each tile query
  float fxscale = 0.f;  // DET: 2^k, grad_value contributions leave the workgroup as round(v * 2^k) in int64
  bool fixed = false;
  if constexpr (DET) {
    fixed = detscale[1] == 0u;
    fxscale = det_scale(detscale[0], S);
  }
  // a grad_value contribution leaving the workgroup
  // (DET: a non-finite contribution -- a NaN / Inf from the projection's offsets or logits, which the pre-pass over
  // grad_output does not see -- goes to grad_value itself in fp32, where the conversion pass adds the fixed-point
  // sum to it: the element is then non-finite as the reference's atomics leave it)
  auto gv_add = [&](float* dst, float v) {
    if constexpr (DET) {
      if (fixed && __builtin_isfinite(v)) {
        atomicAdd(gacc + (dst - gvalue), static_cast<unsigned long long>(__float2ll_rn(v * fxscale)));
        return;
      }
    }
    atomicAdd(dst, v);
  };

  M2F_STAMP(5)
  if (tid < LT) {
    const int l = tid;
    const int y0 = tile_lo(ty, geo.H[l], geo.nty), y1 = tile_lo(ty + 1, geo.H[l], geo.nty);
    const int x0 = tile_lo(tx, geo.W[l], geo.ntx), x1 = tile_lo(tx + 1, geo.W[l], geo.ntx);
    ts.qy0[l] = y0;
    ts.qx0[l] = x0;
    ts.qw[l] = x1 - x0;
    ts.qc[l + 1] = (y1 - y0) * (x1 - x0);
    ts.bb[l][0] = 0x7fffffff; ts.bb[l][1] = -1; ts.bb[l][2] = 0x7fffffff; ts.bb[l][3] = -1;
    ts.H[l] = geo.H[l]; ts.W[l] = geo.W[l]; ts.start[l] = geo.start[l];
    ts.invW[l] = geo.invW[l]; ts.invH[l] = geo.invH[l];
  }
  for (int i = tid; i < (nsamp_max + 31) / 32; i += blockDim.x) oow[i] = 0u;
  for (int i = tid; i <= geo.max_rows; i += blockDim.x) cstart[i] = 0;  // the sort's counters (any window fits)
  if (tid == 0) ts.next_batch = kBwdWaves;
  if (tid < 64) ts.rbin[tid] = 0;
  if (tid < D) gsh[geo.max_qt * D + tid] = 0.f;   // the zero g row
  __syncthreads();
  if (tid == 0) {
    ts.qc[0] = 0;
    for (int l = 0; l < LT; ++l) ts.qc[l + 1] += ts.qc[l];
  }
  __syncthreads();
  const int Qt = ts.qc[LT];
  const int nsamp = Qt * LP;
  for (int qi = tid; qi < Qt; qi += blockDim.x) qmap[qi] = tile_query(ts, qi);
  __syncthreads();
  M2F_STAMP(0)

  // ---- phase 0: this head's grad_output rows of the tile's queries -> LDS (float4 per lane); the sample
  // descriptors (one lane per (query, level)) and the touched-corner boxes.  Every global load of the phase is
  // issued before any of its math or LDS stores (the g rows, then both task rounds' projection rows), so the
  // phase waits out one memory round trip instead of three ---------------------------------------------------
  constexpr int kGPre = 3;  // max_qt * 8 <= 3 * TPB at the default geometries; the rest loops
  f4 gpre[kGPre];
#pragma unroll
  for (int u = 0; u < kGPre; ++u) {
    const int idx = min(tid + u * kBwdThreads, Qt * 8 - 1), qi = idx >> 3, j = idx & 7;
    const int64_t pair = (static_cast<int64_t>(n) * S + qmap[qi]) * M + m;
    gpre[u] = ld4(gout + pair * D + 4 * j);
  }
  {
    int bmin_y[LT], bmax_y[LT], bmin_x[LT], bmax_x[LT];
#pragma unroll
    for (int l = 0; l < LT; ++l) { bmin_y[l] = 0x7fffffff; bmax_y[l] = -1; bmin_x[l] = 0x7fffffff; bmax_x[l] = -1; }
    // FUSED: a quad of lanes per query (lane l < LT handles level l), so the softmax over the pair's L*P
    // logits is shared: each lane exps its level's P logits, the quad max is a DPP reduction (exact), and
    // the sum is carried from lane to lane in logit order (the sequential sum the forward forms)
    // a quad of lanes per query either way (the op-level path with LT lanes per query ran 3-4 % slower: its
    // queries straddled quads and the level boxes took LT full-wave reductions)
    constexpr int TPQ = 4;  // tasks per query
    static_assert(LT <= 4, "one quad lane per level");
    const int ntask = Qt * TPQ;
    struct TaskIn {
      float x[P];      // logits (FUSED) or attention weights
      float2 xy[P];    // offsets (FUSED) or sampling locations
      float2 rf;       // reference point (FUSED)
    };
    auto task_load = [&](int t) {
      TaskIn in;
      t = min(t, ntask - 1);  // a spare round's addresses stay in range (its results are dropped)
      const int qi = t / TPQ, lt = t - qi * TPQ;
      const int l = lt < LT ? lt : LT - 1;
      const int64_t nq = static_cast<int64_t>(n) * S + qmap[qi];
      if constexpr (FUSED) {
        const float* prow = fe.proj + nq * fe.ld;
        const float* lg = prow + fe.lg0(m, M, LP) + l * P;
        const float* of = prow + fe.off0(m, LP) + l * P * 2;
#pragma unroll
        for (int p = 0; p < P; ++p) { in.x[p] = lg[p]; in.xy[p] = *reinterpret_cast<const float2*>(of + 2 * p); }
        in.rf = *reinterpret_cast<const float2*>(fe.ref + n * fe.ref_bs + (static_cast<int64_t>(qmap[qi]) * LT + l) * 2);
      } else {
        const int64_t kb = (nq * M + m) * LP + l * P;
#pragma unroll
        for (int p = 0; p < P; ++p) { in.xy[p] = *reinterpret_cast<const float2*>(loc + 2 * (kb + p)); in.x[p] = attn[kb + p]; }
        in.rf = make_float2(0.f, 0.f);
      }
      return in;
    };
    auto task_run = [&](int t, TaskIn& in) {  // whole quads run it together
      const int qi = t / TPQ, lt = t - qi * TPQ;
      const bool act = lt < LT;
      const int l = act ? lt : LT - 1;  // a spare quad lane mirrors the last level (its results are dropped)
      const int H = ts.H[l], W = ts.W[l];
      float av[P], lx[P], ly[P];
      if constexpr (FUSED) {
        float* x = in.x;
        float mx = -INFINITY;
#pragma unroll
        for (int p = 0; p < P; ++p) mx = fmaxf(mx, x[p]);
        mx = fmaxf(mx, qperm<0xB1>(mx));  // quad lanes 1 0 3 2
        mx = fmaxf(mx, qperm<0x4E>(mx));  // quad lanes 2 3 0 1
#pragma unroll
        for (int p = 0; p < P; ++p) x[p] = expf(x[p] - mx);
        float run = 0.f;
#pragma unroll
        for (int ll = 0; ll < LT; ++ll) {
          float prev = 0.f;
          if (ll > 0) {
            switch (ll) {  // broadcast quad lane ll - 1 (the DPP control must be an immediate)
              case 1: prev = qperm<0x00>(run); break;
              case 2: prev = qperm<0x55>(run); break;
              default: prev = qperm<0xAA>(run); break;
            }
          }
          if (lt == ll) {
            run = prev;
#pragma unroll
            for (int p = 0; p < P; ++p) run += x[p];
          }
        }
        float sum;
        switch (LT) {
          case 1: sum = qperm<0x00>(run); break;
          case 2: sum = qperm<0x55>(run); break;
          case 3: sum = qperm<0xAA>(run); break;
          default: sum = qperm<0xFF>(run); break;
        }
        const float inv = 1.f / sum;
        const float fW = static_cast<float>(W), fH = static_cast<float>(H);
        const float iW = ts.invW[l], iH = ts.invH[l];
        auto points = [&](auto pow2) {  // as msda_fused_fwd: exact reciprocals when W and H are powers of two
          constexpr bool POW2 = decltype(pow2)::value;
#pragma unroll
          for (int p = 0; p < P; ++p) {
            lx[p] = in.rf.x + div_norm(in.xy[p].x, fW, iW, POW2);
            ly[p] = in.rf.y + div_norm(in.xy[p].y, fH, iH, POW2);
            av[p] = x[p] * inv;
          }
        };
        if (((W & (W - 1)) | (H & (H - 1))) == 0) points(std::true_type{});
        else points(std::false_type{});
      } else {
#pragma unroll
        for (int p = 0; p < P; ++p) { lx[p] = in.xy[p].x; ly[p] = in.xy[p].y; av[p] = in.x[p]; }
      }
      if (!act) return;
      float* dq = desc + (qi * LP + l * P) * 4;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        float h = ly[p] * H - 0.5f, w = lx[p] * W - 0.5f;
        const bool ok = h > -1.f && w > -1.f && h < static_cast<float>(H) && w < static_cast<float>(W);
        h = ok ? h : -2.f;
        w = ok ? w : -2.f;
        const float fh = floorf(h), fw = floorf(w);
        const int h0 = static_cast<int>(fh), w0 = static_cast<int>(fw);
        *reinterpret_cast<f4*>(dq + 4 * p) =
            f4{h - fh, w - fw, av[p], __uint_as_float(static_cast<unsigned>(h0 + 2) | (static_cast<unsigned>(w0 + 2) << 16))};
        if (ok) {
#pragma unroll
          for (int ll = 0; ll < LT; ++ll)
            if (ll == l) {
              bmin_y[ll] = min(bmin_y[ll], max(h0, 0)); bmax_y[ll] = max(bmax_y[ll], min(h0 + 1, H - 1));
              bmin_x[ll] = min(bmin_x[ll], max(w0, 0)); bmax_x[ll] = max(bmax_x[ll], min(w0 + 1, W - 1));
            }
        }
      }
    };
    // task rounds in pairs, both rounds' loads first (whole quads enter and leave together: ntask and the
    // round stride are multiples of 4)
    for (int t = tid; t < ntask; t += 2 * kBwdThreads) {
      TaskIn i0 = task_load(t), i1 = task_load(t + kBwdThreads);
      task_run(t, i0);
      if (t + kBwdThreads < ntask) task_run(t + kBwdThreads, i1);
    }
    // the g rows -> LDS (their loads were issued first)
#pragma unroll
    for (int u = 0; u < kGPre; ++u) {
      const int idx = tid + u * kBwdThreads;
      if (idx < Qt * 8) *reinterpret_cast<f4*>(gsh + g_chunk_off(idx >> 3, idx & 7)) = gpre[u];
    }
    for (int idx = tid + kGPre * kBwdThreads; idx < Qt * 8; idx += kBwdThreads) {
      const int qi = idx >> 3, j = idx & 7;
      const int64_t pair = (static_cast<int64_t>(n) * S + qmap[qi]) * M + m;
      *reinterpret_cast<f4*>(gsh + g_chunk_off(qi, j)) = ld4(gout + pair * D + 4 * j);
    }
    // per-level boxes over the wave, then over the workgroup
    {
      // a lane only ever touches its own level (tid & 3: the task stride is a multiple of 4), so the lanes of
      // one level (lane & 3 equal) reduce it over xor 4..32, and lane l < LT publishes level l
      const int ol = (lane & 3) < LT ? (lane & 3) : LT - 1;
      int a0 = 0x7fffffff, a1 = -1, a2 = 0x7fffffff, a3 = -1;
#pragma unroll
      for (int l = 0; l < LT; ++l)
        if (l == ol) { a0 = bmin_y[l]; a1 = bmax_y[l]; a2 = bmin_x[l]; a3 = bmax_x[l]; }
#pragma unroll
      for (int o = 32; o >= 4; o >>= 1) {
        a0 = min(a0, __shfl_xor(a0, o)); a1 = max(a1, __shfl_xor(a1, o));
        a2 = min(a2, __shfl_xor(a2, o)); a3 = max(a3, __shfl_xor(a3, o));
      }
      if (lane < LT && a1 >= 0) {
        atomicMin(&ts.bb[lane][0], a0); atomicMax(&ts.bb[lane][1], a1);
        atomicMin(&ts.bb[lane][2], a2); atomicMax(&ts.bb[lane][3], a3);
      }
    }
  }
  __syncthreads();
  M2F_STAMP(1)

  // ---- window: touched box clipped to the tile +- halo; the halo shrinks until the cells fit ----------
  if (tid == 0) {
    for (int halo = geo.max_halo; halo >= 0; --halo) {
      int rows = 0, cells = 0;
      for (int l = 0; l < LT; ++l) {
        const int H = geo.H[l], W = geo.W[l];
        const int ry0 = max(tile_lo(ty, H, geo.nty) - halo, 0), ry1 = min(tile_lo(ty + 1, H, geo.nty) - 1 + halo, H - 1);
        const int rx0 = max(tile_lo(tx, W, geo.ntx) - halo, 0), rx1 = min(tile_lo(tx + 1, W, geo.ntx) - 1 + halo, W - 1);
        const int wy0 = max(ry0, ts.bb[l][0]), wy1 = min(ry1, ts.bb[l][1]);
        const int wx0 = max(rx0, ts.bb[l][2]), wx1 = min(rx1, ts.bb[l][3]);
        const bool any = wy1 >= wy0 && wx1 >= wx0;
        ts.wy0[l] = wy0; ts.wx0[l] = wx0;
        ts.wh[l] = any ? wy1 - wy0 + 1 : 0; ts.ww[l] = any ? wx1 - wx0 + 1 : 0;
        ts.iww[l] = any ? 1.f / static_cast<float>(ts.ww[l]) : 0.f;
        ts.roff[l] = rows;
        ts.coff[l] = cells;
        rows += ts.wh[l] * ts.ww[l];
        cells += any ? (ts.wh[l] + 1) * (ts.ww[l] + 1) : 0;
      }
      ts.roff[LT] = rows;
      ts.coff[LT] = cells;
      if (cells <= geo.max_rows) break;
      if (halo == 0) {  // cannot happen when the budget covers a tile's own footprint; stay correct anyway
        for (int l = 0; l <= LT; ++l) { ts.roff[l] = 0; ts.coff[l] = 0; }
        for (int l = 0; l < LT; ++l) { ts.wh[l] = 0; ts.ww[l] = 0; }
      }
    }
  }
  __syncthreads();
  const int cells_total = ts.coff[LT];

  // ---- phase 1: counting sort of the in-window samples by cell ------------------------------------------
  {
    int cell[kSortPerThread], rank[kSortPerThread];
#pragma unroll
    for (int r = 0; r < kSortPerThread; ++r) {
      const int sid = tid + r * kBwdThreads;
      cell[r] = -1;
      if (sid < nsamp) {
        const unsigned pk = __float_as_uint(desc[4 * sid + 3]);
        const int h0 = static_cast<int>(pk & 0xffffu) - 2, w0 = static_cast<int>(pk >> 16) - 2;
        if (h0 != -2) {  // ok sample
          const int l = (sid % LP) / P;
          const int c = window_cell(ts, l, h0, w0, ts.H[l], ts.W[l]);
          if (c >= 0) {
            cell[r] = c;
            rank[r] = atomicAdd(cstart + c, 1);
          } else {
            atomicOr(oow + (sid >> 5), 1u << (sid & 31));
          }
        }
      }
    }
    __syncthreads();
    // exclusive scan of cstart[0 .. cells_total] (cstart[cells_total] = 0 -> total)
    const int per = (cells_total + 1 + kBwdThreads - 1) / kBwdThreads;
    const int c0 = tid * per;
    int run = 0;
    for (int i = 0; i < per; ++i) run += (c0 + i <= cells_total) ? cstart[c0 + i] : 0;
    const int incl = wave_incl_scan(run, lane);
    if (lane == 63) ts.wsum[wid] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wid; ++w) wbase += ts.wsum[w];
    int acc = wbase + incl - run;
    for (int i = 0; i < per; ++i) {
      if (c0 + i <= cells_total) {
        const int v = cstart[c0 + i];
        cstart[c0 + i] = acc;
        acc += v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortPerThread; ++r)
      if (cell[r] >= 0) {  // slot = sample index << 16 | g row byte offset: phase 3 decodes it in 3 VALU
        const int sid = tid + r * kBwdThreads, qs = sid / LP;
        slots[cstart[cell[r]] + rank[r]] =
            (static_cast<unsigned>(sid) << 16) | static_cast<unsigned>(4 * g_chunk_off(qs, 0));
      }
  }
  __syncthreads();
  if constexpr (DET) {
    // a cell's slots in sample order (the ranks above come from LDS atomics, in arrival order): insertion sort,
    // one thread per cell (a cell holds a few samples)
    for (int c = tid; c < cells_total; c += kBwdThreads) {
      const int b0 = cstart[c], b1 = cstart[c + 1];
      for (int i = b0 + 1; i < b1; ++i) {
        const unsigned key = slots[i];
        int k = i - 1;
        while (k >= b0 && slots[k] > key) { slots[k + 1] = slots[k]; --k; }
        slots[k + 1] = key;
      }
    }
    __syncthreads();
  }
  // ---- phase-3 rows in order of their record count, heaviest first -------------------------------------------------
  // A phase-3 unit is 16 rows walked in lockstep by the wave's 4-lane groups, so it takes as long as its longest list;
  // in window order neighbouring rows' lists differ several-fold (the lists of a 16-row unit averaged 0.43 of its
  // longest at config 2 near-init, a host count).  A counting sort over 64 bins of 4 records each deals units of rows
  // with lists of nearly equal length.  The permutation lives in the high halves of cstart's words (every cstart value
  // is < 2^16; rows_total <= cells_total), read by phase 3 with 16-bit loads; a window too large for the per-thread
  // row registers keeps window order.
  constexpr int kRowsPT = 4, kRowBins = 64, kRowBinShift = 2;
  // both halves of a cstart word hold 16 bits: a slot position is at most the workgroup's sample count (<= kSortSamples
  // and < 0xffff, make_tile_geom), a sorted row's index is below kRowsPT * TPB
  static_assert(kSortSamples < (1 << 16) && kRowsPT * TPB <= (1 << 16),
                "the row sort shares cstart's words: slot ranges in the low halves, its permutation in the high ones");
  const int rows_all = ts.roff[LT];
  const bool rowsort = geo.rowsort != 0 && rows_all <= kRowsPT * kBwdThreads;
  // window row -> (level, window y, window x, its cell index, the cell grid width)
  auto row_cell = [&](int row, int& l, int& ey, int& ex, int& cbase, int& cw) {
    l = 0;
    while (row >= ts.roff[l + 1]) ++l;
    const int ww = ts.ww[l], rr = row - ts.roff[l];
    // rr / ww by the reciprocal: (rr + 0.5) / ww is at least 0.5 / ww from an integer and the product's error
    // is below wh * ww * 2^-23 / ww, so the truncation is exact for windows of fewer than 2^22 cells
    ey = static_cast<int>((static_cast<float>(rr) + 0.5f) * ts.iww[l]);
    ex = rr - ey * ww;  // window coordinates; cells are offset by (1, 1)
    cw = ww + 1;
    cbase = ts.coff[l] + (ey + 1) * cw + ex + 1;
  };
  const unsigned short* cs16 = reinterpret_cast<const unsigned short*>(cstart);   // the cstart values (low halves)
  if (rowsort) {
    int rk[kRowsPT], bk[kRowsPT];
#pragma unroll
    for (int i = 0; i < kRowsPT; ++i) {
      const int row = tid + i * kBwdThreads;
      bk[i] = -1;
      if (row < rows_all) {
        int l, ey, ex, cbase, cw;
        row_cell(row, l, ey, ex, cbase, cw);
        const int n = (cstart[cbase + 1] - cstart[cbase - 1]) + (cstart[cbase - cw + 1] - cstart[cbase - cw - 1]);
        bk[i] = kRowBins - 1 - min(n >> kRowBinShift, kRowBins - 1);
        rk[i] = atomicAdd(&ts.rbin[bk[i]], 1);
      }
    }
    __syncthreads();
    if (wid == 0) {   // exclusive scan of the 64 bins
      const int v = ts.rbin[lane];
      ts.rbin[lane] = wave_incl_scan(v, lane) - v;
    }
    __syncthreads();
    unsigned short* hi16 = reinterpret_cast<unsigned short*>(cstart);
#pragma unroll
    for (int i = 0; i < kRowsPT; ++i)
      if (bk[i] >= 0) hi16[2 * (ts.rbin[bk[i]] + rk[i]) + 1] = static_cast<unsigned short>(tid + i * kBwdThreads);
    __syncthreads();
  }
  M2F_STAMP(2)

  // ---- phases 2 and 3: one work queue ----------------------------------------------------------------------
  // Phase 2 (16 queries per unit) gathers the samples' corner rows through L1 (texture-path bound); phase 3 (16
  // window rows per unit) walks the slot lists in LDS (LDS bound).  Neither reads what the other writes (phase 3
  // derives its corner coefficients from the {h, w, a} descriptors), so with OVERLAP the units of both kinds are
  // dealt from one LDS counter, interleaved, and the waves of a workgroup run both at once instead of one phase
  // after a barrier.
  {
    const int rows_total = ts.roff[LT];
    constexpr int LPR = kWalkLanes, CPL = D / LPR, RPW = 64 / LPR;  // phase 3: lanes per row, channels per lane, rows per wave
    const int U2 = (Qt + 15) / 16, U3 = (rows_total + RPW - 1) / RPW;
    const int ratio = max(geo.ratio23, 1);
    // phase 2, quad form: a quad of lanes takes one query, lane j owning channels 4j..4j+3 and 16+4j..16+4j+3
    // (one load address per corner row: the second half is the immediate offset).  Per level, lane j derives
    // point j's geometry once; the quad takes the points in turn with the owner's corner byte offsets by DPP
    // broadcast, each lane forming 16 partial channel dots (4 points x 4 corners) over its 8 channels; a two-stage
    // quad transpose-reduce (xor 2, xor 1) leaves lane j the 4 full corner dots of ITS point, so the gradient math
    // and the stores run once per point.
    const int j = lane & 3, gq = lane >> 2;
    const unsigned cjb = 16u * j;
    const char* vbytes = reinterpret_cast<const char*>(value);
    char* gvbytes = reinterpret_cast<char*>(gvalue);
    const int rsb = rs * 4;  // value row stride in bytes; value bytes < 2^31 (host check)
    auto phase2_unit = [&](int unit) {
      const int qi = unit * 16 + gq;
      if (qi >= Qt) return;  // whole quad (same qi) idles together
      const int q = qmap[qi];
      const int64_t nq = static_cast<int64_t>(n) * S + q;
      const f4 gA = *reinterpret_cast<const f4*>(gsh + g_chunk_off(qi, j));
      const f4 gB = *reinterpret_cast<const f4*>(gsh + g_chunk_off(qi, 4 + j));
      const float* dq = desc + qi * LP * 4;
      const int sid0 = qi * LP, sh = sid0 & 31;
      const unsigned w0f = oow[sid0 >> 5], w1f = oow[min((sid0 + LP - 1) >> 5, (nsamp_max + 31) / 32 - 1)];
      const unsigned qfar = (sh ? (w0f >> sh) | (w1f << (32 - sh)) : w0f) & ((1u << LP) - 1u);
      float dot = 0.f;  // FUSED: this lane's points' sum of a * d attn
      float gaown[LT], aown[LT];
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        const int H = geo.H[l], W = geo.W[l];
        const int lbase = ((n * S + geo.start[l]) * M + m) * D * 4;
        // this lane's point (l, j)
        const f4 dk = *reinterpret_cast<const f4*>(dq + 4 * (l * P + j));
        const float a = dk[2];
        // not-ok samples carry floors -2 (every corner outside, ok false)
        const unsigned pk = __float_as_uint(dk[3]);
        const QuadPoint k = quad_point_fl(static_cast<int>(pk & 0xffffu) - 2, static_cast<int>(pk >> 16) - 2, dk[0], dk[1],
                                          H, W, lbase, rsb);
        const bool ok = k.ok;
        const float ly = k.ly, lx = k.lx, hy = 1.f - ly, hx = 1.f - lx;
        const int o1 = k.o1, o2 = k.o2, o3 = k.o3, o4 = k.o4;
        // partial channel dots over this lane's 8 channels, pairs of channels in packed fp32 FMAs (v_pk_fma_f32)
        auto dot8 = [&](const f4& va, const f4& vb) {
          f2 t = f2{va.x, va.y} * f2{gA.x, gA.y};
          t = __builtin_elementwise_fma(f2{va.z, va.w}, f2{gA.z, gA.w}, t);
          t = __builtin_elementwise_fma(f2{vb.x, vb.y}, f2{gB.x, gB.y}, t);
          t = __builtin_elementwise_fma(f2{vb.z, vb.w}, f2{gB.z, gB.w}, t);
          return t.x + t.y;
        };
        const bool hi2 = (j & 2) != 0, hi1 = (j & 1) != 0;
        float s1[2][4];
        // one point at a time (8 corner loads in flight per lane: the texture path, not latency, bounds this phase,
        // and fewer registers keep the merged phase 2/3 loop free of spills); after the points {0, 2} and {1, 3} the
        // first transpose-reduce stage (xor 2) folds their 8 partial dots to 4: lanes {0, 1} keep the lower point,
        // lanes {2, 3} the upper one, summed over the lane pair
        auto point_dots = [&](auto cc, float* part) {
          constexpr int C = decltype(cc)::value;
          const char* vhi = vbytes + 64;  // the row's second half: an immediate offset
          const unsigned b1 = qpermi<C>(o1) + cjb, b2 = qpermi<C>(o2) + cjb;
          const unsigned b3 = qpermi<C>(o3) + cjb, b4 = qpermi<C>(o4) + cjb;
          const f4 v0 = ldb4(vbytes, b1), v1 = ldb4(vhi, b1), v2 = ldb4(vbytes, b2), v3 = ldb4(vhi, b2);
          const f4 v4 = ldb4(vbytes, b3), v5 = ldb4(vhi, b3), v6 = ldb4(vbytes, b4), v7 = ldb4(vhi, b4);
          part[0] = dot8(v0, v1);
          part[1] = dot8(v2, v3);
          part[2] = dot8(v4, v5);
          part[3] = dot8(v6, v7);
        };
        auto stage1 = [&](const float* plo, const float* phi, float* out) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float lo = plo[c] + qpermf<0x4E>(plo[c]), hi = phi[c] + qpermf<0x4E>(phi[c]);
            out[c] = hi2 ? hi : lo;
          }
        };
        {
          float pa_[4], pb_[4];
          point_dots(std::integral_constant<int, 0x00>{}, pa_);
          point_dots(std::integral_constant<int, 0xAA>{}, pb_);
          stage1(pa_, pb_, s1[0]);
          point_dots(std::integral_constant<int, 0x55>{}, pa_);
          point_dots(std::integral_constant<int, 0xFF>{}, pb_);
          stage1(pa_, pb_, s1[1]);
        }
        // second stage (xor 1): lane j holds the full corner dots of point j
        float dd[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float lo = s1[0][c] + qpermf<0xB1>(s1[0][c]);
          const float hi = s1[1][c] + qpermf<0xB1>(s1[1][c]);
          dd[c] = hi1 ? hi : lo;
        }
        // a corner outside the level contributes nothing (as the reference, which skips it)
        const float d1 = k.c1 ? dd[0] : 0.f, d2 = k.c2 ? dd[1] : 0.f, d3 = k.c3 ? dd[2] : 0.f, d4 = k.c4 ? dd[3] : 0.f;
        const float pa = k.w1 * d1 + k.w2 * d2 + k.w3 * d3 + k.w4 * d4;
        const float px = a * (hy * (d2 - d1) + ly * (d4 - d3));
        const float py = a * (hx * (d3 - d1) + lx * (d4 - d2));
        if constexpr (FUSED) {
          const float gak = ok ? pa : 0.f;
          dot = fmaf(a, gak, dot);
          gaown[l] = gak;
          aown[l] = a;
          *reinterpret_cast<float2*>(gloc + nq * (3 * M * LP) + fe.off0(m, LP) + l * P * 2 + 2 * j) =
              ok ? make_float2(px, py) : make_float2(0.f, 0.f);
        } else {
          const unsigned kl = ((static_cast<unsigned>(n * S + q) * M + m) * LT + l) * P + j;  // < 2^28 (host)
          *reinterpret_cast<float*>(reinterpret_cast<char*>(gattn) + kl * 4u) = ok ? pa : 0.f;
          *reinterpret_cast<float2*>(reinterpret_cast<char*>(gloc) + kl * 8u) =
              ok ? make_float2(W * px, H * py) : make_float2(0.f, 0.f);
        }
        // out-of-window points (rare; flags are per query, so quad-uniform): every lane adds its 8 channels of
        // the point's 4 corner rows straight to HBM (fp32 atomics, as the reference)
        if ((qfar >> (l * P)) & 0xFu) {
          const int cf = (k.c1 ? 1 : 0) | (k.c2 ? 2 : 0) | (k.c3 ? 4 : 0) | (k.c4 ? 8 : 0);
          const float wt1 = k.w1 * a, wt2 = k.w2 * a, wt3 = k.w3 * a, wt4 = k.w4 * a;
          auto scatter = [&](auto cc, int p) {
            constexpr int C = decltype(cc)::value;
            const int f = qpermi<C>(cf);
            const unsigned b1 = qpermi<C>(o1) + cjb, b2 = qpermi<C>(o2) + cjb;
            const unsigned b3 = qpermi<C>(o3) + cjb, b4 = qpermi<C>(o4) + cjb;
            const float u1 = qpermf<C>(wt1), u2 = qpermf<C>(wt2), u3 = qpermf<C>(wt3), u4 = qpermf<C>(wt4);
            if ((qfar >> (l * P + p)) & 1u) {
              auto add8 = [&](unsigned boff, float u) {
                float* o = reinterpret_cast<float*>(gvbytes + boff);
                const f4 ta = u * gA, tb = u * gB;
                gv_add(o, ta.x); gv_add(o + 1, ta.y); gv_add(o + 2, ta.z); gv_add(o + 3, ta.w);
                gv_add(o + 16, tb.x); gv_add(o + 17, tb.y); gv_add(o + 18, tb.z); gv_add(o + 19, tb.w);
              };
              if (f & 1) add8(b1, u1);
              if (f & 2) add8(b2, u2);
              if (f & 4) add8(b3, u3);
              if (f & 8) add8(b4, u4);
            }
          };
          scatter(std::integral_constant<int, 0x00>{}, 0);
          scatter(std::integral_constant<int, 0x55>{}, 1);
          scatter(std::integral_constant<int, 0xAA>{}, 2);
          scatter(std::integral_constant<int, 0xFF>{}, 3);
        }
      }
      if constexpr (FUSED) {
        // softmax backward over the pair's L*P logits: d logit_k = a_k (d a_k - sum_i a_i d a_i)
        dot += qpermf<0xB1>(dot);
        dot += qpermf<0x4E>(dot);
        float* gl = gloc + nq * (3 * M * LP) + fe.lg0(m, M, LP);
#pragma unroll
        for (int l = 0; l < LT; ++l) gl[l * P + j] = aown[l] * (gaown[l] - dot);
      }
    };
    // phase 3: per window pixel, the 4 covering slot ranges; one row-contiguous atomic add per row
    const int jl = lane % LPR, rw = lane / LPR;
    float* wst = stage + wid * kStageFloats;               // this wave's flush half: 8 rows x 32 channels
    int* woff = reinterpret_cast<int*>(wst + 8 * 32);      // and their grad_value element offsets
    const char* gbytes = reinterpret_cast<const char*>(gsh);
    const unsigned jlb = static_cast<unsigned>(CPL * 4 * jl);  // this lane's channel bytes (< 128: ORs into a row offset)
    auto phase3_unit = [&](int unit) {
      const int base = unit * RPW;
      int row = base + rw;
      if (rowsort && row < rows_total) row = cs16[2 * row + 1];   // the row sort's permutation
      float acc[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = 0.f;
      int off = -1;  // element offset of channel 0 of this group's grad_value row (-1: none)
      int l = 0, ey = 0, ex = 0;
      bool any = false;
      if (row < rows_total) {
        int cbase, cw;
        row_cell(row, l, ey, ex, cbase, cw);
        // corner 1 of cell (y, x), corner 2 of (y, x-1), corner 3 of (y-1, x), corner 4 of (y-1, x-1).  Cells are
        // numbered row-major, so the slot ranges of (y, x-1) and (y, x) are one contiguous range, as are those of
        // (y-1, x-1) and (y-1, x): two walks, the six range bounds read up front (16-bit reads: the high halves
        // may hold the row sort's permutation)
        const unsigned short* cs = cs16 + 2 * cbase;
        const int b0 = cs[-2], b1 = cs[0], b2 = cs[2];
        const int u0 = cs[-2 * cw - 2], u1 = cs[-2 * cw], u2 = cs[-2 * cw + 2];
        any = b2 > b0 || u2 > u0;
        // HI: the row above (corners 3 / 4: ly a, else (1 - ly) a); a record below `mid` comes from the cell at x-1
        // (corners 2 / 4: times lx, else (1 - lx)); the (1 - t) factors as fmas
        auto walk = [&](auto hi_c, int s0, int mid, int s1) {
          constexpr bool HI = decltype(hi_c)::value;
          // a record: the sample's descriptor {ly, lx, a, -} (one 16-byte read) and its query's g row
          auto rec = [&](unsigned p, int idx) {
            const f4 dk = *reinterpret_cast<const f4*>(reinterpret_cast<const char*>(desc) + ((p >> 12) & 0xffff0u));
            const float ly = dk[0], lx = dk[1], a = dk[2];
            const float A = HI ? ly * a : fmaf(-ly, a, a);
            const f4* g = reinterpret_cast<const f4*>(gbytes + ((p & 0xffffu) | jlb));
            const float cf = idx < mid ? A * lx : fmaf(-A, lx, A);
#pragma unroll
            for (int k = 0; k < CPL / 4; ++k) {  // fma chains (pairs of channels pack into v_pk_fma_f32)
              const f4 v = g[k];
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[4 * k + e] = fmaf(cf, v[e], acc[4 * k + e]);
            }
          };
          // two records per step, the next pair's slots read one step ahead (unclamped: a read past the range, or
          // past the array into its 8-entry pad, is never used), so a step waits on one LDS round trip
          const unsigned* sp = slots + s0;
          unsigned npa = sp[0], npb = sp[1];
          int i = s0;
          for (; i + 1 < s1; i += 2, sp += 2) {
            const unsigned pa = npa, pb = npb;
            npa = sp[2];
            npb = sp[3];
            rec(pa, i);
            rec(pb, i + 1);
          }
          if (i < s1) rec(npa, i);
        };
        // quad form (msda_bwd_walk4, the default): four records per step, lane jl of the row's quad decoding record
        // i + jl once (slot, descriptor, coefficient) and the quad taking the four in turn with the coefficient and
        // the g-row offset broadcast by DPP (the broadcast folds into the FMAs / the address add): per record 1 + 8
        // VALU per lane instead of ~6 + 8 and a quarter of the descriptor reads; a range's tail records carry
        // coefficient 0 (any in-range slot read: the 8-entry pad covers the read past the range)
        auto walk4 = [&](auto hi_c, int s0, int mid, int s1) {
          constexpr bool HI = decltype(hi_c)::value;
          unsigned np = slots[s0 + jl];
          for (int i = s0; i < s1; i += 4) {
            const int idx = i + jl;
            // a padding record: descriptor 0, the zero g row (coefficient 0 times zeros: nothing added, whatever
            // non-finite values other g rows hold)
            const unsigned p = idx < s1 ? np : static_cast<unsigned>(geo.max_qt * D * 4);
            np = slots[idx + 4];
            const f4 dk = *reinterpret_cast<const f4*>(reinterpret_cast<const char*>(desc) + ((p >> 12) & 0xffff0u));
            const float ly = dk[0], lx = dk[1], a = dk[2];
            const float A = HI ? ly * a : fmaf(-ly, a, a);
            float cf = idx < mid ? A * lx : fmaf(-A, lx, A);
            cf = idx < s1 ? cf : 0.f;
            const unsigned gb = p & 0xffffu;
            auto rec4 = [&](auto cc) {
              constexpr int C = decltype(cc)::value;
              const float c = qpermf<C>(cf);
              const f4* g = reinterpret_cast<const f4*>(gbytes + (static_cast<unsigned>(qpermi<C>(static_cast<int>(gb))) | jlb));
#pragma unroll
              for (int k = 0; k < CPL / 4; ++k) {
                const f4 v = g[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * k + e] = fmaf(c, v[e], acc[4 * k + e]);
              }
            };
            rec4(std::integral_constant<int, 0x00>{});
            rec4(std::integral_constant<int, 0x55>{});
            rec4(std::integral_constant<int, 0xAA>{});
            rec4(std::integral_constant<int, 0xFF>{});
          }
        };
        if (geo.walk4) {
          walk4(std::false_type{}, b0, b1, b2);
          walk4(std::true_type{}, u0, u1, u2);
        } else {
          walk(std::false_type{}, b0, b1, b2);
          walk(std::true_type{}, u0, u1, u2);
        }
      }
      if (any) {
        const int y = ts.wy0[l] + ey, x = ts.wx0[l] + ex;
        off = ((n * S + ts.start[l] + y * ts.W[l] + x) * M + m) * D;
      }
      // transpose the wave's RPW rows through LDS, 8 rows at a time, so that each atomic instruction adds two whole
      // 128-B rows, one dword per lane (the L2 takes atomics per 64-B request)
#pragma unroll
      for (int half = 0; half < RPW / 8; ++half) {
        if ((rw >> 3) == half) {
#pragma unroll
          for (int k = 0; k < CPL / 4; ++k)
            *reinterpret_cast<f4*>(wst + (rw & 7) * 32 + CPL * jl + 4 * k) =
                f4{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
          if (jl == 0) woff[rw & 7] = off;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's stage writes are in LDS
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r2 = 2 * i + (lane >> 5);
          const int o = woff[r2];
          const float v = wst[r2 * 32 + (lane & 31)];
          if constexpr (NOFLUSH) {
            asm volatile("" ::"v"(v), "v"(o));
          } else {
            if (o >= 0) gv_add(gvalue + o + (lane & 31), v);
          }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // reads done before the stage is written again
        __builtin_amdgcn_wave_barrier();
      }
    };
    auto next_unit = [&]() {
      int nb = 0;
      if (lane == 0) nb = atomicAdd(&ts.next_batch, 1);
      return __builtin_amdgcn_readlane(nb, 0);   // lane 0's value, uniform (not an LDS permute round trip)
    };
    if constexpr (OVERLAP) {
      // R phase-2 units per phase-3 unit while phase 2 lasts (msda_bwd_ratio, default 1), then the rest of phase 3:
      // with c3(k) = max(min(U3, k / (R + 1)), k - U2) phase-3 units among the first k, unit u is phase-3 unit c3(u)
      // when c3 steps up at u, else phase-2 unit u - c3(u).  Texture-path work early, LDS work to the end (a
      // schedule spreading the phase-2 units evenly over the queue measured 2.7 % slower: a gather unit late in
      // the queue is a straggler); the coarse levels' rows come first (~37 records each at config 2 against ~9)
      const int T = U2 + U3, R1 = ratio + 1;
      for (int u = wid; u < T; u = next_unit()) {
        const int c0 = max(min(U3, u / R1), u - U2), c1 = max(min(U3, (u + 1) / R1), u + 1 - U2);
        if (c1 > c0) phase3_unit(c0);
        else phase2_unit(u - c0);
      }
    } else {
      for (int u = wid; u < U2; u += kBwdWaves) phase2_unit(u);
      __syncthreads();
      M2F_STAMP(3)
      for (int u = wid; u < U3; u = next_unit()) phase3_unit(u);
    }
  }
  if constexpr (STAMP) __syncthreads();
  M2F_STAMP(4)
#undef M2F_STAMP
}

template <int LT, bool FUSED, int TPB>
int launch_tiled_t(const float* value, const float* loc, const float* attn, const FrontEnd& fe, const float* gout,
                   const TileGeom& geo, size_t lds, const Dims& d, float* gv, float* gl, float* ga, bool overlap,
                   const DetBufs& det, hipStream_t st) {
  const dim3 grid(geo.nty * geo.ntx * d.M * d.N);
  const char* fn = "msda tiled backward";
  constexpr int kLds = 160 * 1024 - 1024;   // the static TileState (< 1 KB) shares the 160 KB
  if (det.acc) {
    auto* k = &msda_bwd_f32_tiled<LT, FUSED, TPB, true, true>;
    if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(k), kLds, fn)) return rc;
    k<<<grid, TPB, lds, st>>>(value, loc, attn, fe, gout, geo, d.S, d.M, gv, gl, ga, det.acc, det.scale, nullptr);
  } else if (overlap) {
    auto* k = &msda_bwd_f32_tiled<LT, FUSED, TPB, true>;
    if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(k), kLds, fn)) return rc;
    k<<<grid, TPB, lds, st>>>(value, loc, attn, fe, gout, geo, d.S, d.M, gv, gl, ga, nullptr, nullptr, nullptr);
  } else {
    auto* k = &msda_bwd_f32_tiled<LT, FUSED, TPB, false>;
    if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(k), kLds, fn)) return rc;
    k<<<grid, TPB, lds, st>>>(value, loc, attn, fe, gout, geo, d.S, d.M, gv, gl, ga, nullptr, nullptr, nullptr);
  }
  return M2F_OK;
}

}  // namespace

namespace m2f_msda {

// (an LDS-attribute failure returns before the kernel is launched)
int launch_bwd_tiled(bool fused, const float* value, const float* loc, const float* attn, const FrontEnd& fe,
                     const float* gout, const TileGeom& geo, size_t lds, int threads, const Dims& d, float* gv,
                     float* gl, float* ga, bool overlap, const DetBufs& det, hipStream_t st) {
  int rc = M2F_OK;
  m2f::dispatch_int<1, 4>(d.L, [&](auto lt) {
    m2f::dispatch_bool(fused, [&](auto fu) {
      constexpr int LT = lt.value;
      constexpr bool FUSED = fu.value;
      // four levels run 512-thread workgroups only (make_tile_geom)
      if constexpr (LT < 4) {
        if (threads == 1024) {
          rc = launch_tiled_t<LT, FUSED, 1024>(value, loc, attn, fe, gout, geo, lds, d, gv, gl, ga, overlap, det, st);
          return;
        }
      }
      rc = launch_tiled_t<LT, FUSED, 512>(value, loc, attn, fe, gout, geo, lds, d, gv, gl, ga, overlap, det, st);
    });
  });
  return rc;
}

void launch_det_scale(const float* gout, int64_t n4, const DetBufs& det, hipStream_t st) {
  msda_det_scale_kernel<<<2048, 256, 0, st>>>(reinterpret_cast<const float4*>(gout), n4, det.scale);
}

void launch_det_convert(const DetBufs& det, int64_t nval, int Lq, float* gv, hipStream_t st) {
  msda_det_convert_kernel<<<4096, 256, 0, st>>>(reinterpret_cast<const long long*>(det.acc), nval, Lq, det.scale, gv);
}

// Tile geometry for the tiled backward; false when the configuration does not qualify (then the
// caller uses the untiled kernels).  Lq == S: the queries are the flattened pyramid.
// Options (m2f_set_option):
//   msda_threads (1024; 512 in the deterministic mode): workgroup size, 512 (two workgroups per CU) or 1024 (one);
//   msda_tile / msda_tile_w (12 / 12 at 512 threads, 16 / 16 at 1024): tile on the finest level;
//   msda_halo (8 at 512 threads, 12 at 1024): window halo;  msda_win_rows (cells per workgroup; the halo shrinks until the
//   window fits).  Geometry only: every setting computes the same gradients (tests sweep them).
bool make_tile_geom(const Dims& d, const int64_t* host_shapes, TileGeom& geo, size_t& lds, int& threads) {
  if (!host_shapes || d.D != 32 || d.P != 4 || d.Lq != d.S || d.L > kTileMaxL) return false;
  if (static_cast<int64_t>(d.N) * d.S * d.M * d.D * 4 >= (int64_t{1} << 31)) return false;  // 32-bit byte offsets
  // the op-level (unfused) kernels address loc (8 B per sample) and grad_attn / grad_loc in 32 bits
  if (static_cast<int64_t>(d.N) * d.Lq * d.M * d.L * d.P * 8 >= (int64_t{1} << 31)) return false;
  int64_t total;
  if (fill_levels(d, host_shapes, geo, total) != LevelFill::kOk) return false;
  int fi = 0;
  for (int l = 0; l < d.L; ++l) {
    // phase 2 forms corner offsets (y0 * W + x0) * rs with 24-bit multiplies (__umul24): a level of 2^24 or
    // more pixels would silently wrap, so such shapes take the untiled kernels
    if (static_cast<int64_t>(geo.H[l]) * geo.W[l] >= (int64_t{1} << 24)) return false;
    // the descriptors pack each floor + 2 (-2 .. H - 1) in 16 bits
    if (geo.H[l] > 65533 || geo.W[l] > 65533) return false;
    if (static_cast<int64_t>(geo.H[l]) * geo.W[l] > static_cast<int64_t>(geo.H[fi]) * geo.W[fi]) fi = l;
  }
  // 1024 threads with 16x16 tiles and a halo of 12 (one workgroup per CU): at config 2 1.707 ms with near-init
  // sampling against 1.697 for 512 threads / 12x12 / halo 8 (two per CU), and 2.43 against 4.51 ms with N(0, 4 px)
  // offsets, where the larger tiles flush fewer window rows per owned row and the halo keeps samples out of the
  // direct atomics (profiles/r04_i*_mb.txt).  The deterministic mode keeps 512 / 12x12 / 8 (2.74 vs 3.55 ms).
  const bool det = m2f::option(m2f::kOptMsdaBwdDet, 0) != 0;
  // four levels: 512-thread workgroups only (the L = 4 body needs more than the 128 VGPRs of a 1024-thread one)
  const int first = d.L == 4 ? 512 : m2f::option(m2f::kOptMsdaThreads, det ? 512 : 1024) >= 1024 ? 1024 : 512;
  geo.ratio23 = std::max(1, m2f::option(m2f::kOptMsdaBwdRatio, 1));
  geo.rowsort = m2f::option(m2f::kOptMsdaBwdRowSort, 1) != 0 ? 1 : 0;
  geo.walk4 = m2f::option(m2f::kOptMsdaBwdWalk4, 1) != 0 ? 1 : 0;
  const TileGeom base = geo;
  // a default 1024-thread geometry whose LDS does not fit (e.g. four levels: 16 samples per query) falls back to
  // the 512-thread one; an explicit msda_threads does not
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (attempt == 1 && (first == 512 || m2f::option_raw(m2f::kOptMsdaThreads) >= 0)) break;
    threads = attempt == 0 ? first : 512;
    geo = base;
    const int tile_h = std::max(1, m2f::option(m2f::kOptMsdaTile, threads == 1024 ? 16 : 12));
    const int tile_w = std::max(1, m2f::option(m2f::kOptMsdaTileW, tile_h));
    geo.nty = (geo.H[fi] + tile_h - 1) / tile_h;
    geo.ntx = (geo.W[fi] + tile_w - 1) / tile_w;
    geo.max_halo = std::max(0, m2f::option(m2f::kOptMsdaHalo, threads == 1024 ? 12 : 8));
    // cells of the largest window any workgroup can choose (tile + 2 halo + 1 per axis, clipped to the level),
    // unless a smaller budget is asked for; it must hold every level's share of one tile at halo 0 (tiles
    // span at most ceil(n / nt) pixels per axis, tile_lo) plus the extra cell row / column
    int own = 0, qt = 0, full = 0;
    for (int l = 0; l < d.L; ++l) {
      const int th = (geo.H[l] + geo.nty - 1) / geo.nty, tw = (geo.W[l] + geo.ntx - 1) / geo.ntx;
      own += (std::min(geo.H[l], th + 1) + 1) * (std::min(geo.W[l], tw + 1) + 1);  // clipped like `full`
      full += (std::min(geo.H[l], th + 2 * geo.max_halo) + 1) * (std::min(geo.W[l], tw + 2 * geo.max_halo) + 1);
      qt += th * tw;
    }
    geo.max_rows = m2f::option(m2f::kOptMsdaWinRows, full);
    geo.max_qt = qt;
    const int lp = d.L * d.P;
    // phase 3's 32-bit slots hold the g-row byte offset 128 * qs (qs <= qt: the zero row) in their low 16 bits
    if (own > geo.max_rows || static_cast<int64_t>(qt) * lp >= 0xffff || qt > 511) continue;
    if (static_cast<int64_t>(qt) * lp > kSortSamples) continue;
    const size_t ns = static_cast<size_t>(qt) * lp;
    lds = ((static_cast<size_t>(qt) + 1) * 32 + ns * 4 + (threads / 64) * kStageFloats) * 4 +
          ((static_cast<size_t>(geo.max_rows) + 1 + 3) & ~static_cast<size_t>(3)) * 4 +
          (((ns + 31) / 32 + 3) & ~static_cast<size_t>(3)) * 4 + (ns + 8) * 4 + static_cast<size_t>(qt) * 4;
    if (lds <= 156 * 1024) return true;
  }
  return false;
}

}  // namespace m2f_msda

#ifdef M2F_DIAG
// Diagnostic build only (tools/msda_stamps.py builds it as a separate library): the unfused tiled backward with
// s_memtime stamps at its phase barriers, stamps[wg * 8 + k], k = 0..4.
extern "C" int m2f_diag_msda_bwd_stamps_f32(const float* value, const float* loc, const float* attn,
                                            const float* grad_output, int batch, int spatial_size, int num_heads,
                                            int num_levels, const int64_t* host_spatial_shapes, float* grad_value,
                                            float* grad_loc, float* grad_attn, unsigned long long* stamps,
                                            int noflush, void* stream) {
  using namespace m2f_msda;
  const Dims d{batch, spatial_size, num_heads, 32, num_levels, spatial_size, 4};
  TileGeom geo;
  size_t lds;
  int threads;
  if (num_levels != 3 || !make_tile_geom(d, host_spatial_shapes, geo, lds, threads))
    return m2f::fail(M2F_EUNSUPPORTED, "diag");
  hipStream_t st = static_cast<hipStream_t>(stream);
  (void)m2f::zero_async(grad_value, static_cast<size_t>(d.N) * d.S * d.M * 32 * 4, st);
  const dim3 grid(geo.nty * geo.ntx * d.M * d.N);
  m2f::dispatch_one_of<1024, 512>(threads == 1024 ? 1024 : 512, [&](auto tpb) {
    m2f::dispatch_bool(noflush != 0, [&](auto nf) {
      auto* k = &msda_bwd_f32_tiled<3, false, tpb.value, false, false, true, nf.value>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 1024);
      k<<<grid, tpb.value, lds, st>>>(value, loc, attn, FrontEnd{}, grad_output, geo, d.S, d.M, grad_value, grad_loc,
                                      grad_attn, nullptr, nullptr, stamps);
    });
  });
  return m2f::check_launch("m2f_diag_msda_bwd_stamps_f32");
}
#endif

// Instance views: the label-view geometry of image_views.hip (PIL NEAREST resize, crop, flips, zero canvas) applied to
// one-bit-per-pixel instance masks, a ragged number per view, with the tight box and the area of every output mask.
// The definition is in include/bm2f.h; bm2f_amd/instance_views.py holds it in numpy.
//
// The planes are those of mask_iou.hip and polygon.hip: (H, ceil(W / 32)) int32 per mask in one flat buffer, bit
// x % 32 of word x / 32.  The view rows and the nearest index tables are those of m2f_label_views (view_row.h); a
// second table gives every mask its word offset, its size and its view.
//
//   bits_views_kernel    one workgroup of 4 waves per (mask, band of kBand output rows); the output planes of a call
//                        have one size, so workgroup b is mask b / bands, band b % bands and no table deals them.  A
//                        wave owns every 4th row of the band.  One lane per output pixel: the lane looks its source
//                        column up in the x table, takes its bit from the source row (a row's words are shared by
//                        neighbouring lanes, so the loads are broadcasts out of cache) and a wave ballot forms 64
//                        output bits.  kChunk ballots fill 2 * kChunk lanes with a word each, and these lanes store
//                        them with one vector store; the uint8 form stores each lane's own byte instead.  Rows and
//                        chunks outside canvas, crop or image are stored as zeros without a gather.  The box and the
//                        area come from the ballots (count, first and last set bit), uniform per wave; the waves'
//                        values meet in LDS and thread 0 writes the workgroup's partial.
//   bits_stats_kernel    one thread per mask: its partials in band order -> x0, y0, x1, y1, area, zeros when empty.
// Every output word or byte and every partial is stored exactly once; no atomics, no memset, integers only.
#include "bm2f.h"
#include "common.h"
#include "view_row.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

namespace {

using namespace m2f_view;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kBand = M2F_BITS_VIEW_BAND_ROWS;
constexpr int kMF = M2F_BITS_VIEW_MASK_FIELDS;
constexpr int kChunk = 8;                 // ballots per store: 16 words, 64 bytes, of one output row
static_assert(kBand % kWaves == 0 && 2 * kChunk <= 64, "a wave owns whole rows and a chunk's words fit its lanes");

struct Mask {
  Row g;
  int64_t base;   // word offset of the plane
  int sw;         // words per source row
};

// A mask row and its view row, checked against everything passed by value.
__host__ __device__ inline bool load_mask(const int64_t* r, const int64_t* views, int V, int64_t total_words,
                                          int64_t tables_numel, int out_h, int out_w, Mask* o) {
  const int64_t base = r[0], H = r[1], W = r[2], view = r[3];
  if (view < 0 || view >= V || H <= 0 || W <= 0 || H > kI31 || W > kI31) return false;
  if (!load_row(views + view * kF, false, 1, kMaxNumel, tables_numel, out_h, out_w, &o->g)) return false;
  if (o->g.H != H || o->g.W != W || !mul_le(H, W, kI31)) return false;
  const int64_t sw = (W + 31) / 32;
  if (base < 0 || base > total_words - H * sw) return false;
  o->base = base;
  o->sw = static_cast<int>(sw);
  return true;
}

struct Stats {
  int x0, y0, x1, y1, area;   // x1, y1 inclusive here; area == 0: empty
};

__device__ inline void merge(Stats& a, const Stats& b) {
  a.x0 = min(a.x0, b.x0); a.y0 = min(a.y0, b.y0); a.x1 = max(a.x1, b.x1); a.y1 = max(a.y1, b.y1); a.area += b.area;
}

// grid (M * bands); out (M, Hp, ceil(Wp / 32)) int32 or (M, Hp, Wp) uint8; partials (M * bands, 5)
template <bool BYTES>
__global__ void __launch_bounds__(kThreads) bits_views_kernel(const uint32_t* __restrict__ words, int64_t total_words,
                                                              const int64_t* __restrict__ views, int V,
                                                              const int32_t* __restrict__ tables, int64_t tables_numel,
                                                              const int64_t* __restrict__ masks, int M, int bands,
                                                              void* __restrict__ out, int Hp, int Wp,
                                                              int32_t* __restrict__ partials) {
  __shared__ Stats red[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = static_cast<int>(blockIdx.x / bands), band = static_cast<int>(blockIdx.x % bands);
  if (m >= M) return;   // uniform over the workgroup; the grid is M * bands
  Mask k{};
  const bool ok = load_mask(masks + static_cast<int64_t>(m) * kMF, views, V, total_words, tables_numel, Hp, Wp, &k);
  const Row& g = k.g;
  const int wordsp = (Wp + 31) / 32;
  const int xlim = ok ? min(min(g.Wc, g.cw), Wp) : 0;   // columns at or beyond it are zero
  uint32_t* out32 = static_cast<uint32_t*>(out) + static_cast<int64_t>(m) * Hp * wordsp;
  uint8_t* out8 = static_cast<uint8_t*>(out) + static_cast<int64_t>(m) * Hp * Wp;

  Stats s{INT_MAX, INT_MAX, -1, -1, 0};   // uniform per wave
  for (int yy = wave; yy < kBand; yy += kWaves) {
    const int y = band * kBand + yy;
    if (y >= Hp) break;
    const int64_t ry = static_cast<int64_t>(g.cy0) + y;
    const bool row_ok = ok && y < g.Hc && y < g.ch && ry >= 0 && ry < g.rh;
    const uint32_t* srow = words;
    if (row_ok) srow += k.base + static_cast<int64_t>(min(max(tables[g.ty + ry], 0), g.H - 1)) * k.sw;
    for (int x0 = 0; x0 < Wp; x0 += 64 * kChunk) {
      uint32_t mine = 0u;   // the word lane l < 2 * kChunk stores: output word x0 / 32 + l
      if (row_ok && x0 < xlim) {
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
          const int x = x0 + 64 * c + lane;
          int bit = 0;
          if (x < xlim) {
            const int64_t rx = resized_col(g, x);
            if (rx >= 0 && rx < g.rw) {
              int sx = min(max(tables[g.tx + rx], 0), g.W - 1);
              if (g.flip_in) sx = g.W - 1 - sx;
              bit = static_cast<int>((srow[sx >> 5] >> (sx & 31)) & 1u);
            }
          }
          const unsigned long long vote = __ballot(bit);
          if (BYTES) {
            if (x < Wp) out8[static_cast<int64_t>(y) * Wp + x] = static_cast<uint8_t>(bit);
          } else {
            if (lane == 2 * c) mine = static_cast<uint32_t>(vote);
            if (lane == 2 * c + 1) mine = static_cast<uint32_t>(vote >> 32);
          }
          if (vote) {
            const int xa = x0 + 64 * c;
            s.area += __popcll(vote);
            s.x0 = min(s.x0, xa + __ffsll(static_cast<long long>(vote)) - 1);
            s.x1 = max(s.x1, xa + 63 - __clzll(static_cast<long long>(vote)));
            s.y0 = min(s.y0, y);
            s.y1 = max(s.y1, y);
          }
        }
      } else if (BYTES) {
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
          const int x = x0 + 64 * c + lane;
          if (x < Wp) out8[static_cast<int64_t>(y) * Wp + x] = 0;
        }
      }
      if (!BYTES) {
        const int w = x0 / 32 + lane;
        if (lane < 2 * kChunk && w < wordsp) out32[static_cast<int64_t>(y) * wordsp + w] = mine;
      }
    }
  }
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    Stats t = red[0];
    for (int w = 1; w < kWaves; ++w) merge(t, red[w]);
    int32_t* p = partials + static_cast<int64_t>(blockIdx.x) * 5;
    p[0] = t.x0; p[1] = t.y0; p[2] = t.x1; p[3] = t.y1; p[4] = t.area;
  }
}

// one thread per mask; stats (M, 5)
__global__ void __launch_bounds__(kThreads) bits_stats_kernel(const int32_t* __restrict__ partials, int M, int bands,
                                                              int32_t* __restrict__ stats) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  Stats t{INT_MAX, INT_MAX, -1, -1, 0};
  for (int b = 0; b < bands; ++b) {
    const int32_t* p = partials + (static_cast<int64_t>(m) * bands + b) * 5;
    if (p[4] > 0) merge(t, Stats{p[0], p[1], p[2], p[3], p[4]});
  }
  int32_t* o = stats + static_cast<int64_t>(m) * 5;
  const bool any = t.area > 0;
  o[0] = any ? t.x0 : 0; o[1] = any ? t.y0 : 0; o[2] = any ? t.x1 + 1 : 0; o[3] = any ? t.y1 + 1 : 0; o[4] = t.area;
}

int bands_of(int out_h) { return (out_h + kBand - 1) / kBand; }

}  // namespace

extern "C" int m2f_bits_views_workspace(int num_masks, int out_h, int64_t* words) {
  const char* fn = "m2f_bits_views_workspace";
  if (!words) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_masks <= 0 || out_h <= 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  *words = static_cast<int64_t>(num_masks) * bands_of(out_h) * 5;
  return m2f::ok();
}

extern "C" int m2f_bits_views(const int32_t* words, int64_t total_words, const int64_t* views_host,
                              const int64_t* views_dev, int num_views, const int32_t* tables, int64_t tables_numel,
                              const int64_t* masks_host, const int64_t* masks_dev, int num_masks, int out_form,
                              void* out, int out_h, int out_w, int32_t* stats, int32_t* workspace,
                              int64_t workspace_words, void* stream) {
  const char* fn = "m2f_bits_views";
  if (!words || !views_host || !views_dev || !tables || !masks_host || !masks_dev || !out || !stats || !workspace)
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (total_words <= 0 || num_views <= 0 || tables_numel <= 0 || num_masks <= 0 || out_h <= 0 || out_w <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (out_form != M2F_BITS_VIEW_BITS && out_form != M2F_BITS_VIEW_BYTES)
    return m2f::fail(M2F_EINVAL, "%s: out_form %d", fn, out_form);
  const bool bytes = out_form == M2F_BITS_VIEW_BYTES;
  if (!m2f::aligned(words, 4) || !m2f::aligned(tables, 4) || !m2f::aligned(stats, 4) || !m2f::aligned(workspace, 4) ||
      !m2f::aligned(views_host, 8) || !m2f::aligned(views_dev, 8) || !m2f::aligned(masks_host, 8) ||
      !m2f::aligned(masks_dev, 8) || (!bytes && !m2f::aligned(out, 4)))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (total_words > kI31) return m2f::fail(M2F_EUNSUPPORTED, "%s: a buffer of more than 2^31 - 1 words", fn);
  if (!mul_le(out_h, out_w, kI31)) return m2f::fail(M2F_EUNSUPPORTED, "%s: an output plane beyond 2^31 - 1 pixels", fn);
  // the output in words: a bit plane's own, a quarter of the bytes of the uint8 form
  const int64_t plane = bytes ? (static_cast<int64_t>(out_h) * out_w + 3) / 4
                              : static_cast<int64_t>(out_h) * ((out_w + 31) / 32);
  if (!mul_le(num_masks, plane, kI31)) return m2f::fail(M2F_EUNSUPPORTED, "%s: an output of more than 2^31 - 1 words", fn);
  const int bands = bands_of(out_h);
  const int64_t num_blocks = static_cast<int64_t>(num_masks) * bands;
  if (workspace_words < num_blocks * 5)
    return m2f::fail(M2F_EINVAL, "%s: workspace of %lld words, %lld needed", fn, static_cast<long long>(workspace_words),
                     static_cast<long long>(num_blocks * 5));
  for (int v = 0; v < num_views; ++v) {
    Row g;
    if (!load_row(views_host + static_cast<int64_t>(v) * kF, false, 1, kMaxNumel, tables_numel, out_h, out_w, &g))
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a size is not positive, or the tables or canvas leave their "
                       "ranges", fn, v);
  }
  for (int m = 0; m < num_masks; ++m) {
    Mask k;
    if (!load_mask(masks_host + static_cast<int64_t>(m) * kMF, views_host, num_views, total_words, tables_numel, out_h,
                   out_w, &k))
      return m2f::fail(M2F_EUNSUPPORTED, "%s: mask %d: its view is out of range, its size is not positive or not its "
                       "view's, or its plane leaves the buffer", fn, m);
  }
  unsigned grid;
  if (const int rc = m2f::grid_1d(num_blocks, fn, &grid)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  m2f::dispatch_bool(bytes, [&](auto b) {
    bits_views_kernel<decltype(b)::value><<<grid, kThreads, 0, st>>>(
        reinterpret_cast<const uint32_t*>(words), total_words, views_dev, num_views, tables, tables_numel, masks_dev,
        num_masks, bands, out, out_h, out_w, workspace);
  });
  if (const int rc = m2f::check_launch(fn)) return rc;
  bits_stats_kernel<<<m2f::ceil_div(num_masks, kThreads), kThreads, 0, st>>>(workspace, num_masks, bands, stats);
  return m2f::check_launch(fn);
}

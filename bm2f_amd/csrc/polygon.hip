// The COCO polygon rasteriser (rleFrPoly of pycocotools' maskApi.c, restated in include/bm2f.h and DESIGN.md) on
// one-bit-per-pixel planes: polygons -> the positions p = x * H + y at which a column-major walk of the mask flips
// -> the planes that mask_iou.hip's pair kernels read.
//
//   crossings_kernel   one thread per kept crossing.  The host counts an edge's kept crossings in closed form (they are
//                      the columns c0 .. c0 + n - 1 with 5 c + 2 inside the edge's x-range), so a thread finds its
//                      edge by binary search in the running sums, as sum_ragged_kernel finds its group, and evaluates
//                      its one crossing: two points of the edge's line for a flat edge (|dx| >= |dy|), a binary search
//                      over the edge's steps for a steep one (the x of step t is monotone in t).  No loop over an
//                      edge's length and no atomics: a 3,000-step edge costs its lanes what a 5-step one costs.  A
//                      polygon's closing sentinel H * W is one more table row of a single "crossing".  The thread
//                      stores the key (polygon << 32) | p; one sort of the keys orders every polygon of the batch.
//   decode_kernel      the parity walk of mask_iou.hip's decode_column for an annotation that is the OR of several
//                      polygons.  A lane owns a column and the lanes of a wave 64 consecutive columns; the rows are
//                      walked in chunks of 64 held as one 64-bit mask per lane.  Per chunk and part the lane seeks the
//                      part's cursor by binary search (the number of parts is unbounded, so no cursor is kept), turns
//                      the positions inside the chunk into the chunk's bits by xor-ing suffix masks, and ORs the part
//                      in.  A wave ballot per row is then the two words of the 64 columns, stored by lanes 0 and 32.
//                      Lanes beyond W vote 0, every word of a plane is stored exactly once, padding is not written.
//
// Floating point: rule 2 of the definition rounds every operation of ys + s * t + 0.5 on its own, and hipcc would
// contract s * t + ys into one FMA in device code.  This file is built with -ffp-contract=off (FILE_FLAGS in
// build.py); the pragma below says the same for a build that forgets the flag.  The slope s itself is divided on the
// host and arrives as a double.
//
// The tables live in device memory where the entry points cannot read them, so the kernels check every index they
// take from a table against the sizes passed by value: a malformed table gives unspecified keys or bits, never an
// access outside the buffers.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

constexpr int kEdgeFields = M2F_POLY_EDGE_FIELDS;   // kind, xs, ys, steps, c0, H, W, polygon
constexpr int kFlat = 0, kSteep = 1, kSentinel = 2;
constexpr int kRows = 64;                           // rows per chunk of the decoder: one 64-bit mask per lane
constexpr int64_t kIntMax = 0x7fffffff;

// the x (steep) or y (flat) of step t of an edge: trunc(a + s * t + 0.5) with every operation rounded on its own
__device__ __forceinline__ int line_at(int a, double s, int64_t t) {
  const double prod = s * static_cast<double>(t);
  const double sum = static_cast<double>(a) + prod;
  return static_cast<int>(sum + 0.5);
}

// grid (ceil(total / 256)): crossing i of the batch
__global__ void __launch_bounds__(256) crossings_kernel(const int32_t* __restrict__ edges,
                                                        const double* __restrict__ slopes,
                                                        const int64_t* __restrict__ starts, int64_t num_edges,
                                                        int64_t total, int64_t* __restrict__ keys) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (i >= total) return;
  int64_t lo = 0, hi = num_edges;   // the first edge with start > i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (starts[mid] <= i) lo = mid + 1; else hi = mid;
  }
  const int64_t e = lo - 1;
  int64_t key = kIntMax;            // what a malformed table row stores: a position beyond every pixel
  if (e >= 0) {
    const int32_t* d = edges + e * kEdgeFields;
    const int kind = d[0], xs = d[1], ys = d[2], steps = d[3];
    const int64_t H = d[5], W = d[6], poly = d[7];
    const int64_t c = d[4] + (i - starts[e]);
    const double s = slopes[e];
    if (H > 0 && W > 0 && H * W <= kIntMax && poly >= 0) {
      int64_t p = H * W;
      if (kind != kSentinel && c >= 0 && c < W) {
        const int64_t u = 5 * c + 2;   // the smaller x of the crossing's two points
        int64_t v;                     // the smaller y
        if (kind == kFlat) {
          const int64_t t = u - xs;
          v = min(line_at(ys, s, t), line_at(ys, s, t + 1));
        } else {
          // x(0) <= u < x(steps) when s > 0 and x(0) >= u + 1 > x(steps) when s < 0: the last step on the near side
          int64_t a = 0, b = max(steps, 0);
          for (int it = 0; it < 32 && b - a > 1; ++it) {
            const int64_t mid = (a + b) >> 1;
            const int x = line_at(xs, s, mid);
            if (s > 0 ? x <= u : x >= u + 1) a = mid; else b = mid;
          }
          v = ys + a;
        }
        const int64_t row = v <= 2 ? 0 : min((v + 2) / 5, H);   // ceil((v - 2) / 5) clamped to [0, H]
        p = c * H + row;
      }
      key = (poly << 32) | p;
    }
  }
  keys[i] = key;
}

// grid (num_blocks): blocks (num_blocks, 2) int32 = (annotation, block of 256 columns)
__global__ void __launch_bounds__(256) decode_kernel(const int32_t* __restrict__ positions, int64_t total,
                                                     const int64_t* __restrict__ pos_offsets, int64_t num_polys,
                                                     const int64_t* __restrict__ part_offsets, int num_anns,
                                                     const int32_t* __restrict__ sizes,
                                                     const int64_t* __restrict__ out_offsets,
                                                     const int32_t* __restrict__ blocks, int32_t* __restrict__ out,
                                                     int64_t out_words) {
  const int m = blocks[2 * static_cast<int64_t>(blockIdx.x)];
  const int xb = blocks[2 * static_cast<int64_t>(blockIdx.x) + 1];
  if (m < 0 || m >= num_anns || xb < 0) return;   // uniform over the workgroup, like every return below
  const int H = sizes[2 * m], W = sizes[2 * m + 1];
  if (H <= 0 || W <= 0 || static_cast<int64_t>(H) * W > kIntMax) return;
  if (static_cast<int64_t>(xb) * 256 >= W) return;
  const int words = (W + 31) / 32;
  const int64_t o0 = out_offsets[m];
  if (o0 < 0 || o0 + static_cast<int64_t>(H) * words > out_words) return;
  const int64_t q0 = min(max(part_offsets[m], static_cast<int64_t>(0)), num_polys);
  const int64_t q1 = min(max(part_offsets[m + 1], q0), num_polys);

  const int x = xb * 256 + threadIdx.x;
  const bool live = x < W;
  int32_t* o = out + o0 + (x >> 5);
  const bool writer = (threadIdx.x & 31) == 0 && (x >> 5) < words;
  const int shift = threadIdx.x & 32;
  for (int y0 = 0; y0 < H; y0 += kRows) {
    const int rows = min(kRows, H - y0);
    unsigned long long acc = 0;
    if (live) {
      const int64_t base = static_cast<int64_t>(x) * H + y0;   // the chunk is the pixels [base, base + rows)
      for (int64_t q = q0; q < q1; ++q) {
        const int64_t begin = min(max(pos_offsets[q], static_cast<int64_t>(0)), total);
        const int64_t end = min(max(pos_offsets[q + 1], begin), total);
        const int32_t* t = positions + begin;
        const int64_t n = end - begin;
        int64_t lo = 0, hi = n;   // the number of positions < base
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (t[mid] < base) lo = mid + 1; else hi = mid;
        }
        unsigned long long bits = (lo & 1) ? ~0ull : 0ull;   // the parity the chunk starts with
        for (int64_t k = lo; k < n; ++k) {
          const int64_t r = t[k] - base;
          if (r < 0 || r >= rows) break;   // r < 0: unsorted input, which gives unspecified bits
          bits ^= ~0ull << r;
        }
        acc |= bits;
      }
    }
    for (int r = 0; r < rows; ++r) {
      const unsigned long long vote = __ballot(static_cast<int>((acc >> r) & 1ull));
      if (writer) o[static_cast<int64_t>(y0 + r) * words] = static_cast<int32_t>(static_cast<uint32_t>(vote >> shift));
    }
  }
}

template <size_t kBytes, class... P>
bool all_aligned(const P*... p) {
  return (m2f::aligned(p, kBytes) && ...);
}

}  // namespace

extern "C" int m2f_poly_crossings(const int32_t* edges, const double* slopes, const int64_t* starts,
                                  int64_t num_edges, int64_t total, int64_t* keys, void* stream) {
  const char* fn = "m2f_poly_crossings";
  if (num_edges < 0 || total < 0) return m2f::fail(M2F_EINVAL, "%s: a negative size", fn);
  if (total == 0) return m2f::ok();
  if (!edges || !slopes || !starts || !keys) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_edges == 0) return m2f::fail(M2F_EINVAL, "%s: %lld crossings of no edge", fn, static_cast<long long>(total));
  if (!all_aligned<4>(edges) || !all_aligned<8>(slopes, starts, keys))
    return m2f::fail(M2F_EINVAL, "%s: edges must be 4-byte aligned, slopes, starts and keys 8-byte aligned", fn);
  if (total > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 crossings in one call", fn);
  crossings_kernel<<<m2f::ceil_div(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(edges, slopes, starts,
                                                                                           num_edges, total, keys);
  return m2f::check_launch(fn);
}

extern "C" int m2f_poly_decode_bits_ragged(const int32_t* positions, int64_t total, const int64_t* pos_offsets,
                                           int64_t num_polys, const int64_t* part_offsets, int num_anns,
                                           const int32_t* sizes, const int64_t* out_offsets, const int32_t* blocks,
                                           int64_t num_blocks, int32_t* out, int64_t out_words, void* stream) {
  const char* fn = "m2f_poly_decode_bits_ragged";
  if (!pos_offsets || !part_offsets || !sizes || !out_offsets || !out || (!positions && total > 0) ||
      (!blocks && num_blocks > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_anns <= 0 || num_polys < 0 || total < 0 || num_blocks < 0 || out_words < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (!all_aligned<4>(positions, out, sizes, blocks) || !all_aligned<8>(pos_offsets, part_offsets, out_offsets))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 column blocks", fn);
  if (num_blocks == 0) return m2f::ok();
  decode_kernel<<<static_cast<unsigned>(num_blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
      positions, total, pos_offsets, num_polys, part_offsets, num_anns, sizes, out_offsets, blocks, out, out_words);
  return m2f::check_launch(fn);
}

// COCO run-length encoding of binary masks on the device (the format is restated in include/bm2f.h).
//
// A mask is read column-major, so a lane owns one column of one mask and walks its H rows; the lanes of a wave
// own consecutive columns.  In the byte form a wave reads 64 consecutive bytes of a row per step; in the bit form
// the 32 lanes of a word read the same address (one request, broadcast).  The walk runs twice:
//
//   col_count_kernel   counts the transitions of the column (the one against the previous column's last pixel
//                      included), so that an exclusive scan over (mask, column) gives every column its first run
//                      slot and every mask its total;
//   positions_kernel   repeats the walk and stores the transition positions at those slots; the lane of the last
//                      column appends the closing H * W.
//
// After that the runs are a flat array and a lane owns one count:
//
//   deltas_kernel      finds its mask by a binary search over the masks' first slots, forms counts[i] -
//                      counts[i - 2] from four neighbouring positions and the number of characters it takes;
//   chars_kernel       writes the characters at the offset an inclusive scan of those numbers gives.
//
// Every store address comes from a scan of the previous stage: no atomics, no order between workgroups, the
// same bytes on every run, and no per-mask run capacity.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

namespace {

struct MaskSrc {
  const void* base;
  const int32_t* plane_index;   // nullable
  int src_planes;
  int64_t row, plane;           // strides in elements
};

template <int kForm>
__device__ __forceinline__ unsigned pixel(const void* plane, int64_t row, int y, int x) {
  if (kForm == M2F_RLE_BITS)
    return (static_cast<const uint32_t*>(plane)[static_cast<int64_t>(y) * row + (x >> 5)] >> (x & 31)) & 1u;
  return static_cast<const uint8_t*>(plane)[static_cast<int64_t>(y) * row + x] != 0 ? 1u : 0u;
}

template <int kForm>
__device__ __forceinline__ const void* plane_of(const MaskSrc& s, int m) {
  int64_t p = m;
  if (s.plane_index != nullptr) p = max(0, min(s.plane_index[m], s.src_planes - 1));
  if (kForm == M2F_RLE_BITS) return static_cast<const uint32_t*>(s.base) + p * s.plane;
  return static_cast<const uint8_t*>(s.base) + p * s.plane;
}

// calls f(y) at every row of column x whose pixel differs from the pixel before it in column-major order
template <int kForm, class F>
__device__ __forceinline__ void walk_column(const void* plane, int64_t row, int H, int x, F&& f) {
  unsigned prev = x > 0 ? pixel<kForm>(plane, row, H - 1, x - 1) : 0u;
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    const unsigned v = pixel<kForm>(plane, row, y, x);
    if (v != prev) f(y);
    prev = v;
  }
}

// grid (ceil(W / 256), M)
template <int kForm>
__global__ void __launch_bounds__(256) col_count_kernel(MaskSrc s, int H, int W, int32_t* __restrict__ counts) {
  const int x = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (x >= W) return;
  int n = 0;
  walk_column<kForm>(plane_of<kForm>(s, m), s.row, H, x, [&](int) { ++n; });
  counts[static_cast<int64_t>(m) * W + x] = n;
}

template <int kForm>
__global__ void __launch_bounds__(256) positions_kernel(MaskSrc s, int H, int W,
                                                        const int64_t* __restrict__ col_start,
                                                        int32_t* __restrict__ positions, int64_t capacity) {
  const int x = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (x >= W) return;
  const int64_t col = static_cast<int64_t>(m) * W + x;
  int64_t o = col_start[col] + m;
  const int p0 = x * H;   // < 2^31: checked by the entry point
  walk_column<kForm>(plane_of<kForm>(s, m), s.row, H, x, [&](int y) {
    if (o >= 0 && o < capacity) positions[o] = p0 + y;
    ++o;
  });
  if (x == W - 1) {
    const int64_t e = col_start[col + 1] + m;
    if (e >= 0 && e < capacity) positions[e] = H * W;
  }
}

__device__ __forceinline__ int char_count(int x) {
  int n = 0;
  bool more;
  do {
    const int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? (x != -1) : (x != 0);
    ++n;
  } while (more);
  return n;
}

__global__ void __launch_bounds__(256) deltas_kernel(const int32_t* __restrict__ positions,
                                                     const int64_t* __restrict__ col_start, int M, int W,
                                                     int64_t total, int32_t* __restrict__ delta,
                                                     uint8_t* __restrict__ nchar) {
  const int64_t g = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (g >= total) return;
  // the mask whose first slot col_start[m * W] + m is the last one <= g
  int lo = 0, hi = M;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (col_start[static_cast<int64_t>(mid) * W] + mid <= g) lo = mid; else hi = mid;
  }
  const int64_t first = col_start[static_cast<int64_t>(lo) * W] + lo;
  const int64_t i = g - first;   // index of the count inside its mask
  auto t = [&](int64_t j) { return positions[max(static_cast<int64_t>(0), min(first + j, total - 1))]; };
  int d = t(i) - (i > 0 ? t(i - 1) : 0);
  if (i > 2) d -= t(i - 2) - t(i - 3);
  delta[g] = d;
  nchar[g] = static_cast<uint8_t>(char_count(d));
}

__global__ void __launch_bounds__(256) chars_kernel(const int32_t* __restrict__ delta,
                                                    const uint8_t* __restrict__ nchar,
                                                    const int64_t* __restrict__ char_end, int64_t total,
                                                    uint8_t* __restrict__ out, int64_t capacity) {
  const int64_t g = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (g >= total) return;
  int x = delta[g];
  int64_t o = char_end[g] - nchar[g];
  bool more;
  do {
    int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? (x != -1) : (x != 0);
    if (more) c |= 0x20;
    if (o >= 0 && o < capacity) out[o] = static_cast<uint8_t>(c + 48);
    ++o;
  } while (more);
}

int check_src(const char* fn, const void* masks, int form, const int32_t* plane_index, int src_planes,
              int num_masks, int H, int W, int64_t row_stride, int64_t plane_stride) {
  if (!masks) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (form != M2F_RLE_BITS && form != M2F_RLE_BYTES) return m2f::fail(M2F_EINVAL, "%s: form %d", fn, form);
  if (num_masks <= 0 || H <= 0 || W <= 0 || src_planes <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (static_cast<int64_t>(H) * W > 0x7fffffff)
    return m2f::fail(M2F_EINVAL, "%s: %d x %d pixels do not fit a 32-bit count", fn, H, W);
  const int64_t row = form == M2F_RLE_BITS ? (static_cast<int64_t>(W) + 31) / 32 : W;
  if (row_stride < row)
    return m2f::fail(M2F_EINVAL, "%s: row stride %lld is smaller than the row (%lld)", fn,
                     static_cast<long long>(row_stride), static_cast<long long>(row));
  if (plane_stride < 0 || (src_planes > 1 && plane_stride / H < row_stride))
    return m2f::fail(M2F_EINVAL, "%s: plane stride %lld is smaller than %d rows", fn,
                     static_cast<long long>(plane_stride), H);
  if (plane_index == nullptr && src_planes < num_masks)
    return m2f::fail(M2F_EINVAL, "%s: %d source planes for %d masks", fn, src_planes, num_masks);
  if (form == M2F_RLE_BITS && !m2f::aligned(masks, 4))
    return m2f::fail(M2F_EINVAL, "%s: bit masks must be 4-byte aligned", fn);
  if (num_masks > 65535) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 65535 masks in one call", fn);
  return M2F_OK;
}

}  // namespace

extern "C" int m2f_rle_col_counts(const void* masks, int form, const int32_t* plane_index, int src_planes,
                                  int num_masks, int height, int width, int64_t row_stride, int64_t plane_stride,
                                  int32_t* counts, void* stream) {
  const char* fn = "m2f_rle_col_counts";
  if (!counts) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (const int rc = check_src(fn, masks, form, plane_index, src_planes, num_masks, height, width, row_stride,
                               plane_stride))
    return rc;
  const MaskSrc s{masks, plane_index, src_planes, row_stride, plane_stride};
  const dim3 grid(m2f::ceil_div(width, 256), num_masks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (form == M2F_RLE_BITS)
    col_count_kernel<M2F_RLE_BITS><<<grid, 256, 0, st>>>(s, height, width, counts);
  else
    col_count_kernel<M2F_RLE_BYTES><<<grid, 256, 0, st>>>(s, height, width, counts);
  return m2f::check_launch(fn);
}

extern "C" int m2f_rle_positions(const void* masks, int form, const int32_t* plane_index, int src_planes,
                                 int num_masks, int height, int width, int64_t row_stride, int64_t plane_stride,
                                 const int64_t* col_start, int32_t* positions, int64_t capacity, void* stream) {
  const char* fn = "m2f_rle_positions";
  if (!col_start || !positions) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (const int rc = check_src(fn, masks, form, plane_index, src_planes, num_masks, height, width, row_stride,
                               plane_stride))
    return rc;
  if (capacity < num_masks)
    return m2f::fail(M2F_EINVAL, "%s: capacity %lld holds no closing count per mask", fn,
                     static_cast<long long>(capacity));
  const MaskSrc s{masks, plane_index, src_planes, row_stride, plane_stride};
  const dim3 grid(m2f::ceil_div(width, 256), num_masks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (form == M2F_RLE_BITS)
    positions_kernel<M2F_RLE_BITS><<<grid, 256, 0, st>>>(s, height, width, col_start, positions, capacity);
  else
    positions_kernel<M2F_RLE_BYTES><<<grid, 256, 0, st>>>(s, height, width, col_start, positions, capacity);
  return m2f::check_launch(fn);
}

extern "C" int m2f_rle_deltas(const int32_t* positions, const int64_t* col_start, int num_masks, int width,
                              int64_t total, int32_t* delta, uint8_t* nchar, void* stream) {
  const char* fn = "m2f_rle_deltas";
  if (!positions || !col_start || !delta || !nchar) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_masks <= 0 || width <= 0 || total < num_masks)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive and total >= num_masks", fn);
  if ((total + 255) / 256 > 0x7fffffff) return m2f::fail(M2F_EUNSUPPORTED, "%s: total exceeds the grid range", fn);
  deltas_kernel<<<m2f::ceil_div(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      positions, col_start, num_masks, width, total, delta, nchar);
  return m2f::check_launch(fn);
}

extern "C" int m2f_rle_chars(const int32_t* delta, const uint8_t* nchar, const int64_t* char_end, int64_t total,
                             uint8_t* out, int64_t capacity, void* stream) {
  const char* fn = "m2f_rle_chars";
  if (!delta || !nchar || !char_end || !out) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (total <= 0 || capacity <= 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if ((total + 255) / 256 > 0x7fffffff) return m2f::fail(M2F_EUNSUPPORTED, "%s: total exceeds the grid range", fn);
  chars_kernel<<<m2f::ceil_div(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(delta, nchar, char_end,
                                                                                        total, out, capacity);
  return m2f::check_launch(fn);
}

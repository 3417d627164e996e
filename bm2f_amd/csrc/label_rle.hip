// COCO run-length encoding of the segments of label maps, and its inverse (the entry points are described in
// include/bm2f.h).
//
// A label map read column-major (p = x * H + y) is a sequence of runs of one label, and the RLE of the segment
// `map == v` is a selection of them: a run [s, e) of v contributes the transitions s and, when e < H * W, e.  No
// dense per-segment mask is formed.
//
//   col_count_kernel   the walk of rle.hip's col_count_kernel over labels: a lane owns one column of one image, the
//                      lanes of a wave own consecutive columns (a row step reads 64 consecutive elements), and a run
//                      starts where the label differs from the pixel before it in column-major order (pixel 0 always
//                      starts one).  An exclusive scan over (image, column) gives every column its first run slot.
//   runs_kernel        repeats the walk and stores every run's start and its key (image << 32 | label biased to
//                      unsigned, so that the int64 order is (image, signed label)).
//   One stable sort of the keys (the caller's) groups the runs by segment and keeps them in position order.
//   spans_kernel       a lane owns one sorted run: start, end (the next run of its image, or H * W), the number of
//                      transitions it contributes (0 for a label that is no segment) and whether it is the first run
//                      of a segment.  Scans of the last two give transition slots and segment ranks.
//   seg_keys_kernel    compacts the keys of the segments' first runs (when the caller gives no segment list).
//   segments_kernel    a wave owns one segment: it finds its runs by two binary searches over the sorted keys, stores
//                      their transitions and the closing H * W, and reduces area and box over the wave by shuffles.
//                      Waves beyond the number of segments (known on the device only) write one-entry dummies, so that
//                      the string stage of rle.hip runs unchanged on the capacity the host allocated.
//
//   paint_kernel       the inverse, in gather form: a lane owns one output pixel, walks its image's segments from last
//                      to first and counts each segment's run ends <= p by bisection; the first segment with an odd
//                      count gives the value.  A wave owns 64 consecutive x of one row, so stores are coalesced.
//
// Every store address comes from a scan or a search: no atomics, no order between workgroups, the same bytes on every
// run.  Tables live in device memory, so every index taken from one is checked against the sizes passed by value.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kF = M2F_LABEL_RLE_IMAGE_FIELDS;   // ptr, H, W, row stride, col_base, block_base, ignore key, pixels
constexpr int kHdr = M2F_LABEL_RLE_HEADER_FIELDS;
constexpr int64_t kIntMax = 0x7fffffff;

struct Image {
  const void* base;
  int H, W;
  int64_t row, col_base, ignore_key;
  bool ok;
};

__device__ __forceinline__ Image load_image(const int64_t* __restrict__ images, int64_t i) {
  const int64_t* d = images + i * kF;
  Image r;
  r.base = reinterpret_cast<const void*>(static_cast<uintptr_t>(d[0]));
  r.ok = d[1] > 0 && d[2] > 0 && d[1] * d[2] <= kIntMax && d[3] >= d[2] && d[4] >= 0 && r.base != nullptr;
  r.H = r.ok ? static_cast<int>(d[1]) : 0;
  r.W = r.ok ? static_cast<int>(d[2]) : 0;
  r.row = d[3], r.col_base = d[4], r.ignore_key = d[6];
  return r;
}

// the image whose first block (field 5 of its row) is the last one <= b
__device__ __forceinline__ int64_t image_of_block(const int64_t* __restrict__ images, int num_images, int64_t b) {
  int64_t lo = 0, hi = num_images;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (images[mid * kF + 5] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t make_key(int64_t image, int32_t label) {
  return (image << 32) | static_cast<int64_t>(static_cast<uint32_t>(label) ^ 0x80000000u);
}
__device__ __forceinline__ int32_t key_label(int64_t key) {
  return static_cast<int32_t>(static_cast<uint32_t>(key & 0xffffffff) ^ 0x80000000u);
}

// calls f(y, v) at every row of column x whose label differs from the pixel before it in column-major order
template <class T, class F>
__device__ __forceinline__ void walk_column(const T* __restrict__ base, int64_t row, int H, int x, F&& f) {
  bool have = x > 0;
  int32_t prev = have ? static_cast<int32_t>(base[static_cast<int64_t>(H - 1) * row + x - 1]) : 0;
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    const int32_t v = static_cast<int32_t>(base[static_cast<int64_t>(y) * row + x]);
    if (!have || v != prev) f(y, v);
    prev = v;
    have = true;
  }
}

// grid (num_blocks): block b is 256 columns of the image found by image_of_block
template <class T>
__global__ void __launch_bounds__(256) col_count_kernel(const int64_t* __restrict__ images, int num_images,
                                                        int32_t* __restrict__ counts, int64_t total_cols) {
  const int64_t i = image_of_block(images, num_images, blockIdx.x);
  const Image im = load_image(images, i);
  const int64_t x = (static_cast<int64_t>(blockIdx.x) - images[i * kF + 5]) * 256 + threadIdx.x;
  if (!im.ok || x < 0 || x >= im.W || im.col_base + x >= total_cols) return;
  int n = 0;
  walk_column(static_cast<const T*>(im.base), im.row, im.H, static_cast<int>(x), [&](int, int32_t) { ++n; });
  counts[im.col_base + x] = n;
}

template <class T>
__global__ void __launch_bounds__(256) runs_kernel(const int64_t* __restrict__ images, int num_images,
                                                   const int64_t* __restrict__ col_start, int64_t total_cols,
                                                   int32_t* __restrict__ run_pos, int64_t* __restrict__ run_key,
                                                   int64_t capacity) {
  const int64_t i = image_of_block(images, num_images, blockIdx.x);
  const Image im = load_image(images, i);
  const int64_t x = (static_cast<int64_t>(blockIdx.x) - images[i * kF + 5]) * 256 + threadIdx.x;
  if (!im.ok || x < 0 || x >= im.W || im.col_base + x >= total_cols) return;
  int64_t o = col_start[im.col_base + x];
  const int p0 = static_cast<int>(x) * im.H;   // < 2^31: load_image checked H * W
  walk_column(static_cast<const T*>(im.base), im.row, im.H, static_cast<int>(x), [&](int y, int32_t v) {
    if (o >= 0 && o < capacity) {
      run_pos[o] = p0 + y;
      run_key[o] = make_key(i, v);
    }
    ++o;
  });
}

// the first index in [0, n) with a[index] >= v (kUpper: > v)
template <bool kUpper>
__device__ __forceinline__ int64_t bound(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (kUpper ? a[mid] <= v : a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one lane per sorted run
__global__ void __launch_bounds__(256) spans_kernel(const int64_t* __restrict__ sorted_key,
                                                    const int64_t* __restrict__ perm, int64_t num_runs,
                                                    const int32_t* __restrict__ run_pos,
                                                    const int64_t* __restrict__ run_base,
                                                    const int64_t* __restrict__ images, int num_images,
                                                    const int64_t* __restrict__ seg_key,
                                                    const int64_t* __restrict__ num_segments, int64_t seg_capacity,
                                                    int32_t* __restrict__ start, int32_t* __restrict__ end,
                                                    int32_t* __restrict__ ntrans, int32_t* __restrict__ first) {
  const int64_t j = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (j >= num_runs) return;
  const int64_t key = sorted_key[j], r = perm[j], i = key >> 32;
  int s = 0, e = 0, n = 0, f = 0;
  if (key >= 0 && i < num_images && r >= 0 && r < num_runs) {
    const Image im = load_image(images, i);
    const int pixels = im.H * im.W;
    s = run_pos[r];
    e = (r + 1 < num_runs && r + 1 < run_base[i + 1]) ? run_pos[r + 1] : pixels;
    bool member = im.ok && key != im.ignore_key && s >= 0 && s < e && e <= pixels;
    if (member && seg_key != nullptr) {
      const int64_t S = min(max(*num_segments, static_cast<int64_t>(0)), seg_capacity);
      const int64_t at = bound<false>(seg_key, S, key);
      member = at < S && seg_key[at] == key;
    }
    if (member) {
      n = e < pixels ? 2 : 1;
      f = (j == 0 || sorted_key[j - 1] != key) ? 1 : 0;
    }
  }
  start[j] = s, end[j] = e, ntrans[j] = n, first[j] = f;
}

// seg_rank = inclusive scan of first; the key of a segment's first run goes to its rank
__global__ void __launch_bounds__(256) seg_keys_kernel(const int64_t* __restrict__ sorted_key,
                                                       const int32_t* __restrict__ first,
                                                       const int64_t* __restrict__ seg_rank, int64_t num_runs,
                                                       int64_t* __restrict__ seg_key, int64_t seg_capacity,
                                                       int64_t* __restrict__ num_segments) {
  const int64_t j = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (j >= num_runs) return;
  if (first[j]) {
    const int64_t s = seg_rank[j] - 1;
    if (s >= 0 && s < seg_capacity) seg_key[s] = sorted_key[j];
  }
  if (j == num_runs - 1) *num_segments = min(seg_rank[j], seg_capacity);
}

// one wave per segment slot s < seg_capacity + 1 (4 per workgroup); tscan = inclusive scan of ntrans
__global__ void __launch_bounds__(256) segments_kernel(const int64_t* __restrict__ sorted_key, int64_t num_runs,
                                                       const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ end,
                                                       const int32_t* __restrict__ ntrans,
                                                       const int64_t* __restrict__ tscan,
                                                       const int64_t* __restrict__ images, int num_images,
                                                       const int64_t* __restrict__ seg_key,
                                                       const int64_t* __restrict__ num_segments, int64_t seg_capacity,
                                                       int32_t* __restrict__ positions, int64_t capacity,
                                                       int64_t* __restrict__ seg_start, int32_t* __restrict__ headers) {
  const int lane = threadIdx.x & 63;
  const int64_t s = blockIdx.x * static_cast<int64_t>(4) + (threadIdx.x >> 6);
  if (s > seg_capacity) return;   // uniform over the wave
  const int64_t S = min(max(*num_segments, static_cast<int64_t>(0)), seg_capacity);
  const int64_t all = num_runs > 0 ? tscan[num_runs - 1] : 0;
  int32_t* hdr = headers + s * kHdr;
  if (s >= S) {   // a dummy: one entry (0, from the zeroed buffer) after every real transition
    if (lane == 0) {
      seg_start[s] = all;
      for (int k = 0; k < kHdr; ++k) hdr[k] = 0;
    }
    return;
  }
  const int64_t key = seg_key[s], i = key >> 32;
  const bool good = key >= 0 && i < num_images;
  const Image im = good ? load_image(images, i) : Image{nullptr, 0, 0, 0, 0, -1, false};
  const int H = max(im.H, 1), pixels = im.H * im.W;
  const int64_t lo = bound<false>(sorted_key, num_runs, key);
  const int64_t hi = (im.ok && key != im.ignore_key) ? bound<true>(sorted_key, num_runs, key) : lo;
  const int64_t t0 = lo > 0 ? tscan[lo - 1] : 0, t1 = hi > 0 ? tscan[hi - 1] : 0;
  int64_t area = 0;
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
  for (int64_t j = lo + lane; j < hi; j += 64) {
    const int a = start[j], b = end[j], n = ntrans[j];
    if (n == 0) continue;   // no run of a segment: the spans kernel refused it
    const int64_t o = tscan[j] - n + s;
    if (o >= 0 && o < capacity) positions[o] = a;
    if (n == 2 && o + 1 >= 0 && o + 1 < capacity) positions[o + 1] = b;
    area += b - a;
    const int xa = a / H, xb = (b - 1) / H;
    x0 = min(x0, xa), x1 = max(x1, xb);
    if (xa != xb) {   // the run crosses a column boundary: rows 0 .. H - 1
      y0 = 0, y1 = H - 1;
    } else {
      y0 = min(y0, a - xa * H), y1 = max(y1, b - 1 - xa * H);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    area += __shfl_down(area, d);
    x0 = min(x0, __shfl_down(x0, d)), y0 = min(y0, __shfl_down(y0, d));
    x1 = max(x1, __shfl_down(x1, d)), y1 = max(y1, __shfl_down(y1, d));
  }
  if (lane == 0) {
    const int64_t o = t1 + s;   // the closing count ends at H * W
    if (o >= 0 && o < capacity) positions[o] = pixels;
    seg_start[s] = t0;
    const bool empty = area == 0;
    hdr[0] = static_cast<int32_t>(i), hdr[1] = key_label(key), hdr[2] = static_cast<int32_t>(area);
    hdr[3] = empty ? 0 : x0, hdr[4] = empty ? 0 : y0, hdr[5] = empty ? -1 : x1, hdr[6] = empty ? -1 : y1;
    hdr[7] = pixels;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the inverse
// ---------------------------------------------------------------------------------------------------------------
constexpr int kPF = M2F_LABEL_RLE_PAINT_FIELDS;   // H, W, first segment, end segment, out offset, block_base

// grid (num_blocks): block b of an image is 64 columns x 4 rows; a wave owns one row of it
template <class T>
__global__ void __launch_bounds__(256) paint_kernel(const int32_t* __restrict__ positions, int64_t total,
                                                    const int64_t* __restrict__ offsets, int64_t num_segments,
                                                    const int32_t* __restrict__ values,
                                                    const int64_t* __restrict__ images, int num_images, int32_t fill,
                                                    T* __restrict__ out, int64_t out_elems) {
  int64_t lo = 0, hi = num_images;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (images[mid * kPF + 5] <= static_cast<int64_t>(blockIdx.x)) lo = mid; else hi = mid;
  }
  const int64_t* d = images + lo * kPF;
  const int64_t H = d[0], W = d[1], o0 = d[4], b = static_cast<int64_t>(blockIdx.x) - d[5];
  if (H <= 0 || W <= 0 || H * W > kIntMax || b < 0 || o0 < 0 || o0 + H * W > out_elems) return;
  const int64_t s0 = min(max(d[2], static_cast<int64_t>(0)), num_segments);
  const int64_t s1 = min(max(d[3], s0), num_segments);
  const int64_t bx = (W + 63) / 64;
  const int64_t x = (b % bx) * 64 + (threadIdx.x & 63), y = (b / bx) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int p = static_cast<int>(x * H + y);
  int32_t v = fill;
  for (int64_t s = s1 - 1; s >= s0; --s) {
    const int64_t begin = min(max(offsets[s], static_cast<int64_t>(0)), total);
    const int64_t end = min(max(offsets[s + 1], begin), total);
    const int32_t* t = positions + begin;
    int64_t a = 0, n = end - begin;   // the number of run ends <= p
    while (a < n) {
      const int64_t mid = (a + n) >> 1;
      if (t[mid] <= p) a = mid + 1; else n = mid;
    }
    if (a & 1) {
      v = values[s];
      break;
    }
  }
  out[o0 + y * W + x] = static_cast<T>(v);
}

template <class F>
bool dispatch_label(int bytes, F&& f) {
  if (bytes == 1) f(m2f::Tag<uint8_t>{});
  else if (bytes == 2) f(m2f::Tag<int16_t>{});
  else if (bytes == 4) f(m2f::Tag<int32_t>{});
  else return false;
  return true;
}

int check_walk(const char* fn, const int64_t* images, int num_images, int64_t num_blocks, int label_bytes,
               int64_t total_cols) {
  if (!images) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_images <= 0 || num_blocks < 0 || total_cols < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4)
    return m2f::fail(M2F_EINVAL, "%s: labels are 1 (uint8), 2 (int16) or 4 (int32) bytes, got dtype %d", fn,
                     label_bytes);
  if (!m2f::aligned(images, 8)) return m2f::fail(M2F_EINVAL, "%s: images must be 8-byte aligned", fn);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 column blocks", fn);
  return M2F_OK;
}

}  // namespace

extern "C" int m2f_label_rle_col_counts(const int64_t* images, int num_images, int64_t num_blocks, int label_bytes,
                                        int32_t* counts, int64_t total_cols, void* stream) {
  const char* fn = "m2f_label_rle_col_counts";
  if (!counts) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (const int rc = check_walk(fn, images, num_images, num_blocks, label_bytes, total_cols)) return rc;
  if (num_blocks == 0) return m2f::ok();
  dispatch_label(label_bytes, [&](auto t) {
    using T = typename decltype(t)::type;
    col_count_kernel<T><<<static_cast<unsigned>(num_blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
        images, num_images, counts, total_cols);
  });
  return m2f::check_launch(fn);
}

extern "C" int m2f_label_rle_runs(const int64_t* images, int num_images, int64_t num_blocks, int label_bytes,
                                  const int64_t* col_start, int64_t total_cols, int32_t* run_pos, int64_t* run_key,
                                  int64_t capacity, void* stream) {
  const char* fn = "m2f_label_rle_runs";
  if (!col_start || !run_pos || !run_key) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (const int rc = check_walk(fn, images, num_images, num_blocks, label_bytes, total_cols)) return rc;
  if (capacity < 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (num_blocks == 0) return m2f::ok();
  dispatch_label(label_bytes, [&](auto t) {
    using T = typename decltype(t)::type;
    runs_kernel<T><<<static_cast<unsigned>(num_blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
        images, num_images, col_start, total_cols, run_pos, run_key, capacity);
  });
  return m2f::check_launch(fn);
}

extern "C" int m2f_label_rle_spans(const int64_t* sorted_key, const int64_t* perm, int64_t num_runs,
                                   const int32_t* run_pos, const int64_t* run_base, const int64_t* images,
                                   int num_images, const int64_t* seg_key, const int64_t* num_segments,
                                   int64_t seg_capacity, int32_t* start, int32_t* end, int32_t* ntrans,
                                   int32_t* first, void* stream) {
  const char* fn = "m2f_label_rle_spans";
  if (!sorted_key || !perm || !run_pos || !run_base || !images || !start || !end || !ntrans || !first ||
      (seg_key && !num_segments))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_runs <= 0 || num_images <= 0 || seg_capacity < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  unsigned grid;
  if (const int rc = m2f::grid_1d((num_runs + 255) / 256, fn, &grid)) return rc;
  spans_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sorted_key, perm, num_runs, run_pos, run_base,
                                                                   images, num_images, seg_key, num_segments,
                                                                   seg_capacity, start, end, ntrans, first);
  return m2f::check_launch(fn);
}

extern "C" int m2f_label_rle_seg_keys(const int64_t* sorted_key, const int32_t* first, const int64_t* seg_rank,
                                      int64_t num_runs, int64_t* seg_key, int64_t seg_capacity,
                                      int64_t* num_segments, void* stream) {
  const char* fn = "m2f_label_rle_seg_keys";
  if (!sorted_key || !first || !seg_rank || !seg_key || !num_segments)
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_runs <= 0 || seg_capacity < 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  unsigned grid;
  if (const int rc = m2f::grid_1d((num_runs + 255) / 256, fn, &grid)) return rc;
  seg_keys_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sorted_key, first, seg_rank, num_runs, seg_key,
                                                                      seg_capacity, num_segments);
  return m2f::check_launch(fn);
}

extern "C" int m2f_label_rle_segments(const int64_t* sorted_key, int64_t num_runs, const int32_t* start,
                                      const int32_t* end, const int32_t* ntrans, const int64_t* tscan,
                                      const int64_t* images, int num_images, const int64_t* seg_key,
                                      const int64_t* num_segments, int64_t seg_capacity, int32_t* positions,
                                      int64_t capacity, int64_t* seg_start, int32_t* headers, void* stream) {
  const char* fn = "m2f_label_rle_segments";
  if (!sorted_key || !start || !end || !ntrans || !tscan || !images || !seg_key || !num_segments || !positions ||
      !seg_start || !headers)
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_runs <= 0 || num_images <= 0 || seg_capacity < 0 || capacity < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  unsigned grid;
  if (const int rc = m2f::grid_1d((seg_capacity + 1 + 3) / 4, fn, &grid)) return rc;
  segments_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sorted_key, num_runs, start, end, ntrans, tscan,
                                                                      images, num_images, seg_key, num_segments,
                                                                      seg_capacity, positions, capacity, seg_start,
                                                                      headers);
  return m2f::check_launch(fn);
}

extern "C" int m2f_rle_paint_labels(const int32_t* positions, int64_t total, const int64_t* offsets,
                                    int64_t num_segments, const int32_t* values, const int64_t* images,
                                    int num_images, int64_t num_blocks, int64_t fill, int label_bytes, void* out,
                                    int64_t out_elems, void* stream) {
  const char* fn = "m2f_rle_paint_labels";
  if (!offsets || !images || !out || (!positions && total > 0) || (!values && num_segments > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_images <= 0 || total < 0 || num_segments < 0 || num_blocks < 0 || out_elems < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4)
    return m2f::fail(M2F_EINVAL, "%s: labels are 1 (uint8), 2 (int16) or 4 (int32) bytes, got dtype %d", fn,
                     label_bytes);
  if (!m2f::aligned(positions, 4) || !m2f::aligned(values, 4) || !m2f::aligned(offsets, 8) ||
      !m2f::aligned(images, 8) || !m2f::aligned(out, label_bytes))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 pixel blocks", fn);
  if (num_blocks == 0) return m2f::ok();
  dispatch_label(label_bytes, [&](auto t) {
    using T = typename decltype(t)::type;
    paint_kernel<T><<<static_cast<unsigned>(num_blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
        positions, total, offsets, num_segments, values, images, num_images, static_cast<int32_t>(fill),
        static_cast<T*>(out), out_elems);
  });
  return m2f::check_launch(fn);
}

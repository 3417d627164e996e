// Mask IoU of instance sequences on one-bit-per-pixel planes (the format is restated in include/bm2f.h).
//
// The uniform kernels serve the instance sequences of one video, all of one size; the ragged kernels serve many
// images of different sizes per launch (the COCO evaluator), dealt to workgroups by host-built tables.  Both are the
// same three device pieces and differ only in where a workgroup's arguments come from:
//
//   decode_column   the reverse of rle.hip: run ends (cumulative counts in the column-major order p = x * H + y) ->
//                   a bit plane (H, words).  A lane owns one column of one mask and the lanes of a wave own 64
//                   consecutive columns.  The pixel p is set when an odd number of run ends is <= p, so the lane
//                   finds the number of ends <= x * H by a binary search and walks its H rows with a cursor; a wave
//                   ballot per row is the two words of those 64 columns, stored by lanes 0 and 32.  Lanes beyond W
//                   vote 0, which zeroes the tail bits.  Every word of the plane is stored exactly once.
//   tile_counts     inter[d][g] = sum popcount(a_d & b_g), area_a[d], area_b[g] of a kTA x kTB tile of planes over
//                   kChunk word positions of one frame.  A thread loads 4 consecutive words (one 128-bit load where
//                   every plane is 16-byte aligned) of each of the kTA + kTB planes and keeps the kVals counts in
//                   registers; tail bits of a row's last word are masked here.  reduce_store sums the counts over
//                   the wave by shuffles, over the four waves through LDS, and stores one int32 partial per workgroup.
//   sum_slot        the tile whose partials hold an output of inter, area_a or area_b, and its slot among them; one
//                   thread per output sums its partials in index order into int64.
//
//   decode_kernel, pair_kernel, sum_kernel   grids (ceil(W / 256), M), (chunks, T, tiles) and one thread per output:
//       the block indices are the arguments.  A is read ceil(Db / kTB) times and B ceil(Da / kTA) times per launch.
//   decode_ragged_kernel   a per-mask (H, W) and output word offset; a table row is (mask, block of 256 columns).
//   pair_ragged_kernel     one frame per group, planes at word offsets into one flat buffer; a table row is (group,
//       a-tile, b-tile, chunk).  A workgroup loads 128 bits when the buffer and all of its planes' offsets are 16-byte
//       aligned (the host pads planes to 4 words); the words such a load reads beyond a plane's end are dropped.
//   sum_ragged_kernel      finds its group by binary search.
//
// The tables live in device memory where the entry points cannot read them, so the ragged kernels check every index
// they take from a table against the sizes passed by value: a malformed table gives unspecified counts, never an
// access outside the buffers.
//
// No atomics and no zeroed buffer: every partial that is summed was stored by the launch before it.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kTA = M2F_PAIR_TA, kTB = M2F_PAIR_TB;
constexpr int kThreads = 256, kVec = 4, kIters = 4;
constexpr int kChunk = kThreads * kVec * kIters;          // word positions of one frame per workgroup
constexpr int kVals = kTA * kTB + kTA + kTB;
static_assert(kChunk == M2F_PAIR_CHUNK_WORDS, "header constant");
static_assert(kVals <= kThreads, "one thread per value in the cross-wave sum");
constexpr int kGroupFields = M2F_RAGGED_GROUP_FIELDS;   // H, W, na, nb, a_start, b_start, inter_start, tile_start
constexpr int64_t kIntMax = 0x7fffffff;

// Column x of mask m -> bit x % 32 of word x / 32 of the H rows of `plane`.  Thread i of a workgroup of 256 has
// x = 256 * k + i, and every thread of a wave calls this, lanes beyond W included: the rows are wave ballots.
// H * W < 2^31: checked by the callers.
__device__ __forceinline__ void decode_column(const int32_t* __restrict__ positions, int64_t total,
                                              const int64_t* __restrict__ offsets, int m, int x, int H, int W,
                                              int words, int32_t* __restrict__ plane) {
  const bool live = x < W;
  const int64_t begin = min(max(offsets[m], static_cast<int64_t>(0)), total);
  const int64_t end = min(max(offsets[m + 1], begin), total);
  const int32_t* t = positions + begin;   // the run ends of the mask, clamped to the buffer
  const int64_t n = live ? end - begin : 0;
  const int p0 = live ? x * H : 0;
  // the number of run ends <= p0
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (t[mid] <= p0) lo = mid + 1; else hi = mid;
  }
  int64_t cur = lo;
  int next = cur < n ? t[cur] : 0x7fffffff;
  int32_t* o = plane + (x >> 5);
  const bool writer = (threadIdx.x & 31) == 0 && (x >> 5) < words;
  const int shift = threadIdx.x & 32;
  for (int y = 0; y < H; ++y) {
    const int p = p0 + y;
    while (next <= p) {
      ++cur;
      next = cur < n ? t[cur] : 0x7fffffff;
    }
    const unsigned long long vote = __ballot(static_cast<int>(cur & 1));
    if (writer) o[static_cast<int64_t>(y) * words] = static_cast<int32_t>(static_cast<uint32_t>(vote >> shift));
  }
}

// i0 is a multiple of 4; on the wide path p + i0 is 16-byte aligned and the four words lie inside the buffer: n is a
// multiple of 4 (pair_kernel), or the plane is followed by words the caller masks (pair_ragged_kernel)
__device__ __forceinline__ void load4(bool wide, const uint32_t* __restrict__ p, int i0, int n, uint32_t (&v)[kVec]) {
  if (p == nullptr || (wide && i0 >= n)) {
    v[0] = v[1] = v[2] = v[3] = 0u;
  } else if (wide) {
    const uint4 q = *reinterpret_cast<const uint4*>(p + i0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < kVec; ++k) v[k] = i0 + k < n ? p[i0 + k] : 0u;
  }
}

// The counts of one workgroup: planes pa[i] / pb[j] of frame_words words in rows of `words` (a null pointer is an
// absent plane; the pointers and `wide` are uniform over the workgroup), word positions [chunk0, chunk0 + kChunk).
// With kPadded the words a wide load reads beyond the plane's end are dropped; without it frame_words is a multiple
// of 4 on the wide path and there are none.
template <bool kPadded>
__device__ __forceinline__ void tile_counts(bool wide, const uint32_t* const (&pa)[kTA],
                                            const uint32_t* const (&pb)[kTB], int64_t chunk0, int frame_words,
                                            int words, uint32_t tail_mask, int (&acc)[kTA][kTB], int (&na)[kTA],
                                            int (&nb)[kTB]) {
#pragma unroll 1
  for (int it = 0; it < kIters; ++it) {
    const int64_t pos = chunk0 + (it * kThreads + threadIdx.x) * kVec;   // word position inside the frame
    if (pos < frame_words) {
      const int i0 = static_cast<int>(pos);
      uint32_t keep[kVec];
      int col = i0 % words;
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
        keep[k] = col == words - 1 ? tail_mask : 0xffffffffu;
        if (kPadded && i0 + k >= frame_words) keep[k] = 0u;
        col = col + 1 == words ? 0 : col + 1;
      }
      uint32_t va[kTA][kVec], vb[kTB][kVec];
#pragma unroll
      for (int i = 0; i < kTA; ++i) load4(wide, pa[i], i0, frame_words, va[i]);
#pragma unroll
      for (int j = 0; j < kTB; ++j) load4(wide, pb[j], i0, frame_words, vb[j]);
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
#pragma unroll
        for (int i = 0; i < kTA; ++i) {
          va[i][k] &= keep[k];
          na[i] += __popc(va[i][k]);
        }
#pragma unroll
        for (int j = 0; j < kTB; ++j) {
          vb[j][k] &= keep[k];
          nb[j] += __popc(vb[j][k]);
        }
#pragma unroll
        for (int i = 0; i < kTA; ++i)
#pragma unroll
          for (int j = 0; j < kTB; ++j) acc[i][j] += __popc(va[i][k] & vb[j][k]);
      }
    }
  }
}

// the counts of a workgroup -> its kVals int32 partials at `row`: over the wave by shuffles, over the four waves
// through LDS
__device__ __forceinline__ void reduce_store(const int (&acc)[kTA][kTB], const int (&na)[kTA], const int (&nb)[kTB],
                                             int32_t* __restrict__ row) {
  __shared__ int wave_sum[kThreads / 64][kVals];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto reduce = [&](int v, int slot) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    if (lane == 0) wave_sum[wave][slot] = v;
  };
#pragma unroll
  for (int i = 0; i < kTA; ++i)
#pragma unroll
    for (int j = 0; j < kTB; ++j) reduce(acc[i][j], i * kTB + j);
#pragma unroll
  for (int i = 0; i < kTA; ++i) reduce(na[i], kTA * kTB + i);
#pragma unroll
  for (int j = 0; j < kTB; ++j) reduce(nb[j], kTA * kTB + kTA + j);
  __syncthreads();
  if (threadIdx.x < kVals) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += wave_sum[w][threadIdx.x];
    row[threadIdx.x] = s;
  }
}

// Output `local` of inter (nb columns, row-major), area_a or area_b -> the tile (a-tile * tiles_b + b-tile) whose
// partials hold it and its slot among their kVals values.  The areas are read from the first tile of the other side.
enum SumPart { kInter, kAreaA, kAreaB };
__device__ __forceinline__ void sum_slot(SumPart part, int64_t local, int64_t nb, int64_t tiles_b, int64_t* tile,
                                         int* slot) {
  if (part == kInter) {
    const int64_t i = local / nb, j = local % nb;
    *tile = (i / kTA) * tiles_b + j / kTB;
    *slot = static_cast<int>((i % kTA) * kTB + j % kTB);
  } else if (part == kAreaA) {
    *tile = (local / kTA) * tiles_b;
    *slot = static_cast<int>(kTA * kTB + local % kTA);
  } else {
    *tile = local / kTB;
    *slot = static_cast<int>(kTA * kTB + kTA + local % kTB);
  }
}

// grid (ceil(W / 256), M)
__global__ void __launch_bounds__(256) decode_kernel(const int32_t* __restrict__ positions, int64_t total,
                                                     const int64_t* __restrict__ offsets, int H, int W, int words,
                                                     int32_t* __restrict__ out) {
  decode_column(positions, total, offsets, blockIdx.y, blockIdx.x * 256 + threadIdx.x, H, W, words,
                out + static_cast<int64_t>(blockIdx.y) * H * words);
}

// grid (chunks, T, tiles_a * tiles_b)
template <bool kWide>
__global__ void __launch_bounds__(kThreads) pair_kernel(const uint32_t* __restrict__ a, int Da, int64_t stride_a,
                                                        const uint32_t* __restrict__ b, int Db, int64_t stride_b,
                                                        int frame_words, int words, uint32_t tail_mask, int tiles_b,
                                                        int32_t* __restrict__ partial) {
  const int chunk = blockIdx.x, t = blockIdx.y;
  const int ia0 = (blockIdx.z / tiles_b) * kTA, ib0 = (blockIdx.z % tiles_b) * kTB;
  const int64_t frame = static_cast<int64_t>(t) * frame_words;
  const uint32_t *pa[kTA], *pb[kTB];
#pragma unroll
  for (int i = 0; i < kTA; ++i) pa[i] = ia0 + i < Da ? a + (ia0 + i) * stride_a + frame : nullptr;
#pragma unroll
  for (int j = 0; j < kTB; ++j) pb[j] = ib0 + j < Db ? b + (ib0 + j) * stride_b + frame : nullptr;
  int acc[kTA][kTB], na[kTA], nb[kTB];   // zeroed in the kernel's body: a helper costs a wave of occupancy
#pragma unroll
  for (int i = 0; i < kTA; ++i) {
    na[i] = 0;
#pragma unroll
    for (int j = 0; j < kTB; ++j) acc[i][j] = 0;
  }
#pragma unroll
  for (int j = 0; j < kTB; ++j) nb[j] = 0;
  tile_counts<false>(kWide, pa, pb, static_cast<int64_t>(chunk) * kChunk, frame_words, words, tail_mask, acc, na, nb);
  const int64_t block = (static_cast<int64_t>(blockIdx.z) * gridDim.y + t) * gridDim.x + chunk;
  reduce_store(acc, na, nb, partial + block * kVals);
}

// one thread per output: inter (Da, Db), then area_a (Da, T), then area_b (Db, T)
__global__ void __launch_bounds__(256) sum_kernel(const int32_t* __restrict__ partial, int Da, int Db, int T,
                                                  int chunks, int tiles_b, int64_t* __restrict__ inter,
                                                  int64_t* __restrict__ area_a, int64_t* __restrict__ area_b) {
  const int64_t g = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  const int64_t n_inter = static_cast<int64_t>(Da) * Db, n_a = static_cast<int64_t>(Da) * T;
  if (g >= n_inter + n_a + static_cast<int64_t>(Db) * T) return;
  int64_t tile;
  int slot, t0 = 0, t1 = T;   // inter sums every frame, an area one
  int64_t* dst = inter + g;
  if (g < n_inter) {
    sum_slot(kInter, g, Db, tiles_b, &tile, &slot);
  } else {
    const bool is_a = g < n_inter + n_a;
    const int64_t r = g - n_inter - (is_a ? 0 : n_a);
    sum_slot(is_a ? kAreaA : kAreaB, r / T, Db, tiles_b, &tile, &slot);
    t0 = static_cast<int>(r % T), t1 = t0 + 1;
    dst = (is_a ? area_a : area_b) + r;
  }
  const int32_t* p = partial + (tile * T + t0) * chunks * kVals + slot;
  int64_t s = 0;
  for (int64_t i = 0; i < static_cast<int64_t>(t1 - t0) * chunks; ++i) s += p[i * kVals];
  *dst = s;
}

// grid (num_blocks): blocks (num_blocks, 2) int32 = (mask, block of 256 columns)
__global__ void __launch_bounds__(256) decode_ragged_kernel(const int32_t* __restrict__ positions, int64_t total,
                                                            const int64_t* __restrict__ offsets, int num_masks,
                                                            const int32_t* __restrict__ sizes,
                                                            const int64_t* __restrict__ out_offsets,
                                                            const int32_t* __restrict__ blocks,
                                                            int32_t* __restrict__ out, int64_t out_words) {
  const int m = blocks[2 * static_cast<int64_t>(blockIdx.x)];
  const int xb = blocks[2 * static_cast<int64_t>(blockIdx.x) + 1];
  if (m < 0 || m >= num_masks || xb < 0) return;   // uniform over the workgroup, like every return below
  const int H = sizes[2 * m], W = sizes[2 * m + 1];
  if (H <= 0 || W <= 0 || static_cast<int64_t>(H) * W > kIntMax) return;
  if (static_cast<int64_t>(xb) * 256 >= W) return;
  const int words = (W + 31) / 32;
  const int64_t o0 = out_offsets[m];
  if (o0 < 0 || o0 + static_cast<int64_t>(H) * words > out_words) return;
  decode_column(positions, total, offsets, m, xb * 256 + threadIdx.x, H, W, words, out + o0);
}

struct RaggedGroup {
  int64_t H, W, na, nb, a0, b0, inter0, tile0;
  int words, frame_words, tiles_b, chunks;
  bool ok;
};

__device__ __forceinline__ RaggedGroup load_group(const int64_t* __restrict__ groups, int64_t g, int64_t total_a,
                                                  int64_t total_b) {
  const int64_t* d = groups + g * kGroupFields;
  RaggedGroup r;
  r.H = d[0], r.W = d[1], r.na = d[2], r.nb = d[3], r.a0 = d[4], r.b0 = d[5], r.inter0 = d[6], r.tile0 = d[7];
  r.ok = r.H > 0 && r.W > 0 && r.H <= kIntMax && r.W <= kIntMax && r.na >= 0 && r.nb >= 0 && r.na <= kIntMax &&
         r.nb <= kIntMax && r.a0 >= 0 && r.b0 >= 0 && r.a0 <= total_a - r.na && r.b0 <= total_b - r.nb &&
         r.inter0 >= 0 && r.tile0 >= 0;
  r.words = r.ok ? static_cast<int>((r.W + 31) / 32) : 1;
  r.ok = r.ok && r.H * r.words <= kIntMax;
  r.frame_words = r.ok ? static_cast<int>(r.H * r.words) : 0;
  r.tiles_b = r.ok ? static_cast<int>(max((r.nb + kTB - 1) / kTB, static_cast<int64_t>(1))) : 1;
  r.chunks = (r.frame_words + kChunk - 1) / kChunk;
  return r;
}

// grid (num_tiles): tiles (num_tiles, 4) int32 = (group, a-tile, b-tile, chunk); partial row = the table row
__global__ void __launch_bounds__(kThreads) pair_ragged_kernel(const uint32_t* __restrict__ w, int64_t total_words,
                                                               int base_wide, const int64_t* __restrict__ groups,
                                                               int num_groups, const int64_t* __restrict__ a_off,
                                                               int64_t total_a, const int64_t* __restrict__ b_off,
                                                               int64_t total_b, const int32_t* __restrict__ tiles,
                                                               int32_t* __restrict__ partial) {
  const int32_t* tile = tiles + 4 * static_cast<int64_t>(blockIdx.x);
  const int g = tile[0], ta = tile[1], tb = tile[2], chunk = tile[3];
  int acc[kTA][kTB], na[kTA], nb[kTB];
#pragma unroll
  for (int i = 0; i < kTA; ++i) {
    na[i] = 0;
#pragma unroll
    for (int j = 0; j < kTB; ++j) acc[i][j] = 0;
  }
#pragma unroll
  for (int j = 0; j < kTB; ++j) nb[j] = 0;
  if (g >= 0 && g < num_groups && ta >= 0 && tb >= 0 && chunk >= 0) {   // uniform; a bad row stores zeros
    const RaggedGroup r = load_group(groups, g, total_a, total_b);
    if (r.ok) {
      const int64_t wide_words = (static_cast<int64_t>(r.frame_words) + 3) & ~static_cast<int64_t>(3);
      const int64_t ia0 = static_cast<int64_t>(ta) * kTA, ib0 = static_cast<int64_t>(tb) * kTB;
      const uint32_t *pa[kTA], *pb[kTB];
      bool wide = base_wide != 0;
      auto plane = [&](const int64_t* __restrict__ table, int64_t index, int64_t count) -> const uint32_t* {
        if (index >= count) return nullptr;
        const int64_t off = table[index];
        if (off < 0 || off > total_words - r.frame_words) return nullptr;
        wide = wide && (off & 3) == 0 && off <= total_words - wide_words;
        return w + off;
      };
#pragma unroll
      for (int i = 0; i < kTA; ++i) pa[i] = plane(a_off + r.a0, ia0 + i, r.na);
#pragma unroll
      for (int j = 0; j < kTB; ++j) pb[j] = plane(b_off + r.b0, ib0 + j, r.nb);
      const uint32_t tail_mask = r.W % 32 ? (1u << (r.W % 32)) - 1u : 0xffffffffu;
      tile_counts<true>(wide, pa, pb, static_cast<int64_t>(chunk) * kChunk, r.frame_words, r.words, tail_mask, acc, na,
                        nb);
    }
  }

  reduce_store(acc, na, nb, partial + static_cast<int64_t>(blockIdx.x) * kVals);
}

// the last group whose start (field `field`) is <= v; the starts are non-decreasing
__device__ __forceinline__ int64_t find_group(const int64_t* __restrict__ groups, int num_groups, int field,
                                              int64_t v) {
  int64_t lo = 0, hi = num_groups;   // the first group with start > v
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (groups[mid * kGroupFields + field] <= v) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// one thread per output: inter (n_inter), then area_a (total_a), then area_b (total_b)
__global__ void __launch_bounds__(256) sum_ragged_kernel(const int32_t* __restrict__ partial, int64_t num_tiles,
                                                         const int64_t* __restrict__ groups, int num_groups,
                                                         int64_t n_inter, int64_t total_a, int64_t total_b,
                                                         int64_t* __restrict__ inter, int64_t* __restrict__ area_a,
                                                         int64_t* __restrict__ area_b) {
  const int64_t o = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  if (o >= n_inter + total_a + total_b) return;
  const SumPart part = o < n_inter ? kInter : o < n_inter + total_a ? kAreaA : kAreaB;
  const int64_t local = o - (part == kInter ? 0 : part == kAreaA ? n_inter : n_inter + total_a);
  int64_t* dst = (part == kInter ? inter : part == kAreaA ? area_a : area_b) + local;
  int64_t s = 0;
  // the group fields inter_start, a_start, b_start
  const int64_t g = find_group(groups, num_groups, part == kInter ? 6 : part == kAreaA ? 4 : 5, local);
  if (g >= 0) {
    const RaggedGroup r = load_group(groups, g, total_a, total_b);
    const int64_t e = local - (part == kInter ? r.inter0 : part == kAreaA ? r.a0 : r.b0);
    if (r.ok && e < (part == kInter ? r.na * r.nb : part == kAreaA ? r.na : r.nb)) {
      int64_t tile;
      int slot;
      sum_slot(part, e, r.nb, r.tiles_b, &tile, &slot);
      const int64_t row0 = r.tile0 + tile * r.chunks;
      for (int c = 0; c < r.chunks; ++c)
        if (row0 + c < num_tiles) s += partial[(row0 + c) * kVals + slot];
    }
  }
  *dst = s;
}

template <size_t kBytes, class... P>
bool all_aligned(const P*... p) {
  return (m2f::aligned(p, kBytes) && ...);
}

int check_pixels(const char* fn, int height, int width) {
  if (static_cast<int64_t>(height) * width > kIntMax)
    return m2f::fail(M2F_EINVAL, "%s: %d x %d pixels do not fit a 32-bit count", fn, height, width);
  return M2F_OK;
}

struct PairGeom {
  int words, frame_words, chunks, tiles_a, tiles_b;
  int64_t partial_bytes;
};

int pair_geom(const char* fn, int da, int db, int frames, int height, int width, PairGeom* g) {
  if (da <= 0 || db <= 0 || frames <= 0 || height <= 0 || width <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (const int rc = check_pixels(fn, height, width)) return rc;
  g->words = (width + 31) / 32;
  g->frame_words = height * g->words;
  g->chunks = static_cast<int>(m2f::ceil_div(g->frame_words, kChunk));
  g->tiles_a = static_cast<int>(m2f::ceil_div(da, kTA));
  g->tiles_b = static_cast<int>(m2f::ceil_div(db, kTB));
  if (frames > 65535 || static_cast<int64_t>(g->tiles_a) * g->tiles_b > 65535)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: %d frames or %d x %d instances exceed the grid range", fn, frames, da, db);
  g->partial_bytes = static_cast<int64_t>(g->tiles_a) * g->tiles_b * frames * g->chunks * kVals * 4;
  return M2F_OK;
}

}  // namespace

extern "C" int m2f_rle_decode_bits(const int32_t* positions, int64_t total, const int64_t* offsets, int num_masks,
                                   int height, int width, int32_t* out, void* stream) {
  const char* fn = "m2f_rle_decode_bits";
  if (!offsets || !out || (!positions && total > 0)) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_masks <= 0 || height <= 0 || width <= 0 || total < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (const int rc = check_pixels(fn, height, width)) return rc;
  if (!all_aligned<4>(positions, out) || !all_aligned<8>(offsets))
    return m2f::fail(M2F_EINVAL, "%s: positions and out must be 4-byte aligned, offsets 8-byte aligned", fn);
  if (num_masks > 65535) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 65535 masks in one call", fn);
  const dim3 grid(m2f::ceil_div(width, 256), num_masks);
  decode_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(positions, total, offsets, height, width,
                                                                    (width + 31) / 32, out);
  return m2f::check_launch(fn);
}

extern "C" int m2f_bits_pair_tiles(int* ta, int* tb, int* chunk_words) {
  if (!ta || !tb || !chunk_words) return m2f::fail(M2F_EINVAL, "m2f_bits_pair_tiles: null pointer");
  *ta = kTA;
  *tb = kTB;
  *chunk_words = kChunk;
  return m2f::ok();
}

extern "C" int m2f_bits_pair_workspace(int da, int db, int frames, int height, int width, int64_t* bytes) {
  const char* fn = "m2f_bits_pair_workspace";
  if (!bytes) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  PairGeom g;
  if (const int rc = pair_geom(fn, da, db, frames, height, width, &g)) return rc;
  *bytes = g.partial_bytes;
  return m2f::ok();
}

extern "C" int m2f_bits_pair_counts(const int32_t* a, int da, int64_t a_stride, const int32_t* b, int db,
                                    int64_t b_stride, int frames, int height, int width, int64_t* inter,
                                    int64_t* area_a, int64_t* area_b, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  const char* fn = "m2f_bits_pair_counts";
  if (!a || !b || !inter || !area_a || !area_b || !workspace) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  PairGeom g;
  if (const int rc = pair_geom(fn, da, db, frames, height, width, &g)) return rc;
  const int64_t instance = static_cast<int64_t>(frames) * g.frame_words;
  if ((da > 1 && a_stride < instance) || (db > 1 && b_stride < instance) || a_stride < 0 || b_stride < 0)
    return m2f::fail(M2F_EINVAL, "%s: instance stride is smaller than the instance (%lld words)", fn,
                     static_cast<long long>(instance));
  if (!all_aligned<4>(a, b, workspace) || !all_aligned<8>(inter, area_a, area_b))
    return m2f::fail(M2F_EINVAL, "%s: planes and workspace must be 4-byte aligned, outputs 8-byte aligned", fn);
  if (workspace_bytes < g.partial_bytes)
    return m2f::fail(M2F_EINVAL, "%s: workspace of %lld bytes, %lld needed", fn,
                     static_cast<long long>(workspace_bytes), static_cast<long long>(g.partial_bytes));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t tail_mask = width % 32 ? (1u << (width % 32)) - 1u : 0xffffffffu;
  const dim3 grid(g.chunks, frames, g.tiles_a * g.tiles_b);
  const uint32_t* ua = reinterpret_cast<const uint32_t*>(a);
  const uint32_t* ub = reinterpret_cast<const uint32_t*>(b);
  int32_t* partial = static_cast<int32_t*>(workspace);
  // 128-bit loads need every instance and frame to start on 16 bytes
  const bool wide = all_aligned<16>(a, b) && a_stride % 4 == 0 && b_stride % 4 == 0 && g.frame_words % 4 == 0;
  (wide ? pair_kernel<true> : pair_kernel<false>)<<<grid, kThreads, 0, st>>>(
      ua, da, a_stride, ub, db, b_stride, g.frame_words, g.words, tail_mask, g.tiles_b, partial);
  if (const int rc = m2f::check_launch(fn)) return rc;
  const int64_t outputs = static_cast<int64_t>(da) * db + static_cast<int64_t>(da + db) * frames;
  sum_kernel<<<m2f::ceil_div(outputs, 256), 256, 0, st>>>(partial, da, db, frames, g.chunks, g.tiles_b, inter,
                                                          area_a, area_b);
  return m2f::check_launch(fn);
}

extern "C" int m2f_rle_decode_bits_ragged(const int32_t* positions, int64_t total, const int64_t* offsets,
                                          int num_masks, const int32_t* sizes, const int64_t* out_offsets,
                                          const int32_t* blocks, int64_t num_blocks, int32_t* out, int64_t out_words,
                                          void* stream) {
  const char* fn = "m2f_rle_decode_bits_ragged";
  if (!offsets || !sizes || !out_offsets || !out || (!positions && total > 0) || (!blocks && num_blocks > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_masks <= 0 || total < 0 || num_blocks < 0 || out_words < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (!all_aligned<4>(positions, out, sizes, blocks) || !all_aligned<8>(offsets, out_offsets))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 column blocks", fn);
  if (num_blocks == 0) return m2f::ok();
  decode_ragged_kernel<<<static_cast<unsigned>(num_blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
      positions, total, offsets, num_masks, sizes, out_offsets, blocks, out, out_words);
  return m2f::check_launch(fn);
}

extern "C" int m2f_bits_pair_ragged_workspace(int64_t num_tiles, int64_t* bytes) {
  const char* fn = "m2f_bits_pair_ragged_workspace";
  if (!bytes) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_tiles < 0) return m2f::fail(M2F_EINVAL, "%s: a negative number of tiles", fn);
  if (num_tiles > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 tiles", fn);
  *bytes = num_tiles * kVals * 4;
  return m2f::ok();
}

extern "C" int m2f_bits_pair_counts_ragged(const int32_t* words, int64_t total_words, const int64_t* groups,
                                           int num_groups, const int64_t* a_offsets, int64_t total_a,
                                           const int64_t* b_offsets, int64_t total_b, const int32_t* tiles,
                                           int64_t num_tiles, int64_t num_inter, int64_t* inter, int64_t* area_a,
                                           int64_t* area_b, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "m2f_bits_pair_counts_ragged";
  if (!groups || (!words && total_words > 0) || (!a_offsets && total_a > 0) || (!b_offsets && total_b > 0) ||
      (!tiles && num_tiles > 0) || (!workspace && num_tiles > 0) || (!inter && num_inter > 0) ||
      (!area_a && total_a > 0) || (!area_b && total_b > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_groups <= 0 || total_words < 0 || total_a < 0 || total_b < 0 || num_tiles < 0 || num_inter < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (!all_aligned<4>(words, tiles, workspace) || !all_aligned<8>(groups, a_offsets, b_offsets, inter, area_a, area_b))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (num_tiles > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 tiles", fn);
  if (total_words > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: a buffer of more than 2^31 - 1 words", fn);
  if (workspace_bytes < num_tiles * kVals * 4)
    return m2f::fail(M2F_EINVAL, "%s: workspace of %lld bytes, %lld needed", fn,
                     static_cast<long long>(workspace_bytes), static_cast<long long>(num_tiles * kVals * 4));
  const int64_t outputs = num_inter + total_a + total_b;
  if (m2f::ceil_div(outputs, 256) > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: too many outputs", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* partial = static_cast<int32_t*>(workspace);
  if (num_tiles > 0) {
    pair_ragged_kernel<<<static_cast<unsigned>(num_tiles), kThreads, 0, st>>>(
        reinterpret_cast<const uint32_t*>(words), total_words, m2f::aligned(words, 16) ? 1 : 0, groups, num_groups,
        a_offsets, total_a, b_offsets, total_b, tiles, partial);
    if (const int rc = m2f::check_launch(fn)) return rc;
  }
  if (outputs == 0) return m2f::ok();
  sum_ragged_kernel<<<static_cast<unsigned>(m2f::ceil_div(outputs, 256)), 256, 0, st>>>(
      partial, num_tiles, groups, num_groups, num_inter, total_a, total_b, inter, area_a, area_b);
  return m2f::check_launch(fn);
}

// Mask IoU of instance sequences on one-bit-per-pixel planes (the format is restated in include/bm2f.h).
//
//   decode_kernel   the reverse of rle.hip: run ends (cumulative counts in the column-major order p = x * H + y)
//                   -> bit planes (M, H, words).  A lane owns one column of one mask and the lanes of a wave own 64
//                   consecutive columns.  The pixel p is set when an odd number of run ends is <= p, so the lane
//                   finds the number of ends <= x * H by a binary search and walks its H rows with a cursor; a wave
//                   ballot per row is the two words of those 64 columns, stored by lanes 0 and 32.  Lanes beyond W
//                   vote 0, which zeroes the tail bits.  Every word of the output is stored exactly once.
//
//   pair_kernel     inter[d][g] = sum popcount(a_d & b_g), area_a[d][t], area_b[g][t].  A workgroup takes kChunk
//                   word positions of one frame and a kTA x kTB tile of instances; a thread loads 4 consecutive words
//                   (one 128-bit load) of each of the kTA + kTB instances and keeps the kTA * kTB + kTA + kTB counts
//                   in registers.  A is read ceil(Db / kTB) times and B ceil(Da / kTA) times per launch.  The tail
//                   bits of a row's last word are masked here.  The counts are reduced over the wave by shuffles,
//                   over the four waves through LDS, and stored as one int32 partial per (tile, frame, chunk).
//   sum_kernel      one thread per output sums its partials in index order into int64.
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

// grid (ceil(W / 256), M)
__global__ void __launch_bounds__(256) decode_kernel(const int32_t* __restrict__ positions, int64_t total,
                                                     const int64_t* __restrict__ offsets, int H, int W, int words,
                                                     int32_t* __restrict__ out) {
  const int m = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  const bool live = x < W;
  const int64_t begin = min(max(offsets[m], static_cast<int64_t>(0)), total);
  const int64_t end = min(max(offsets[m + 1], begin), total);
  const int32_t* t = positions + begin;
  const int64_t n = live ? end - begin : 0;
  const int p0 = live ? x * H : 0;   // < 2^31: checked by the entry point
  // the number of run ends <= p0
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (t[mid] <= p0) lo = mid + 1; else hi = mid;
  }
  int64_t cur = lo;
  int next = cur < n ? t[cur] : 0x7fffffff;
  int32_t* o = out + static_cast<int64_t>(m) * H * words + (x >> 5);
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

template <bool kWide>
__device__ __forceinline__ void load4(const uint32_t* __restrict__ p, int i0, int n, uint32_t (&v)[kVec]) {
  if (kWide) {   // i0 and n are multiples of 4 and p + i0 is 16-byte aligned
    if (i0 < n) {
      const uint4 q = *reinterpret_cast<const uint4*>(p + i0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kVec; ++k) v[k] = i0 + k < n ? p[i0 + k] : 0u;
  }
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
  int acc[kTA][kTB], na[kTA], nb[kTB];
#pragma unroll
  for (int i = 0; i < kTA; ++i) {
    na[i] = 0;
#pragma unroll
    for (int j = 0; j < kTB; ++j) acc[i][j] = 0;
  }
#pragma unroll
  for (int j = 0; j < kTB; ++j) nb[j] = 0;

  for (int it = 0; it < kIters; ++it) {
    const int i0 = chunk * kChunk + (it * kThreads + threadIdx.x) * kVec;   // word position inside the frame
    if (i0 < frame_words) {
      uint32_t keep[kVec];
      int col = i0 % words;
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
        keep[k] = col == words - 1 ? tail_mask : 0xffffffffu;
        col = col + 1 == words ? 0 : col + 1;
      }
      uint32_t va[kTA][kVec], vb[kTB][kVec];
#pragma unroll
      for (int i = 0; i < kTA; ++i) {
        if (ia0 + i < Da) {   // uniform over the workgroup
          load4<kWide>(a + (ia0 + i) * stride_a + frame, i0, frame_words, va[i]);
        } else {
#pragma unroll
          for (int k = 0; k < kVec; ++k) va[i][k] = 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < kTB; ++j) {
        if (ib0 + j < Db) {
          load4<kWide>(b + (ib0 + j) * stride_b + frame, i0, frame_words, vb[j]);
        } else {
#pragma unroll
          for (int k = 0; k < kVec; ++k) vb[j][k] = 0u;
        }
      }
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
    const int64_t block = (static_cast<int64_t>(blockIdx.z) * gridDim.y + t) * gridDim.x + chunk;
    partial[block * kVals + threadIdx.x] = s;
  }
}

// one thread per output: inter (Da, Db), then area_a (Da, T), then area_b (Db, T)
__global__ void __launch_bounds__(256) sum_kernel(const int32_t* __restrict__ partial, int Da, int Db, int T,
                                                  int chunks, int tiles_b, int64_t* __restrict__ inter,
                                                  int64_t* __restrict__ area_a, int64_t* __restrict__ area_b) {
  const int64_t g = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
  const int64_t n_inter = static_cast<int64_t>(Da) * Db, n_a = static_cast<int64_t>(Da) * T;
  if (g >= n_inter + n_a + static_cast<int64_t>(Db) * T) return;
  int tile, slot, t0, t1;
  int64_t* dst;
  if (g < n_inter) {
    const int d = static_cast<int>(g / Db), j = static_cast<int>(g % Db);
    tile = (d / kTA) * tiles_b + j / kTB;
    slot = (d % kTA) * kTB + j % kTB;
    t0 = 0, t1 = T;
    dst = inter + g;
  } else if (g < n_inter + n_a) {
    const int64_t r = g - n_inter;
    const int d = static_cast<int>(r / T);
    tile = (d / kTA) * tiles_b;            // the first tile of B
    slot = kTA * kTB + d % kTA;
    t0 = static_cast<int>(r % T), t1 = t0 + 1;
    dst = area_a + r;
  } else {
    const int64_t r = g - n_inter - n_a;
    const int j = static_cast<int>(r / T);
    tile = j / kTB;                        // the first tile of A
    slot = kTA * kTB + kTA + j % kTB;
    t0 = static_cast<int>(r % T), t1 = t0 + 1;
    dst = area_b + r;
  }
  const int32_t* p = partial + (static_cast<int64_t>(tile) * T + t0) * chunks * kVals + slot;
  int64_t s = 0;
  for (int64_t i = 0; i < static_cast<int64_t>(t1 - t0) * chunks; ++i) s += p[i * kVals];
  *dst = s;
}

struct PairGeom {
  int words, frame_words, chunks, tiles_a, tiles_b;
  int64_t partial_bytes;
};

int pair_geom(const char* fn, int da, int db, int frames, int height, int width, PairGeom* g) {
  if (da <= 0 || db <= 0 || frames <= 0 || height <= 0 || width <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (static_cast<int64_t>(height) * width > 0x7fffffff)
    return m2f::fail(M2F_EINVAL, "%s: %d x %d pixels do not fit a 32-bit count", fn, height, width);
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
  if (static_cast<int64_t>(height) * width > 0x7fffffff)
    return m2f::fail(M2F_EINVAL, "%s: %d x %d pixels do not fit a 32-bit count", fn, height, width);
  if (!m2f::aligned(positions, 4) || !m2f::aligned(out, 4) || !m2f::aligned(offsets, 8))
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
  if (!m2f::aligned(a, 4) || !m2f::aligned(b, 4) || !m2f::aligned(workspace, 4) || !m2f::aligned(inter, 8) ||
      !m2f::aligned(area_a, 8) || !m2f::aligned(area_b, 8))
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
  const bool wide = m2f::aligned(a, 16) && m2f::aligned(b, 16) && a_stride % 4 == 0 && b_stride % 4 == 0 &&
                    g.frame_words % 4 == 0;
  if (wide)
    pair_kernel<true><<<grid, kThreads, 0, st>>>(ua, da, a_stride, ub, db, b_stride, g.frame_words, g.words,
                                                 tail_mask, g.tiles_b, partial);
  else
    pair_kernel<false><<<grid, kThreads, 0, st>>>(ua, da, a_stride, ub, db, b_stride, g.frame_words, g.words,
                                                  tail_mask, g.tiles_b, partial);
  if (const int rc = m2f::check_launch(fn)) return rc;
  const int64_t outputs = static_cast<int64_t>(da) * db + static_cast<int64_t>(da + db) * frames;
  sum_kernel<<<m2f::ceil_div(outputs, 256), 256, 0, st>>>(partial, da, db, frames, g.chunks, g.tiles_b, inter,
                                                          area_a, area_b);
  return m2f::check_launch(fn);
}

// Mask planes -> boundary planes for COCO Boundary AP (the definition is restated in include/bm2f.h):
//   boundary = mask & ~erode(mask, d),  erode: pixel (y, x) survives when every pixel of the (2d + 1) x (2d + 1) window
//   centred on it lies inside the image and is set.
// The planes are the ragged one-bit-per-pixel planes of mask_iou.hip: (H, words) int32, bit x % 32 of word x / 32.
//
// The square window is separable, and on bit planes both halves are ANDs of shifted copies.  With n = 2d + 1 and
// G_k(i) = AND of k consecutive elements starting at i:  G_2k(i) = G_k(i) & G_k(i + k), and for the largest power of
// two p <= n:  G_n(i) = G_p(i) & G_p(i + n - p); the eroded element is G_n(i - d).  That is floor(log2 n) + 1 ANDs per
// word and direction whatever d is.
//
//   boundary_ragged_kernel   one workgroup per table row = (plane, tile): a band of kBand rows and kTileW words of
//       one plane.  With hw = ceil(d / 32) the workgroup
//         1. loads the (kBand + 2d) x (kTileW + 2 hw) words around its tile into LDS, once; rows and words outside the
//            image are zero and the bits x >= W of a row's last word are cleared, so "outside counts as zero" needs
//            no further case; the tile's own words are also kept aside for step 4;
//         2. erodes vertically: AND of LDS rows r and r + k between two LDS buffers, one barrier per doubling;
//         3. erodes horizontally: a thread takes the 2 hw + 1 words around one output word into registers and runs
//            the same doubling on that bit string, every shift a compile-time power of two (v_alignbit across word
//            edges, whole-word moves from 32 on); one last funnel shift by 32 hw - d aligns G_n(x - d) with x;
//         4. stores mask & ~eroded, each output word once.
//       Input tail bits and the words between planes are never used: a word is loaded only when it lies inside its
//       plane and is masked on load.  Output tail bits are zero because the masked input is the left operand.
//
// No atomics, no memset, no second pass through global memory.  The table lives in device memory, so the kernel checks
// every value it takes from it against the sizes passed by value: a malformed table gives unspecified planes, never an
// access outside the two buffers.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kBand = M2F_BOUNDARY_BAND_ROWS, kTileW = M2F_BOUNDARY_TILE_WORDS, kDMax = M2F_BOUNDARY_D_MAX;
constexpr int kHaloMax = (kDMax + 31) / 32;   // words of halo on either side at d = kDMax
static_assert(kDMax == 128 && kHaloMax == 4, "the shift ladders below stop at 128 and the dispatch at 4 halo words");
constexpr int64_t kIntMax = 0x7fffffff;

__host__ __device__ constexpr int halo_words(int d) { return (d + 31) / 32; }
// bytes of LDS for dilations up to d: two (kBand + 2d) x (kTileW + 2 hw) buffers and the tile's own words
__host__ __device__ constexpr int lds_bytes(int d) {
  return (2 * (kBand + 2 * d) * (kTileW + 2 * halo_words(d)) + kBand * kTileW) * 4;
}

// b >>= K as one little-endian bit string of NW words (bit i of the result = bit i + K of b), zeros shifted in
template <int NW, int K>
__device__ __forceinline__ void shift_down(uint32_t (&b)[NW]) {
  constexpr int q = K / 32, r = K % 32;
#pragma unroll
  for (int i = 0; i < NW; ++i) {   // ascending: b[i] is built from words that are still the old ones
    const uint32_t lo = i + q < NW ? b[i + q] : 0u;
    const uint32_t hi = i + q + 1 < NW ? b[i + q + 1] : 0u;
    b[i] = r == 0 ? lo : (lo >> r) | (hi << ((32 - r) & 31));
  }
}

// b &= b >> K
template <int NW, int K>
__device__ __forceinline__ void and_shifted(uint32_t (&b)[NW]) {
  uint32_t c[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) c[i] = b[i];
  shift_down<NW, K>(c);
#pragma unroll
  for (int i = 0; i < NW; ++i) b[i] &= c[i];
}

template <int NW, int K>
__device__ __forceinline__ void double_ladder(uint32_t (&b)[NW], int n) {
  if constexpr (K <= kDMax && K < 32 * NW) {
    if (2 * K <= n) and_shifted<NW, K>(b);   // the window grows from K to 2K bits
    double_ladder<NW, 2 * K>(b, n);
  }
}

template <int NW, int K>
__device__ __forceinline__ void shift_ladder(uint32_t (&c)[NW], int s) {
  if constexpr (K <= kDMax && K < 32 * NW) {
    if (s & K) shift_down<NW, K>(c);
    shift_ladder<NW, 2 * K>(c, s);
  }
}

// The horizontal erosion of one output word: row[0 .. 2 HW] are the vertically eroded words hw before to hw after
// it, n = 2d + 1, p the largest power of two <= n.  -> the word of G_n(x - d) for its 32 columns x.
template <int HW>
__device__ __forceinline__ uint32_t erode_word(const uint32_t* __restrict__ row, int d, int n, int p) {
  constexpr int NW = 2 * HW + 1;
  uint32_t b[NW], c[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) b[i] = row[i];
  double_ladder<NW, 1>(b, n);      // b = G_p
#pragma unroll
  for (int i = 0; i < NW; ++i) c[i] = b[i];
  shift_ladder<NW, 1>(c, n - p);   // 0 < n - p < p: n is odd
#pragma unroll
  for (int i = 0; i < NW; ++i) b[i] &= c[i];   // b = G_n, bit s of the string = G_n(32 (word - HW) + s)
  const int o = 32 * HW - d;       // 0 <= o < 32 for HW = ceil(d / 32)
  const uint64_t both = (static_cast<uint64_t>(b[1]) << 32) | b[0];
  return static_cast<uint32_t>(both >> o);
}

// grid (num_blocks): blocks (num_blocks, 2) int32 = (plane, tile), tile = band * ceil(words / kTileW) + column tile
__global__ void __launch_bounds__(kThreads) boundary_ragged_kernel(const uint32_t* __restrict__ in,
                                                                   int64_t total_words, int num_planes,
                                                                   const int32_t* __restrict__ sizes,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ dilations,
                                                                   const int32_t* __restrict__ blocks, int max_dilation,
                                                                   uint32_t* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int m = blocks[2 * static_cast<int64_t>(blockIdx.x)];
  const int tile = blocks[2 * static_cast<int64_t>(blockIdx.x) + 1];
  if (m < 0 || m >= num_planes || tile < 0) return;   // uniform over the workgroup, like every return below
  const int H = sizes[2 * m], W = sizes[2 * m + 1], d = dilations[m];
  if (H <= 0 || W <= 0 || d < 1 || d > max_dilation || d > kDMax) return;
  const int words = (W + 31) / 32;
  if (static_cast<int64_t>(H) * words > kIntMax) return;
  const int64_t base = offsets[m];
  if (base < 0 || base > total_words - static_cast<int64_t>(H) * words) return;
  const int col_tiles = (words + kTileW - 1) / kTileW;
  const int y0 = (tile / col_tiles) * kBand, w0 = (tile % col_tiles) * kTileW;
  if (y0 >= H) return;

  const int hw = halo_words(d), n = 2 * d + 1;
  const int R = kBand + 2 * d, S = kTileW + 2 * hw;   // the staged rows y0 - d .., words w0 - hw ..
  uint32_t* buf0 = lds;
  uint32_t* buf1 = lds + R * S;
  uint32_t* centre = lds + 2 * R * S;                 // the tile's own words, (kBand, kTileW)
  const uint32_t tail_mask = W % 32 ? (1u << (W % 32)) - 1u : 0xffffffffu;
  const uint32_t* plane = in + base;

  // 1. stage
  for (int i = threadIdx.x; i < R * S; i += kThreads) {
    const int r = i / S, s = i - r * S;
    const int y = y0 - d + r, w = w0 - hw + s;
    uint32_t v = 0u;
    if (y >= 0 && y < H && w >= 0 && w < words) {
      v = plane[static_cast<int64_t>(y) * words + w];
      if (w == words - 1) v &= tail_mask;
    }
    buf0[i] = v;
    if (r >= d && r < d + kBand && s >= hw && s < hw + kTileW) centre[(r - d) * kTileW + (s - hw)] = v;
  }
  __syncthreads();

  // 2. vertical: after the loop src holds G_p over rows, then G_n for the band's rows r < kBand
  uint32_t *src = buf0, *dst = buf1;
  int p = 1;
  for (; 2 * p <= n; p *= 2) {
    const int live = (R - p) * S;   // rows whose partner r + p is staged; the others are never needed again
    for (int i = threadIdx.x; i < live; i += kThreads) dst[i] = src[i] & src[i + p * S];
    __syncthreads();
    uint32_t* t = src;
    src = dst;
    dst = t;
  }
  const int rem = n - p;            // the band's rows reach r + rem + p - 1 <= kBand + 2d - 1: inside the stage
  for (int i = threadIdx.x; i < kBand * S; i += kThreads) dst[i] = src[i] & src[i + rem * S];
  __syncthreads();

  // 3. horizontal and 4. store
  for (int i = threadIdx.x; i < kBand * kTileW; i += kThreads) {
    const int r = i / kTileW, s = i - r * kTileW;
    const int y = y0 + r, w = w0 + s;
    if (y >= H || w >= words) continue;
    const uint32_t* row = dst + r * S + s;   // staged words s .. s + 2 hw = plane words w - hw .. w + hw
    uint32_t e;
    switch (hw) {
      case 1: e = erode_word<1>(row, d, n, p); break;
      case 2: e = erode_word<2>(row, d, n, p); break;
      case 3: e = erode_word<3>(row, d, n, p); break;
      default: e = erode_word<4>(row, d, n, p); break;
    }
    out[base + static_cast<int64_t>(y) * words + w] = centre[i] & ~e;
  }
}

}  // namespace

extern "C" int m2f_bits_boundary_tiles(int* band_rows, int* tile_words, int* d_max) {
  if (!band_rows || !tile_words || !d_max) return m2f::fail(M2F_EINVAL, "m2f_bits_boundary_tiles: null pointer");
  *band_rows = kBand;
  *tile_words = kTileW;
  *d_max = kDMax;
  return m2f::ok();
}

extern "C" int m2f_bits_boundary_ragged(const int32_t* words, int64_t total_words, int num_planes,
                                        const int32_t* sizes, const int64_t* offsets, const int32_t* dilations,
                                        const int32_t* blocks, int64_t num_blocks, int max_dilation, int32_t* out,
                                        void* stream) {
  const char* fn = "m2f_bits_boundary_ragged";
  if (!words || !out || !sizes || !offsets || !dilations || (!blocks && num_blocks > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_planes <= 0 || total_words <= 0 || num_blocks < 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (max_dilation < 1 || max_dilation > kDMax)
    return m2f::fail(M2F_EINVAL, "%s: max_dilation %d is outside [1, %d]", fn, max_dilation, kDMax);
  if (!m2f::aligned(words, 4) || !m2f::aligned(out, 4) || !m2f::aligned(sizes, 4) || !m2f::aligned(dilations, 4) ||
      !m2f::aligned(blocks, 4) || !m2f::aligned(offsets, 8))
    return m2f::fail(M2F_EINVAL, "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned", fn);
  if (total_words > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: a buffer of more than 2^31 - 1 words", fn);
  const int32_t* lo = words < out ? words : out;
  const int32_t* hi = words < out ? out : words;
  if (hi - lo < total_words) return m2f::fail(M2F_EINVAL, "%s: words and out overlap", fn);
  unsigned grid;
  if (const int rc = m2f::grid_1d(num_blocks, fn, &grid)) return rc;
  if (grid == 0) return m2f::ok();
  if (const int rc = m2f::set_max_lds(reinterpret_cast<const void*>(&boundary_ragged_kernel), lds_bytes(kDMax), fn))
    return rc;
  boundary_ragged_kernel<<<grid, kThreads, lds_bytes(max_dilation), static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const uint32_t*>(words), total_words, num_planes, sizes, offsets, dilations, blocks,
      max_dilation, reinterpret_cast<uint32_t*>(out));
  return m2f::check_launch(fn);
}

// Label-pair counts of a ragged batch of images: for image i with P_i pixels and two label planes a (ground truth)
// and b (prediction), table_i[row(a[p])][b[p]] += 1 over its pixels (the contract is restated in include/bm2f.h).
// Semantic mIoU (one confusion matrix shared by the batch) and panoptic PQ (one table of ground-truth segment x
// predicted segment per image) are both read off these tables on the host (bm2f_amd/sem_seg_eval.py, panoptic_eval.py).
//
//   count_kernel<TA, TB, kLds>   one workgroup of kThreads = 1024 per table row (image, chunk): kIters * kThreads
//       vectors of kVec = 8 consecutive pixels of one image.  A lane owns one vector per iteration, so a wave reads
//       512 consecutive pixels of either plane per load.
//
//   Loads.  The vectors are laid on the grid of a's *element index* (a_off rounded down to a multiple of 8), so after
//       the first vector of an image every load of a is aligned: one 8-byte (uint8), one 16-byte (int16) or two
//       16-byte (int32) loads per lane.  b is read the same way when b_off - a_off is a multiple of 8 (the Python
//       layer pads host planes so that it is) and with one scalar load per pixel otherwise.  A 16-byte piece is
//       loaded only when it holds at least one pixel of the image, so no load touches an aligned 16-byte block
//       that holds no byte of the plane; the elements of the head and tail vectors that belong to a neighbour are
//       masked.  An unaligned base pointer sends the plane down the scalar loads; the Python layer therefore passes
//       the lowest plane address rounded down to 16 bytes as the base and counts the offsets from there.
//
//   Keys.  Direct mode: ignore -> row rows - 1, v in [0, rows - 1) -> row v, anything else is `bad`.  Id-list mode:
//       the image's sorted ids (<= kMaxIds = 1024 int32, 4 KiB) are staged in LDS and bisected; a lane repeats the
//       search only when its value differs from the previous pixel's.  b in [0, cols) is the column, anything else
//       `bad`.  key = row * cols + col < 2^31.
//
//   Adds (wave_add).  Label maps are piecewise constant, and 64 lanes adding to one address serialise in LDS and at
//       the memory side alike.  So equal keys are merged across the wave first: take the first pending lane's key,
//       ballot the lanes that hold it, and let that lane add the popcount; kRounds = 4 such rounds, then every lane
//       still pending adds its own 1 (a wave of 64 different keys pays 4 wasted rounds, not 64 serial ones).
//       kLds:  32-bit LDS atomics into the workgroup's private copy of the image's table (dynamic LDS, zeroed on
//              entry); at the end the non-zero bins are flushed with one 64-bit global atomic each.  A chunk holds
//              65,536 pixels, so a bin cannot overflow.
//       !kLds: the merged counts go straight to the output with 64-bit global atomics.
//
//   All counters are integers and integer addition commutes: the tables are the same on every run whatever the
//   scheduling.  The output is 64-bit, so no batch overflows it.
//
// LDS budget and occupancy.  kLdsBins = 24,576 bins = 96 KiB of the CU's 160 KiB, chosen so that the semantic table
// of ADE20K, 151 x 151 = 22,801 bins (89 KiB), stays private; with the 4 KiB id list that is 100 KiB, one workgroup
// per CU.  That is why the workgroup is 1024 threads: one resident workgroup is still 16 waves per CU, 4 per SIMD, to
// cover the latency of the streaming loads (launch_bounds(1024) caps a lane at 128 VGPRs; the kernel needs far
// fewer).  The dynamic size is the launch's largest table, so a panoptic batch (a few thousand bins) gets two
// workgroups per CU, the 32-wave cap.  Zeroing and flushing 22,801 bins is 23 LDS accesses per lane against the 64
// pixels a lane counts per chunk; tables beyond the budget, and launches forced to, take the global path.
// A chunk of 65,536 pixels keeps that overhead small but makes short grids: 16 images of 512 x 683 are 96 workgroups
// and 16 of 800 x 1216 are 240, on 256 CUs, so such batches leave CUs idle (DESIGN.md §3 has the measured times); a
// smaller chunk for small tables was not tried.
// The compiler reports 33 to 42 VGPRs, no VGPR spill and no scratch for every instantiation; the LDS ones spill 2 to
// 4 SGPRs, which go to lanes of a VGPR and cost no memory traffic.
//
// Label histograms (m2f_label_histogram_ragged: which classes an image holds and their areas, for the training
// targets of bm2f_amd/label_targets.py) are the same kernel without the second plane (kPair = false): the table of an
// image is rows x 1, the column is always 0 and b is neither checked nor read.  Loads, keys of a, wave-merged adds,
// the LDS copy and the 64-bit counters are shared.
//
// The tables live in device memory where the entry point cannot read them, so the kernel checks every field against
// the sizes passed by value: a malformed table counts nothing or unspecified values, never outside the buffers.
#include "bm2f.h"
#include "common.h"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

constexpr int kThreads = 1024, kVec = M2F_LABEL_VEC, kIters = 8;
constexpr int kChunkVecs = kThreads * kIters;
static_assert(kChunkVecs == M2F_LABEL_CHUNK_VECS, "header constant");
constexpr int kLdsBins = M2F_LABEL_LDS_BINS;
constexpr int kMaxIds = M2F_LABEL_MAX_IDS;
constexpr int kRounds = 4;
constexpr int kFields = M2F_LABEL_IMAGE_FIELDS;   // a_off, b_off, pixels, rows, cols, out_off, id_off, id_count
constexpr int64_t kIntMax = 0x7fffffff;
constexpr int64_t kNoIgnore = INT64_MIN;
using u64 = unsigned long long;

// a label as an int: values an int cannot hold are no valid row or column, they become -1 (always `bad`)
template <class T>
__device__ __forceinline__ int as_label(T v) {
  if constexpr (sizeof(T) == 8) return v < 0 || v > kIntMax ? -1 : static_cast<int>(v);
  else return static_cast<int>(v);
}

// Elements [e0, e0 + kVec) of `base` -> v, those outside [lo, hi) as 0.  e0 may be negative or the vector may end
// beyond hi: only elements in [lo, hi) are touched on the scalar path, only aligned pieces that hold one on the wide
// path (e0 is then a multiple of kVec and base 16-byte aligned).
template <class T>
__device__ __forceinline__ void load_vec(const T* __restrict__ base, int64_t e0, int64_t lo, int64_t hi, bool wide,
                                         int (&v)[kVec]) {
  constexpr int kPieceBytes = kVec * sizeof(T) < 16 ? kVec * sizeof(T) : 16;
  constexpr int kPer = kPieceBytes / sizeof(T), kPieces = kVec / kPer;
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int64_t p0 = e0 + q * kPer;
    T tmp[kPer];
    if (wide && p0 + kPer > lo && p0 < hi) {
      if constexpr (kPieceBytes == 16) {
        const uint4 raw = *reinterpret_cast<const uint4*>(base + p0);
        memcpy(tmp, &raw, 16);
      } else {
        const uint2 raw = *reinterpret_cast<const uint2*>(base + p0);
        memcpy(tmp, &raw, 8);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPer; ++k) tmp[k] = !wide && p0 + k >= lo && p0 + k < hi ? base[p0 + k] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[q * kPer + k] = as_label(tmp[k]);
  }
}

// table[key] += 1 for every lane with `pending`, equal keys merged across the wave; called by all lanes of a wave
template <bool kLds>
__device__ __forceinline__ void wave_add(int key, bool pending, uint32_t* __restrict__ lds, u64* __restrict__ out) {
  auto add = [&](int k, int n) {
    if (kLds) atomicAdd(lds + k, static_cast<uint32_t>(n));
    else atomicAdd(out + k, static_cast<u64>(n));
  };
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(pending);
#pragma unroll 1
  for (int r = 0; r < kRounds && todo != 0; ++r) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
    const int k0 = __builtin_amdgcn_readlane(key, leader);
    const bool mine = pending && key == k0;
    const u64 same = __ballot(mine);
    if (lane == leader) add(k0, __popcll(same));
    pending = pending && !mine;
    todo &= ~same;
  }
  if (pending) add(key, 1);
}

struct Image {
  int64_t a_off, b_off, pixels, out_off, id_off;
  int rows, cols, ids, bins;
  bool ok;
};

// pair: the image has a plane of b to be checked
__device__ __forceinline__ Image load_image(const int64_t* __restrict__ images, int64_t i, int64_t a_elems, bool pair,
                                            int64_t b_elems, int64_t total_ids, int64_t out_len) {
  const int64_t* d = images + i * kFields;
  Image r;
  r.a_off = d[0], r.b_off = d[1], r.pixels = d[2], r.out_off = d[5], r.id_off = d[6];
  const int64_t rows = d[3], cols = d[4], ids = d[7];
  r.ok = r.pixels >= 0 && r.a_off >= 0 && r.a_off <= a_elems - r.pixels &&
         (!pair || (r.b_off >= 0 && r.b_off <= b_elems - r.pixels)) && (pair || cols == 1) && rows >= 1 && cols >= 1 && rows <= kIntMax && cols <= kIntMax &&
         rows * cols <= kIntMax && r.out_off >= 0 && r.out_off <= out_len - rows * cols &&
         (ids < 0 || (ids <= kMaxIds && ids <= rows - 1 && r.id_off >= 0 && r.id_off <= total_ids - ids));
  r.rows = r.ok ? static_cast<int>(rows) : 1;
  r.cols = r.ok ? static_cast<int>(cols) : 1;
  r.ids = r.ok ? static_cast<int>(ids < 0 ? -1 : ids) : -1;
  r.bins = r.rows * r.cols;
  return r;
}

// grid (num_blocks): blocks (num_blocks, 2) int32 = (image, chunk of kChunkVecs vectors).  !kPair: a histogram of a
// alone (cols = 1); b is not read.
template <class TA, class TB, bool kLds, bool kPair = true>
__global__ void __launch_bounds__(kThreads) count_kernel(const TA* __restrict__ a, int64_t a_elems, int a_wide,
                                                         const TB* __restrict__ b, int64_t b_elems, int b_wide,
                                                         const int64_t* __restrict__ images, int num_images,
                                                         const int32_t* __restrict__ ids, int64_t total_ids,
                                                         const int32_t* __restrict__ blocks, int64_t ignore,
                                                         int lds_bins, u64* __restrict__ out, int64_t out_len,
                                                         u64* __restrict__ bad) {
  extern __shared__ uint32_t bins[];
  __shared__ int32_t id_list[kMaxIds];
  const int i = blocks[2 * static_cast<int64_t>(blockIdx.x)];
  const int chunk = blocks[2 * static_cast<int64_t>(blockIdx.x) + 1];
  if (i < 0 || i >= num_images || chunk < 0) return;   // uniform over the workgroup, like every return below
  const Image im = load_image(images, i, a_elems, kPair, b_elems, total_ids, out_len);
  if (!im.ok || (kLds && im.bins > lds_bins)) return;
  const int64_t a0 = im.a_off - im.a_off % kVec;                         // the vector grid: a's element index
  const int64_t nvec = (im.a_off + im.pixels - a0 + kVec - 1) / kVec;
  const int64_t vec0 = static_cast<int64_t>(chunk) * kChunkVecs;
  if (vec0 >= nvec) return;
  const bool wide_b = kPair && b_wide != 0 && (im.b_off - im.a_off) % kVec == 0;
  if (kLds)
    for (int k = threadIdx.x; k < im.bins; k += kThreads) bins[k] = 0u;
  for (int k = threadIdx.x; k < im.ids; k += kThreads) id_list[k] = ids[im.id_off + k];
  __syncthreads();

  u64* table = out + im.out_off;
  const int last_row = im.rows - 1;
  int nbad = 0, seen = 0, seen_row = -1;   // the last value searched in the id list and its row
  bool have_seen = false;
#pragma unroll 1
  for (int it = 0; it < kIters; ++it) {
    const int64_t first = vec0 + static_cast<int64_t>(it) * kThreads;
    if (first >= nvec) break;   // uniform
    const int64_t e0 = a0 + (first + threadIdx.x) * kVec;              // a's element index of the vector
    const int64_t p0 = e0 - im.a_off;                                   // its first pixel, in [-7, pixels + 7]
    int va[kVec], vb[kVec];
    load_vec(a, e0, im.a_off, im.a_off + im.pixels, a_wide != 0, va);
    if constexpr (kPair) load_vec(b, im.b_off + p0, im.b_off, im.b_off + im.pixels, wide_b, vb);
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
      const bool live = p0 + k >= 0 && p0 + k < im.pixels;
      int row;
      if (im.ids < 0) {
        row = va[k] == ignore ? last_row : va[k] >= 0 && va[k] < last_row ? va[k] : -1;
      } else if (have_seen && va[k] == seen) {
        row = seen_row;
      } else {
        int lo = 0, hi = im.ids;   // the first id >= va[k]
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (id_list[mid] < va[k]) lo = mid + 1; else hi = mid;
        }
        row = lo < im.ids && id_list[lo] == va[k] ? lo : last_row;
        seen = va[k], seen_row = row, have_seen = true;
      }
      const int col = !kPair ? 0 : vb[k] >= 0 && vb[k] < im.cols ? vb[k] : -1;
      const bool good = live && row >= 0 && col >= 0;
      nbad += live && !good ? 1 : 0;
      wave_add<kLds>(good ? row * im.cols + col : 0, good, bins, table);
    }
  }
  if (nbad > 0) atomicAdd(bad + i, static_cast<u64>(nbad));
  if (kLds) {
    __syncthreads();
    for (int k = threadIdx.x; k < im.bins; k += kThreads) {
      const uint32_t n = bins[k];
      if (n != 0u) atomicAdd(table + k, static_cast<u64>(n));
    }
  }
}

template <class TA, class TB, bool kPair = true>
int launch(const char* fn, bool lds, int lds_bins, unsigned grid, hipStream_t st, const void* a, int64_t a_elems,
           const void* b, int64_t b_elems, const int64_t* images, int num_images, const int32_t* ids,
           int64_t total_ids, const int32_t* blocks, int64_t ignore, int64_t* out, int64_t out_len, int64_t* bad) {
  const int a_wide = m2f::aligned(a, 16) ? 1 : 0, b_wide = m2f::aligned(b, 16) ? 1 : 0;
  auto* kern = lds ? &count_kernel<TA, TB, true, kPair> : &count_kernel<TA, TB, false, kPair>;
  const int bytes = lds ? lds_bins * 4 : 0;
  if (lds)
    if (const int rc = m2f::set_max_lds(reinterpret_cast<const void*>(kern), kLdsBins * 4, fn)) return rc;
  kern<<<grid, kThreads, bytes, st>>>(static_cast<const TA*>(a), a_elems, a_wide, static_cast<const TB*>(b), b_elems,
                                      b_wide, images, num_images, ids, total_ids, blocks, ignore, lds_bins,
                                      reinterpret_cast<u64*>(out), out_len, reinterpret_cast<u64*>(bad));
  return m2f::check_launch(fn);
}

// the label type of BYTES bytes per element
template <int BYTES>
using Label = std::conditional_t<BYTES == 1, uint8_t,
                                 std::conditional_t<BYTES == 2, int16_t, std::conditional_t<BYTES == 4, int32_t, int64_t>>>;

}  // namespace

extern "C" int m2f_label_counts_geometry(int* vec, int* chunk_vecs, int* lds_bins, int* max_ids) {
  if (!vec || !chunk_vecs || !lds_bins || !max_ids)
    return m2f::fail(M2F_EINVAL, "m2f_label_counts_geometry: null pointer");
  *vec = kVec;
  *chunk_vecs = kChunkVecs;
  *lds_bins = kLdsBins;
  *max_ids = kMaxIds;
  return m2f::ok();
}

extern "C" int m2f_label_pair_counts_ragged(const void* a, int a_bytes, int64_t a_elems, const void* b, int b_bytes,
                                            int64_t b_elems, const int64_t* images, int num_images,
                                            const int32_t* ids, int64_t total_ids, const int32_t* blocks,
                                            int64_t num_blocks, int has_ignore, int ignore, int64_t max_bins,
                                            int path, int64_t* out, int64_t out_len, int64_t* bad, void* stream) {
  const char* fn = "m2f_label_pair_counts_ragged";
  if (!images || !out || !bad || (!a && a_elems > 0) || (!b && b_elems > 0) || (!ids && total_ids > 0) ||
      (!blocks && num_blocks > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_images <= 0 || a_elems < 0 || b_elems < 0 || total_ids < 0 || num_blocks < 0 || out_len < 0 || max_bins < 1)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if ((a_bytes != 1 && a_bytes != 2 && a_bytes != 4) || (b_bytes != 1 && b_bytes != 2 && b_bytes != 4 && b_bytes != 8))
    return m2f::fail(M2F_EINVAL, "%s: a is 1, 2 or 4 bytes per label and b 1, 2, 4 or 8, got %d and %d", fn, a_bytes,
                     b_bytes);
  if (!m2f::aligned(a, a_bytes) || !m2f::aligned(b, b_bytes) || !m2f::aligned(ids, 4) || !m2f::aligned(blocks, 4) ||
      !m2f::aligned(images, 8) || !m2f::aligned(out, 8) || !m2f::aligned(bad, 8))
    return m2f::fail(M2F_EINVAL, "%s: a buffer is not aligned to its element size", fn);
  if (path < 0 || path > 2) return m2f::fail(M2F_EINVAL, "%s: path %d is not 0 (auto), 1 (lds) or 2 (global)", fn, path);
  if (max_bins > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: a table of more than 2^31 - 1 counters", fn);
  if (path == 1 && max_bins > kLdsBins)
    return m2f::fail(M2F_EINVAL, "%s: a table of %lld counters is beyond the %d of the LDS path", fn,
                     static_cast<long long>(max_bins), kLdsBins);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 table rows", fn);
  if (num_blocks == 0) return m2f::ok();
  const bool lds = path == 1 || (path == 0 && max_bins <= kLdsBins);
  const int64_t ign = has_ignore ? static_cast<int64_t>(ignore) : kNoIgnore;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(num_blocks);
  const int lds_bins = static_cast<int>(max_bins < kLdsBins ? max_bins : kLdsBins);
  int rc = M2F_OK;
  m2f::dispatch_one_of<1, 2, 4>(a_bytes, [&](auto ab) {     // both widths were checked above
    m2f::dispatch_one_of<1, 2, 4, 8>(b_bytes, [&](auto bb) {
      rc = launch<Label<ab.value>, Label<bb.value>>(fn, lds, lds_bins, grid, st, a, a_elems, b, b_elems, images,
                                                    num_images, ids, total_ids, blocks, ign, out, out_len, bad);
    });
  });
  return rc;
}

extern "C" int m2f_label_histogram_ragged(const void* a, int a_bytes, int64_t a_elems, const int64_t* images,
                                          int num_images, const int32_t* blocks, int64_t num_blocks, int has_ignore,
                                          int ignore, int64_t max_bins, int path, int64_t* out, int64_t out_len,
                                          int64_t* bad, void* stream) {
  const char* fn = "m2f_label_histogram_ragged";
  if (!images || !out || !bad || (!a && a_elems > 0) || (!blocks && num_blocks > 0))
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_images <= 0 || a_elems < 0 || num_blocks < 0 || out_len < 0 || max_bins < 1)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (a_bytes != 1 && a_bytes != 2 && a_bytes != 4)
    return m2f::fail(M2F_EINVAL, "%s: a is 1, 2 or 4 bytes per label, got %d", fn, a_bytes);
  if (!m2f::aligned(a, a_bytes) || !m2f::aligned(blocks, 4) || !m2f::aligned(images, 8) || !m2f::aligned(out, 8) ||
      !m2f::aligned(bad, 8))
    return m2f::fail(M2F_EINVAL, "%s: a buffer is not aligned to its element size", fn);
  if (path < 0 || path > 2) return m2f::fail(M2F_EINVAL, "%s: path %d is not 0 (auto), 1 (lds) or 2 (global)", fn, path);
  if (max_bins > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: a table of more than 2^31 - 1 counters", fn);
  if (path == 1 && max_bins > kLdsBins)
    return m2f::fail(M2F_EINVAL, "%s: a table of %lld counters is beyond the %d of the LDS path", fn,
                     static_cast<long long>(max_bins), kLdsBins);
  if (num_blocks > kIntMax) return m2f::fail(M2F_EUNSUPPORTED, "%s: more than 2^31 - 1 table rows", fn);
  if (num_blocks == 0) return m2f::ok();
  const bool lds = path == 1 || (path == 0 && max_bins <= kLdsBins);
  const int64_t ign = has_ignore ? static_cast<int64_t>(ignore) : kNoIgnore;
  const int lds_bins = static_cast<int>(max_bins < kLdsBins ? max_bins : kLdsBins);
  int rc = M2F_OK;
  m2f::dispatch_one_of<1, 2, 4>(a_bytes, [&](auto ab) {     // the width was checked above
    using TA = Label<ab.value>;
    rc = launch<TA, TA, false>(fn, lds, lds_bins, static_cast<unsigned>(num_blocks), static_cast<hipStream_t>(stream),
                               a, a_elems, nullptr, 0, images, num_images, nullptr, 0, blocks, ign, out, out_len, bad);
  });
  return rc;
}

// One row of the view table of include/bm2f.h (M2F_VIEW_FIELDS int64), decoded and checked the same way on the host
// and in the kernels of image_views.hip and bits_views.hip.
#pragma once

#include <cstdint>

#include "bm2f.h"

namespace m2f_view {

constexpr int kF = M2F_VIEW_FIELDS;
constexpr int kMaxK = M2F_VIEW_MAX_KSIZE;
constexpr int64_t kI31 = 0x7fffffff, kMaxNumel = int64_t{1} << 48;

struct Row {
  int64_t off, stride, pstride, tx, ty;
  int H, W, rh, rw, cy0, cx0, ch, cw, Hc, Wc, kx, ky, fill;
  bool flip_in, flip_out;
};

__host__ __device__ inline bool in31(int64_t v) { return v >= -kI31 && v <= kI31; }
// a * b <= limit for non-negative values, without forming a product that could overflow
__host__ __device__ inline bool mul_le(int64_t a, int64_t b, int64_t limit) { return a == 0 || b <= limit / a; }

// One table row, checked against everything passed by value.  A source pixel is 3 elements of an image (HWC bytes) and
// 1 of a label plane; planes is 1 for an image.  image: the bilinear tables (2 * out bounds + out * ksize coefficients per
// resized axis, none for a skipped one); else the nearest tables (out indices per axis).
__host__ __device__ inline bool load_row(const int64_t* r, bool image, int planes, int64_t src_numel,
                                         int64_t tables_numel, int out_h, int out_w, Row* o) {
  for (int i = 1; i < kF; ++i)
    if (!in31(r[i]) && i != 3 && i != 14 && i != 15 && i != 17) return false;
  const int64_t off = r[0], H = r[1], W = r[2], stride = r[3], rh = r[4], rw = r[5], ch = r[8], cw = r[9], Hc = r[10],
                Wc = r[11], tx = r[14], ty = r[15], fill = r[16], ps = r[17], kx = r[18], ky = r[19];
  const int64_t e = image ? 3 : 1;
  if (H <= 0 || W <= 0 || rh <= 0 || rw <= 0 || ch <= 0 || cw <= 0 || Hc <= 0 || Wc <= 0) return false;
  if (Hc > out_h || Wc > out_w) return false;
  if (src_numel > kMaxNumel || off < 0 || off > src_numel || stride < W * e || ps < 0) return false;
  // the last element read is off + (planes - 1) ps + (H - 1) stride + W e - 1: three terms of at most 2^48 each
  const int64_t room = src_numel - off;
  if (!mul_le(planes - 1, ps, room) || !mul_le(H - 1, stride, room)) return false;
  if ((planes - 1) * ps + (H - 1) * stride + W * e > room) return false;
  if (tx < 0 || ty < 0 || tx > tables_numel || ty > tables_numel) return false;
  if (image) {
    if (fill < 0 || fill > 255) return false;
    if (kx < 0 || ky < 0 || kx > kMaxK || ky > kMaxK) return false;
    if ((kx == 0) != (rw == W) || (ky == 0) != (rh == H)) return false;
    // an axis's table is 2 * out bounds, then out * ksize coefficients, indexed with 32 bits
    if (rw * (2 + kx) > kI31 || rh * (2 + ky) > kI31) return false;
    if (kx && rw * (2 + kx) > tables_numel - tx) return false;
    if (ky && rh * (2 + ky) > tables_numel - ty) return false;
  } else {
    if (rw > tables_numel - tx || rh > tables_numel - ty) return false;
  }
  o->off = off; o->stride = stride; o->pstride = ps; o->tx = tx; o->ty = ty;
  o->H = static_cast<int>(H); o->W = static_cast<int>(W); o->rh = static_cast<int>(rh); o->rw = static_cast<int>(rw);
  o->cy0 = static_cast<int>(r[6]); o->cx0 = static_cast<int>(r[7]); o->ch = static_cast<int>(ch);
  o->cw = static_cast<int>(cw); o->Hc = static_cast<int>(Hc); o->Wc = static_cast<int>(Wc);
  o->kx = static_cast<int>(kx); o->ky = static_cast<int>(ky); o->fill = static_cast<int>(fill);
  o->flip_in = r[12] != 0; o->flip_out = r[13] != 0;
  return true;
}

// the resized column of canvas column x (a 64-bit value: cx0 is any int32), valid when x < cw and it is in [0, rw)
__host__ __device__ inline int64_t resized_col(const Row& g, int x) {
  return static_cast<int64_t>(g.cx0) + (g.flip_out ? g.cw - 1 - x : x);
}

}  // namespace m2f_view

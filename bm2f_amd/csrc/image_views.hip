// The input pipeline of the reference on the device: the mappers' PIL resize (ResizeTransform ->
// Image.resize(BILINEAR) for images, NEAREST for label maps and masks), their crop, flip and pad, and the model's
// (x - pixel_mean) / pixel_std and ImageList.from_tensors, for all V views of a call in one launch.
//
// m2f_image_views.  Pillow's 8-bit resize (Resample.c) is integer arithmetic and is restated exactly: per axis a
// table of (xmin, n) bounds and ksize int32 coefficients at PRECISION_BITS = 22 (built on the host,
// bm2f_amd/image_views.py), each pass  out = clip8((2^21 + sum_k pixel[xmin + k] * coeff[k]) >> 22),  horizontal
// first, the intermediate rounded to uint8, an axis whose size does not change skipped.  A view's row of the table
// (include/bm2f.h) adds a crop window in resized coordinates, a canvas, a mirror of the source (flip_in) or of the
// crop (flip_out) and a fill byte.  An output element is, in this order,
//   outside the canvas           pad_value, stored as is
//   inside crop and image        the PIL pixel p          } as p itself (uint8), float(p), or (float(p) - mean[c]) /
//   elsewhere in the canvas      the fill byte as p       } std[c]: an fp32 subtract and a correctly rounded fp32
//                                                           divide (no reciprocal), rounded once more for 16 bits
//
// Tile.  A workgroup of 256 threads owns kTW = 64 columns x th rows of one view's (Hp, Wp) output, all 3 channels.
// 64 columns make a channel's row segment 256 B of fp32 (64 B of uint8), one full-width store per wave, and keep the
// horizontal halo (ksize - 1 source columns per tile) small against the tile.  th is 16 where it fits and halves
// (8, 4, 2, 1) until the tallest intermediate of the call fits the budget below; one th serves every view of a
// launch, so a strongly reduced view makes the others' tiles shorter too.  Per tile:
//   1. the tile's bounds are read and clamped into LDS (a wrong table can then only give wrong pixels);
//   2. the source rows the vertical taps of the tile span are staged, kStage bytes at a time, as the contiguous HWC
//      byte runs the horizontal taps span;
//   3. the horizontal pass writes the uint8 intermediate [3][rows][64] (planar, so the vertical pass reads
//      neighbouring bytes in neighbouring lanes) -- it exists only in LDS;
//   4. the vertical pass, the crop / flip addressing, HWC -> CHW and the normalisation are the epilogue; every
//      element of the tile is stored once, pads included.  No atomics.
//
// LDS budget (bytes): intermediate kInter = 49152 (256 rows), stage kStage = 24576, bounds (16 + 64) * 12 = 960:
// 74688, so that two workgroups share a CU's 163840 B.  The kernel is a chain of dependent LDS reads and integer
// multiply-adds with no MFMA; two workgroups (8 waves per CU) are what the LDS leaves, and registers do not bind
// before that.  Speed was not a design input beyond this; tools/input_pipeline_bench.py records what it reaches.
//
// Limits: ksize <= M2F_VIEW_MAX_KSIZE = 131 per axis, i.e. any up-scale and a down-scale of at most 65x.  At th = 1
// the intermediate holds ksize + 1 <= 132 rows and a staged row spans at most 63 * 65 + 132 columns = 12681 B, so
// every admitted view fits; anything beyond is refused with M2F_EUNSUPPORTED before a launch.
//
// m2f_label_views is the nearest-neighbour gather (ImagingScaleAffine's index tables, built on the host) with the
// same crop, flips, canvas and pad on (P, H, W) planes of 1, 2 or 4 byte elements: one thread per output element.
//
// m2f_image_views_color is the same kernel body instantiated with a colour stage (MODE kColor): detectron2's
// ColorAugSSDTransform (OpenCV's 8-bit HSV restated) and the video mappers' brightness / contrast / saturation blends,
// defined in bm2f_amd/color_aug.py, applied per pixel to its three channels between the vertical pass and the store.
// The epilogue then walks pixels, not elements: a thread forms the three channels of a pixel, so a tile costs three
// vertical passes per thread step instead of one, with the same LDS traffic in total.  Fill and pad are never
// coloured.  A view's operation list is a row of fp64 in device memory (decoded into registers with constant indices);
// the two 256-entry HSV division tables ride in `tables` and are copied into 2 KiB of LDS per workgroup (76736 B,
// still two workgroups per CU).  The contrast blend needs the mean of the whole view first: m2f_image_views_sum runs
// the same body (MODE kSum) with the operations before the blend, sums the shown pixels per tile as integers and
// reduces the tiles per view in a fixed order; the colour launch divides that sum by the count in fp64.
//
// Both entry points take the table twice: views_host is checked row by row against the source, table and output
// ranges before anything is launched (M2F_EUNSUPPORTED names the row), views_dev is what the kernels read, and
// they repeat the same check on it, so a device copy that differs from the checked one is skipped, not trusted.
#include "bm2f.h"
#include "common.h"
#include "view_row.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

using namespace m2f_view;  // Row, load_row, resized_col and their constants: shared with bits_views.hip

constexpr int kTW = 64, kTHMax = 16;
constexpr int kInter = 49152, kStage = 24576;
constexpr int kInterRows = kInter / (3 * kTW);  // 256

struct Bound {  // one output row / column of a tile: first tap relative to the window, taps, coefficient offset
  int start, n, coef;
};

template <typename T>
struct Store {
  static __device__ __forceinline__ T pixel(int p, bool norm, float mean, float sd) {
    const float f = static_cast<float>(p);
    return static_cast<T>(norm ? __fdiv_rn(__fsub_rn(f, mean), sd) : f);
  }
  static __device__ __forceinline__ T pad(float v) { return static_cast<T>(v); }
};
template <>
struct Store<uint8_t> {
  static __device__ __forceinline__ uint8_t pixel(int p, bool, float, float) { return static_cast<uint8_t>(p); }
  static __device__ __forceinline__ uint8_t pad(float v) {
    return static_cast<uint8_t>(min(max(static_cast<int>(v), 0), 255));
  }
};

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> 22, 0), 255); }

struct Norm {  // read with constant indices only: a kernel argument indexed at run time would move to scratch
  float m0, m1, m2, s0, s1, s2;
  int on;
};

// ---------------------------------------------------------------------------------------------- colour stage
// The photometric operations of bm2f_amd/color_aug.py (the definition) on the three channels of one pixel, between
// the vertical pass and Store<T>::pixel.  Every fp32 / fp64 product and sum is rounded on its own; the _rn intrinsics
// say so to the reader, but to the compiler they are plain operators, so this file is built with -ffp-contract=off
// (bm2f_amd/build.py) and the pragma below repeats it.  The one FMA chain is the one the definition spells out.
#pragma clang fp contract(off)
constexpr int kCF = M2F_COLOR_FIELDS, kMaxOps = M2F_COLOR_MAX_OPS;
constexpr int kDivs = 512;  // sdiv[256], hdiv[256]
constexpr double kHueMax = 1048576.0;

enum Mode { kPlain = 0, kColor = 1, kSum = 2 };

struct Color {  // like Norm: constant indices only (the loops over k are fully unrolled)
  int n, ci, code[kMaxOps];
  bool swap, hsv;
  double a[kMaxOps], b[kMaxOps];
};

struct ColorArgs {
  const double* colors;   // (V, kCF)
  const int64_t* sums;    // (V), read by kColor for views with a contrast blend
  int64_t* partials;      // (V, tiles), written by kSum
  int64_t hsv_off;        // sdiv / hdiv in `tables`
};

__host__ __device__ inline bool small_int(double x, double lo, double hi) {
  return x >= lo && x <= hi && x == static_cast<double>(static_cast<int>(x));
}

__host__ __device__ inline bool load_color(const double* r, Color* o) {
  if (!small_int(r[0], 0, kMaxOps) || !small_int(r[2], -1, kMaxOps - 1)) return false;
  o->n = static_cast<int>(r[0]);
  o->ci = static_cast<int>(r[2]);
  o->swap = r[1] != 0.0;
  o->hsv = false;
  int contrast = -1, contrasts = 0;
#pragma unroll
  for (int k = 0; k < kMaxOps; ++k) {
    o->code[k] = 0;
    o->a[k] = o->b[k] = 0.0;
    if (k < o->n) {
      const double c = r[4 + 3 * k], a = r[5 + 3 * k], b = r[6 + 3 * k];
      if (!small_int(c, M2F_COLOR_CONVERT, M2F_COLOR_SATURATION)) return false;
      if (!(a - a == 0.0) || !(b - b == 0.0)) return false;  // finite
      const int code = static_cast<int>(c);
      if (code == M2F_COLOR_SSD_HUE && !small_int(a, -kHueMax, kHueMax)) return false;
      if (code == M2F_COLOR_SSD_HUE || code == M2F_COLOR_SSD_SAT) o->hsv = true;
      if (code == M2F_COLOR_CONTRAST) {
        contrast = k;
        ++contrasts;
      }
      o->code[k] = code;
      o->a[k] = a;
      o->b[k] = b;
    }
  }
  return contrasts <= 1 && contrast == o->ci;
}

// canvas pixels of a view that show the resized image
__device__ inline int64_t shown_pixels(const Row& g) {
  const int64_t my = min(g.ch, g.Hc), mx = min(g.cw, g.Wc);
  const int64_t ya = max(static_cast<int64_t>(g.cy0), int64_t{0});
  const int64_t yb = min(static_cast<int64_t>(g.cy0) + my - 1, static_cast<int64_t>(g.rh) - 1);
  const int64_t a = resized_col(g, 0), b = resized_col(g, static_cast<int>(mx) - 1);
  const int64_t xa = max(min(a, b), int64_t{0}), xb = min(max(a, b), static_cast<int64_t>(g.rw) - 1);
  return max(yb - ya + 1, int64_t{0}) * max(xb - xa + 1, int64_t{0});
}

__device__ __forceinline__ int convert8(int p, float a, float b) {
  const float f = __fadd_rn(__fmul_rn(static_cast<float>(p), a), b);
  return static_cast<int>(fminf(fmaxf(f, 0.f), 255.f));
}

__device__ __forceinline__ int blend8(double src, float w, int p) {
  const double d = __dadd_rn(src, static_cast<double>(__fmul_rn(w, static_cast<float>(p))));
  return static_cast<int>(fmin(fmax(d, 0.0), 255.0));
}

// OpenCV's 8-bit BGR -> HSV with H in [0, 180): integers; divs = sdiv[256], hdiv[256]
__device__ __forceinline__ void bgr2hsv(const int* __restrict__ divs, int b, int g, int r, int& h, int& s, int& v) {
  v = max(max(b, g), r);
  const int diff = v - min(min(b, g), r);
  s = (diff * divs[v] + 2048) >> 12;
  const int h0 = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h0 * divs[256 + diff] + 2048) >> 12;
  h += h < 0 ? 180 : 0;
  h = min(max(h, 0), 255);
}

__device__ __forceinline__ int unit8(float x) { return min(max(__float2int_rn(__fmul_rn(x, 255.f)), 0), 255); }

// OpenCV's 8-bit HSV -> BGR: fp32 on h, s / 255, v / 255
__device__ __forceinline__ void hsv2bgr(int hi, int si, int vi, int& b, int& g, int& r) {
  const float v = __fdiv_rn(static_cast<float>(vi), 255.f);
  if (si == 0) {
    b = g = r = unit8(v);
    return;
  }
  const float s = __fdiv_rn(static_cast<float>(si), 255.f);
  float h = __fmul_rn(static_cast<float>(hi), 6.f / 180.f);
  const float fl = floorf(h);
  int sector = static_cast<int>(fl);
  h = __fsub_rn(h, fl);
  if (sector < 0 || sector > 5) {
    sector = 0;
    h = 0.f;
  }
  const float t0 = v, t1 = __fmul_rn(v, __fsub_rn(1.f, s)), t2 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, h))),
              t3 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, h))));
  // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], as selects
  const float fb = sector <= 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
  const float fg = sector == 0 ? t3 : (sector <= 2 ? t0 : (sector == 3 ? t2 : t1));
  const float fr = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  b = unit8(fb);
  g = unit8(fg);
  r = unit8(fr);
}

// operations [0, stop) of a view on one pixel; mean is read by the contrast blend only
__device__ __forceinline__ void apply_color(const Color& cl, int stop, const int* __restrict__ divs, double mean,
                                            int& p0, int& p1, int& p2) {
  int c0 = cl.swap ? p2 : p0, c1 = p1, c2 = cl.swap ? p0 : p2;
#pragma unroll
  for (int k = 0; k < kMaxOps; ++k) {
    if (k >= stop) break;
    const int code = cl.code[k];
    const double a = cl.a[k], b = cl.b[k];
    if (code == M2F_COLOR_CONVERT) {
      const float fa = static_cast<float>(a), fb = static_cast<float>(b);
      c0 = convert8(c0, fa, fb);
      c1 = convert8(c1, fa, fb);
      c2 = convert8(c2, fa, fb);
    } else if (code == M2F_COLOR_SSD_SAT || code == M2F_COLOR_SSD_HUE) {
      int h, s, v;
      bgr2hsv(divs, c0, c1, c2, h, s, v);
      if (code == M2F_COLOR_SSD_SAT) {
        s = convert8(s, static_cast<float>(a), 0.f);
      } else {
        h = (h + static_cast<int>(a)) % 180;
        h += h < 0 ? 180 : 0;
      }
      hsv2bgr(h, s, v, c0, c1, c2);
    } else if (code == M2F_COLOR_CONTRAST || code == M2F_COLOR_SATURATION) {
      const double m = code == M2F_COLOR_CONTRAST
                           ? mean
                           : __fma_rn(static_cast<double>(c2), 0.114,
                                      __fma_rn(static_cast<double>(c1), 0.587, __dmul_rn(static_cast<double>(c0), 0.299)));
      const double srcv = __dmul_rn(a, m);
      const float w = static_cast<float>(b);
      c0 = blend8(srcv, w, c0);
      c1 = blend8(srcv, w, c1);
      c2 = blend8(srcv, w, c2);
    }
  }
  p0 = cl.swap ? c2 : c0;
  p1 = c1;
  p2 = cl.swap ? c0 : c2;
}

// grid (ceil(Wp / 64), ceil(Hp / th), V), 256 threads, dynamic LDS kInter + kStage + bounds (+ kDivs ints with colour).
// kPlain is m2f_image_views; kColor adds the colour stage; kSum runs the same resize and the operations before a
// view's contrast blend and writes the tile's integer sum of the shown pixels to ca.partials instead of pixels to out.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) image_views_kernel(const uint8_t* __restrict__ src, int64_t src_numel,
                                                          const int64_t* __restrict__ views,
                                                          const int32_t* __restrict__ tables, int64_t tables_numel,
                                                          Norm nm, float pad_value, T* __restrict__ out, int Hp,
                                                          int Wp, int th, ColorArgs ca) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* inter = smem;              // [3][kInterRows][kTW]
  uint8_t* stage = smem + kInter;     // [rows of a chunk][span * 3]
  Bound* ys = reinterpret_cast<Bound*>(smem + kInter + kStage);  // [kTHMax]
  Bound* xs = ys + kTHMax;                                       // [kTW]
  int* divs = reinterpret_cast<int*>(xs + kTW);                  // [kDivs], colour modes only
  __shared__ int s_win[4];            // window: first source row, rows, first table column, columns

  const int tid = threadIdx.x, v = blockIdx.z;
  const int y0 = blockIdx.y * th, x0 = blockIdx.x * kTW;
  Row g;
  Color cl;
  bool ok = load_row(views + static_cast<int64_t>(v) * kF, true, 1, src_numel, tables_numel, Hp, Wp, &g);
  if constexpr (MODE != kPlain) {
    ok = ok && load_color(ca.colors + static_cast<int64_t>(v) * kCF, &cl);
    ok = ok && (!cl.hsv || (ca.hsv_off >= 0 && ca.hsv_off <= tables_numel - kDivs));
    ok = ok && (MODE == kSum || cl.ci < 0 || ca.sums != nullptr);
  }
  const int64_t tile = static_cast<int64_t>(v) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x;
  if constexpr (MODE == kSum) {
    if (ok && cl.ci < 0) return;  // no contrast blend: its partials are never read
    if (!ok) {
      if (tid == 0) ca.partials[tile] = 0;
      return;
    }
  } else {
    if (!ok) return;
  }
  if constexpr (MODE != kPlain) {
    if (cl.hsv)
      for (int i = tid; i < kDivs; i += 256) divs[i] = tables[ca.hsv_off + i];
  }

  // the tile's rows and columns that show the resized image: both ranges are contiguous
  const int ye = min(min(y0 + th, g.ch), g.Hc), xe = min(min(x0 + kTW, g.cw), g.Wc);
  int64_t rya = 0, ryb = -1, rxa = 0, rxb = -1;
  if (ye > y0 && xe > x0) {
    rya = max(static_cast<int64_t>(g.cy0) + y0, int64_t{0});
    ryb = min(static_cast<int64_t>(g.cy0) + ye - 1, static_cast<int64_t>(g.rh) - 1);
    const int64_t a = resized_col(g, x0), b = resized_col(g, xe - 1);
    rxa = max(min(a, b), int64_t{0});
    rxb = min(max(a, b), static_cast<int64_t>(g.rw) - 1);
  }
  const int ny = static_cast<int>(max(ryb - rya + 1, int64_t{0})), nx = static_cast<int>(max(rxb - rxa + 1, int64_t{0}));
  const bool any = ny > 0 && nx > 0;  // uniform
  const int32_t* tY = tables + g.ty;
  const int32_t* tX = tables + g.tx;

  if (any) {
    // bounds of the tile's resized rows (wave 0) and columns (wave 1), clamped to the source
    if (tid < kTHMax) {
      Bound b{0, 0, 0};
      if (tid < ny) {
        const int ry = static_cast<int>(rya) + tid;
        if (g.ky) {
          b.start = min(max(tY[2 * ry], 0), g.H);
          b.n = min(min(max(tY[2 * ry + 1], 0), g.ky), g.H - b.start);
          b.coef = 2 * g.rh + ry * g.ky;
        } else {
          b.start = ry;
          b.n = 1;
        }
      }
      ys[tid] = b;
    } else if (tid >= 64 && tid < 64 + kTW) {
      const int j = tid - 64;
      Bound b{0, 0, 0};
      if (j < nx) {
        const int rx = static_cast<int>(rxa) + j;
        if (g.kx) {
          b.start = min(max(tX[2 * rx], 0), g.W);
          b.n = min(min(max(tX[2 * rx + 1], 0), g.kx), g.W - b.start);
          b.coef = 2 * g.rw + rx * g.kx;
        } else {
          b.start = rx;
          b.n = 1;
        }
      }
      xs[j] = b;
    }
    __syncthreads();
    if (tid == 0) {
      int lo = 0x7fffffff, hi = 0;
      for (int i = 0; i < ny; ++i) {
        lo = min(lo, ys[i].start);
        hi = max(hi, ys[i].start + ys[i].n);
      }
      s_win[0] = min(lo, hi);
      s_win[1] = min(max(hi - lo, 0), kInterRows);
    } else if (tid == 64) {
      int lo = 0x7fffffff, hi = 0;
      for (int i = 0; i < nx; ++i) {
        lo = min(lo, xs[i].start);
        hi = max(hi, xs[i].start + xs[i].n);
      }
      s_win[2] = min(lo, hi);
      s_win[3] = min(max(hi - lo, 0), kStage / 3);
    }
    __syncthreads();
    const int wy = s_win[0], R = s_win[1], wx = s_win[2], span = s_win[3];
    // taps relative to the window; a tap past it (only a wrong table has one) is dropped
    if (tid < ny) {
      Bound b = ys[tid];
      b.start -= wy;
      b.n = max(min(b.n, R - b.start), 0);
      ys[tid] = b;
    } else if (tid >= 64 && tid < 64 + nx) {
      Bound b = xs[tid - 64];
      b.start -= wx;
      b.n = max(min(b.n, span - b.start), 0);
      xs[tid - 64] = b;
    }
    const int rowbytes = span * 3;
    // table columns [wx, wx + span) are source columns [W - wx - span, W - wx) of a mirrored source
    const int scol0 = g.flip_in ? g.W - wx - span : wx;
    const int RC = rowbytes > 0 ? min(kStage / rowbytes, R) : 0;
    __syncthreads();
    for (int r0 = 0; r0 < R && RC > 0; r0 += RC) {
      const int rows = min(RC, R - r0);
      const uint8_t* sp = src + g.off + static_cast<int64_t>(wy + r0) * g.stride + static_cast<int64_t>(scol0) * 3;
      for (int idx = tid; idx < rows * rowbytes; idx += 256) {
        const int rr = idx / rowbytes, b = idx - rr * rowbytes;
        stage[idx] = sp[static_cast<int64_t>(rr) * g.stride + b];
      }
      __syncthreads();
      for (int idx = tid; idx < rows * 3 * nx; idx += 256) {
        const int col = idx % nx, q = idx / nx, c = q % 3, rr = q / 3;
        const Bound b = xs[col];
        const uint8_t* sr = stage + rr * rowbytes + c;
        int p;
        if (g.kx) {
          int acc = 1 << 21;
          const int32_t* kk = tX + b.coef;
          for (int k = 0; k < b.n; ++k) {
            const int i = b.start + k;
            acc += static_cast<int>(sr[(g.flip_in ? span - 1 - i : i) * 3]) * kk[k];
          }
          p = clip8(acc);
        } else {
          p = b.n ? sr[(g.flip_in ? span - 1 - b.start : b.start) * 3] : 0;
        }
        inter[(c * kInterRows + r0 + rr) * kTW + col] = static_cast<uint8_t>(p);
      }
      __syncthreads();
    }
  }

  // the vertical pass of channel c at resized (ry, rx), both inside the tile's ranges
  auto vertical = [&](int c, int64_t ry, int64_t rx) -> int {
    const Bound b = ys[static_cast<int>(ry - rya)];
    const uint8_t* ic = inter + (c * kInterRows + b.start) * kTW + static_cast<int>(rx - rxa);
    if (g.ky) {
      int acc = 1 << 21;
      const int32_t* kk = tY + b.coef;
      for (int k = 0; k < b.n; ++k) acc += static_cast<int>(ic[k * kTW]) * kk[k];
      return clip8(acc);
    }
    return b.n ? ic[0] : 0;
  };
  const int64_t plane = static_cast<int64_t>(Hp) * Wp;
  if constexpr (MODE == kPlain) {
    T* ov = out + static_cast<int64_t>(v) * 3 * plane;
    for (int idx = tid; idx < 3 * th * kTW; idx += 256) {
      const int x = idx % kTW, q = idx / kTW, y = q % th, c = q / th;
      const int gy = y0 + y, gx = x0 + x;
      if (gy >= Hp || gx >= Wp) continue;
      T val;
      if (gy >= g.Hc || gx >= g.Wc) {
        val = Store<T>::pad(pad_value);
      } else {
        int p = g.fill;
        const int64_t ry = static_cast<int64_t>(g.cy0) + gy, rx = resized_col(g, gx);
        if (any && gy < g.ch && gx < g.cw && ry >= rya && ry <= ryb && rx >= rxa && rx <= rxb) p = vertical(c, ry, rx);
        val = Store<T>::pixel(p, nm.on != 0, c == 0 ? nm.m0 : c == 1 ? nm.m1 : nm.m2,
                              c == 0 ? nm.s0 : c == 1 ? nm.s1 : nm.s2);
      }
      ov[c * plane + static_cast<int64_t>(gy) * Wp + gx] = val;
    }
  } else {
    // one pixel per thread and step: the operations need its three channels together
    __syncthreads();  // divs
    const int stop = MODE == kSum ? cl.ci : cl.n;
    double mean = 0.0;
    if constexpr (MODE == kColor) {
      const int64_t shown = shown_pixels(g);
      if (cl.ci >= 0 && shown > 0) mean = __ddiv_rn(static_cast<double>(ca.sums[v]), static_cast<double>(3 * shown));
    }
    int64_t total = 0;
    for (int idx = tid; idx < th * kTW; idx += 256) {
      const int x = idx % kTW, y = idx / kTW;
      const int gy = y0 + y, gx = x0 + x;
      if (gy >= Hp || gx >= Wp) continue;
      const bool pad = gy >= g.Hc || gx >= g.Wc;
      const int64_t ry = static_cast<int64_t>(g.cy0) + gy, rx = resized_col(g, gx);
      const bool shown = !pad && any && gy < g.ch && gx < g.cw && ry >= rya && ry <= ryb && rx >= rxa && rx <= rxb;
      int p0 = g.fill, p1 = g.fill, p2 = g.fill;
      if (shown) {
        p0 = vertical(0, ry, rx);
        p1 = vertical(1, ry, rx);
        p2 = vertical(2, ry, rx);
        apply_color(cl, stop, divs, mean, p0, p1, p2);
        total += p0 + p1 + p2;
      }
      if constexpr (MODE == kColor) {
        T* o = out + static_cast<int64_t>(v) * 3 * plane + static_cast<int64_t>(gy) * Wp + gx;
        const bool on = nm.on != 0;
        o[0] = pad ? Store<T>::pad(pad_value) : Store<T>::pixel(p0, on, nm.m0, nm.s0);
        o[plane] = pad ? Store<T>::pad(pad_value) : Store<T>::pixel(p1, on, nm.m1, nm.s1);
        o[2 * plane] = pad ? Store<T>::pad(pad_value) : Store<T>::pixel(p2, on, nm.m2, nm.s2);
      }
    }
    if constexpr (MODE == kSum) {
      // the tile's sum: integers, so any order gives the same bits; a fixed tree all the same
      int64_t* red = reinterpret_cast<int64_t*>(stage);
      __syncthreads();
      red[tid] = total;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      if (tid == 0) ca.partials[tile] = red[0];
    }
  }
}

// one workgroup per view: sums[v] = the view's partials in a fixed order (0 for a view without a contrast blend)
__global__ void __launch_bounds__(256) views_sum_reduce_kernel(const double* __restrict__ colors,
                                                               const int64_t* __restrict__ partials, int tiles,
                                                               int64_t* __restrict__ sums) {
  __shared__ int64_t red[256];
  const int tid = threadIdx.x, v = blockIdx.x;
  Color cl;
  const bool ok = load_color(colors + static_cast<int64_t>(v) * kCF, &cl) && cl.ci >= 0;  // uniform
  int64_t total = 0;
  if (ok)
    for (int i = tid; i < tiles; i += 256) total += partials[static_cast<int64_t>(v) * tiles + i];
  red[tid] = total;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) sums[v] = red[0];
}

// one thread per output element, grid-stride; out (V, P, Hp, Wp)
template <typename T>
__global__ void __launch_bounds__(256) label_views_kernel(const T* __restrict__ src, int64_t src_numel,
                                                          const int64_t* __restrict__ views, int V, int P,
                                                          const int32_t* __restrict__ tables, int64_t tables_numel,
                                                          T* __restrict__ out, int Hp, int Wp) {
  const int64_t plane = static_cast<int64_t>(Hp) * Wp, per_view = plane * P, total = per_view * V;
  Row g;
  int cur = -1;
  bool ok = false;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += 256ll * gridDim.x) {
    const int v = static_cast<int>(i / per_view);
    const int64_t rem = i - v * per_view;
    const int p = static_cast<int>(rem / plane);
    const int64_t pix = rem - p * plane;
    const int gy = static_cast<int>(pix / Wp), gx = static_cast<int>(pix - static_cast<int64_t>(gy) * Wp);
    if (v != cur) {  // a thread's elements change their view rarely
      cur = v;
      ok = load_row(views + static_cast<int64_t>(v) * kF, false, P, src_numel, tables_numel, Hp, Wp, &g);
    }
    if (!ok) continue;
    T val = static_cast<T>(g.fill);  // the canvas fill is the batch pad as well
    const int64_t ry = static_cast<int64_t>(g.cy0) + gy, rx = resized_col(g, gx);
    if (gy < g.ch && gx < g.cw && gy < g.Hc && gx < g.Wc && ry >= 0 && ry < g.rh && rx >= 0 && rx < g.rw) {
      const int sy = min(max(tables[g.ty + ry], 0), g.H - 1);
      int sx = min(max(tables[g.tx + rx], 0), g.W - 1);
      if (g.flip_in) sx = g.W - 1 - sx;
      val = src[g.off + p * g.pstride + sy * g.stride + sx];
    }
    out[i] = val;
  }
}

// rows of the intermediate / columns of the stage that `tile` outputs of an axis reduced by in / out can span
int span_bound(int tile, int64_t in, int64_t out, int ksize) {
  if (ksize == 0) return tile;
  const double scale = static_cast<double>(in) / static_cast<double>(out);
  return static_cast<int>(std::ceil((tile - 1) * scale)) + ksize + 1;
}

int check_common(const char* fn, const void* src, int64_t src_numel, const int64_t* vh, const int64_t* vd, int V,
                 const int32_t* tables, int64_t tables_numel, const void* out, int out_h, int out_w) {
  if (!src || !vh || !vd || !tables || !out) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (V <= 0 || src_numel <= 0 || tables_numel <= 0 || out_h <= 0 || out_w <= 0)
    return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (src_numel > kMaxNumel || V > 65535 || out_h > 65535 || static_cast<int64_t>(out_h) * out_w > kI31)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  return M2F_OK;
}


// the tile height a view's vertical reduction allows, starting from th; 0 when even one row does not fit
int fit_th(int th, int64_t H, int64_t rh, int ky) {
  while (th > 1 && span_bound(th, H, rh, ky) > kInterRows) th >>= 1;
  return span_bound(th, H, rh, ky) > kInterRows ? 0 : th;
}

// Everything m2f_image_views checks before its launch, for the three entry points that run image_views_kernel:
// on M2F_OK *th is the launch's tile height.  colors_host == nullptr: no colour table.
int plan_views(const char* fn, const void* src, int64_t src_numel, const int64_t* views_host,
               const int64_t* views_dev, int num_views, const int32_t* tables, int64_t tables_numel,
               const double* colors_host, const double* colors_dev, bool colored, int64_t hsv_offset, bool need_sums,
               const void* sums, const void* out, int out_h, int out_w, int* th_out) {
  if (int rc = check_common(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, out, out_h,
                            out_w))
    return rc;
  if (colored && (!colors_host || !colors_dev)) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  int th = kTHMax;
  for (int v = 0; v < num_views; ++v) {
    const int64_t* r = views_host + static_cast<int64_t>(v) * kF;
    Row g;
    if (r[18] > kMaxK || r[19] > kMaxK)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: ksize (%lld, %lld) > %d, a down-scale beyond 65x", fn, v,
                       static_cast<long long>(r[19]), static_cast<long long>(r[18]), kMaxK);
    if (!load_row(r, true, 1, src_numel, tables_numel, out_h, out_w, &g))
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a size is not positive, or the source, tables or canvas leave "
                       "their ranges", fn, v);
    // a resampled axis's ksize is the one its sizes imply, so that the bounds below hold for a correct table
    const int want_x = g.kx ? 2 * static_cast<int>(std::ceil(std::fmax(static_cast<double>(g.W) / g.rw, 1.0))) + 1 : 0;
    const int want_y = g.ky ? 2 * static_cast<int>(std::ceil(std::fmax(static_cast<double>(g.H) / g.rh, 1.0))) + 1 : 0;
    if (g.kx != want_x || g.ky != want_y)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: ksize (%d, %d) does not belong to its sizes", fn, v, g.ky, g.kx);
    if (span_bound(kTW, g.W, g.rw, g.kx) * 3 > kStage)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a tile's source columns exceed the stage", fn, v);
    th = fit_th(th, g.H, g.rh, g.ky);
    if (th == 0)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a tile's source rows exceed the intermediate", fn, v);
    if (colored) {
      Color cl;
      if (!load_color(colors_host + static_cast<int64_t>(v) * kCF, &cl))
        return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: its colour row is not a list of known operations with finite "
                         "parameters and at most one contrast blend", fn, v);
      if (cl.hsv && (hsv_offset < 0 || hsv_offset > tables_numel - kDivs))
        return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: hsv_offset %lld leaves the tables", fn, v,
                         static_cast<long long>(hsv_offset));
      if (need_sums && cl.ci >= 0 && !sums)
        return m2f::fail(M2F_EINVAL, "%s: view %d has a contrast blend and sums is null", fn, v);
    }
  }
  *th_out = th;
  return M2F_OK;
}

constexpr int kLds = kInter + kStage + (kTHMax + kTW) * static_cast<int>(sizeof(Bound));
constexpr int kLdsColor = kLds + kDivs * static_cast<int>(sizeof(int));

int check_store(const char* fn, int normalize, float std0, float std1, float std2, int out_dtype) {
  if (!m2f::is_float_dtype(out_dtype) && out_dtype != M2F_U8)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype %d", fn, out_dtype);
  if (normalize && out_dtype == M2F_U8)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: a uint8 output takes no mean / std", fn);
  if (normalize && !(std0 != 0.f && std1 != 0.f && std2 != 0.f))
    return m2f::fail(M2F_EINVAL, "%s: std must be nonzero", fn);
  return M2F_OK;
}

}  // namespace

extern "C" int m2f_image_views(const void* src, int64_t src_numel, const int64_t* views_host, const int64_t* views_dev,
                               int num_views, const int32_t* tables, int64_t tables_numel, int normalize, float mean0,
                               float mean1, float mean2, float std0, float std1, float std2, float pad_value,
                               int out_dtype, void* out, int out_h, int out_w, void* stream) {
  const char* fn = "m2f_image_views";
  if (int rc = check_common(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, out, out_h,
                            out_w))
    return rc;
  if (int rc = check_store(fn, normalize, std0, std1, std2, out_dtype)) return rc;
  int th = 0;
  if (int rc = plan_views(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, nullptr, nullptr,
                          false, -1, false, nullptr, out, out_h, out_w, &th))
    return rc;
  const Norm nm{mean0, mean1, mean2, std0, std1, std2, normalize != 0};
  const dim3 grid(m2f::ceil_div(out_w, kTW), m2f::ceil_div(out_h, th), num_views);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = M2F_OK;
  auto launch = [&](auto tag) {
    using T = typename decltype(tag)::type;
    rc = m2f::set_max_lds(reinterpret_cast<const void*>(&image_views_kernel<T, kPlain>), kLds, fn);
    if (rc) return;
    image_views_kernel<T, kPlain><<<grid, 256, kLds, st>>>(static_cast<const uint8_t*>(src), src_numel, views_dev,
                                                           tables, tables_numel, nm, pad_value, static_cast<T*>(out),
                                                           out_h, out_w, th, ColorArgs{nullptr, nullptr, nullptr, -1});
    rc = m2f::check_launch(fn);
  };
  if (out_dtype == M2F_U8) launch(m2f::Tag<uint8_t>{});
  else m2f::dispatch_float(out_dtype, launch);
  return rc;
}

extern "C" int m2f_image_views_color(const void* src, int64_t src_numel, const int64_t* views_host,
                                     const int64_t* views_dev, int num_views, const int32_t* tables,
                                     int64_t tables_numel, const double* colors_host, const double* colors_dev,
                                     int64_t hsv_offset, const int64_t* sums, int normalize, float mean0, float mean1,
                                     float mean2, float std0, float std1, float std2, float pad_value, int out_dtype,
                                     void* out, int out_h, int out_w, void* stream) {
  const char* fn = "m2f_image_views_color";
  if (int rc = check_common(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, out, out_h,
                            out_w))
    return rc;
  if (int rc = check_store(fn, normalize, std0, std1, std2, out_dtype)) return rc;
  if (sums && !m2f::aligned(sums, 8)) return m2f::fail(M2F_EINVAL, "%s: misaligned pointer", fn);
  int th = 0;
  if (int rc = plan_views(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, colors_host,
                          colors_dev, true, hsv_offset, true, sums, out, out_h, out_w, &th))
    return rc;
  const Norm nm{mean0, mean1, mean2, std0, std1, std2, normalize != 0};
  const dim3 grid(m2f::ceil_div(out_w, kTW), m2f::ceil_div(out_h, th), num_views);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = M2F_OK;
  auto launch = [&](auto tag) {
    using T = typename decltype(tag)::type;
    rc = m2f::set_max_lds(reinterpret_cast<const void*>(&image_views_kernel<T, kColor>), kLdsColor, fn);
    if (rc) return;
    image_views_kernel<T, kColor><<<grid, 256, kLdsColor, st>>>(
        static_cast<const uint8_t*>(src), src_numel, views_dev, tables, tables_numel, nm, pad_value,
        static_cast<T*>(out), out_h, out_w, th, ColorArgs{colors_dev, sums, nullptr, hsv_offset});
    rc = m2f::check_launch(fn);
  };
  if (out_dtype == M2F_U8) launch(m2f::Tag<uint8_t>{});
  else m2f::dispatch_float(out_dtype, launch);
  return rc;
}

// int64 words: V sums, then one partial per tile of the launch m2f_image_views_sum makes
extern "C" int m2f_image_views_sum_workspace(const int64_t* views_host, int num_views, int out_h, int out_w,
                                             int64_t* words) {
  const char* fn = "m2f_image_views_sum_workspace";
  if (!views_host || !words) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (num_views <= 0 || out_h <= 0 || out_w <= 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (num_views > 65535 || out_h > 65535 || static_cast<int64_t>(out_h) * out_w > kI31)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: sizes exceed the grid / index range", fn);
  int th = kTHMax;
  for (int v = 0; v < num_views; ++v) {
    const int64_t* r = views_host + static_cast<int64_t>(v) * kF;
    if (r[1] <= 0 || r[4] <= 0 || r[1] > kI31 || r[4] > kI31 || r[19] < 0 || r[19] > kMaxK)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a size is not positive or ksize > %d", fn, v, kMaxK);
    th = fit_th(th, r[1], r[4], static_cast<int>(r[19]));
    if (th == 0)
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a tile's source rows exceed the intermediate", fn, v);
  }
  const int64_t tiles = static_cast<int64_t>(m2f::ceil_div(out_w, kTW)) * m2f::ceil_div(out_h, th);
  *words = num_views * (tiles + 1);
  return m2f::ok();
}

extern "C" int m2f_image_views_sum(const void* src, int64_t src_numel, const int64_t* views_host,
                                   const int64_t* views_dev, int num_views, const int32_t* tables,
                                   int64_t tables_numel, const double* colors_host, const double* colors_dev,
                                   int64_t hsv_offset, int out_h, int out_w, int64_t* workspace,
                                   int64_t workspace_words, void* stream) {
  const char* fn = "m2f_image_views_sum";
  if (int rc = check_common(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, workspace,
                            out_h, out_w))
    return rc;
  if (!m2f::aligned(workspace, 8)) return m2f::fail(M2F_EINVAL, "%s: misaligned pointer", fn);
  int th = 0;
  if (int rc = plan_views(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, colors_host,
                          colors_dev, true, hsv_offset, false, nullptr, workspace, out_h, out_w, &th))
    return rc;
  const dim3 grid(m2f::ceil_div(out_w, kTW), m2f::ceil_div(out_h, th), num_views);
  const int64_t tiles = static_cast<int64_t>(grid.x) * grid.y;
  if (tiles > kI31 || workspace_words < num_views * (tiles + 1))
    return m2f::fail(M2F_EINVAL, "%s: workspace of %lld words, %lld needed", fn,
                     static_cast<long long>(workspace_words), static_cast<long long>(num_views * (tiles + 1)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = m2f::set_max_lds(reinterpret_cast<const void*>(&image_views_kernel<uint8_t, kSum>), kLdsColor, fn);
  if (rc) return rc;
  int64_t* partials = workspace + num_views;
  image_views_kernel<uint8_t, kSum><<<grid, 256, kLdsColor, st>>>(
      static_cast<const uint8_t*>(src), src_numel, views_dev, tables, tables_numel, Norm{0, 0, 0, 1, 1, 1, 0}, 0.f,
      nullptr, out_h, out_w, th, ColorArgs{colors_dev, nullptr, partials, hsv_offset});
  if ((rc = m2f::check_launch(fn))) return rc;
  views_sum_reduce_kernel<<<num_views, 256, 0, st>>>(colors_dev, partials, static_cast<int>(tiles), workspace);
  return m2f::check_launch(fn);
}

extern "C" int m2f_label_views(const void* src, int elem_bytes, int64_t src_numel, const int64_t* views_host,
                               const int64_t* views_dev, int num_views, int num_planes, const int32_t* tables,
                               int64_t tables_numel, void* out, int out_h, int out_w, void* stream) {
  const char* fn = "m2f_label_views";
  if (int rc = check_common(fn, src, src_numel, views_host, views_dev, num_views, tables, tables_numel, out, out_h,
                            out_w))
    return rc;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: element size %d", fn, elem_bytes);
  if (num_planes <= 0) return m2f::fail(M2F_EINVAL, "%s: sizes must be positive", fn);
  if (!m2f::aligned(src, elem_bytes) || !m2f::aligned(out, elem_bytes))
    return m2f::fail(M2F_EINVAL, "%s: misaligned pointer", fn);
  for (int v = 0; v < num_views; ++v) {
    Row g;
    if (!load_row(views_host + static_cast<int64_t>(v) * kF, false, num_planes, src_numel, tables_numel, out_h, out_w,
                  &g))
      return m2f::fail(M2F_EUNSUPPORTED, "%s: view %d: a size is not positive, or the source, tables or canvas leave "
                       "their ranges", fn, v);
  }
  const int64_t total = static_cast<int64_t>(num_views) * num_planes * out_h * out_w;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>((total + 255) / 256, 8192));
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto tag) {
    using T = typename decltype(tag)::type;
    label_views_kernel<T><<<grid, 256, 0, st>>>(static_cast<const T*>(src), src_numel, views_dev, num_views, num_planes,
                                                tables, tables_numel, static_cast<T*>(out), out_h, out_w);
  };
  if (elem_bytes == 1) launch(m2f::Tag<uint8_t>{});
  else if (elem_bytes == 2) launch(m2f::Tag<int16_t>{});
  else launch(m2f::Tag<int32_t>{});
  return m2f::check_launch(fn);
}

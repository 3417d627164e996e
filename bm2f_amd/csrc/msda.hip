// Multi-scale deformable attention (MSDA) forward / backward for gfx950.
//
// Semantics follow the reference op exactly (mask2former/modeling/pixel_decoder/ops):
//   * sampling point:  h = loc_y * H_l - 0.5, w = loc_x * W_l - 0.5; the point contributes only if
//     -1 < h < H_l and -1 < w < W_l (ms_deform_im2col_cuda.cuh:290-296);
//   * bilinear with per-corner zero padding, value = w1*v1 + w2*v2 + w3*v3 + w4*v4 (.cuh:38-89);
//   * backward: grad_value[corner] += w_corner * g * a; grad_attn = sum_c g * val;
//     grad_loc = (W * sum_c dval/dw * g * a, H * sum_c dval/dh * g * a)  (.cuh:92-164).
//
// Layout choices (MI355X-first, not the reference's thread-per-channel/1024-thread blocks):
//   * fp32 fast path: a pair (n, q, m) is served by G = D/4 lanes, each owning 4 consecutive
//     channels (one float4).  A wave64 therefore handles 64/G pairs; for D = 32 that is the 8 heads
//     of one query, every corner fetch is one 128-byte row per pair, and the channel reductions of
//     the backward are an in-lane sum of 4 followed by log2(G) xor-shuffles (no LDS, no barriers).
//   * the backward's grad_value scatter is the costly part (one 128-B row add per corner per
//     point).  With host spatial shapes and Lq == S (the encoder), queries are grouped into spatial
//     tiles and the adds go to a per-workgroup LDS window of the sampled neighbourhood, flushed to
//     HBM once with row-contiguous atomics; samples falling outside the window take the direct path.
//   * fp64 and channel counts the fast path does not cover use straightforward generic kernels.
//
// This file holds the C ABI entry points and the dispatch policy: validate, pick a kernel for the dims and options,
// launch.  The kernels live by family in msda_generic.hip, msda_bwd_tiled.hip, msda_fwd_quad.hip and
// msda_fwd_lds.hip, each behind the launchers of msda_host.h.
#include "msda_host.h"

#include <algorithm>
#include <type_traits>

namespace {

using namespace m2f_msda;

int check_dims(const char* fn, const void* value, const void* shapes, const void* lsi, const void* loc,
               const void* attn, const Dims& d, int im2col_step) {
  if (!value || !shapes || !lsi || !loc || !attn)
    return m2f::fail(M2F_EINVAL, "%s: null input pointer", fn);
  if (d.N <= 0 || d.S <= 0 || d.M <= 0 || d.D <= 0 || d.L <= 0 || d.Lq <= 0 || d.P <= 0)
    return m2f::fail(M2F_EINVAL, "%s: non-positive size (N=%d S=%d M=%d D=%d L=%d Lq=%d P=%d)", fn, d.N,
                     d.S, d.M, d.D, d.L, d.Lq, d.P);
  if (im2col_step <= 0) return m2f::fail(M2F_EINVAL, "%s: im2col_step must be positive", fn);
  const int step = std::min(d.N, im2col_step);
  if (d.N % step != 0)
    return m2f::fail(M2F_EINVAL, "%s: batch(%d) must divide im2col_step(%d)", fn, d.N, step);
  return M2F_OK;
}

bool fast_f32_ok(const Dims& d, const void* value, const void* loc, const void* out4) {
  const bool dims = (d.D == 16 || d.D == 32 || d.D == 64) && d.L <= kMaxLevels;
  return dims && m2f::aligned(value, 16) && m2f::aligned(loc, 8) && m2f::aligned(out4, 16);
}

// the three options that together select the LDS-window forward, fused or not
bool fwd_windowed() {
  return m2f::option(m2f::kOptMsdaFwdLds, 1) != 0 && m2f::option(m2f::kOptMsdaFwdQuad, 1) != 0 &&
         m2f::option(m2f::kOptMsdaFwdTiled, 1) != 0;
}

// The reference op's forward (materialised loc / attn) on the LDS-window kernel: encoder layout with host shapes,
// the options that select the windowed forward, and every byte offset under 2^31; false otherwise.
bool launch_fwd_lds_unfused(const char* fn, const float* value, const float* loc, const float* attn, const Dims& d,
                            const int64_t* host_shapes, float* out, hipStream_t st) {
  if (!host_shapes || d.D != 32 || d.P != 4 || d.Lq != d.S || d.L < 1 || d.L > kTileMaxL) return false;
  if (!fwd_windowed()) return false;
  if (!m2f::aligned(loc, 8) || static_cast<int64_t>(d.N) * d.S * d.M * d.L * d.P * 8 >= (int64_t{1} << 31)) return false;
  TileGeom base, geo;
  int64_t total;
  if (fill_levels(d, host_shapes, base, total) != LevelFill::kOk) return false;
  if (!make_fwd_lds_geom(d, 0, base, geo)) return false;
  if (tile_blocks(geo, d) > 0x7fffffff) return false;
  return launch_fwd_lds(fn, value, FrontEnd{}, geo, d, out, st, loc, attn) == M2F_OK;
}

template <typename T>
int fwd_impl(const char* fn, const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc,
             const T* attn, const Dims& d, int im2col_step, T* out, hipStream_t st,
             const int64_t* host_shapes = nullptr) {
  int rc = check_dims(fn, value, shapes, lsi, loc, attn, d, im2col_step);
  if (rc) return rc;
  if (!out) return m2f::fail(M2F_EINVAL, "%s: null output", fn);
  bool done = false;
  if constexpr (std::is_same<T, float>::value) {
    if (fast_f32_ok(d, value, loc, out)) {
      if (launch_fwd_lds_unfused(fn, value, loc, attn, d, host_shapes, out, st)) rc = M2F_OK;
      else if (d.D == 32 && d.P == 4 && m2f::option(m2f::kOptMsdaFwdQuad, 1) != 0 &&
               static_cast<int64_t>(d.N) * d.S * d.M * d.D * 4 < (int64_t{1} << 31))
        rc = launch_fwd_q4(value, shapes, lsi, loc, attn, d, out, st);
      else rc = launch_fwd_vec(value, shapes, lsi, loc, attn, d, out, st);
      done = true;
    }
  }
  if (!done) rc = launch_fwd_generic<T>(value, shapes, lsi, loc, attn, d, out, st);
  if (rc) return rc;
  return m2f::check_launch(fn);
}

template <typename T>
int bwd_impl(const char* fn, const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc,
             const T* attn, const T* gout, const Dims& d, int im2col_step, const int64_t* host_shapes, T* gv,
             T* gl, T* ga, hipStream_t st) {
  int rc = check_dims(fn, value, shapes, lsi, loc, attn, d, im2col_step);
  if (rc) return rc;
  if (!gout || !gv || !gl || !ga) return m2f::fail(M2F_EINVAL, "%s: null gradient pointer", fn);
  const size_t gv_bytes = static_cast<size_t>(d.N) * d.S * d.M * d.D * sizeof(T);
  hipError_t e = m2f::zero_async(gv, gv_bytes, st);
  if (e != hipSuccess) return m2f::fail(M2F_ELAUNCH, "%s: memset grad_value: %s", fn, hipGetErrorString(e));
  bool done = false;
  if constexpr (std::is_same<T, float>::value) {
    if (fast_f32_ok(d, value, loc, gout) && m2f::aligned(gv, 16) && m2f::aligned(gl, 8)) {
      TileGeom geo;
      size_t lds;
      int threads;
      // the tiled kernel where it applies (encoder layout with host shapes), else the direct-atomic one
      if (m2f::option(m2f::kOptMsdaBwdTiled, 1) != 0 && make_tile_geom(d, host_shapes, geo, lds, threads))
        rc = launch_bwd_tiled(false, value, loc, attn, FrontEnd{}, gout, geo, lds, threads, d, gv, gl, ga,
                              m2f::option(m2f::kOptMsdaBwdOverlap, 1) != 0, DetBufs{}, st);
      else rc = launch_bwd_vec(value, shapes, lsi, loc, attn, gout, d, gv, gl, ga, st);
      done = true;
    }
  } else {
    (void)host_shapes;
  }
  if (!done) rc = launch_bwd_generic<T>(fn, value, shapes, lsi, loc, attn, gout, d, gv, gl, ga, st);
  if (rc) return rc;
  return m2f::check_launch(fn);
}

}  // namespace

extern "C" int m2f_msda_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const float* sampling_loc, const float* attn_weight, int batch, int spatial_size,
                                int num_heads, int channels, int num_levels, int num_query, int num_point,
                                int im2col_step, const int64_t* host_spatial_shapes, float* output, void* stream) {
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  return fwd_impl<float>("m2f_msda_fwd_f32", value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                         d, im2col_step, output, static_cast<hipStream_t>(stream), host_spatial_shapes);
}

extern "C" int m2f_msda_fwd_f64(const double* value, const int64_t* spatial_shapes,
                                const int64_t* level_start_index, const double* sampling_loc,
                                const double* attn_weight, int batch, int spatial_size, int num_heads, int channels,
                                int num_levels, int num_query, int num_point, int im2col_step,
                                const int64_t* host_spatial_shapes, double* output, void* stream) {
  (void)host_spatial_shapes;
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  return fwd_impl<double>("m2f_msda_fwd_f64", value, spatial_shapes, level_start_index, sampling_loc,
                          attn_weight, d, im2col_step, output, static_cast<hipStream_t>(stream));
}

extern "C" int m2f_msda_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                int num_query, int num_point, int im2col_step, const int64_t* host_spatial_shapes,
                                float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                                void* stream) {
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  return bwd_impl<float>("m2f_msda_bwd_f32", value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                         grad_output, d, im2col_step, host_spatial_shapes, grad_value, grad_sampling_loc,
                         grad_attn_weight, static_cast<hipStream_t>(stream));
}

extern "C" int m2f_msda_bwd_f64(const double* value, const int64_t* spatial_shapes,
                                const int64_t* level_start_index, const double* sampling_loc,
                                const double* attn_weight, const double* grad_output, int batch, int spatial_size,
                                int num_heads, int channels, int num_levels, int num_query, int num_point,
                                int im2col_step, const int64_t* host_spatial_shapes, double* grad_value,
                                double* grad_sampling_loc, double* grad_attn_weight, void* stream) {
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  return bwd_impl<double>("m2f_msda_bwd_f64", value, spatial_shapes, level_start_index, sampling_loc,
                          attn_weight, grad_output, d, im2col_step, host_spatial_shapes, grad_value,
                          grad_sampling_loc, grad_attn_weight, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------
// Fused front end C ABI
// ------------------------------------------------------------------------------------------------
namespace {

int64_t det_workspace_bytes(const Dims& d) {
  return static_cast<int64_t>(d.N) * d.S * d.M * d.D * 8 + 16;  // int64 grad_value accumulator + scale words
}

int fused_check(const char* fn, const float* value, const float* proj, int ld, const float* ref,
                const int64_t* host_shapes, const Dims& d, TileGeom& geo) {
  if (!value || !proj || !ref || !host_shapes) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (d.N <= 0 || d.S <= 0 || d.M <= 0 || d.Lq <= 0) return m2f::fail(M2F_EINVAL, "%s: non-positive size", fn);
  if (d.D != 32 || d.P != 4 || d.L < 1 || d.L > kTileMaxL)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: needs channels 32, points 4, 1..4 levels (got D=%d P=%d L=%d)", fn,
                     d.D, d.P, d.L);
  if (ld < d.M * d.L * d.P * 3 || (ld & 1))
    return m2f::fail(M2F_EINVAL, "%s: projection row stride %d (need even, >= %d)", fn, ld, d.M * d.L * d.P * 3);
  if (!m2f::aligned(value, 16) || !m2f::aligned(proj, 8) || !m2f::aligned(ref, 8))
    return m2f::fail(M2F_EINVAL, "%s: misaligned input", fn);
  int64_t total;
  switch (fill_levels(d, host_shapes, geo, total)) {
    case LevelFill::kBadShape: return m2f::fail(M2F_EINVAL, "%s: bad level shape", fn);
    case LevelFill::kBadTotal: return m2f::fail(M2F_EINVAL, "%s: sum of H*W (%lld) != spatial_size (%d)", fn,
                                                static_cast<long long>(total), d.S);
    case LevelFill::kOk: break;
  }
  return M2F_OK;
}

}  // namespace

static int fused_fwd(int hm, const char* fn, const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes, int batch,
                                      int spatial_size, int num_heads, int channels, int num_levels,
                                      int num_query, int num_point, float* output, void* stream) {
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  TileGeom geo;
  int rc = fused_check(fn, value, proj, proj_ld, ref, host_spatial_shapes, d, geo);
  if (rc) return rc;
  if (!output || !m2f::aligned(output, 16)) return m2f::fail(M2F_EINVAL, "%s: bad output", fn);
  const FrontEnd fe{proj, proj_ld, ref, ref_batch_stride, hm};
  hipStream_t st = static_cast<hipStream_t>(stream);
  // value and out hold N * Lq(=S) * M * 32 elements; 32-bit offsets when those fit
  const bool off32 = static_cast<int64_t>(d.N) * std::max(d.S, d.Lq) * d.M * d.D < (int64_t{1} << 31);
  // quad form: byte offsets in 32-bit int arithmetic (value bytes < 2^31)
  const bool boff31 = static_cast<int64_t>(d.N) * d.S * d.M * d.D * 4 < (int64_t{1} << 31);
  TileGeom lgeo;
  const bool windowed = fwd_windowed();
  const bool quad = m2f::option(m2f::kOptMsdaFwdQuad, 1) != 0, tiled = m2f::option(m2f::kOptMsdaFwdTiled, 1) != 0;
  if (windowed && m2f::option(m2f::kOptMsdaFwdPair, 0) != 0 && make_fwd_lds_geom(d, proj_ld, geo, lgeo, true)) {
    rc = launch_fused_fwd_pair(fn, value, fe, lgeo, d, output, st);
  } else if (windowed && make_fwd_lds_geom(d, proj_ld, geo, lgeo)) {
    rc = launch_fwd_lds(fn, value, fe, lgeo, d, output, st);
  } else if (boff31 && d.Lq == d.S && quad && tiled) {
    const int pb = m2f::option(m2f::kOptMsdaFwdPb, 2);  // points per load batch (1, 2 or 4)
    rc = launch_fused_fwd_q4(fn, value, fe, geo, d, pb == 1 ? 1 : pb >= 4 ? 4 : 2, output, st);
  } else {
    rc = launch_fused_fwd(fn, value, fe, geo, d, tiled && d.Lq == d.S, off32, output, st);
  }
  if (rc) return rc;
  return m2f::check_launch(fn);
}

extern "C" int m2f_msda_fused_bwd_workspace(const int64_t* host_spatial_shapes, int batch, int spatial_size,
                                            int num_heads, int channels, int num_levels, int num_point,
                                            int64_t* workspace_bytes) {
  const char* fn = "m2f_msda_fused_bwd_workspace";
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, spatial_size, num_point};
  if (!host_spatial_shapes || !workspace_bytes) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  TileGeom geo;
  size_t lds;
  int threads;
  if (!make_tile_geom(d, host_spatial_shapes, geo, lds, threads))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: needs the encoder layout", fn);
  // deterministic mode (msda_bwd_det): the int64 grad_value accumulator and two scale words; otherwise none
  *workspace_bytes = m2f::option(m2f::kOptMsdaBwdDet, 0) != 0 ? det_workspace_bytes(d) : 0;
  return m2f::ok();
}

static int fused_bwd(int hm, const char* fn, const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes,
                                      const float* grad_output, int batch, int spatial_size, int num_heads,
                                      int channels, int num_levels, int num_query, int num_point,
                                      float* grad_value, float* grad_proj, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  const Dims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  TileGeom geo0;
  int rc = fused_check(fn, value, proj, proj_ld, ref, host_spatial_shapes, d, geo0);
  if (rc) return rc;
  if (!grad_output || !grad_value || !grad_proj || !m2f::aligned(grad_output, 16) || !m2f::aligned(grad_value, 16))
    return m2f::fail(M2F_EINVAL, "%s: bad gradient pointer", fn);
  TileGeom geo;
  size_t lds;
  int threads;
  if (!make_tile_geom(d, host_spatial_shapes, geo, lds, threads))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: needs the encoder layout (num_query == spatial_size), value under 2 GiB "
                     "and levels under 2^24 pixels", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nval = static_cast<int64_t>(d.N) * d.S * d.M * d.D;
  const size_t gv_bytes = static_cast<size_t>(nval) * sizeof(float);
  hipError_t e = m2f::zero_async(grad_value, gv_bytes, st);
  if (e != hipSuccess) return m2f::fail(M2F_ELAUNCH, "%s: memset grad_value: %s", fn, hipGetErrorString(e));
  const FrontEnd fe{proj, proj_ld, ref, ref_batch_stride, hm};
  DetBufs det;
  if (m2f::option(m2f::kOptMsdaBwdDet, 0) != 0) {
    const int64_t need = det_workspace_bytes(d);
    if (!workspace || workspace_bytes < need || !m2f::aligned(workspace, 16))
      return m2f::fail(M2F_EINVAL, "%s: deterministic mode needs a 16-byte aligned workspace of %lld bytes "
                       "(m2f_msda_fused_bwd_workspace)", fn, static_cast<long long>(need));
    det.acc = static_cast<unsigned long long*>(workspace);
    det.scale = reinterpret_cast<unsigned*>(det.acc + nval);
    e = m2f::zero_async(workspace, static_cast<size_t>(need), st);
    if (e != hipSuccess) return m2f::fail(M2F_ELAUNCH, "%s: memset workspace: %s", fn, hipGetErrorString(e));
    const int64_t n4 = static_cast<int64_t>(d.N) * d.Lq * d.M * d.D / 4;  // grad_output (N, Lq, M*32) fp32
    launch_det_scale(grad_output, n4, det, st);
  }
  if ((rc = launch_bwd_tiled(true, value, nullptr, nullptr, fe, grad_output, geo, lds, threads, d, grad_value, grad_proj,
                             nullptr, m2f::option(m2f::kOptMsdaBwdOverlap, 1) != 0, det, st)))
    return rc;
  if (det.acc) launch_det_convert(det, nval, d.Lq, grad_value, st);
  return m2f::check_launch(fn);
}

extern "C" int m2f_msda_fused_fwd_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes, int batch,
                                      int spatial_size, int num_heads, int channels, int num_levels,
                                      int num_query, int num_point, float* output, void* stream) {
  return fused_fwd(0, "m2f_msda_fused_fwd_f32", value, proj, proj_ld, ref, ref_batch_stride, host_spatial_shapes,
                   batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, output, stream);
}

extern "C" int m2f_msda_fused_fwd_hm_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes, int batch,
                                      int spatial_size, int num_heads, int channels, int num_levels,
                                      int num_query, int num_point, float* output, void* stream) {
  return fused_fwd(1, "m2f_msda_fused_fwd_hm_f32", value, proj, proj_ld, ref, ref_batch_stride, host_spatial_shapes,
                   batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, output, stream);
}

extern "C" int m2f_msda_fused_bwd_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes,
                                      const float* grad_output, int batch, int spatial_size, int num_heads,
                                      int channels, int num_levels, int num_query, int num_point,
                                      float* grad_value, float* grad_proj, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  return fused_bwd(0, "m2f_msda_fused_bwd_f32", value, proj, proj_ld, ref, ref_batch_stride, host_spatial_shapes,
                   grad_output, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point,
                   grad_value, grad_proj, workspace, workspace_bytes, stream);
}

extern "C" int m2f_msda_fused_bwd_hm_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                                      int64_t ref_batch_stride, const int64_t* host_spatial_shapes,
                                      const float* grad_output, int batch, int spatial_size, int num_heads,
                                      int channels, int num_levels, int num_query, int num_point,
                                      float* grad_value, float* grad_proj, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  return fused_bwd(1, "m2f_msda_fused_bwd_hm_f32", value, proj, proj_ld, ref, ref_batch_stride, host_spatial_shapes,
                   grad_output, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point,
                   grad_value, grad_proj, workspace, workspace_bytes, stream);
}

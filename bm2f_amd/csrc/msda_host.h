// Host side shared by the MSDA files: the dims of a call, the level-geometry fill, and the launchers and geometry
// builders that each kernel-family file exposes to the dispatch file (msda.hip).  Internal.
//
// A kernel template is launched from the file that defines it.  A launcher takes dims and geometry that the entry
// point has validated, issues its kernel on `st` and returns M2F_OK, or the M2F status (message in last_error,
// in `fn`'s name) of what kept it from launching; the launch's own error is left to the entry point's
// m2f::check_launch, once per call.  Which launcher runs for which dims and options is msda.hip's business.
#pragma once

#include "common.h"
#include "msda_device.h"

namespace m2f_msda {

constexpr int kMaxLevels = 16;  // levels of the op-level (device spatial shapes) fp32 fast paths; more go generic

struct Dims {
  int N, S, M, D, L, Lq, P;
  int64_t npairs() const { return static_cast<int64_t>(N) * Lq * M; }
};

// The level part of a TileGeom (L, H, W, start, invW, invH; everything else zero) from host spatial shapes
// (d.L <= kTileMaxL).  `total` is the pixel count of the levels filled so far.
enum class LevelFill { kOk, kBadShape /* an H or W <= 0 */, kBadTotal /* sum of H*W != d.S */ };
inline LevelFill fill_levels(const Dims& d, const int64_t* host_shapes, TileGeom& geo, int64_t& total) {
  geo = TileGeom{};
  geo.L = d.L;
  total = 0;
  for (int l = 0; l < d.L; ++l) {
    geo.H[l] = static_cast<int>(host_shapes[2 * l]);
    geo.W[l] = static_cast<int>(host_shapes[2 * l + 1]);
    if (geo.H[l] <= 0 || geo.W[l] <= 0) return LevelFill::kBadShape;
    geo.start[l] = static_cast<int>(total);
    geo.invW[l] = 1.f / static_cast<float>(geo.W[l]);
    geo.invH[l] = 1.f / static_cast<float>(geo.H[l]);
    total += static_cast<int64_t>(geo.H[l]) * geo.W[l];
  }
  return total == d.S ? LevelFill::kOk : LevelFill::kBadTotal;
}

// workgroups of a kernel that runs one per (tile, head, image)
inline int64_t tile_blocks(const TileGeom& geo, const Dims& d) {
  return static_cast<int64_t>(geo.nty) * geo.ntx * d.M * d.N;
}

// ---- msda_generic.hip: any channel count in fp32 / fp64 (T), and the fp32 float4-per-lane kernels (D = 16, 32, 64)
template <typename T>
int launch_fwd_generic(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* attn,
                       const Dims& d, T* out, hipStream_t st);
template <typename T>
int launch_bwd_generic(const char* fn, const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc,
                       const T* attn, const T* gout, const Dims& d, T* gv, T* gl, T* ga, hipStream_t st);
int launch_fwd_vec(const float* value, const int64_t* shapes, const int64_t* lsi, const float* loc,
                   const float* attn, const Dims& d, float* out, hipStream_t st);
int launch_bwd_vec(const float* value, const int64_t* shapes, const int64_t* lsi, const float* loc,
                   const float* attn, const float* gout, const Dims& d, float* gv, float* gl, float* ga,
                   hipStream_t st);

// ---- msda_fwd_quad.hip: the forwards that gather from HBM (D = 32, P = 4)
// op-level quad forward (value bytes < 2^31, d.L <= kMaxLevels)
int launch_fwd_q4(const float* value, const int64_t* shapes, const int64_t* lsi, const float* loc, const float* attn,
                  const Dims& d, float* out, hipStream_t st);
// fused quad forward (encoder layout, value bytes < 2^31); pb: points per load batch, 1, 2 or 4
int launch_fused_fwd_q4(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                        int pb, float* out, hipStream_t st);
// fused 8-lane forward; tiled needs the encoder layout, off32 value / out elements < 2^31
int launch_fused_fwd(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                     bool tiled, bool off32, float* out, hipStream_t st);

// ---- msda_fwd_lds.hip: the forwards that stage value windows in LDS
// Geometry of the LDS-window forward (pair: of the two-lanes-per-query one) from `base`'s levels; false when the
// configuration does not qualify.
bool make_fwd_lds_geom(const Dims& d, int proj_ld, const TileGeom& base, TileGeom& geo, bool pair = false);
// the lane-quad kernel on make_fwd_lds_geom's geometry: fused (fe), or op-level when loc / attn are given
int launch_fwd_lds(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                   float* out, hipStream_t st, const float* loc = nullptr, const float* attn = nullptr);
int launch_fused_fwd_pair(const char* fn, const float* value, const FrontEnd& fe, const TileGeom& geo, const Dims& d,
                          float* out, hipStream_t st);

// ---- msda_bwd_tiled.hip: the spatially tiled fp32 backward
// Deterministic-mode buffers (msda_bwd_det): the int64 accumulator of grad_value and the scale words.
struct DetBufs {
  unsigned long long* acc = nullptr;
  unsigned* scale = nullptr;  // [max |g| bits, non-finite flag]
};
// Tile geometry, dynamic LDS bytes and workgroup size; false when the configuration does not qualify.
bool make_tile_geom(const Dims& d, const int64_t* host_shapes, TileGeom& geo, size_t& lds, int& threads);
// fused: samples from fe and gl = grad_proj (ga unused); else from loc / attn.  det.acc selects the deterministic
// kernel, otherwise `overlap` the merged phase-2/3 queue.
int launch_bwd_tiled(bool fused, const float* value, const float* loc, const float* attn, const FrontEnd& fe,
                     const float* gout, const TileGeom& geo, size_t lds, int threads, const Dims& d, float* gv,
                     float* gl, float* ga, bool overlap, const DetBufs& det, hipStream_t st);
// deterministic mode: the scale pass over grad_output (n4 float4s) before the kernel, the conversion pass after it
// (nothing keeps either from launching: no status)
void launch_det_scale(const float* gout, int64_t n4, const DetBufs& det, hipStream_t st);
void launch_det_convert(const DetBufs& det, int64_t nval, int Lq, float* gv, hipStream_t st);

}  // namespace m2f_msda

// Shared helpers for the libbm2f C ABI: per-thread error strings and launch checking.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "bm2f.h"

namespace m2f {

std::string& last_error();

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

inline int ok() {
  last_error().clear();
  return M2F_OK;
}

// Check the launch that was just issued on this thread (hipGetLastError clears the sticky state).
inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(M2F_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return ok();
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

inline unsigned ceil_div(int64_t a, int64_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// one of the three floating-point element types of the C ABI
inline bool is_float_dtype(int dtype) { return dtype == M2F_F32 || dtype == M2F_F16 || dtype == M2F_BF16; }

// Runtime value -> kernel template argument, once for every entry point.  f is a generic lambda that launches;
// it returns nothing and reports through what it captures.  The dispatch_* that can miss return false without
// calling f, and the caller answers with its own message.
template <typename T>
struct Tag { using type = T; };

template <typename F>
inline bool dispatch_half(int dtype, F&& f) {
  if (dtype == M2F_BF16) f(Tag<__bf16>{});
  else if (dtype == M2F_F16) f(Tag<_Float16>{});
  else return false;
  return true;
}

template <typename F>
inline bool dispatch_float(int dtype, F&& f) {
  if (dtype == M2F_F32) f(Tag<float>{});
  else return dispatch_half(dtype, f);
  return true;
}

template <typename F>
inline void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// K = v for v in Ks..., else no call
template <int... Ks, typename F>
inline bool dispatch_one_of(int v, F&& f) {
  return ((v == Ks && (f(std::integral_constant<int, Ks>{}), true)) || ...);
}

// K = v for LO <= v < HI; every other v takes HI, as the `default:` of a switch over a level count did
template <int LO, int HI, typename F>
inline void dispatch_int(int v, F&& f) {
  if constexpr (LO < HI) {
    if (v == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_int<LO + 1, HI>(v, f);
  } else {
    f(std::integral_constant<int, HI>{});
  }
}

// nb workgroups as a 1-D grid: a count that the grid cannot hold is refused in fn's name
inline int grid_1d(int64_t nb, const char* fn, unsigned* grid) {
  if (nb > 0x7fffffff) return fail(M2F_EUNSUPPORTED, "%s: too many workgroups", fn);
  *grid = static_cast<unsigned>(nb);
  return M2F_OK;
}

// Explicit tuning options (m2f_set_option, include/bm2f.h): geometry and engine overrides for tests and
// tools.  The library never reads the environment; an unset option means the built-in default.  Every
// option changes the partition or the kernel variant only, never the arithmetic's result.
// The one list of options: X(enumerator, "name").  enum Option below and the name table of library.hip both
// come from it, so a new option is one line here.
#define M2F_OPTIONS(X)                                                                                          \
  X(kOptMsdaThreads, "msda_threads") X(kOptMsdaTile, "msda_tile") X(kOptMsdaTileW, "msda_tile_w")               \
  X(kOptMsdaHalo, "msda_halo") X(kOptMsdaWinRows, "msda_win_rows") X(kOptMsdaBwdTiled, "msda_bwd_tiled")        \
  X(kOptMsdaFwdTiled, "msda_fwd_tiled") X(kOptMattnDqAtomic, "mattn_dq_atomic") X(kOptGemmNtCfg, "gemm_nt_cfg") \
  X(kOptX3TnNw, "x3_tn_nw") X(kOptX3TnBlocks, "x3_tn_blocks") X(kOptX3NtCfg, "x3_nt_cfg")                       \
  X(kOptMsdaFwdQuad, "msda_fwd_quad") X(kOptMsdaBwdOverlap, "msda_bwd_overlap") X(kOptMsdaBwdDet, "msda_bwd_det") \
  X(kOptMsdaFwdPb, "msda_fwd_pb") X(kOptMsdaBwdRatio, "msda_bwd_ratio") X(kOptMsdaFwdLds, "msda_fwd_lds")       \
  X(kOptMsdaFwdTile, "msda_fwd_tile") X(kOptMsdaFwdTileW, "msda_fwd_tile_w") X(kOptMsdaFwdCap, "msda_fwd_cap")  \
  X(kOptMsdaFwdHalo, "msda_fwd_halo") X(kOptMattnFwdMinblk, "mattn_fwd_minblk")                                 \
  X(kOptMattnBwdMinblk, "mattn_bwd_minblk") X(kOptMaskDfStage, "mask_df_stage")                                 \
  X(kOptMattnBwdKeys, "mattn_bwd_keys") X(kOptMattnXcd, "mattn_xcd") X(kOptMattnCombine, "mattn_combine")       \
  X(kOptMsdaBwdRowSort, "msda_bwd_rowsort") X(kOptMsdaBwdWalk4, "msda_bwd_walk4") X(kOptMsdaFwdXcd, "msda_fwd_xcd") \
  X(kOptMsdaFwdPair, "msda_fwd_pair") X(kOptInferVideoCap, "infer_video_cap")
enum Option : int {
#define M2F_OPTION_ENUM(id, name) id,
  M2F_OPTIONS(M2F_OPTION_ENUM)
#undef M2F_OPTION_ENUM
  kOptCount
};
int64_t option_raw(Option o);  // -1 when unset

// Zero `bytes` bytes at p on stream st with a kernel, not hipMemsetAsync: on this ROCm a memset captured in a HIP
// graph is not re-run correctly when the graph is replayed (tools/graph_memset_check.py), and callers capture the
// library's launches in graphs (bench_model.GraphStep).  Returns a HIP error code.
hipError_t zero_async(void* p, size_t bytes, hipStream_t st);
// The same for a rows x cols fp32 matrix at row stride ld floats (a kernel: no memset node in a captured graph).
hipError_t zero2d_f32_async(float* p, int64_t ld, int64_t cols, int64_t rows, hipStream_t st);
// Raise `kernel`'s dynamic-LDS limit to `bytes` on the current device, once per (kernel, device, bytes) and
// thread-safe; returns M2F_OK or an M2F_ELAUNCH status (with the HIP error in last_error) naming `fn`.
int set_max_lds(const void* kernel, int bytes, const char* fn);
inline int option(Option o, int dflt) {
  const int64_t v = option_raw(o);
  return v < 0 ? dflt : static_cast<int>(v);
}

}  // namespace m2f

// Shifted-window attention of the Swin block (reference backbone/swin.py:131-171, :257-284): everything between the
// qkv linear and the proj linear in one forward and one backward kernel.
//
//   qkv  (B, Hp, Wp, 3C)  [q | k | v], each nH x 32, as nn.Linear(C, 3C) writes it       fp32 / fp16 / bf16
//   out  (B, Hp, Wp, C)   unshifted, unpartitioned, read by proj as it is
//   lse  (B, nH, Hp*Wp)   fp32 log-sum-exp of every query row (all the forward saves)
//
// The cyclic shift, the window partition and their inverses are addresses: token t = (ty, tx) of window (wy, wx) is
// the pixel ((wy*ws + ty + shift) mod Hp, (wx*ws + tx + shift) mod Wp).  The relative-position bias is gathered from
// the ((2ws-1)^2, nH) table with rel computed from the (ty, tx) pairs, and the shift mask (-100 where the nine-region
// labels of :416-440 differ) from the shifted coordinates; no (nW, N, N) tensor exists.
//
// Work distribution: one workgroup per (image, window, head), one wave per 16-token tile of the window (NT = ceil(N /
// 16) waves, N = ws^2 <= 144).  A wave computes the transposed score tile S^T = K Q^T, so the MFMA result has its
// query on the lane (col = lane & 15) and 4 keys per tile in the registers (row = 4 (lane >> 4) + r): the softmax is
// per lane plus two shuffles, and the tile is the next MFMA's B operand (contraction over keys) without any lane
// movement -- the contraction index is only summed over, so slot (g, j) of the 16x16x32 form takes key 4g + j of the
// even tile (j < 4) or of the odd tile (j >= 4), and the A operand (V^T, keys contiguous in LDS) is read to match.
// fp32 I/O runs the same structure on the exact fp32 MFMA (16x16x4), whose one-element operands need no transposed
// image.  DESIGN.md section 3 "Shifted-window attention" has the LDS / VGPR budget.
#include "common.h"
#include "device_util.h"

#include <type_traits>

namespace {

using m2f::bf8, m2f::f4, m2f::h8, m2f::s4, m2f::s8;
using u4 = unsigned __attribute__((ext_vector_type(4)));
using i4 = int __attribute__((ext_vector_type(4)));

constexpr int kD = 32;        // head dim of every Swin variant
constexpr int kMinWs = 2, kMaxWs = 12;
constexpr float kMasked = -100.0f;   // swin.py:438, not -inf: no row is ever fully masked

// device_util.h's element traits (k16) plus this file's LDS layout
template <typename T> struct WinElt : m2f::Elt<T> {
  using m2f::Elt<T>::k16;
  // row pitch (elements) of a row-major (token, 32) LDS image: 80 B (16-bit) / 144 B (fp32) rows keep the 16-byte
  // alignment of the staging stores and spread the 16 rows a fragment read touches over the banks
  static constexpr int KS = k16 ? 40 : 36;
  static constexpr int EPC = 16 / sizeof(T);   // elements per 16-byte chunk
  static constexpr int CPR = kD / EPC;         // chunks per row
};

struct Geo {
  int B, nH, Hp, Wp, ws, shift, nWy, nWx;
};

// sizes shared by host and device ------------------------------------------------------------------------------------
__host__ __device__ inline int pad32(int n) { return (n + 31) & ~31; }
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int tiles_of(int ws) { return (ws * ws + 15) / 16; }
// pitch (elements) of a transposed (32, token) 16-bit image: NP + 4 keeps the 8-byte alignment of the fragment reads
// and puts the 16 rows of a read on distinct bank pairs
__host__ __device__ inline int tpitch(int NP) { return NP + 4; }

template <typename T> __host__ __device__ inline int rowmajor_elems(int NP) { return NP * WinElt<T>::KS; }
template <typename T> __host__ __device__ inline int trans_elems(int NP) { return WinElt<T>::k16 ? kD * tpitch(NP) : 0; }
// bias table (floats), then token codes and pixel offsets (ints)
__host__ __device__ inline int small_words(int ws, int NP) { return pad4((2 * ws - 1) * (2 * ws - 1)) + 2 * NP; }

template <typename T> inline size_t fwd_lds_bytes(int ws) {
  const int NP = pad32(ws * ws);
  return static_cast<size_t>(rowmajor_elems<T>(NP) + (WinElt<T>::k16 ? trans_elems<T>(NP) : rowmajor_elems<T>(NP))) *
             sizeof(T) + static_cast<size_t>(small_words(ws, NP)) * 4;
}
// backward: phase A holds K, V (row-major), K^T and the per-wave table-gradient bins; phase B reuses the space for
// Q, dO (row-major), Q^T and dO^T; the per-row D and lse (2 NP floats) live beside the small tables through both
template <typename T> __host__ __device__ inline int bwd_big_bytes(int ws) {
  const int NP = pad32(ws * ws), TBp = pad4((2 * ws - 1) * (2 * ws - 1));
  const int a = (2 * rowmajor_elems<T>(NP) + trans_elems<T>(NP)) * static_cast<int>(sizeof(T)) + tiles_of(ws) * TBp * 4;
  const int b = (2 * rowmajor_elems<T>(NP) + 2 * trans_elems<T>(NP)) * static_cast<int>(sizeof(T));
  return a > b ? a : b;
}
template <typename T> inline size_t bwd_lds_bytes(int ws) {
  const int NP = pad32(ws * ws);
  return static_cast<size_t>(bwd_big_bytes<T>(ws)) + static_cast<size_t>(small_words(ws, NP) + 2 * NP) * 4;
}

// operands -----------------------------------------------------------------------------------------------------------
// One row's 32 channels as the operand of a contraction over the head dimension.  16-bit: elements 8g .. 8g+7 (one
// 16x16x32 MFMA); fp32: elements 4kk + g, kk = 0..7 (eight 16x16x4 MFMAs).
template <typename T> struct Frag {
  s8 v;
  __device__ __forceinline__ void load(const T* row, int g) { v = *reinterpret_cast<const s8*>(row + 8 * g); }
};
template <> struct Frag<float> {
  float v[8];
  __device__ __forceinline__ void load(const float* row, int g) {
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) v[kk] = row[4 * kk + g];
  }
};

template <typename T> __device__ __forceinline__ f4 mma_k32(s8 a, s8 b, f4 c) {
  if constexpr (std::is_same<T, _Float16>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}

// c[4g + r][lane & 15] += sum_d a_row(lane & 15)[d] * b_row(lane & 15)[d]  (a's rows down, b's rows across)
template <typename T> __device__ __forceinline__ f4 mma_d(const Frag<T>& a, const Frag<T>& b, f4 c) {
  if constexpr (WinElt<T>::k16) {
    return mma_k32<T>(a.v, b.v, c);
  } else {
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[kk], b.v[kk], c, 0, 0, 0);
    return c;
  }
}

template <typename T> __device__ __forceinline__ s8 pack8(f4 lo, f4 hi) {
  if constexpr (std::is_same<T, _Float16>::value) {
    h8 p = {static_cast<_Float16>(lo[0]), static_cast<_Float16>(lo[1]), static_cast<_Float16>(lo[2]),
            static_cast<_Float16>(lo[3]), static_cast<_Float16>(hi[0]), static_cast<_Float16>(hi[1]),
            static_cast<_Float16>(hi[2]), static_cast<_Float16>(hi[3])};
    return __builtin_bit_cast(s8, p);
  } else {
    bf8 p = {static_cast<__bf16>(lo[0]), static_cast<__bf16>(lo[1]), static_cast<__bf16>(lo[2]),
            static_cast<__bf16>(lo[3]), static_cast<__bf16>(hi[0]), static_cast<__bf16>(hi[1]),
            static_cast<__bf16>(hi[2]), static_cast<__bf16>(hi[3])};
    return __builtin_bit_cast(s8, p);
  }
}

// Contraction over the window's tokens of X, NT result tiles of mma_d (token 16t + 4g + r in register r of tile t,
// the other index on the lane):  o0[4g + r][lane & 15] += sum_tok M[tok][4g' ...] -- i.e. o0 = M[:, 0:16]^T X and
// o1 = M[:, 16:32]^T X.  16-bit reads M^T (`img` = the transposed image, pitch `ld`); fp32 reads the row-major image.
template <typename T, int NT>
__device__ __forceinline__ void mma_tok(const T* img, int ld, const f4 (&X)[NT], f4& o0, f4& o1, int r16, int g) {
  if constexpr (WinElt<T>::k16) {
#pragma unroll
    for (int c = 0; c < (NT + 1) / 2; ++c) {
      const f4 zero = {0.f, 0.f, 0.f, 0.f};
      const f4 x1 = (2 * c + 1 < NT) ? X[(2 * c + 1 < NT) ? 2 * c + 1 : 0] : zero;
      const s8 b = pack8<T>(X[2 * c], x1);
      const T* a0 = img + r16 * ld + 32 * c + 4 * g;
      const T* a1 = a0 + 16 * ld;
      const s8 f0 = __builtin_shufflevector(*reinterpret_cast<const s4*>(a0), *reinterpret_cast<const s4*>(a0 + 16),
                                            0, 1, 2, 3, 4, 5, 6, 7);
      const s8 f1 = __builtin_shufflevector(*reinterpret_cast<const s4*>(a1), *reinterpret_cast<const s4*>(a1 + 16),
                                            0, 1, 2, 3, 4, 5, 6, 7);
      o0 = mma_k32<T>(f0, b, o0);
      o1 = mma_k32<T>(f1, b, o1);
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = img + (16 * t + 4 * g + r) * ld;
        o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(row[r16], X[t][r], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 + r16], X[t][r], o1, 0, 0, 0);
      }
    }
  }
}

// four consecutive channels of one token
template <typename T> __device__ __forceinline__ void store4(T* p, f4 v) {
  if constexpr (WinElt<T>::k16) {
    const s8 q = pack8<T>(v, v);
    *reinterpret_cast<s4*>(p) = __builtin_shufflevector(q, q, 0, 1, 2, 3);
  } else {
    *reinterpret_cast<f4*>(p) = v;
  }
}

__device__ __forceinline__ float wave_max4(float x) {   // over the four 16-lane groups
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float wave_sum4(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// tables of one window: sPos[t] = pixel offset row * Wp + col of token t, sTok[t] = (ty * (2ws-1) + tx) | region <<
// 16, sBias = this head's column of the table.  Tokens N .. NP-1 repeat token N-1 (in range, never stored) and carry
// the sign bit, which tail_pen turns into a -inf score: the tail is excluded by data, with no per-element compare
// (compares of 16t + 4g + r against N are the same in every phase, and kept as lane masks they spill SGPRs).
__device__ __forceinline__ float tail_pen(int tok) { return __int_as_float((tok >> 31) & static_cast<int>(0xff800000u)); }
// -100 where the two tokens' region labels differ, else 0, in integer arithmetic (no lane mask): the differing region
// bits negated have the sign bit set, which an arithmetic shift spreads over the bit pattern of -100.0f
__device__ __forceinline__ float region_pen(int tok_a, int tok_b) {
  const int x = (tok_a ^ tok_b) & 0x000f0000;
  return __int_as_float(((0 - x) >> 31) & __float_as_int(kMasked));
}
__device__ __forceinline__ void window_tables(const Geo& G, int wy, int wx, int h, const float* __restrict__ table,
                                              float* sBias, int* sTok, int* sPos, int NP) {
  const int ws = G.ws, N = ws * ws, TW = 2 * ws - 1;
  for (int j = threadIdx.x; j < NP; j += blockDim.x) {
    const int jj = j < N ? j : N - 1;
    const int ty = jj / ws, tx = jj - ty * ws;
    const int ys = wy * ws + ty, xs = wx * ws + tx;   // coordinates in the shifted map
    int row = ys + G.shift, col = xs + G.shift;
    if (row >= G.Hp) row -= G.Hp;
    if (col >= G.Wp) col -= G.Wp;
    int region = 0;
    if (G.shift > 0) {
      const int ry = ys < G.Hp - ws ? 0 : (ys < G.Hp - G.shift ? 1 : 2);
      const int rx = xs < G.Wp - ws ? 0 : (xs < G.Wp - G.shift ? 1 : 2);
      region = ry * 3 + rx;
    }
    sPos[j] = row * G.Wp + col;
    sTok[j] = (ty * TW + tx) | (region << 16) | (j < N ? 0 : static_cast<int>(0x80000000u));
  }
  for (int x = threadIdx.x; x < TW * TW; x += blockDim.x) sBias[x] = table[static_cast<int64_t>(x) * G.nH + h];
}

// Stage 32 channels of every token of the window (src + pos * stride) as a row-major image and, for 16-bit with
// `trans`, a transposed one; tokens N .. NP-1 are zeros.
template <typename T>
__device__ __forceinline__ void stage(const T* __restrict__ src, int64_t stride, const int* sPos, int N, int NP,
                                      T* rowmajor, T* trans) {
  constexpr int EPC = WinElt<T>::EPC, CPR = WinElt<T>::CPR, KS = WinElt<T>::KS;
  const int TS = tpitch(NP);
  for (int c = threadIdx.x; c < NP * CPR; c += blockDim.x) {
    const int j = c / CPR, ch = c - j * CPR;
    u4 v = {0u, 0u, 0u, 0u};
    if (j < N) v = *reinterpret_cast<const u4*>(src + sPos[j] * stride + ch * EPC);
    if (rowmajor) *reinterpret_cast<u4*>(rowmajor + j * KS + ch * EPC) = v;
    if constexpr (WinElt<T>::k16) {
      if (trans) {
        const s8 e = __builtin_bit_cast(s8, v);
#pragma unroll
        for (int u = 0; u < 8; ++u) reinterpret_cast<short*>(trans)[(ch * 8 + u) * TS + j] = e[u];
      }
    }
  }
}

struct Block {
  int b, wy, wx, h;
};
__device__ __forceinline__ Block decode_block(const Geo& G) {
  Block k;
  int w = blockIdx.x;
  k.h = w % G.nH;
  w /= G.nH;
  k.wx = w % G.nWx;
  w /= G.nWx;
  k.wy = w % G.nWy;
  k.b = w / G.nWy;
  return k;
}

// forward ------------------------------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(64 * NT) void wattn_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ table,
                                                            T* __restrict__ out, float* __restrict__ lse, Geo G,
                                                            float scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int KS = WinElt<T>::KS;
  const int ws = G.ws, N = ws * ws, NP = pad32(N), TW = 2 * ws - 1, C = G.nH * kD;
  T* sK = reinterpret_cast<T*>(smem);
  T* sV = sK + rowmajor_elems<T>(NP);   // 16-bit: V^T (32, tpitch); fp32: V row-major
  float* sBias = reinterpret_cast<float*>(sV + (WinElt<T>::k16 ? trans_elems<T>(NP) : rowmajor_elems<T>(NP)));
  int* sTok = reinterpret_cast<int*>(sBias + pad4(TW * TW));
  int* sPos = sTok + NP;

  const Block k = decode_block(G);
  const int64_t img = static_cast<int64_t>(k.b) * G.Hp * G.Wp;
  const T* base = qkv + img * 3 * C + k.h * kD;
  window_tables(G, k.wy, k.wx, k.h, table, sBias, sTok, sPos, NP);
  __syncthreads();
  stage<T>(base + C, 3 * C, sPos, N, NP, sK, nullptr);
  if constexpr (WinElt<T>::k16) stage<T>(base + 2 * C, 3 * C, sPos, N, NP, nullptr, sV);
  else stage<T>(base + 2 * C, 3 * C, sPos, N, NP, sV, nullptr);
  __syncthreads();

  const int qt = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
  const int iq = 16 * qt + r16;
  const bool valid = iq < N;
  const int iqc = valid ? iq : N - 1;
  const int posq = sPos[iqc], tokq = sTok[iqc];
  const int aq = (tokq & 0xffff) + (ws - 1) * TW + (ws - 1);
  Frag<T> fq;
  fq.load(base + static_cast<int64_t>(posq) * 3 * C, g);

  f4 S[NT];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    Frag<T> fk;
    fk.load(sK + (16 * t + r16) * KS, g);
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    S[t] = mma_d<T>(fk, fq, zero);
    const i4 tk = *reinterpret_cast<const i4*>(sTok + 16 * t + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // tail keys get -inf and take no part in the softmax
      const float s = S[t][r] * scale + sBias[aq - (tk[r] & 0xffff)] + region_pen(tk[r], tokq) +
                      tail_pen(tk[r]);
      S[t][r] = s;
      m = fmaxf(m, s);
    }
  }
  m = wave_max4(m);
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __expf(S[t][r] - m);
      S[t][r] = p;
      l += p;
    }
  l = wave_sum4(l);
  f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
  mma_tok<T, NT>(sV, WinElt<T>::k16 ? tpitch(NP) : KS, S, o0, o1, r16, g);
  if (valid) {   // tail query rows are not stored
    const float inv = 1.f / l;
    T* o = out + (img + posq) * C + k.h * kD + 4 * g;
    store4<T>(o, o0 * inv);
    store4<T>(o + 16, o1 * inv);
    if (g == 0) lse[(static_cast<int64_t>(k.b) * G.nH + k.h) * G.Hp * G.Wp + posq] = m + __logf(l);
  }
}

// backward -----------------------------------------------------------------------------------------------------------
// Phase A, a wave per query tile (transposed tiles, query on the lane): P and dP = V dO^T recomputed, D = rowsum(P dP),
// dS = P (dP - D), dQ = scale dS K, and dS added into this wave's (2ws-1)^2 table-gradient bins.  Phase B, a wave per
// key tile (key on the lane): P and dS recomputed, dV = P^T dO, dK = scale dS^T Q.  Every dqkv element has one owner.
//
// Table-gradient bins without atomics: within one register (t, r) the 16 lanes of a group g share the key and differ
// in the query, so their bins differ; the four groups take turns in a loop, each turn fenced (see the loop).  The
// per-wave bins are then summed wave 0, 1, ... into part[block].
template <typename T, int NT>
__global__ __launch_bounds__(64 * NT) void wattn_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ table,
                                                            const T* __restrict__ dout, const float* __restrict__ lse,
                                                            T* __restrict__ dqkv, float* __restrict__ part, Geo G,
                                                            float scale) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int KS = WinElt<T>::KS;
  constexpr bool k16 = WinElt<T>::k16;
  const int ws = G.ws, N = ws * ws, NP = pad32(N), TW = 2 * ws - 1, TB = TW * TW, TBp = pad4(TB), C = G.nH * kD;
  const int TS = tpitch(NP), RM = rowmajor_elems<T>(NP), TR = trans_elems<T>(NP);
  // phase A                      phase B
  T* sK = reinterpret_cast<T*>(smem);          // Q
  T* sV = sK + RM;                             // dO
  T* sKt = sV + RM;                            // Q^T   (16-bit only)
  float* sBins = reinterpret_cast<float*>(sKt + TR);   // dO^T starts here in phase B
  T* sdOt = sKt + TR;
  float* sBias = reinterpret_cast<float*>(smem + bwd_big_bytes<T>(ws));
  int* sTok = reinterpret_cast<int*>(sBias + TBp);
  int* sPos = sTok + NP;
  float* sD = reinterpret_cast<float*>(sPos + NP);
  float* sL = sD + NP;

  const Block k = decode_block(G);
  const int64_t img = static_cast<int64_t>(k.b) * G.Hp * G.Wp;
  const T* base = qkv + img * 3 * C + k.h * kD;
  const T* dbase = dout + img * C + k.h * kD;
  T* gbase = dqkv + img * 3 * C + k.h * kD;
  const float* lbase = lse + (static_cast<int64_t>(k.b) * G.nH + k.h) * G.Hp * G.Wp;
  window_tables(G, k.wy, k.wx, k.h, table, sBias, sTok, sPos, NP);
  for (int x = threadIdx.x; x < NT * TBp; x += blockDim.x) sBins[x] = 0.f;
  __syncthreads();
  stage<T>(base + C, 3 * C, sPos, N, NP, sK, k16 ? sKt : nullptr);
  stage<T>(base + 2 * C, 3 * C, sPos, N, NP, sV, nullptr);
  __syncthreads();

  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
  const int relc = (ws - 1) * TW + (ws - 1);
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  {
    const int iq = 16 * wv + r16;
    const bool valid = iq < N;
    const int iqc = valid ? iq : N - 1;
    const int posq = sPos[iqc], tokq = sTok[iqc];
    const int aq = (tokq & 0xffff) + relc;
    Frag<T> fq, fdo;
    fq.load(base + static_cast<int64_t>(posq) * 3 * C, g);
    fdo.load(dbase + static_cast<int64_t>(posq) * C, g);
    // a tail query row takes lse = +inf, so that every probability of the row is exp(-inf) = 0, here and in phase B
    const float lq = valid ? lbase[posq] : INFINITY;
    f4 P[NT], dP[NT];
    float dsum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      Frag<T> fk, fv;
      fk.load(sK + (16 * t + r16) * KS, g);
      fv.load(sV + (16 * t + r16) * KS, g);
      P[t] = mma_d<T>(fk, fq, zero);
      dP[t] = mma_d<T>(fv, fdo, zero);
      const i4 tk = *reinterpret_cast<const i4*>(sTok + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = P[t][r] * scale + sBias[aq - (tk[r] & 0xffff)] + region_pen(tk[r], tokq) +
                        tail_pen(tk[r]);
        const float p = __expf(s - lq);   // tail keys and tail queries: exp(-inf) = 0
        P[t][r] = p;
        dsum += p * dP[t][r];
      }
    }
    dsum = wave_sum4(dsum);
    float* bins = sBins + wv * TBp;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dP[t][r] = P[t][r] * (dP[t][r] - dsum);   // dS (0 at tail keys and tail queries)
    // The four lane groups add their dS into the wave's bins one group at a time.  Correctness rests on two things:
    // inside a turn no two active lanes touch one bin in the same instruction (same key, different queries), and a
    // turn's writes are complete before the next turn's reads.  The second is made explicit, not left to the
    // scheduler.  Tail keys repeat token N-1's code and carry dS = 0 exactly, so they need no predicate: within a
    // turn they too are one key against different queries.  The turn loop is a real loop (never unrolled or merged,
    // although g is provably 0..3), and each turn ends with a wavefront-scope release fence (the LDS writes are
    // waited for) and a wave barrier.  Inside a turn a lane's read-modify-writes stay in program order because the
    // bin indices come from LDS and may alias.
#pragma unroll 1
    for (int turn = 0; turn < 4; ++turn) {
      if (g == turn && valid) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const i4 tk = *reinterpret_cast<const i4*>(sTok + 16 * t + 4 * turn);
#pragma unroll
          for (int r = 0; r < 4; ++r) bins[aq - (tk[r] & 0xffff)] += dP[t][r];   // tail keys add their exact 0
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    f4 o0 = zero, o1 = zero;
    mma_tok<T, NT>(k16 ? sKt : sK, k16 ? TS : KS, dP, o0, o1, r16, g);
    if (valid) {
      T* o = gbase + static_cast<int64_t>(posq) * 3 * C + 4 * g;
      store4<T>(o, o0 * scale);
      store4<T>(o + 16, o1 * scale);
    }
    if (g == 0) {
      sD[iq] = dsum;
      sL[iq] = lq;
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < TB; x += blockDim.x) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < NT; ++w) acc += sBins[w * TBp + x];
    part[static_cast<int64_t>(blockIdx.x) * TB + x] = acc;
  }
  __syncthreads();
  stage<T>(base, 3 * C, sPos, N, NP, sK, k16 ? sKt : nullptr);
  stage<T>(dbase, C, sPos, N, NP, sV, k16 ? sdOt : nullptr);
  __syncthreads();
  {
    const int jk = 16 * wv + r16;
    const bool valid = jk < N;
    const int jkc = valid ? jk : N - 1;
    const int posk = sPos[jkc], tokk = sTok[jkc];
    const int ak = relc - (tokk & 0xffff);
    const float kpen = valid ? 0.f : -INFINITY;   // a tail key column: every probability exp(-inf) = 0
    Frag<T> fk, fv;
    fk.load(base + static_cast<int64_t>(posk) * 3 * C + C, g);
    fv.load(base + static_cast<int64_t>(posk) * 3 * C + 2 * C, g);
    f4 P[NT], dS[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      Frag<T> fq, fdo;
      fq.load(sK + (16 * t + r16) * KS, g);
      fdo.load(sV + (16 * t + r16) * KS, g);
      P[t] = mma_d<T>(fq, fk, zero);
      dS[t] = mma_d<T>(fdo, fv, zero);
      const i4 tq = *reinterpret_cast<const i4*>(sTok + 16 * t + 4 * g);
      const f4 lq = *reinterpret_cast<const f4*>(sL + 16 * t + 4 * g);
      const f4 dq = *reinterpret_cast<const f4*>(sD + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = P[t][r] * scale + sBias[(tq[r] & 0xffff) + ak] + region_pen(tq[r], tokk) +
                        kpen;
        const float p = __expf(s - lq[r]);   // tail queries carry lse = +inf: exp(-inf) = 0
        P[t][r] = p;
        dS[t][r] = p * (dS[t][r] - dq[r]);
      }
    }
    f4 v0 = zero, v1 = zero, k0 = zero, k1 = zero;
    mma_tok<T, NT>(k16 ? sdOt : sV, k16 ? TS : KS, P, v0, v1, r16, g);
    mma_tok<T, NT>(k16 ? sKt : sK, k16 ? TS : KS, dS, k0, k1, r16, g);
    if (valid) {
      T* o = gbase + static_cast<int64_t>(posk) * 3 * C + C + 4 * g;
      store4<T>(o, k0 * scale);
      store4<T>(o + 16, k1 * scale);
      store4<T>(o + C, v0);
      store4<T>(o + C + 16, v1);
    }
  }
}

// dtable[x, h] = sum over (image, window) of part[(image, window), h, x], in a fixed order: eight contiguous segments
// of the window list summed in sequence each, then the eight sums added 0, 1, ...
constexpr int kSeg = 8;
__global__ __launch_bounds__(64 * kSeg) void wattn_dtable_kernel(const float* __restrict__ part,
                                                                 float* __restrict__ dtable, int nwin, int nH, int TB) {
  __shared__ float acc[kSeg][64];
  const int xl = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + xl, h = blockIdx.y;
  const int per = (nwin + kSeg - 1) / kSeg;
  const int w0 = seg * per, w1 = min(nwin, w0 + per);
  float a = 0.f;
  if (x < TB)
    for (int w = w0; w < w1; ++w) a += part[(static_cast<int64_t>(w) * nH + h) * TB + x];
  acc[seg][xl] = a;
  __syncthreads();
  if (seg == 0 && x < TB) {
    float s = acc[0][xl];
#pragma unroll
    for (int i = 1; i < kSeg; ++i) s += acc[i][xl];
    dtable[static_cast<int64_t>(x) * nH + h] = s;
  }
}

// host ---------------------------------------------------------------------------------------------------------------
int check_geometry(const char* fn, int batch, int heads, int head_dim, int hp, int wp, int ws, int shift) {
  if (batch < 0 || heads <= 0 || hp <= 0 || wp <= 0)
    return m2f::fail(M2F_EINVAL, "%s: bad sizes (batch %d, heads %d, grid %d x %d)", fn, batch, heads, hp, wp);
  if (ws < kMinWs || ws > kMaxWs)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: window size %d outside [%d, %d]", fn, ws, kMinWs, kMaxWs);
  if (head_dim != kD) return m2f::fail(M2F_EUNSUPPORTED, "%s: head_dim %d (only %d is built)", fn, head_dim, kD);
  if (hp % ws != 0 || wp % ws != 0)
    return m2f::fail(M2F_EINVAL, "%s: grid %d x %d is not a multiple of the window size %d", fn, hp, wp, ws);
  if (shift < 0 || shift >= ws) return m2f::fail(M2F_EINVAL, "%s: shift %d outside [0, %d)", fn, shift, ws);
  if (static_cast<int64_t>(batch) * (hp / ws) * (wp / ws) * heads > 0x7fffffffLL ||
      static_cast<int64_t>(hp) * wp > 0x7fffffffLL)
    return m2f::fail(M2F_EUNSUPPORTED, "%s: too many windows for one launch", fn);
  return M2F_OK;
}

Geo make_geo(int batch, int heads, int hp, int wp, int ws, int shift) {
  return Geo{batch, heads, hp, wp, ws, shift, hp / ws, wp / ws};
}

template <typename T, int NT>
int launch_fwd(const void* qkv, const float* table, void* out, float* lse, const Geo& G, float scale, hipStream_t st) {
  const size_t lds = fwd_lds_bytes<T>(G.ws);
  const unsigned blocks = static_cast<unsigned>(G.B) * G.nWy * G.nWx * G.nH;
  wattn_fwd_kernel<T, NT><<<blocks, 64 * NT, lds, st>>>(static_cast<const T*>(qkv), table, static_cast<T*>(out), lse, G,
                                                        scale);
  return m2f::check_launch("m2f_window_attn_fwd");
}

template <typename T, int NT>
int launch_bwd(const void* qkv, const float* table, const void* dout, const float* lse, void* dqkv, float* part,
               const Geo& G, float scale, hipStream_t st) {
  const size_t lds = bwd_lds_bytes<T>(G.ws);
  if (int rc = m2f::set_max_lds(reinterpret_cast<const void*>(&wattn_bwd_kernel<T, NT>), 160 * 1024,
                                "m2f_window_attn_bwd"))
    return rc;
  const unsigned blocks = static_cast<unsigned>(G.B) * G.nWy * G.nWx * G.nH;
  wattn_bwd_kernel<T, NT><<<blocks, 64 * NT, lds, st>>>(static_cast<const T*>(qkv), table, static_cast<const T*>(dout),
                                                        lse, static_cast<T*>(dqkv), part, G, scale);
  return m2f::check_launch("m2f_window_attn_bwd");
}

// f(Tag<T>, NT) for the element type and NT = ceil(ws^2 / 16), which for ws = 2 .. 12 is one of 1, 2, 3, 4, 6, 7, 8, 9;
// false, without a call, for any other dtype code or tile count
template <typename F>
bool by_type_and_tiles(int dtype, int ws, F&& f) {
  bool built = false;
  m2f::dispatch_float(dtype, [&](auto t) {
    built = m2f::dispatch_one_of<1, 2, 3, 4, 6, 7, 8, 9>(tiles_of(ws), [&](auto nt) { f(t, nt); });
  });
  return built;
}

int64_t part_floats(const Geo& G) {
  const int TW = 2 * G.ws - 1;
  return static_cast<int64_t>(G.B) * G.nWy * G.nWx * G.nH * TW * TW;
}

}  // namespace

extern "C" int m2f_window_attn_workspace(int batch, int heads, int hp, int wp, int ws, int64_t* bytes) {
  if (!bytes) return m2f::fail(M2F_EINVAL, "m2f_window_attn_workspace: null bytes");
  if (int rc = check_geometry("m2f_window_attn_workspace", batch, heads, kD, hp, wp, ws, 0)) return rc;
  *bytes = part_floats(make_geo(batch, heads, hp, wp, ws, 0)) * static_cast<int64_t>(sizeof(float));
  return m2f::ok();
}

extern "C" int m2f_window_attn_fwd(int dtype, const void* qkv, const float* table, int batch, int heads, int head_dim,
                                   int hp, int wp, int ws, int shift, float scale, void* out, float* lse,
                                   void* stream) {
  const char* fn = "m2f_window_attn_fwd";
  if (!qkv || !table || !out || !lse) return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (int rc = check_geometry(fn, batch, heads, head_dim, hp, wp, ws, shift)) return rc;
  if (!m2f::aligned(qkv, 16) || !m2f::aligned(out, 16))
    return m2f::fail(M2F_EINVAL, "%s: qkv and out must be 16-byte aligned", fn);
  if (batch == 0) return m2f::ok();
  const Geo G = make_geo(batch, heads, hp, wp, ws, shift);
  int rc = M2F_OK;
  if (!by_type_and_tiles(dtype, ws, [&](auto t, auto nt) {
        rc = launch_fwd<typename decltype(t)::type, nt.value>(qkv, table, out, lse, G, scale,
                                                              static_cast<hipStream_t>(stream));
      }))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype code %d", fn, dtype);
  return rc;
}

extern "C" int m2f_window_attn_bwd(int dtype, const void* qkv, const float* table, const void* dout, const float* lse,
                                   int batch, int heads, int head_dim, int hp, int wp, int ws, int shift, float scale,
                                   void* dqkv, float* dtable, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "m2f_window_attn_bwd";
  if (!qkv || !table || !dout || !lse || !dqkv || !dtable || !workspace)
    return m2f::fail(M2F_EINVAL, "%s: null pointer", fn);
  if (int rc = check_geometry(fn, batch, heads, head_dim, hp, wp, ws, shift)) return rc;
  if (!m2f::aligned(qkv, 16) || !m2f::aligned(dout, 16) || !m2f::aligned(dqkv, 16) || !m2f::aligned(workspace, 4))
    return m2f::fail(M2F_EINVAL, "%s: qkv, dout and dqkv must be 16-byte aligned", fn);
  const Geo G = make_geo(batch, heads, hp, wp, ws, shift);
  if (workspace_bytes < part_floats(G) * static_cast<int64_t>(sizeof(float)))
    return m2f::fail(M2F_EINVAL, "%s: workspace of %lld bytes, %lld needed", fn, static_cast<long long>(workspace_bytes),
                     static_cast<long long>(part_floats(G) * sizeof(float)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  int rc = M2F_OK;
  if (!by_type_and_tiles(dtype, ws, [&](auto t, auto nt) {
        if (batch > 0)
          rc = launch_bwd<typename decltype(t)::type, nt.value>(qkv, table, dout, lse, dqkv, part, G, scale, st);
      }))
    return m2f::fail(M2F_EUNSUPPORTED, "%s: dtype code %d", fn, dtype);
  if (rc) return rc;
  const int TW = 2 * ws - 1, TB = TW * TW;
  // with no window the sums are empty: the kernel writes zeros
  wattn_dtable_kernel<<<dim3(m2f::ceil_div(TB, 64), heads), 64 * kSeg, 0, st>>>(part, dtable, batch * G.nWy * G.nWx,
                                                                                heads, TB);
  return m2f::check_launch(fn);
}

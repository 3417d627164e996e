/*
 * bm2f.h — C ABI of the MI355X (gfx950) Mask2Former hot-path library `libbm2f.so`.
 *
 * Every entry point takes plain device pointers, sizes and a `hipStream_t` passed as `void*`
 * (torch's current stream on the Python side), launches asynchronously on that stream and
 * returns 0 on success or a nonzero M2F_E* code; `m2f_last_error()` then holds a message for the
 * calling thread.  Outputs are allocated by the caller; each function fully initialises them
 * (the reference zero-fills with at::zeros, ms_deform_attn_cuda.cu:59 / :126-128).
 *
 * Reference interfaces replaced (paths relative to the reference root,
 * ops = mask2former/modeling/pixel_decoder/ops):
 *   m2f_msda_fwd_{f32,f64}  <- ms_deform_attn_forward   (ops/src/vision.cpp:19, ops/src/ms_deform_attn.h:25-44,
 *                                                        ops/src/cuda/ms_deform_attn_cuda.cu:25-85)
 *   m2f_msda_bwd_{f32,f64}  <- ms_deform_attn_backward  (ops/src/vision.cpp:20, ops/src/ms_deform_attn.h:46-67,
 *                                                        ops/src/cuda/ms_deform_attn_cuda.cu:88-157)
 *   m2f_attn_mask_*         <- MultiScaleMaskedTransformerDecoder.forward_prediction_heads resize+threshold
 *                              (transformer_decoder/mask2former_transformer_decoder.py:446-450) and the
 *                              fully-masked-row fix (:400)
 *   m2f_masked_attn_*       <- the attention core of nn.MultiheadAttention(attn_mask=bool) used by
 *                              CrossAttentionLayer.forward_post (mask2former_transformer_decoder.py:98-110)
 *   m2f_gemm_f32_*          <- the nn.Linear layers of MSDeformAttnTransformerEncoderLayer (value_proj /
 *                              sampling_offsets+attention_weights / output_proj, ms_deform_attn.py:59-62;
 *                              linear1 / linear2 + ReLU, msdeformattn.py:101-106) in fp32 (:314,320)
 *   m2f_add_layernorm_*     <- norm1(src + dropout1(src2)) / norm2(src + dropout3(src2)) of
 *                              MSDeformAttnTransformerEncoderLayer (pixel_decoder/msdeformattn.py:92-131)
 *
 * Preconditions mirrored from the reference (ms_deform_attn_cuda.cu:33-43, :55-57, :98-124):
 *   batch % min(batch, im2col_step) == 0, else M2F_EINVAL.  All tensors contiguous (checked by the
 *   Python wrapper, which owns the strides).  spatial_shapes / level_start_index are int64 device
 *   arrays of (L,2) and (L,).
 */
#ifndef BM2F_H_
#define BM2F_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  M2F_OK = 0,
  M2F_EINVAL = 1,      /* bad sizes / null pointers / precondition violated */
  M2F_ELAUNCH = 2,     /* HIP launch or runtime error */
  M2F_EUNSUPPORTED = 3 /* configuration this build does not implement */
};

/* Element types of the decoder entry points (`dtype` arguments). */
enum { M2F_F32 = 0, M2F_F16 = 1, M2F_BF16 = 2 };

/* Message for the last nonzero return on this thread ("" if none). */
const char* m2f_last_error(void);
/* ABI version, bumped whenever a signature below changes. */
int m2f_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale deformable attention.
 *   value            (N, S, M, D)          S = sum_l H_l*W_l
 *   spatial_shapes   (L, 2) int64 [H, W]   device
 *   level_start_index(L,)   int64          device
 *   sampling_loc     (N, Lq, M, L, P, 2)   [x, y] normalised to [0,1]
 *   attn_weight      (N, Lq, M, L, P)
 *   output           (N, Lq, M*D)
 * host_spatial_shapes: optional host copy of spatial_shapes (L*2 int64, may be NULL).  When given
 * and Lq == S (encoder self-attention over the flattened pyramid) the forward reads each level's
 * touched box from LDS windows (bit-identical to the untiled forward) and the backward groups queries
 * by spatial tile and accumulates grad_value in LDS windows (results agree with the untiled path up to
 * the order of fp32 additions).  Both tiled paths take each level's start as the prefix sum of the host
 * shapes and do NOT read spatial_shapes / level_start_index: the caller guarantees spatial_shapes ==
 * host_spatial_shapes and level_start_index == their prefix sums (the Python layer checks both once per
 * tensor, bm2f_amd/msda.py attach_host_shapes / _check_level_starts).  Pass NULL to have the kernels
 * read the device arrays as they are.
 * ------------------------------------------------------------------------------------------- */
int m2f_msda_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const float* sampling_loc, const float* attn_weight,
                     int batch, int spatial_size, int num_heads, int channels,
                     int num_levels, int num_query, int num_point, int im2col_step,
                     const int64_t* host_spatial_shapes, float* output, void* stream);

int m2f_msda_fwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const double* sampling_loc, const double* attn_weight,
                     int batch, int spatial_size, int num_heads, int channels,
                     int num_levels, int num_query, int num_point, int im2col_step,
                     const int64_t* host_spatial_shapes, double* output, void* stream);

/* grad_value (N,S,M,D) is zeroed and accumulated; grad_sampling_loc / grad_attn_weight are
 * written for every element (zero where the sample fell outside its level). */
int m2f_msda_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const float* sampling_loc, const float* attn_weight, const float* grad_output,
                     int batch, int spatial_size, int num_heads, int channels,
                     int num_levels, int num_query, int num_point, int im2col_step,
                     const int64_t* host_spatial_shapes,
                     float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, void* stream);

int m2f_msda_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const double* sampling_loc, const double* attn_weight, const double* grad_output,
                     int batch, int spatial_size, int num_heads, int channels,
                     int num_levels, int num_query, int num_point, int im2col_step,
                     const int64_t* host_spatial_shapes,
                     double* grad_value, double* grad_sampling_loc, double* grad_attn_weight, void* stream);

/* MSDA with the sampling front end fused in (encoder layout: num_query == spatial_size, the queries
 * being the flattened pyramid; channels 32, points 4, 1..4 levels).  Replaces the chain
 * sampling_offsets / attention_weights Linear -> softmax -> ref + offset / (W, H) -> ms_deform_attn
 * (ops/modules/ms_deform_attn.py:102-117) after the two projections, so sampling_loc / attn_weight are
 * never materialised:
 *   proj  (N, Lq, proj_ld) fp32: columns [0, M*L*P*2) are the offsets (M, L, P, 2), the next M*L*P the
 *         attention logits (M, L*P) -- the concatenated output of the two Linear layers;
 *   ref   reference points (N, Lq, L, 2) [x, y], batch stride ref_batch_stride elements (0 = broadcast);
 *   host_spatial_shapes (L*2 int64, host, required).
 * The backward writes grad_value (zeroed + accumulated) and grad_proj (N, Lq, M*L*P*3) contiguous:
 * d offsets and d logits (the softmax backward applied in-kernel).  Reference points get no gradient. */
int m2f_msda_fused_fwd_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                           int64_t ref_batch_stride, const int64_t* host_spatial_shapes, int batch,
                           int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                           int num_point, float* output, void* stream);

/* grad_value rows are added with fp32 atomics from the tiled workgroups' LDS windows (each window row is
 * flushed once; values repeat to within fp32 rounding, not bit for bit), and no workspace is needed
 * (m2f_msda_fused_bwd_workspace() reports 0 bytes).  Deterministic mode (m2f_set_option("msda_bwd_det", 1)):
 * grad_value is bitwise repeatable -- each workgroup sums its window rows in a fixed order and adds them, and
 * the out-of-window samples, as 64-bit fixed point (scale 2^k from the launch's max |grad_output|, resolution
 * max|g| * 2^-(61 - ceil(log2 Lq))) with integer atomics, then a pass converts to fp32; it needs the workspace
 * m2f_msda_fused_bwd_workspace() then reports (8 bytes per grad_value element + 16, 16-byte aligned) and
 * returns M2F_EINVAL without it.  A non-finite grad_output sends it down the fp32 atomics (as the reference). */
int m2f_msda_fused_bwd_workspace(const int64_t* host_spatial_shapes, int batch, int spatial_size, int num_heads,
                                 int channels, int num_levels, int num_point, int64_t* workspace_bytes);
int m2f_msda_fused_bwd_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                           int64_t ref_batch_stride, const int64_t* host_spatial_shapes,
                           const float* grad_output, int batch, int spatial_size, int num_heads, int channels,
                           int num_levels, int num_query, int num_point, float* grad_value, float* grad_proj,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* The same two calls with the projection rows head-major: per head m one record
 * [offsets (L, P, 2) | logits (L*P)] of 3*L*P floats, the heads in order (a row permutation of the projection
 * weight, which the module applies: bm2f_amd.msda.MSDeformAttn); grad_proj comes back in the same layout.  Each
 * head's slice is then one 12*L*P-byte piece of the row instead of two, so the 8 heads' workgroups -- dealt to
 * different XCDs -- share fewer 128-byte lines (config 2: backward FETCH -16 %, -2.8 % time; forward -1.5 %).
 * Results are those of the reference layout, bit for bit. */
int m2f_msda_fused_fwd_hm_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                              int64_t ref_batch_stride, const int64_t* host_spatial_shapes, int batch,
                              int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                              int num_point, float* output, void* stream);
int m2f_msda_fused_bwd_hm_f32(const float* value, const float* proj, int proj_ld, const float* ref,
                              int64_t ref_batch_stride, const int64_t* host_spatial_shapes,
                              const float* grad_output, int batch, int spatial_size, int num_heads, int channels,
                              int num_levels, int num_query, int num_point, float* grad_value, float* grad_proj,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Masked-attention decoder (mask2former_transformer_decoder.py).
 *
 * m2f_attn_mask_bits: logits (B, Q, frames, in_h, in_w) of `dtype` -> bits (B, Q, nwords) uint32, bit k
 * of word w = 1 when key 32*w + k (frame-major, then row-major in out_h x out_w) is BLOCKED, i.e.
 *   dtype( sigmoid( dtype( bilinear_resize(logits, (out_h, out_w), align_corners=False) ) ) ) < 0.5
 * exactly as F.interpolate(...).sigmoid() < 0.5 in that dtype (reference :446-449).  With row_fix != 0
 * a row whose every pixel is blocked is cleared, the fix the reference applies before each
 * cross-attention (:400).  One bit per (b, q, pixel) serves all heads (the reference repeats the
 * bool mask per head).  nwords >= ceil(frames*out_h*out_w / 32); unused tail bits are 0.  frames > 1 is
 * the video decoder's per-frame resize of (B, Q, T, H, W) logits (video_..._decoder.py:453-458).
 * ------------------------------------------------------------------------------------------- */
int m2f_attn_mask_bits(const void* logits, int dtype, int batch, int num_queries, int frames, int in_h,
                       int in_w, int out_h, int out_w, int row_fix, uint32_t* bits, int nwords, void* stream);

/* Mask head with the bitmask epilogue (reference :437-452; video_..._decoder.py:444-461):
 *   masks[b, q, t, n] = dtype( sum_c embed[b, q, c] * feats[b, c, t, n] )      (n = y * width + x)
 * embed (B, Q, C), feats (B, C, frames, height, width), masks (B, Q, frames, height, width), all of `dtype`
 * (bf16 or f16; fp32 accumulation).  With target_h > 0 it also writes into `bits` (zeroed, (B, Q, nwords))
 * the blocked bits m2f_attn_mask_bits would compute from `masks` for (target_h, target_w) before its row
 * fix; height / target_h = width / target_w must be an even integer dividing 128.  Constraints: C % 32 == 0,
 * width % 8 == 0, Q <= 256, 16-byte aligned operands. */
int m2f_mask_heads_fwd(int dtype, const void* embed, const void* feats, int batch, int num_queries, int channels,
                       int frames, int height, int width, int target_h, int target_w, void* masks, uint32_t* bits,
                       int nwords, void* stream);

/* Fully-masked-row fix (:400) after m2f_mask_heads_fwd: each of `rows` bit rows whose `keys` bits are all set
 * is cleared. */
int m2f_mask_row_fix(uint32_t* bits, int rows, int nwords, int keys, void* stream);

/* Mask-head einsum backward (autograd of :442 / video :449), dtype bf16 or f16, fp32 accumulation.
 * m2f_mask_heads_bwd_embed: grad_embed (B, Q, 256) = dtype( grad_masks (B, Q, n) . feats (B, 256, n)^T ), split
 *   over n with fp32 partials summed in a fixed order; workspace from m2f_mask_heads_bwd_workspace.
 *   Needs n % 16 == 0, Q <= 256.
 * m2f_mask_heads_bwd_feats: grad_feats (B, 256, n) = out_dtype( sum_h embed_h^T . grad_masks_h ) over `heads`
 *   heads' gradients (an array of device pointers, each (B, Q, n), no concatenation); embed_t is the
 *   heads' embeds transposed, Et[b][c][k] = embed_{k / padded_queries}[b][k % padded_queries][c] for k < heads *
 *   padded_queries (zero past Q in each head's padded_queries slots, a multiple of 16), stored in MFMA
 *   fragment order: element (b, c, k) at ((((b * 8 + c / 32) * (K / 16) + k / 16) * 2 + (k / 8) % 2) * 32 +
 *   c % 32) * 8 + k % 8, K = heads * padded_queries.  out_dtype = dtype, or M2F_F32 when the features are fp32
 *   (autocast's copy): one rounding either way.  heads <= 16, n % 8 == 0. */
int m2f_mask_heads_bwd_workspace(int batch, int num_queries, int64_t n, int64_t* workspace_bytes);
int m2f_mask_heads_bwd_embed(int dtype, const void* grad_masks, const void* feats, int batch, int num_queries,
                             int channels, int64_t n, void* grad_embed, void* workspace, int64_t workspace_bytes,
                             void* stream);
int m2f_mask_heads_bwd_feats(int dtype, const void* const* grad_masks, int heads, const void* embed_t, int batch,
                             int num_queries, int padded_queries, int channels, int64_t n, int out_dtype,
                             void* grad_feats, void* stream);

/* Work split of the masked attention for these sizes: keys are processed in `num_chunks` ranges of
 * `chunk_len`; the forward / backward need the returned fp32 workspace sizes (0 when one chunk). */
int m2f_masked_attn_plan(int batch, int num_queries, int num_keys, int num_heads, int* chunk_len,
                         int* num_chunks, int64_t* fwd_workspace_bytes, int64_t* bwd_workspace_bytes);

/* out = softmax(scale * q k^T, masked by bits) v, per (batch, head); head_dim must be 32.
 *   q   (B, Lq, H*32) with row stride q_row_stride elements;  k, v (B, Lk, H*32), row stride kv_row_stride
 *   out (B, Lq, H*32) contiguous;  lse (B, H, Lq) fp32 log-sum-exp (base-2, internal) for the backward.
 * A query row with every key blocked yields zeros (the reference never passes one: row_fix). */
int m2f_masked_attn_fwd(int dtype, const void* q, const void* k, const void* v, const uint32_t* bits,
                        int batch, int num_queries, int num_keys, int num_heads, int head_dim,
                        int q_row_stride, int kv_row_stride, int mask_words, float scale, void* out,
                        float* lse, void* workspace, int64_t workspace_bytes, void* stream);

/* Gradients of m2f_masked_attn_fwd: grad_q (B, Lq, H*32), grad_k / grad_v (B, Lk, H*32), all
 * contiguous and fully written.  grad_q is summed over key chunks in a fixed order. */
int m2f_masked_attn_bwd(int dtype, const void* q, const void* k, const void* v, const uint32_t* bits,
                        const void* out, const void* grad_out, const float* lse, int batch,
                        int num_queries, int num_keys, int num_heads, int head_dim, int q_row_stride,
                        int kv_row_stride, int mask_words, float scale, void* grad_q, void* grad_k,
                        void* grad_v, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Residual add + LayerNorm over the last dimension (fp32), the encoder layer's post-norm:
 *   y = (x - mean) * rstd * gamma + beta,  x = a + b (b may be NULL: plain LayerNorm),
 *   mean / rstd per row (rows,), rstd = 1 / sqrt(var + eps) with the biased variance.
 * a, b, y, grad_* are (rows, C) row-major, 16-byte aligned; C % 4 == 0 and C <= 1024.
 * The backward recomputes x from a and b and returns grad_x (the gradient of both a and b);
 * grad_gamma / grad_beta (may be NULL) are reduced in a fixed order (deterministic) through a
 * caller-provided workspace of m2f_add_layernorm_workspace() bytes. */
int m2f_add_layernorm_workspace(int64_t rows, int C, int64_t* workspace_bytes);
int m2f_add_layernorm_fwd_f32(const float* a, const float* b, const float* gamma, const float* beta,
                              int64_t rows, int C, float eps, float* y, float* mean, float* rstd,
                              void* stream);
int m2f_add_layernorm_bwd_f32(const float* grad_y, const float* a, const float* b, const float* gamma,
                              const float* mean, const float* rstd, int64_t rows, int C, float* grad_x,
                              float* grad_gamma, float* grad_beta, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact-fp32 GEMMs on the f32 MFMA (row-major; lda/ldb/ldc/ldm are row pitches in elements).
 *
 * m2f_gemm_f32_nt:  C[M,N] = A[M,K] . B[N,K]^T  (+ bias[N] if bias) then ReLU if relu, or
 *                   C *= (mask[M,N] > 0) if mask (ReLU backward through the saved activation).
 *   K, lda, ldb multiples of 4; A, B 16-byte aligned.  Forward of nn.Linear is B = weight;
 *   its input gradient is B = weight^T (the caller transposes the weight).
 * m2f_gemm_f32_tn:  C[N1,N2] = A[M,N1]^T . B[M,N2] and, if colsum, colsum[N1] = sum_m A[m,:]
 *   (weight and bias gradients of nn.Linear: A = grad_out, B = input).  Rows are split over
 *   workgroups; the fp32 partial slabs are summed in a fixed order (deterministic) through a
 *   workspace of m2f_gemm_f32_tn_workspace() bytes.  N1, N2, lda, ldb multiples of 4. */
int m2f_gemm_f32_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int relu,
                    const float* mask, int64_t ldm, float* C, int64_t ldc, int M, int N, int K, void* stream);
int m2f_gemm_f32_tn_workspace(int M, int N1, int N2, int64_t* workspace_bytes);
int m2f_gemm_f32_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                    float* colsum, int M, int N1, int N2, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 GEMMs on the bf16 MFMA by exact three-way operand splitting (x = h + m + l, three bf16
 * planes; the six products of order <= 2^-16 kept: error at the level of one fp32 rounding), at
 * 2.7x the f32-MFMA peak.  Same math as m2f_gemm_f32_nt / _tn above (fp32 in, fp32 out).
 * m2f_gemm_f32x3_nt:  B is [N][K] (ldb >= K), or [K][N] when b_kn (ldb >= N; e.g. the weight
 *   itself for an input gradient, no transpose copy).  Needs m2f_gemm_f32x3_nt_workspace() bytes
 *   (16-byte aligned) for the split B.  K, lda multiples of 4; A 16-byte aligned.
 * m2f_gemm_f32x3_tn:  as m2f_gemm_f32_tn, with m2f_gemm_f32x3_tn_workspace() bytes; no alignment
 *   requirement. */
int m2f_gemm_f32x3_nt_workspace(int N, int K, int64_t* workspace_bytes);
int m2f_gemm_f32x3_nt(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kn, const float* bias,
                      int relu, const float* mask, int64_t ldm, float* C, int64_t ldc, int M, int N, int K,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* m2f_gemm_f32x3_nt_add: as m2f_gemm_f32x3_nt with C = A.B^T (+ bias) + D1 (+ D2), the addends
 *   [M][N] with row stride ldd (C may alias D1 or D2).  Replaces the autograd gradient sums
 *   (AccumulateGrad / AddBackward) over a tensor with several consumers in the encoder layer
 *   (msdeformattn.py:115-131: src feeds value_proj, the query and the residual; its FFN input feeds
 *   linear1 and the residual).  Addends exclude relu and mask; N, ldd, ldc multiples of 4; D1, D2, C
 *   16-byte aligned. */
int m2f_gemm_f32x3_nt_add(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kn, const float* bias,
                          int relu, const float* mask, int64_t ldm, const float* D1, const float* D2, int64_t ldd,
                          float* C, int64_t ldc, int M, int N, int K, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* m2f_gemm_f32x3_nt_rowadd: C = A.B^T + R[m % period] -- a row-periodic addend (R [period][N], row stride ldr).  The
 *   encoder's query projection (src + pos) Wq^T + bq (ms_deform_attn.py:97-103 with msdeformattn.py:115) for a
 *   position embedding shared by the batch: R = pos Wq^T + bq is formed once per layer on the S rows of one image,
 *   so the (N*S, C) sum src + pos is never materialised.  Same constraints as the addends of _nt_add. */
int m2f_gemm_f32x3_nt_rowadd(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kn, const float* R,
                             int64_t ldr, int period, float* C, int64_t ldc, int M, int N, int K, void* workspace,
                             int64_t workspace_bytes, void* stream);
/* m2f_gemm_f32x3_nt_bits: the FFN's ReLU as a 1-bit mask (msdeformattn.py:101-106).  With bits_out (relu != 0):
 *   C = relu(A.B^T + bias) and bits_out[m][n / 32] bit n % 32 = (C[m][n] > 0).  With bits_in (relu == 0):
 *   C = (A.B^T + bias) where the bit is set, else 0 -- the ReLU backward of grad_h = grad_y . W2 read from
 *   M*N/8 bytes instead of the (M, N) fp32 activation.  Exactly one of bits_out / bits_in; N % 32 == 0,
 *   ldbits (in 32-bit words) >= N / 32, ldc % 4 == 0, C 16-byte aligned. */
int m2f_gemm_f32x3_nt_bits(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kn, const float* bias,
                           int relu, uint32_t* bits_out, const uint32_t* bits_in, int64_t ldbits, float* C,
                           int64_t ldc, int M, int N, int K, void* workspace, int64_t workspace_bytes, void* stream);
int m2f_gemm_f32x3_tn_workspace(int M, int N1, int N2, int64_t* workspace_bytes);
int m2f_gemm_f32x3_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                      float* colsum, int M, int N1, int N2, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 convolutions on the x3 engine (NCHW, stride 1, 1x1 or 3x3 with "same" padding, no groups):
 * the pixel decoder's input_proj / adapter / layer / mask_features convs (msdeformattn.py:213-292),
 * replacing cuDNN/MIOpen calls of F.conv2d.  Needs channels % 16 == 0, H*W % 128 == 0, W % 8 == 0.
 * m2f_conv_f32x3: mode 0 O[N][Co][H][W] = conv(I[N][Ci][H][W], W[Co][Ci][k][k]) (+ bias[Co]);
 *                 mode 1 O[N][Ci][H][W] = input gradient of I = grad_out[N][Co][H][W] (no bias).
 * m2f_conv_f32x3_wgrad: dW_tck[k*k][Ci][Co] (tap-major: the caller permutes to [Co][Ci][k][k]) and,
 *                 if dbias, dbias[Co]; split over pixels, slabs summed in a fixed order.
 * All three take m2f_conv_f32x3_workspace() bytes (16-byte aligned). */
int m2f_conv_f32x3_workspace(int N, int Ci, int Co, int H, int W, int ksize, int64_t* workspace_bytes);
int m2f_conv_f32x3(const float* I, const float* W, const float* bias, float* O, int N, int Ci, int Co, int H, int Wd,
                   int ksize, int mode, void* workspace, int64_t workspace_bytes, void* stream);
int m2f_conv_f32x3_wgrad(const float* grad_out, const float* I, float* dW_tck, float* dbias, int N, int Ci, int Co,
                         int H, int Wd, int ksize, void* workspace, int64_t workspace_bytes, void* stream);
/* The 3x3 weight gradient in one tap-fused kernel on the NCHW operands (no padded copies, no per-tap
 * launches): dW[Co][Ci][3][3], the layout of the weight itself, and, if dbias, dbias[Co].  The pixels are
 * split into slabs (splits = 0: chosen by the library; > 0: that many, at most one per 4-row x 8-pixel
 * chunk) summed in a fixed order: bitwise repeatable.  Same shape rules as above; the workspace query
 * takes the same splits. */
int m2f_conv_f32x3_wgrad3_fused_workspace(int N, int Ci, int Co, int H, int Wd, int splits, int64_t* workspace_bytes);
int m2f_conv_f32x3_wgrad3_fused(const float* grad_out, const float* I, float* dW, float* dbias, int N, int Ci, int Co,
                                int H, int Wd, int splits, void* workspace, int64_t workspace_bytes, void* stream);
/* The same convolutions on the backbone's 16-bit features without the reference's .float() copy
 * (msdeformattn.py:320, 336; the conversion is exact, so the results are those of the fp32 calls on
 * the upcast tensor): 1x1 only.  m2f_conv_x3_io mode 0 reads I as i_dtype (M2F_F32 / M2F_F16 /
 * M2F_BF16), NCHW or (i_nhwc, 16-bit only) NHWC, and writes fp32 NCHW (o_dtype M2F_F32, o_nhwc 0);
 * mode 1 reads fp32 NCHW grad_out and writes the input gradient as o_dtype, NCHW or (o_nhwc) NHWC,
 * rounded to nearest even (the cast's backward).  m2f_conv_x3_wgrad_io: as m2f_conv_f32x3_wgrad with
 * I of i_dtype / i_nhwc.  Workspace as above. */
int m2f_conv_x3_io(const void* I, int i_dtype, int i_nhwc, const float* W, const float* bias, void* O, int o_dtype,
                   int o_nhwc, int N, int Ci, int Co, int H, int Wd, int ksize, int mode, void* workspace,
                   int64_t workspace_bytes, void* stream);
int m2f_conv_x3_wgrad_io(const float* grad_out, const void* I, int i_dtype, int i_nhwc, float* dW_tck, float* dbias,
                         int N, int Ci, int Co, int H, int Wd, int ksize, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* out[n] (fp32) = ((s_0 + s_1) + ...) + s_{k-1}, every term converted to fp32 (dtype M2F_F16 / M2F_BF16 /
 * M2F_F32) and added in fp32 in order -- the values of out = s_0.float() and k - 1 in-place mixed-dtype adds, in
 * one pass.  srcs: a host array of k <= 8 device pointers; n % 8 == 0, 16-byte aligned.  Replaces the autograd
 * sums of the decoder's memory-token input gradients (mask2former_transformer_decoder.py:103-108). */
int m2f_sum_to_f32(const void* const* srcs, int k, int64_t n, int dtype, float* out, void* stream);

/* Fused per-channel bias (+ residual) + ReLU in place over an NCHW activation (dtype M2F_BF16, M2F_F16
 * or M2F_F32), memory NCHW or (channels_last != 0) NHWC: x = max(x + residual + bias[c], 0).  The
 * benchmark backbone's FrozenBN shift + shortcut + ReLU in one pass (not on the reference's hot path).
 * H*W (NCHW) or C (NHWC) % 8 (bf16 / fp16) / % 4 (fp32), 16-byte aligned. */
int m2f_bias_act_nchw(void* x, const void* residual, const float* bias, int64_t N, int C, int64_t HW, int dtype,
                      int channels_last, void* stream);

/* ReLU backward over the summed gradients of up to 4 consumers of one activation y (the benchmark
 * backbone's block outputs): out = (grads[0] + ... + grads[ngrads-1]) where !(y <= 0), else 0 (torch's
 * threshold_backward rule: a NaN y passes the gradient), summed in fp32 in the given order and rounded once;
 * bf16, fp16 or fp32, contiguous, n % 8 (16-bit) / % 4 (fp32), 16-byte aligned (else M2F_EUNSUPPORTED).
 * Replaces the autograd engine's accumulating adds plus torch's threshold_backward (one pass, k + 1 reads). */
int m2f_relu_bwd_sum(const void* const* grads, int ngrads, const void* y, void* out, int64_t n, int dtype,
                     void* stream);

/* The benchmark backbone's stem max pool (kernel 3, stride 2, padding 1; detectron2 BasicStem; not on the
 * reference's hot path), NCHW, dtype M2F_BF16, M2F_F16 or M2F_F32, planes = N*C, output (H-1)/2+1 x (W-1)/2+1.
 * m2f_maxpool3s2_fwd: torch's max_pool2d_with_indices rule (first maximum in window order, NaN wins); the
 *   winner's window position (0..8) goes to window[planes][OH][OW] (1 byte instead of an int64 index).
 * m2f_maxpool3s2_bwd: grad_x = each input pixel's sum over the windows it won (torch's order, fp32). */
int m2f_maxpool3s2_fwd(const void* x, void* y, uint8_t* window, int64_t planes, int H, int W, int dtype, void* stream);
int m2f_maxpool3s2_bwd(const void* grad_y, const uint8_t* window, void* grad_x, int64_t planes, int H, int W, int dtype,
                       void* stream);
/* The same max pool on a channels-last (NHWC) 16-bit tensor (N, H, W, C), C % 8 == 0: backward = 0 reads src = x
 * and writes dst = y (N, OH, OW, C) and window (N, OH, OW, C) bytes; backward = 1 reads src = grad_y and window and
 * writes dst = grad_x (N, H, W, C). */
int m2f_maxpool3s2_nhwc(int backward, const void* src, void* dst, uint8_t* window, int N, int H, int W, int C,
                        int dtype, void* stream);

/* Explicit tuning options: geometry / engine overrides for tests and tools (the library never reads the
 * environment).  value < 0 restores the built-in default.  Names: msda_threads, msda_tile, msda_tile_w,
 * msda_halo, msda_win_rows, msda_bwd_tiled, msda_fwd_tiled, msda_fwd_quad, msda_fwd_pb, msda_bwd_overlap,
 * msda_bwd_ratio, msda_bwd_det, msda_fwd_lds, msda_fwd_tile, msda_fwd_tile_w, msda_fwd_cap, msda_fwd_halo (MSDA
 * partitions, variants, LDS windows, deterministic mode), msda_bwd_rowsort, msda_bwd_walk4 (tiled backward phase 3:
 * rows by record count, four records per step; both 1 by default), msda_fwd_pair (LDS-window forward with two lanes
 * per query: 1, or a lane quad: 0, the default), msda_fwd_xcd (forward blocks: all heads of a tile on one XCD: 1, or
 * the head fastest: 0, the default), mattn_dq_atomic, mattn_fwd_minblk, mattn_bwd_minblk,
 * mattn_bwd_keys, mattn_xcd (masked-attention dQ variant, key blocks per workgroup at least, keys per wave in the
 * backward: 32 or 16, the heads of one image and key chunk on one XCD: 1 or 0), mattn_combine (forward chunk
 * combine: a thread per row part 0, a wave per row 1), mask_df_stage (mask-einsum feature
 * gradient: k-steps per LDS stage, 4 or 1), gemm_nt_cfg, x3_tn_nw, x3_tn_blocks,
 * x3_nt_cfg (GEMM tilings), infer_video_cap (m2f_infer_video's LDS budget in source texels).  Every option changes
 * the partition or kernel variant only; results agree to fp32 rounding (summation order may differ between
 * variants).  Process-wide; not synchronised with launches in flight on other threads.  Unknown names return
 * M2F_EINVAL. */
int m2f_set_option(const char* name, int64_t value);
int m2f_get_option(const char* name, int64_t* value);

/* Achievable-HBM probe (BASELINE.md §4 asks for measured peaks beside the spec sheet's): out = in over
 * nbytes (16-byte aligned, nbytes % 16 == 0); moves 2 * nbytes.  mode 0: one pass of plain 16-byte loads and
 * stores (4 per thread); mode 1: a fixed grid striding with nontemporal loads and stores. */
int m2f_stream_copy(const void* in, void* out, int64_t nbytes, int mode, void* stream);

/* Achievable L2-gather probe (the MSDA kernels' binding path): n pseudo-random 128-byte rows of `table`
 * (rows x 32 floats, 16-byte aligned) gathered by 8-lane groups, a float4 per lane, four rows in flight;
 * out receives 2048 * 256 floats (out_len >= that).  Gathered bytes = 128 * n. */
int m2f_gather_probe(const float* table, int rows, int64_t n, float* out, int out_len, void* stream);

/* Batched fp32 transpose out[b][q][r] = in[b][r][q] (row strides in_ld / out_ld, batch strides in_bs /
 * out_bs, in elements; B <= 65535): the pixel decoder's level flatten, cat([x_l.flatten(2).transpose(1, 2)],
 * 1) (msdeformattn.py:64-74), and its backward. */
int m2f_transpose_f32(const float* in, int64_t in_bs, int64_t in_ld, float* out, int64_t out_bs, int64_t out_ld,
                      int B, int R, int Q, void* stream);

/* Column sums out[c] = sum_r src[r][c] in fp32 over a row-major (rows, cols) matrix (dtype f32, f16 or bf16):
 * fp32 partials per 1024-row chunk (workspace from m2f_colsum_workspace), added in chunk order, no memset.
 * The gradients of the decoder's memory-token projection biases (nn.MultiheadAttention in_proj,
 * mask2former_transformer_decoder.py:103-108) and of the level embeddings (:376, msdeformattn.py:75). */
int m2f_colsum_workspace(int64_t rows, int cols, int64_t* workspace_floats);
int m2f_colsum(int dtype, const void* src, int64_t rows, int cols, float* workspace, int64_t workspace_floats,
               float* out, void* stream);

/* GroupNorm (+ ReLU when relu != 0) over fp32 NCHW x (N, C, H*W = HW), G groups, affine gamma/beta (may
 * be null): the pixel decoder's GN layers (msdeformattn.py:216-219, :269-281; nn.GroupNorm(32, C)
 * semantics, biased variance, eps).  fwd writes y and the per-(n, g) mean / rstd (N*G floats each) the
 * backward takes; bwd recomputes the ReLU mask from x and writes dx, and dgamma / dbeta if non-null.
 * Statistics and reductions in fp64 with fixed-order combines (deterministic).  HW % 4 == 0; x, y, dy,
 * dx and the workspace (m2f_group_norm_workspace bytes) 16-byte aligned. */
int m2f_group_norm_workspace(int N, int C, int G, int64_t HW, int64_t* workspace_bytes);
int m2f_group_norm_fwd_f32(const float* x, const float* gamma, const float* beta, int N, int C, int G, int64_t HW,
                           float eps, int relu, float* y, float* mean, float* rstd, void* workspace,
                           int64_t workspace_bytes, void* stream);
int m2f_group_norm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, int N, int C, int G, int64_t HW, int relu, float* dx, float* dgamma,
                           float* dbeta, void* workspace, int64_t workspace_bytes, void* stream);

/* FPN merge of the pixel decoder, msdeformattn.py:343-349 (the lateral plus the bilinear upsample of the
 * coarser map, F.interpolate(..., mode="bilinear", align_corners=False)) for the exact 2x case, fp32:
 * m2f_upsample2x_add_fwd_f32:  out[N][C][2h][2w] = lateral + up2x(src); src (N, C, h, w) read through
 *   element strides (sN, sC, sY, sX), so a transposed (N, HW, C) view needs no copy.  2w % 4 == 0;
 *   lateral and out contiguous, 16-byte aligned.
 * m2f_upsample2x_bwd_f32:  grad_src[N][C][h][w] (contiguous) = the adjoint of up2x applied to
 *   grad_out[N][C][2h][2w] (a gather with the forward's weights: deterministic, no atomics).  The
 *   lateral's gradient is grad_out itself. */
int m2f_upsample2x_add_fwd_f32(const float* src, int64_t sN, int64_t sC, int64_t sY, int64_t sX, const float* lateral,
                               float* out, int N, int C, int h, int w, void* stream);
int m2f_upsample2x_bwd_f32(const float* grad_out, float* grad_src, int N, int C, int h, int w, void* stream);
/* Channels-last coarse map (the encoder's (N, HW, C) output seen as (N, C, h, w); msdeformattn.py:335-349): src is
 * (N, h, w, C) with batch stride sN elements (sN >= h*w*C, a multiple of 4: the level's slice of the (N, S, C) encoder
 * output), grad_src (N, h, w, C) contiguous, lateral / out / grad_out NCHW; C % 64 == 0, even w <= 256; same
 * taps, products and summation order as the NCHW pair above.  Replace the transposing copy before the forward and the
 * mixed-layout gradient sum after the backward. */
int m2f_upsample2x_add_fwd_nhwc_f32(const float* src, int64_t sN, const float* lateral, float* out, int N, int C, int h,
                                    int w, void* stream);
int m2f_upsample2x_bwd_nhwc_f32(const float* grad_out, float* grad_src, int N, int C, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weak-supervision criterion (SUP_TYPE "mask_projection_and_pairwise"), SURVEY 8(f) ranks 1 and 3.
 * ------------------------------------------------------------------------------------------- */

/* Batched linear sum assignment, replacing scipy.optimize.linear_sum_assignment on C.cpu()
 * (mask2former/modeling/matcher.py:309-311; same shortest-augmenting-path algorithm and tie rule,
 * in fp64).  Problem b is cost[b*batch_stride + r*max_cols + c] for r < rows[b], c < cols[b]
 * (cols == NULL: max_cols).  match[b*max_rows + r] = matched column or -1.  status[b] = 0 ok,
 * 1 infeasible, 2 too large, 3 NaN / -inf entry (scipy raises ValueError for 1 and 3).
 * Limits per problem: min(rows, cols) <= 256, max(rows, cols) <= 1024.  One wavefront per problem. */
int m2f_lsap_batched(const float* cost, int batch, int max_rows, int max_cols, int64_t batch_stride,
                     const int* rows, const int* cols, int* match, int* status, void* stream);

/* Pairwise affinity term s(p,q) = -log(sig(x_p)sig(x_q) + sig(-x_p)sig(-x_q)) over the 8 dilated
 * neighbours of each pixel (criterion.py:156-181, matcher.py:48-83, weaksup_utils.py:7-31; zero
 * padding outside the image as F.unfold).  Row r reads mask x[x_row[r]] (H, W) fp32, neighbour
 * bits[t_row[r]] (H*W bytes, bit k = similarity_k >= thresh) and weight box[box_row[r]] (or 1).
 * NULL index arrays mean identity.  mode 0: out[r, p] = sum_k bit_k s_k;  mode 1: per-tile
 * partials out[r, t] = sum_p w sum_k bit_k s_k and out_den[r, t] = sum_p w popcount(bits), with
 * t < m2f_pairwise_tiles(H, W);  mode 2: out[r, k, p] = s_k (bits unused).  1 <= dilation <= 4,
 * R <= 65535. */
int m2f_pairwise_tiles(int H, int W);
int m2f_pairwise_rows(const float* x, const int* x_row, int R, int H, int W, int dilation, const uint8_t* bits,
                      const int* t_row, const float* box, const int* box_row, int mode, float* out, float* out_den,
                      void* stream);
/* The matcher's fused pass over the (B*Q, H, W) mask logits x (query q of image b is row b*Q+q):
 * part_cost[r, t, g] = sum_{p in tile t} box[b, g, p] sum_k bit_k s_k (bits[b]: the image's neighbour
 * bits; box (B, Gm, H, W); 0 for g >= gcount[b]), rowmax[r, y, tx] / colmax[r, ty, x] = per-tile maxima
 * of x along W / H (tiles: 16 rows x 64 columns, t = ty * ceil(W/64) + tx).  gbox (B, Gm, 4) int32
 * [y0, y1, x0, x1) must contain every nonzero pixel of box[b, g] (tiles outside it are skipped).
 * Gm <= 256. */
int m2f_pairwise_match_cost(const float* x, int B, int Q, int H, int W, int dilation, const uint8_t* bits,
                            const float* box, const int* gcount, const int* gbox, int Gm, float* part_cost,
                            float* rowmax, float* colmax, void* stream);
/* Gradient of sum_r grad_scale[r] * (mode-1 numerator of row r) w.r.t. x[x_row[r]], written to
 * grad[r] (R, H, W) (not accumulated). */
int m2f_pairwise_rows_bwd(const float* x, const int* x_row, int R, int H, int W, int dilation, const uint8_t* bits,
                          const int* t_row, const float* box, const int* box_row, const float* grad_scale,
                          float* grad, void* stream);
/* bits[n, p] = sum_k (sim[n, k, p] >= thr) << k for an (N, 8, HW) similarity. */
int m2f_threshold_bits(const float* sim, int N, int64_t HW, float thr, uint8_t* bits, void* stream);

/* Target preparation (maskformer_model.py:417-440): images (B, 3, Hp, Wp) fp32 in 0..255 (zero
 * padded) -> lab (B, 3, Hp/stride, Wp/stride): stride x stride average pool, Tensor.byte(),
 * skimage.color.rgb2lab (D65/2deg, double precision) -> fp32. */
int m2f_weaksup_lab(const float* images, int B, int Hp, int Wp, int stride, float* lab, void* stream);
/* sim (B, 8, h, w) = exp(-0.5 * ||lab_p - lab_q||) * mask_q, q = p + dilation * tap_k (0 outside),
 * get_images_color_similarity (weaksup_utils.py:34-57) batched over images. */
int m2f_color_similarity(const float* lab, const float* mask, int B, int h, int w, int dilation, float* sim,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box-supervised video criterion (mask2former_video/modeling/criterion_proj_spatpair_temppair.py):
 * temporal pairwise loss and temporal pair mining.  Pairs are packed as four int32 arrays of length P:
 * pair_row (flat target row, < 0: dead pair), pair_t (frame t in [0, T-1)), pair_p0 / pair_p1 (linear
 * pixel y*W + x in frame t / t+1).  row_of_target (n_targets,) int32 maps a target row to its matched
 * row n of src (N, T, H, W) fp32 contiguous, or -1.  A pair with any index out of range, or whose
 * target is unmatched, is dead: it adds nothing and is not counted.  H*W < 2^31.
 * ------------------------------------------------------------------------------------------- */

/* Number of per-block partials the forward writes for P pairs. */
int m2f_temporal_blocks(int P);
/* part_sum[k] = sum over block k's live pairs of s = -log(sig(a)sig(b) + sig(-a)sig(-b)) (log-space
 * form of m2f_pairwise_rows), a = src[n, t, p0], b = src[n, t+1, p1]; part_cnt[k] = its live pairs.
 * The caller sums the m2f_temporal_blocks(P) partials (fixed order; no host synchronisation). */
int m2f_temporal_pairs_fwd(const float* src, int N, int T, int H, int W, const int* row_of_target, int n_targets,
                           const int* pair_row, const int* pair_t, const int* pair_p0, const int* pair_p1, int P,
                           float* part_sum, int* part_cnt, void* stream);
/* grad (N, T, H, W), zeroed by the caller, gets grad_scale[0] * d(sum of s)/d src.  ep_key / ep_code
 * (2P): the endpoints of all pairs sorted (stably) by ep_key = (pair_row * T + frame) * H*W + pixel
 * (-1 for a dead pair), ep_code = 2 * pair + side (side 1: the frame t+1 endpoint).  The thread on
 * the first endpoint of each run of equal keys sums the run in stored order and writes the pixel
 * once: no atomics, bitwise repeatable. */
int m2f_temporal_pairs_bwd(const float* src, int N, int T, int H, int W, const int* row_of_target, int n_targets,
                           const int* pair_row, const int* pair_t, const int* pair_p0, const int* pair_p1, int P,
                           const int64_t* ep_key, const int* ep_code, const float* grad_scale, float* grad,
                           void* stream);
/* Temporal pair mining (utils/weaksup_utils.py:64-165 with topk_match = 1) over all (instance, frame
 * pair) segments in one launch.  feats (T, D, h, w) fp32.  segs (n_segs, 10) int32: t, cx0, cy0, cw,
 * nc, nx0, ny0, nw, nn, out_off -- the frame-t box (origin, width, pixel count), the frame-(t+1) box
 * and the segment's offset in out_p1; boxes lie inside the frame.  blocks (n_blocks, 2) int32:
 * (segment, 64-pixel tile of its current box), one workgroup each.  out_p1[out_off + j] = linear
 * pixel y*w + x of the next-box pixel at the smallest squared L2 feature distance (summed as
 * (a-b)^2 in fp32; first minimum in row-major order) from current-box pixel j (row-major). */
int m2f_temporal_mine(const float* feats, int T, int D, int h, int w, const int* segs, int n_segs,
                      const int* blocks, int n_blocks, int* out_p1, int n_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Point sampling of the mask-supervised matcher and criterion (modeling/matcher.py:479-597,
 * modeling/criterion.py:775-955 and their mask2former_video twins).  Common conventions:
 *   point_sample(x, u), u = (ux, uy) normalised: grid_sample(bilinear, zeros, align_corners=False), i.e.
 *          pixel (ux * Wn - 0.5, uy * Hn - 0.5); a corner outside the plane contributes 0;
 *   masks  (n_planes, H, W) logits of `dtype` (M2F_F32 / M2F_F16 / M2F_BF16), evaluated in fp32;
 *   tgt_dtype  0: uint8 / bool planes, 1: fp32 planes, read in place through int64 pointer tables;
 *   H * W < 2^31 for every plane; plane offsets are 64-bit.  Nothing synchronises with the host.
 * ------------------------------------------------------------------------------------------- */

/* Floats of workspace m2f_point_match_cost needs. */
int m2f_point_match_workspace(int B, int T, int Q, int Gm, int K, int64_t* floats);
/* cost (B, Q, Gm) fp32 = w_mask * (sum softplus(x) - sum x t) / (T K) + w_class * cost_class +
 * w_dice * (1 - (2 sum sig(x) t + 1) / (sum sig(x) + sum t + 1)), sums over the T frames and the K points
 * coords (B, K, 2) of image b, shared by its Q predictions masks (B, Q, T, H, W) and its targets.
 * tgt (B, 4) int64 device table [pointer to (G_b, T, Ht, Wt) planes, G_b, Ht, Wt]: targets are sampled at
 * their own size.  Columns g >= G_b are 0.  cost_class (B, Q, Gm) fp32 may be NULL.  Per-tile partial
 * sums go through `workspace` and are reduced in a fixed order in fp64: bitwise repeatable. */
int m2f_point_match_cost(const void* masks, int dtype, int B, int Q, int T, int H, int W, const float* coords,
                         int K, const int64_t* tgt, int tgt_dtype, int Gm, const float* cost_class,
                         float w_class, float w_mask, float w_dice, float* workspace, int64_t ws_floats,
                         float* cost, void* stream);
/* out (R, P) fp32 = -|point_sample(masks[plane[r]], coords[r, p])|, coords (R, P, 2), plane (R,) int64
 * (a row whose plane is outside [0, n_planes) gets 0). */
int m2f_point_uncertainty(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane,
                          int R, const float* coords, int P, float* out, void* stream);
/* Chunks of points per row of m2f_point_loss_fwd's partials. */
int m2f_point_loss_chunks(int K);
/* part (R, chunks, 4) fp32: per row and chunk of its K points coords (R, K, 2), the sums of
 * BCE-with-logits(x, t), sig(x) t, sig(x) and t, x = point_sample(masks[plane[r]]), t = point_sample of
 * the row's target.  tgt (R, 5) int64 device table [plane pointer, Ht, Wt, Hn, Wn]: the target is
 * (Ht, Wt) and the coordinates are normalised over (Hn, Wn) >= (Ht, Wt), as if zero-padded to it. */
int m2f_point_loss_fwd(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane, int R,
                       const float* coords, int K, const int64_t* tgt, int tgt_dtype, float* part,
                       void* stream);
/* grad (n_planes, H, W) fp32, zeroed by the caller, += d / d masks of sum_r (grad_rows[r, 0] BCE_r +
 * grad_rows[r, 1] sum sig(x) t + grad_rows[r, 2] sum sig(x)), scattered through the bilinear weights
 * with fp32 atomics (the sum order, hence the last bits, varies from run to run). */
int m2f_point_loss_bwd(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane, int R,
                       const float* coords, int K, const int64_t* tgt, int tgt_dtype, const float* grad_rows,
                       float* grad, void* stream);
/* The same three on label-map targets: the G_b targets of image b are one (Ht, Wt) map of labels (label_bytes
 * 1 = uint8, 2 = int16, 4 = int32) and G_b int32 ids, target g being the set map == ids[g].  The value of a tap
 * is (label == id) ? 1 : 0, summed in the dense kernels' order, so every output is bitwise what the dense uint8
 * planes map[None] == ids[:, None, None] give through the entry points above; those planes are never formed.
 *   m2f_point_match_cost_labels  images only (T = 1; workspace from m2f_point_match_workspace with T = 1).
 *       tgt (B, 5) int64 [map pointer, G_b, Ht, Wt, pointer to the G_b ids].  A workgroup reads the four corner
 *       labels of each of its points once, whatever G_b is.
 *   m2f_point_loss_fwd_labels / _bwd_labels  tgt (R, 6) int64 [map pointer, id, Ht, Wt, Hn, Wn].  A corner beyond
 *       the map contributes 0, as does a pixel whose label is no id (ignored / VOID). */
int m2f_point_match_cost_labels(const void* masks, int dtype, int B, int Q, int H, int W, const float* coords, int K,
                                const int64_t* tgt, int label_bytes, int Gm, const float* cost_class,
                                float w_class, float w_mask, float w_dice, float* workspace, int64_t ws_floats,
                                float* cost, void* stream);
int m2f_point_loss_fwd_labels(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane,
                              int R, const float* coords, int K, const int64_t* tgt, int label_bytes, float* part,
                              void* stream);
int m2f_point_loss_bwd_labels(const void* masks, int dtype, int64_t n_planes, int H, int W, const int64_t* plane,
                              int R, const float* coords, int K, const int64_t* tgt, int label_bytes,
                              const float* grad_rows, float* grad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Inference heads: the eval branch of MaskFormer.forward (maskformer_model.py:333-377) from the
 * decoder's low-resolution mask logits.  Common arguments:
 *   logits (B, Q, in_h, in_w) of `dtype` (M2F_F32 / M2F_F16 / M2F_BF16), converted to fp32 on load;
 *          everything after is fp32, so for 16-bit logits the result is the reference's on
 *          logits.float();
 *   pad_h, pad_w  the padded batch size the reference upsamples to (:337-342);
 *   sizes  (B, 4) int32 device table [Hc, Wc, Ho, Wo] per image: the crop (image size) and the
 *          output size of sem_seg_postprocess (:355-357); the second bilinear resize is skipped
 *          when (Ho, Wo) == (Hc, Wc).  Entries are clamped to pad_* / out_*;
 *   out_h, out_w  row and column counts of the output buffers; rows and columns beyond an image's
 *          (Ho, Wo) are left untouched.
 * The full-resolution logit of a pixel is torch's upsample_bilinear2d (align_corners=False) formula
 * evaluated literally, stage by stage (bm2f_amd/csrc/resize_device.h).  Q <= 256, else
 * M2F_EUNSUPPORTED.  No entry point synchronises with the host.
 * ------------------------------------------------------------------------------------------- */

/* semantic_inference (:509-513): semseg (B, K, out_h, out_w) fp32 = sum_q probs[b, k, q] *
 * sigmoid(logit_q), probs (B, K, Q) fp32 = softmax(pred_logits)[..., :-1] transposed; exact fp32 on
 * the f32 MFMA.  With labels != NULL it writes labels (B, out_h, out_w) int16 = argmax_k (first
 * maximum, as torch.argmax) instead and semseg is not touched (may be NULL).  K <= 256.  Non-finite
 * logits are not handled as torch does: a pixel whose scores are all NaN gets label -1. */
int m2f_infer_semantic(const void* logits, int dtype, const float* probs, const int32_t* sizes, int batch,
                       int num_queries, int num_classes, int in_h, int in_w, int pad_h, int pad_w, int out_h,
                       int out_w, float* semseg, int16_t* labels, void* stream);
/* Semantic test-time augmentation (SemanticSegmentorWithTTA._inference_one_image,
 * test_time_augmentation.py:71-98): the mean over the num_views augmented views of ONE image of each
 * view's semantic scores, mirrored back where the view was flipped, in one launch:
 *   semseg (K, out_h, out_w) fp32 = (sum_v sum_q probs[v, k, q] * s_vq(y, flip_v ? out_w - 1 - x : x)) / V.
 * logits  logits_numel elements of `dtype`: one flat buffer, or the address range that spans the
 *         views' separate allocations, holding every view's (Q, h_v, w_v) low-resolution mask
 *         logits; only the views' own elements are read;
 * probs   (V, K, Q) fp32, softmax(pred_logits_v)[..., :-1] transposed, as m2f_infer_semantic takes it;
 * views   (V, M2F_TTA_VIEW_FIELDS) int64 device table, one row per view:
 *         [element offset of the view's logits in `logits`, h, w, pad_h, pad_w, Hc, Wc, flip];
 *         Hc, Wc are clamped to [1, pad_*]; a row with a non-positive size, or whose Q * h * w
 *         elements do not lie inside the buffer, contributes nothing (the divisor stays V);
 * before  nonzero: s = sigmoid of the chained logit (resize to the pad, crop, resize to the output;
 *         sem_seg_postprocess_before_inference).  Zero: the reference's default order, the view's
 *         scores are computed on the crop and resized after, s = the stage-2 bilinear blend of the
 *         sigmoids of the four stage-1 logits.  Both orders skip stage 2 when (Hc, Wc) equals
 *         (out_h, out_w).
 * With labels != NULL it writes labels (out_h, out_w) int16 = argmax_k (first maximum; a pixel whose
 * scores are all NaN gets -1) and no (K, out_h, out_w) buffer exists anywhere; semseg may be NULL.
 * The sum runs in a fixed order without atomics: bitwise repeatable.  1 <= V <= 32, K <= 256,
 * Q <= 256, else M2F_EUNSUPPORTED; null pointers M2F_EINVAL. */
enum { M2F_TTA_VIEW_FIELDS = 8 };
int m2f_infer_semantic_tta(const void* logits, int dtype, int64_t logits_numel, const float* probs,
                           const int64_t* views, int num_views, int num_queries, int num_classes, int out_h,
                           int out_w, int before, float* semseg, int16_t* labels, void* stream);
/* The pixel pass of panoptic_inference (:515-571).  keep_idx / keep_score (B, Q): the kept queries
 * of each image in ascending order and their scores, num_keep (B,) int32 how many.  Outputs:
 * winner (B, out_h, out_w) int16 = index into the kept list of argmax_k score_k * sigmoid(logit_k)
 * (first maximum; -1 when num_keep == 0); inside (B, out_h, out_w) uint8 = the winner's own
 * sigmoid >= 0.5; counters (B, Q, 3) int32 = [mask_area, original_area, intersection] per kept query
 * (:544-548), zeroed here and counted with integer atomics (exact).  The caller runs the segment
 * merging loop (:541-569) on the copied counters and maps winner through a segment-id table. */
int m2f_infer_panoptic_pass(const void* logits, int dtype, const int32_t* keep_idx, const float* keep_score,
                            const int32_t* num_keep, const int32_t* sizes, int batch, int num_queries, int in_h,
                            int in_w, int pad_h, int pad_w, int out_h, int out_w, int16_t* winner, uint8_t* inside,
                            int32_t* counters, void* stream);
/* The pixel pass of instance_inference (:573-624).  sel_idx (B, max_sel) int32: distinct selected
 * queries per image, num_sel (B,) how many.  masks (B, max_sel, out_h, out_w) uint8 = logit > 0
 * (:615); sums (B, max_sel, 2) fp32 = [sum(sigmoid * binary), sum(binary)] (:621), reduced in a
 * fixed order through partials (B, max_sel, num_tiles, 2) fp32 with
 * num_tiles = ceil(out_h * out_w / 1024).  Slots >= num_sel get zero sums and untouched masks.
 * out_h * out_w <= 2^24 (the pixel count is summed in fp32 and stays exact), else M2F_EUNSUPPORTED. */
int m2f_infer_instance(const void* logits, int dtype, const int32_t* sel_idx, const int32_t* num_sel,
                       const int32_t* sizes, int batch, int num_queries, int max_sel, int in_h, int in_w, int pad_h,
                       int pad_w, int out_h, int out_w, int num_tiles, uint8_t* masks, float* partials, float* sums,
                       void* stream);

/* The eval branch of VideoMaskFormer.forward (mask2former_video/video_maskformer_model.py:372-393) and the
 * pixel pass of inference_video (:651-694) on clip 0: logits (Q, T, in_h, in_w) of `dtype`, read in place;
 * slot_query (num_slots,) int32: the distinct selected queries, num_sel (device, may be NULL = all slots)
 * how many of them are live.  The value of a pixel is the resize chain above with one image geometry for
 * the whole clip: interpolate to (pad_h, pad_w), crop to (crop_h, crop_w), interpolate to (out_h, out_w)
 * (skipped when equal), then > 0 (:666).  packed = 0: out (num_slots, T, out_h, out_w) uint8 0/1;
 * packed = 1: out (num_slots, T, out_h, ceil(out_w / 32)) int32, bit x % 32 of word x / 32, tail bits
 * zero.  Slots >= *num_sel are left untouched.  A workgroup stages its tile's source box in LDS when the
 * box has at most `infer_video_cap` texels (m2f_set_option; default 1536, 0 = never, at most 12288) and
 * reads global memory otherwise; both paths give identical bits.  out 4-byte aligned and crop <= pad, else
 * M2F_EINVAL.  T, num_slots <= 65535, in_h * in_w and out_h * out_w < 2^31, else M2F_EUNSUPPORTED. */
int m2f_infer_video(const void* logits, int dtype, const int32_t* slot_query, const int32_t* num_sel,
                    int num_queries, int num_slots, int num_frames, int in_h, int in_w, int pad_h, int pad_w,
                    int crop_h, int crop_w, int out_h, int out_w, int packed, void* out, void* stream);
/* The DINO feature resize of prepare_weaksup_targets (video_maskformer_model.py:506-517): feats (planes,
 * src_h, src_w) of `dtype` -> out (planes, out_h, out_w) fp32 = torch's bilinear F.interpolate
 * (align_corners=False) of the features zero-padded bottom/right to (pad_h, pad_w), without building the
 * padded copy: taps are clamped to the padded size, a tap at or beyond (src_h, src_w) contributes 0.  The
 * source coordinate and tap weights are exact (integer arithmetic) and the four-tap blend is fp32, so the
 * result is within fp32 rounding of the fp64 interpolation, and equal to torch's fp32 result bit for bit
 * where torch's own weights are exact (integer ratios such as the stride-4 resize).  src <= pad, else M2F_EINVAL; plane sizes < 2^31, else M2F_EUNSUPPORTED. */
int m2f_feat_resize_pad(const void* feats, int dtype, int64_t planes, int src_h, int src_w, int pad_h, int pad_w,
                        int out_h, int out_w, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shifted-window attention of the Swin block (reference backbone/swin.py:131-171, :257-284): what lies
 * between the qkv linear and the proj linear, with the cyclic shift, the window partition, the
 * relative-position bias gather and the shift mask (-100 where the nine-region labels differ) computed
 * from addresses inside the kernels.
 *   qkv    (batch, hp, wp, 3 * heads * head_dim) of `dtype` (M2F_F32 / M2F_F16 / M2F_BF16), [q | k | v]
 *   table  ((2 ws - 1)^2, heads) fp32 relative-position bias table
 *   out    (batch, hp, wp, heads * head_dim) of `dtype`, unshifted and unpartitioned
 *   lse    (batch, heads, hp * wp) fp32 log-sum-exp of every query row (all the backward needs saved)
 * hp and wp are multiples of ws, 0 <= shift < ws (else M2F_EINVAL); 2 <= ws <= 12 and head_dim == 32
 * (else M2F_EUNSUPPORTED).  qkv, out, dout and dqkv are 16-byte aligned and contiguous.
 * The backward writes every element of dqkv (same shape as qkv) with plain stores and dtable
 * ((2 ws - 1)^2, heads) fp32 as a fixed-order sum of per-workgroup partials held in `workspace`
 * (m2f_window_attn_workspace bytes): no atomics, no memset, bitwise repeatable. */
int m2f_window_attn_workspace(int batch, int heads, int hp, int wp, int ws, int64_t* bytes);
int m2f_window_attn_fwd(int dtype, const void* qkv, const float* table, int batch, int heads, int head_dim, int hp,
                        int wp, int ws, int shift, float scale, void* out, float* lse, void* stream);
int m2f_window_attn_bwd(int dtype, const void* qkv, const float* table, const void* dout, const float* lse,
                        int batch, int heads, int head_dim, int hp, int wp, int ws, int shift, float scale,
                        void* dqkv, float* dtable, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO run-length encoding of binary masks on the device (the form the reference's evaluators get from
 * pycocotools.mask.encode, mask2former_video/data_video/ytvis_eval.py:256-293), restated here:
 *   a mask (H, W) is read column-major, pixel p = x * H + y; t_0 < ... < t_{k-1} are the positions with
 *   pixel(p) != pixel(p - 1), pixel(-1) = 0; counts = [t_0, t_1 - t_0, ..., H * W - t_{k-1}] (k + 1 values,
 *   counts[0] == 0 when pixel 0 is set); count i goes out as delta = counts[i] - (i > 2 ? counts[i - 2] : 0)
 *   in 5-bit groups, low group first, each group + 48 with bit 0x20 set while more groups follow (at most
 *   7 characters).
 * `num_masks` masks of one size are read in place from `masks`, form M2F_RLE_BITS or M2F_RLE_BYTES:
 *   bits   int32 words, bit x % 32 of word x / 32 (what m2f_infer_video writes with packed = 1); a set tail
 *          bit beyond `width` is never read; 4-byte aligned
 *   bytes  uint8 / bool, non-zero = set
 * with `row_stride` and `plane_stride` in elements (words or bytes).  Mask m is source plane
 * plane_index[m] clamped to [0, src_planes) when plane_index (device int32) is given, else plane m; the
 * source then holds src_planes planes (>= num_masks without a table).
 * Four stages, each a launch on `stream`; the two scans between them are the caller's (an inclusive
 * int64 prefix sum, e.g. torch.cumsum) and the caller reads col_start[M * W] to size `positions`:
 *   m2f_rle_col_counts   counts (M, W) int32: transitions in column x of mask m, the one between the column's
 *                        first pixel and the previous column's last pixel (virtual 0 before column 0) included
 *   m2f_rle_positions    col_start (M * W + 1) int64 = exclusive scan of counts.  positions (R + M) int32,
 *                        R = col_start[M * W]: mask m owns [col_start[m * W] + m, col_start[(m + 1) * W] + m]:
 *                        its t_j in order, then H * W.  A slot at or beyond `capacity` is never written.
 *   m2f_rle_deltas       per count g < total = R + M: delta[g] int32 and nchar[g] uint8 (1..7)
 *   m2f_rle_chars        char_end (total) int64 = inclusive scan of nchar; the characters of count g go to
 *                        out[char_end[g] - nchar[g] ...]; mask m's string is out[e(s_m - 1) : e(s_{m+1} - 1)]
 *                        with s_m = col_start[m * W] + m, e = char_end and e(-1) = 0.  A byte at or beyond
 *                        `capacity` is never written.
 * Every offset comes from a scan: no atomics, no dependence on workgroup order, identical bytes from run to
 * run, and no per-mask run capacity.  Null pointers, non-positive sizes, H * W >= 2^31, a row stride
 * smaller than the row or a plane stride smaller than H rows give M2F_EINVAL; num_masks > 65535 gives
 * M2F_EUNSUPPORTED; all before any HIP call.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_RLE_BITS = 0, M2F_RLE_BYTES = 1 };
int m2f_rle_col_counts(const void* masks, int form, const int32_t* plane_index, int src_planes, int num_masks,
                       int height, int width, int64_t row_stride, int64_t plane_stride, int32_t* counts,
                       void* stream);
int m2f_rle_positions(const void* masks, int form, const int32_t* plane_index, int src_planes, int num_masks,
                      int height, int width, int64_t row_stride, int64_t plane_stride, const int64_t* col_start,
                      int32_t* positions, int64_t capacity, void* stream);
int m2f_rle_deltas(const int32_t* positions, const int64_t* col_start, int num_masks, int width, int64_t total,
                   int32_t* delta, uint8_t* nchar, void* stream);
int m2f_rle_chars(const int32_t* delta, const uint8_t* nchar, const int64_t* char_end, int64_t total, uint8_t* out,
                  int64_t capacity, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mask IoU of instance sequences on bit planes: what the reference's video evaluator gets from
 * pycocotools.mask.merge / area per (detection, ground truth, frame)
 * (mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:176-222).
 * A plane is (H, words) int32, words = ceil(W / 32), bit x % 32 of word x / 32 (M2F_RLE_BITS above).
 *
 *   m2f_rle_decode_bits   the reverse of the encoder.  positions (total) int32 holds, mask after mask, the
 *                         cumulative run ends of the masks (counts summed up: the last one is H * W) in the
 *                         column-major order p = x * H + y; mask m owns positions[offsets[m] : offsets[m + 1]],
 *                         offsets (M + 1) int64 (clamped to [0, total] by the kernel).  Pixel p is set when an
 *                         odd number of run ends is <= p, so equal ends (zero counts) are allowed and a mask
 *                         with no ends is all zero.  out (M, H, words) int32: every word is written once with
 *                         a plain store, tail bits zero; no memset, no atomics, the same bytes on every run.
 *                         The ends must be non-decreasing inside a mask (the caller's check); unsorted ends
 *                         give unspecified bits and no out-of-range access.
 *   m2f_bits_pair_counts  a (Da, T, H, words) and b (Db, T, H, words), each instance contiguous, instance i at
 *                         a + i * a_stride words (b likewise, on its own base pointer).
 *                           inter  (Da, Db) int64  sum over T, H, W of popcount(a & b)
 *                           area_a (Da, T)  int64, area_b (Db, T) int64
 *                         Bits beyond `width` in a row's last word are masked by the kernel.  A workgroup
 *                         takes M2F_PAIR_CHUNK_WORDS word positions of one frame and an M2F_PAIR_TA x
 *                         M2F_PAIR_TB tile of instances, so a is read ceil(Db / M2F_PAIR_TB) times and b
 *                         ceil(Da / M2F_PAIR_TA) times; 128-bit loads when both bases are 16-byte aligned and
 *                         both strides and H * words are multiples of 4, 32-bit loads otherwise.  Per-workgroup
 *                         int32 partials go to `workspace` (m2f_bits_pair_workspace bytes, contents on entry
 *                         irrelevant) and are summed in index order: no atomics, no zeroed buffer.
 *   m2f_bits_pair_tiles   the three constants, for callers that size their batches by them.
 * Null pointers, non-positive sizes, H * W >= 2^31, a stride smaller than an instance, a misaligned pointer
 * or a short workspace give M2F_EINVAL; more than 65535 masks, frames or instance tiles M2F_EUNSUPPORTED;
 * all before any HIP call.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_PAIR_TA = 8, M2F_PAIR_TB = 4, M2F_PAIR_CHUNK_WORDS = 4096 };
int m2f_rle_decode_bits(const int32_t* positions, int64_t total, const int64_t* offsets, int num_masks, int height,
                        int width, int32_t* out, void* stream);
int m2f_bits_pair_tiles(int* ta, int* tb, int* chunk_words);
int m2f_bits_pair_workspace(int da, int db, int frames, int height, int width, int64_t* bytes);
int m2f_bits_pair_counts(const int32_t* a, int da, int64_t a_stride, const int32_t* b, int db, int64_t b_stride,
                         int frames, int height, int width, int64_t* inter, int64_t* area_a, int64_t* area_b,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The ragged forms: masks of many images of different sizes in one launch (COCO instance AP,
 * bm2f_amd/coco_eval.py).  All planes live in one flat int32 word buffer; plane m of H_m x W_m pixels
 * occupies H_m * ceil(W_m / 32) words at a word offset the caller chooses, in the layout above.  The
 * tables are built by the caller on the host and passed in device memory (one upload carries them all;
 * mask_iou.rle_to_bits_ragged and mask_pair_counts_ragged are the model callers).  The kernels check every
 * index they take from a table against the sizes passed here by value: a malformed table gives unspecified
 * values, never an access outside positions, words, the workspace or the outputs.
 *
 *   m2f_rle_decode_bits_ragged   positions / total / offsets as m2f_rle_decode_bits.  sizes (M, 2) int32 =
 *                         (H, W) per mask; out_offsets (M) int64 = the word offset of mask m in out
 *                         (out_words words); blocks (num_blocks, 2) int32 = (mask, block of 256 columns),
 *                         one row per workgroup: ceil(W_m / 256) rows for mask m, so the grid is the sum over
 *                         the masks and not M times the widest.  Every word of every plane is stored exactly
 *                         once, tail bits zero; words between planes (padding) are not written.
 *   m2f_bits_pair_counts_ragged  a batch of groups (a group is one image).  groups (G,
 *                         M2F_RAGGED_GROUP_FIELDS) int64 = H, W, na, nb, a_start, b_start, inter_start,
 *                         tile_start: the group's planes are words + a_offsets[a_start + i], i < na, and
 *                         words + b_offsets[b_start + j], j < nb (a_offsets (total_a), b_offsets (total_b)
 *                         int64 word offsets); a_start, b_start and inter_start are the running sums of na, nb
 *                         and na * nb, tile_start of the group's tile rows.  tiles (num_tiles, 4) int32 =
 *                         (group, a-tile, b-tile, chunk), one row per workgroup, for group g in the order
 *                         ((a-tile * tiles_b + b-tile) * chunks + chunk) with tiles_a = max(1, ceil(na /
 *                         M2F_PAIR_TA)), tiles_b = max(1, ceil(nb / M2F_PAIR_TB)), chunks = ceil(H * words /
 *                         M2F_PAIR_CHUNK_WORDS), and no rows when na = nb = 0: a small image costs its own
 *                         tiles only.  Outputs, int64:
 *                           inter  (num_inter = sum na * nb)  group-major, row-major (na, nb) within a group
 *                           area_a (total_a), area_b (total_b)
 *                         Two launches whatever G is.  A workgroup uses 128-bit loads when `words` is 16-byte
 *                         aligned, the offsets of all planes of its tile are multiples of 4 and four-word
 *                         reads stay inside the buffer, 32-bit loads otherwise; bits beyond W in a row's last
 *                         word and words beyond the plane's end are masked.  int32 partials per tile row go to
 *                         `workspace` (m2f_bits_pair_ragged_workspace bytes, contents on entry irrelevant) and
 *                         are summed in row order: no atomics, no zeroed buffer, the same bytes on every run.
 * Null pointers, negative sizes, misaligned pointers or a short workspace give M2F_EINVAL; more than 2^31 - 1
 * table rows M2F_EUNSUPPORTED; all before any HIP call.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_RAGGED_GROUP_FIELDS = 8 };
int m2f_rle_decode_bits_ragged(const int32_t* positions, int64_t total, const int64_t* offsets, int num_masks,
                               const int32_t* sizes, const int64_t* out_offsets, const int32_t* blocks,
                               int64_t num_blocks, int32_t* out, int64_t out_words, void* stream);
int m2f_bits_pair_ragged_workspace(int64_t num_tiles, int64_t* bytes);
int m2f_bits_pair_counts_ragged(const int32_t* words, int64_t total_words, const int64_t* groups, int num_groups,
                                const int64_t* a_offsets, int64_t total_a, const int64_t* b_offsets, int64_t total_b,
                                const int32_t* tiles, int64_t num_tiles, int64_t num_inter, int64_t* inter,
                                int64_t* area_a, int64_t* area_b, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Label-pair counts of a ragged batch of images (semantic mIoU and panoptic PQ, bm2f_amd/label_counts.py).
 * Image i has P_i pixels and two label planes: a (ground truth; a_bytes 1 = uint8, 2 = int16, 4 = int32) at element
 * offset a_off of the flat buffer `a` (a_elems elements) and b (prediction; b_bytes 1 = uint8, 2 = int16, 4 = int32,
 * 8 = int64) at b_off of `b`.  Offsets are in elements and need not be aligned; aligned parts are read 8 or 16
 * bytes at a time when the buffer starts on 16 bytes.  Such a load stays inside an aligned 16-byte block that holds
 * at least one byte of the plane; the neighbours' elements it brings along are masked.
 *
 *   images (G, M2F_LABEL_IMAGE_FIELDS) int64 = a_off, b_off, pixels, rows, cols, out_off, id_off, id_count.
 *       The image's table is rows x cols int64 counters, row-major, at out + out_off; rows * cols < 2^31.
 *       Several images may name one out_off (of equal cols): the kernel adds, the caller zeroes `out` and `bad`.
 *   row of a value v of a:
 *       id_count < 0 (direct)   v == ignore (when has_ignore) -> rows - 1; else v in [0, rows - 1) -> v;
 *                               anything else adds 1 to bad[i] and the pixel is not counted.
 *       id_count >= 0 (id list) ids[id_off .. id_off + id_count) int32, sorted ascending without repeats,
 *                               id_count <= min(M2F_LABEL_MAX_IDS, rows - 1): v found at index j -> j, v not in
 *                               the list -> rows - 1.  Any int32 id works.
 *   column of a value w of b:   w in [0, cols) -> w; anything else adds 1 to bad[i], the pixel is not counted.
 *   blocks (num_blocks, 2) int32 = (image, chunk), one row per workgroup: image i has ceil(n_i /
 *       M2F_LABEL_CHUNK_VECS) rows with n_i = ceil((a_off % M2F_LABEL_VEC + P_i) / M2F_LABEL_VEC), none when
 *       P_i = 0.
 *   path 0: tables are privatised in LDS when max_bins, the largest rows * cols of the batch, is at most
 *       M2F_LABEL_LDS_BINS, else added with wave-merged global atomics; 1 forces LDS (M2F_EINVAL when max_bins is
 *       beyond it), 2 forces the global path.  Either way the counts are exact integers, the same on every run.
 * One launch whatever G is.  Null pointers, negative sizes, unknown widths or paths, or misaligned buffers give
 * M2F_EINVAL; more than 2^31 - 1 table rows or counters M2F_EUNSUPPORTED; all before any HIP call.  The kernel checks
 * every field it takes from a table against the sizes passed by value.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_LABEL_IMAGE_FIELDS = 8, M2F_LABEL_VEC = 8, M2F_LABEL_CHUNK_VECS = 8192, M2F_LABEL_LDS_BINS = 24576,
       M2F_LABEL_MAX_IDS = 1024 };
int m2f_label_counts_geometry(int* vec, int* chunk_vecs, int* lds_bins, int* max_ids);
int m2f_label_pair_counts_ragged(const void* a, int a_bytes, int64_t a_elems, const void* b, int b_bytes,
                                 int64_t b_elems, const int64_t* images, int num_images, const int32_t* ids,
                                 int64_t total_ids, const int32_t* blocks, int64_t num_blocks, int has_ignore,
                                 int ignore, int64_t max_bins, int path, int64_t* out, int64_t out_len, int64_t* bad,
                                 void* stream);
/* Label histograms of a ragged batch (which classes an image holds, and their areas): the same kernel without
 * the plane b.  images as above with cols = 1, id_count = -1 and b_off unused: the table of image i is its rows
 * counters at out + out_off, row v counting the pixels of value v in [0, rows - 1), row rows - 1 those equal to
 * `ignore` (when has_ignore); any other value adds 1 to bad[i].  blocks, max_bins, path, the exact 64-bit counters
 * and the argument checks are those of m2f_label_pair_counts_ragged. */
int m2f_label_histogram_ragged(const void* a, int a_bytes, int64_t a_elems, const int64_t* images, int num_images,
                               const int32_t* blocks, int64_t num_blocks, int has_ignore, int ignore,
                               int64_t max_bins, int path, int64_t* out, int64_t out_len, int64_t* bad,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO polygons -> bit planes (bm2f_amd/polygon.py; the definition, a restatement of rleFrPoly of
 * pycocotools' maskApi.c, is in DESIGN.md §3).  A polygon's mask is given by its crossings: positions
 * p = c * H + y in the column-major order, pixel q being set when an odd number of them is <= q.
 *
 *   m2f_poly_crossings    one thread per kept crossing of a batch of polygons.  edges (E,
 *                         M2F_POLY_EDGE_FIELDS) int32 = kind, xs, ys, steps, c0, H, W, polygon: the edge's
 *                         oriented start in fifths of a pixel (flat, kind 0: the smaller x; steep, kind 1: the
 *                         smaller y), its number of steps max(|dx|, |dy|), the first kept column c0 and the
 *                         image size and index of its polygon; slopes (E) fp64 = dy / dx (flat) or dx / dy
 *                         (steep), divided by the caller; starts (E) int64 = the running sum of the edges'
 *                         crossing counts, non-decreasing, starts[0] = 0; total = their sum.  Crossing j of
 *                         edge e is at the column c = c0 + j, u = 5 c + 2, and its row is
 *                         clamp(ceil((v - 2) / 5), 0, H) with
 *                           flat:  v = min(y(u - xs), y(u - xs + 1)),  y(t) = trunc(ys + s * t + 0.5)
 *                           steep: v = ys + t, t the last step in [0, steps] with x(t) <= u (s > 0) or
 *                                  x(t) >= u + 1 (s < 0), found by bisection, x(t) = trunc(xs + s * t + 0.5)
 *                         in fp64 with every operation rounded on its own (no FMA).  A row of kind 2 is one
 *                         "crossing" at H * W, the sentinel that closes a polygon.  keys (total) int64 =
 *                         (polygon << 32) | p: sorting them orders every polygon's positions.  No atomics, no
 *                         loop over an edge's length.
 *   m2f_poly_decode_bits_ragged   annotation a is the OR of the polygons part_offsets[a] .. part_offsets[a + 1]
 *                         (part_offsets (A + 1) int64, clamped to [0, num_polys]; none: a zero plane); polygon q
 *                         owns the sorted positions[pos_offsets[q] : pos_offsets[q + 1]] (pos_offsets
 *                         (num_polys + 1) int64, clamped to [0, total]).  sizes, out_offsets, blocks, out and
 *                         out_words as m2f_rle_decode_bits_ragged, per annotation: every word of every plane
 *                         is stored exactly once, tail bits zero, padding words are not written.
 * Null pointers, negative sizes or misaligned pointers give M2F_EINVAL; more than 2^31 - 1 crossings or
 * table rows M2F_EUNSUPPORTED; all before any HIP call.  The kernels check every index they take from a table
 * against the sizes passed by value.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_POLY_EDGE_FIELDS = 8 };
int m2f_poly_crossings(const int32_t* edges, const double* slopes, const int64_t* starts, int64_t num_edges,
                       int64_t total, int64_t* keys, void* stream);
int m2f_poly_decode_bits_ragged(const int32_t* positions, int64_t total, const int64_t* pos_offsets,
                                int64_t num_polys, const int64_t* part_offsets, int num_anns, const int32_t* sizes,
                                const int64_t* out_offsets, const int32_t* blocks, int64_t num_blocks, int32_t* out,
                                int64_t out_words, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mask planes -> boundary planes (COCO Boundary AP, bm2f_amd/mask_boundary.py).  The definition is
 * mask_to_boundary of the boundary-iou-api, restated:  boundary = mask & ~erode(mask), where pixel (y, x)
 * survives the erosion when every pixel of the (2d + 1) x (2d + 1) window centred on it lies inside the
 * image and is set (cv2.erode with a 3 x 3 kernel, d iterations, on the mask padded by a ring of zeros).
 *
 *   m2f_bits_boundary_ragged   words (total_words) int32 holds the planes in the layout above, plane m of
 *                         sizes[m] = (H, W) int32 at the word offset offsets[m] (int64, any alignment);
 *                         dilations (M) int32 = d per plane, 1 <= d <= max_dilation <= M2F_BOUNDARY_D_MAX
 *                         (max_dilation sizes the kernel's LDS; a plane with a larger d is not written).
 *                         blocks (num_blocks, 2) int32 = (plane, tile), one row per workgroup: plane m has
 *                         ceil(H / M2F_BOUNDARY_BAND_ROWS) * ceil(words / M2F_BOUNDARY_TILE_WORDS) rows,
 *                         tile = band * ceil(words / M2F_BOUNDARY_TILE_WORDS) + column tile.  out
 *                         (total_words) int32 receives the boundary planes at the same offsets: every word
 *                         of every plane is stored exactly once, tail bits (x >= W) zero; words between
 *                         planes are not written.  Set tail bits of the input and the words between its
 *                         planes are ignored: x >= W is outside the image.  d >= H or d >= W is allowed
 *                         (the erosion is empty and the boundary is the mask).  One launch whatever M is;
 *                         no atomics, no memset; words and out must not overlap.
 *   m2f_bits_boundary_tiles    the three constants, for callers that build the table.
 * Null pointers, non-positive sizes, max_dilation outside [1, M2F_BOUNDARY_D_MAX], misaligned or
 * overlapping buffers give M2F_EINVAL; more than 2^31 - 1 words or table rows M2F_EUNSUPPORTED; all before
 * any HIP call.  The kernel checks every value it takes from a table against the sizes passed by value.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_BOUNDARY_BAND_ROWS = 64, M2F_BOUNDARY_TILE_WORDS = 24, M2F_BOUNDARY_D_MAX = 128 };
int m2f_bits_boundary_tiles(int* band_rows, int* tile_words, int* d_max);
int m2f_bits_boundary_ragged(const int32_t* words, int64_t total_words, int num_planes, const int32_t* sizes,
                             const int64_t* offsets, const int32_t* dilations, const int32_t* blocks,
                             int64_t num_blocks, int max_dilation, int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Input views (bm2f_amd/image_views.py; the definition, a restatement of Pillow's 8-bit resize, is in DESIGN.md
 * §3): resize, crop, flip, canvas fill, normalise, pad and stack of the V views of a call in one launch.
 *
 *   views (V, M2F_VIEW_FIELDS) int64, one row per view =
 *       0 src_off   element offset of the view's source in `src`      1 H, 2 W   source size
 *       3 stride    elements between source rows (>= 3 W for an image, >= W for a plane: a crop view of a larger
 *                   tensor is read in place)
 *       4 rh, 5 rw  the resized size                 6 cy0, 7 cx0, 8 ch, 9 cw   crop window in resized coordinates
 *       10 Hc, 11 Wc  the canvas (<= out_h, out_w)   12 flip_in   mirror the source columns before the resize
 *       13 flip_out   mirror the crop window's columns after the resize
 *       14 tab_x, 15 tab_y   element offsets of the two axes' tables in `tables`
 *       16 fill     the value of a canvas element outside crop and resized image
 *       17 plane_stride   elements between the planes of a label source (images: unused)
 *       18 kx, 19 ky      ksize per axis of an image, 0 for an axis whose size does not change (labels: unused)
 *     Output element (y, x) of view v:  y >= Hc or x >= Wc: the pad.  Else with ry = cy0 + y and rx = cx0 + (flip_out ?
 *     cw - 1 - x : x): the resized pixel (ry, rx) when y < ch, x < cw, 0 <= ry < rh and 0 <= rx < rw, else fill.
 *   tables  int32.  Image axis (in -> out, ksize k > 0): 2 * out values (xmin, n) then out * k coefficients at 22
 *           fractional bits, a pass being clip8((2^21 + sum_{j < n} pixel[xmin + j] * coeff[j]) >> 22); horizontal
 *           first, its result rounded to uint8.  k must be 2 * ceil(max(in / out, 1)) + 1 <= M2F_VIEW_MAX_KSIZE.
 *           Label axis: out source indices.  The kernels clamp what they read from `tables` into the source.
 *   views_host / views_dev   the same table in host and in device memory: the host copy is checked row by row
 *           before anything is launched, the kernels read the device copy and skip a row that fails the same check.
 *
 *   m2f_image_views   src uint8 HWC with 3 channels; out (V, 3, out_h, out_w) of out_dtype (M2F_F32 / F16 / BF16 /
 *                     M2F_U8).  A pixel p is stored as p (uint8), float(p), or with `normalize`
 *                     (float(p) - mean[c]) / std[c] in fp32 with a correctly rounded division, rounded once more for
 *                     a 16-bit output; fill is stored the same way, pad_value as it is.
 *   m2f_label_views   src (num_planes, H, W) planes of elem_bytes 1, 2 or 4 per view, out (V, num_planes, out_h,
 *                     out_w) of the same element type; nearest gather; the pad is the view's fill.
 * Every output element is stored exactly once; no atomics.  Null pointers, non-positive counts or misaligned
 * pointers give M2F_EINVAL.  An unknown dtype, mean / std with a uint8 output, a ksize beyond
 * M2F_VIEW_MAX_KSIZE (a down-scale beyond 65x) and a row whose sizes are not positive or whose source, tables
 * or canvas leave src_numel, tables_numel or (out_h, out_w) give M2F_EUNSUPPORTED.  All before any HIP call.
 *
 * Colour stage (bm2f_amd/color_aug.py is the definition): m2f_image_views_color is m2f_image_views
 * with photometric operations applied to every pixel that shows the image (never to fill or pad), on the three
 * channels of the pixel together, between the vertical pass and the normalisation.
 *   colors (V, M2F_COLOR_FIELDS) fp64, one row per view =
 *       0 n   operations, 0 .. M2F_COLOR_MAX_OPS      1 swap   the operations see channels 2, 1, 0
 *       2 ci  index of the one M2F_COLOR_CONTRAST operation, -1 without       3 unused
 *       4 + 3 k, 5 + 3 k, 6 + 3 k   code, a, b of operation k:
 *         M2F_COLOR_CONVERT     clip(fp32(p) * fp32(a) + fp32(b), 0, 255), truncated; two fp32 roundings
 *         M2F_COLOR_SSD_SAT     OpenCV's 8-bit BGR -> HSV, S = convert(S, a, 0), HSV -> BGR
 *         M2F_COLOR_SSD_HUE     BGR -> HSV, H = (H + int(a)) mod 180 (non-negative), HSV -> BGR
 *         M2F_COLOR_CONTRAST    clip(a * mean + fp64(fp32(b) * fp32(p)), 0, 255), truncated; mean = sum / count in
 *                               fp64 over the 3 channels of the pixels the view shows, after operations 0 .. ci - 1
 *         M2F_COLOR_SATURATION  the same with gray = fma(p2, 0.114, fma(p1, 0.587, p0 * 0.299)) in fp64 for mean
 *   hsv_offset   element offset in `tables` of sdiv[256] then hdiv[256] (OpenCV's division tables); read only when a
 *                view has an SSD_SAT or SSD_HUE operation, else it may be -1
 *   sums         (V) int64 in device memory, what m2f_image_views_sum wrote; read only for views with ci >= 0 and
 *                required (non-null) when there is one
 *   m2f_image_views_sum   per view with ci >= 0 the exact integer sum the mean is formed from, to workspace[v]
 *                (the host never needs it): per-workgroup partial sums in workspace[V ..], then one fixed-order
 *                reduction per view; integer arithmetic throughout, so the result is bitwise repeatable.
 *                m2f_image_views_sum_workspace gives the int64 words it needs.
 * Rows of `colors` are checked like rows of `views` (M2F_EUNSUPPORTED names the row): n, ci and the codes must be the
 * integers above, a and b finite, |a| <= 2^20 for SSD_HUE.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_U8 = 3 };
enum { M2F_VIEW_FIELDS = 20, M2F_VIEW_MAX_KSIZE = 131 };
enum { M2F_COLOR_FIELDS = 16, M2F_COLOR_MAX_OPS = 4 };
enum { M2F_COLOR_CONVERT = 1, M2F_COLOR_SSD_SAT = 2, M2F_COLOR_SSD_HUE = 3, M2F_COLOR_CONTRAST = 4,
       M2F_COLOR_SATURATION = 5 };
int m2f_image_views(const void* src, int64_t src_numel, const int64_t* views_host, const int64_t* views_dev,
                    int num_views, const int32_t* tables, int64_t tables_numel, int normalize, float mean0,
                    float mean1, float mean2, float std0, float std1, float std2, float pad_value, int out_dtype,
                    void* out, int out_h, int out_w, void* stream);
int m2f_label_views(const void* src, int elem_bytes, int64_t src_numel, const int64_t* views_host,
                    const int64_t* views_dev, int num_views, int num_planes, const int32_t* tables,
                    int64_t tables_numel, void* out, int out_h, int out_w, void* stream);
int m2f_image_views_color(const void* src, int64_t src_numel, const int64_t* views_host, const int64_t* views_dev,
                          int num_views, const int32_t* tables, int64_t tables_numel, const double* colors_host,
                          const double* colors_dev, int64_t hsv_offset, const int64_t* sums, int normalize,
                          float mean0, float mean1, float mean2, float std0, float std1, float std2, float pad_value,
                          int out_dtype, void* out, int out_h, int out_w, void* stream);
int m2f_image_views_sum_workspace(const int64_t* views_host, int num_views, int out_h, int out_w, int64_t* words);
int m2f_image_views_sum(const void* src, int64_t src_numel, const int64_t* views_host, const int64_t* views_dev,
                        int num_views, const int32_t* tables, int64_t tables_numel, const double* colors_host,
                        const double* colors_dev, int64_t hsv_offset, int out_h, int out_w, int64_t* workspace,
                        int64_t workspace_words, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance views (bm2f_amd/instance_views.py): the views above applied to one-bit-per-pixel instance
 * masks, a ragged number per image, with the tight box and the area of every output mask.  It restates
 * transform_instance_annotations on a decoded mask (PIL NEAREST resize, crop, flip, zero pad) followed by
 * BitMasks.get_bounding_boxes and a pixel count.
 *
 *   words   (total_words) int32, the flat buffer of m2f_rle_decode_bits_ragged / m2f_poly_decode_bits_ragged: mask m
 *           is H x ceil(W / 32) words at its word offset, bit x % 32 of word x / 32.  Set tail bits (x >= W) and the
 *           words between planes are ignored.
 *   views, tables, views_host / views_dev   the view table of m2f_label_views (label axes: `tables` holds source
 *           indices).  Fields 0, 3, 16 and 17 (source offset, strides, fill) are not read, but are checked as rows of
 *           a source of unbounded length: pass 0, W, 0, 0.
 *   masks   (M, M2F_BITS_VIEW_MASK_FIELDS) int64, one row per mask = 0 word offset, 1 H, 2 W, 3 view index.  H and W
 *           must be those of the view's row.  masks_host / masks_dev as for the views.
 *   Output pixel (y, x) of mask m under its view:  y >= Hc or x >= Wc: 0.  Else with ry = cy0 + y and rx = cx0 +
 *           (flip_out ? cw - 1 - x : x): the source bit (taby[ry], flip_in ? W - 1 - tabx[rx] : tabx[rx]) when y < ch,
 *           x < cw, 0 <= ry < rh and 0 <= rx < rw, else 0.
 *   out     out_form M2F_BITS_VIEW_BITS: (M, out_h, ceil(out_w / 32)) int32 bit planes, tail bits zero;
 *           M2F_BITS_VIEW_BYTES: (M, out_h, out_w) uint8, 0 or 1.  Every word or byte is stored exactly once.
 *   stats   (M, 5) int32 = x0, y0, x1, y1, area of the output mask, x1 and y1 exclusive: the first and last set
 *           column and row (+ 1) and the number of set pixels; an empty mask gives five zeros.
 *   workspace   int32 words, m2f_bits_views_workspace(num_masks, out_h) of them: a workgroup owns
 *           M2F_BITS_VIEW_BAND_ROWS rows of one mask's plane (workgroup b: mask b / bands, band b % bands, bands =
 *           ceil(out_h / M2F_BITS_VIEW_BAND_ROWS)) and writes its partial stats there; a second kernel reduces each
 *           mask's partials in band order.  Two launches whatever M and V are; no atomics, no memset; integer
 *           arithmetic throughout, so out and stats are bitwise repeatable.
 * Null pointers, non-positive counts, misaligned pointers, an unknown out_form or a workspace that is too small
 * give M2F_EINVAL.  More than 2^31 - 1 words in or out (bytes / 4 for the uint8 form), out_h * out_w or H * W beyond
 * 2^31 - 1, a view row as for m2f_label_views, and a mask row whose view is out of range, whose size is not positive
 * or not the view's, or whose plane leaves the buffer give M2F_EUNSUPPORTED naming the row.  All before any HIP
 * call.  The kernel repeats the row checks on the device copies and writes zeros for a mask that fails them.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_BITS_VIEW_MASK_FIELDS = 4, M2F_BITS_VIEW_BAND_ROWS = 32 };
enum { M2F_BITS_VIEW_BITS = 0, M2F_BITS_VIEW_BYTES = 1 };
int m2f_bits_views_workspace(int num_masks, int out_h, int64_t* words);
int m2f_bits_views(const int32_t* words, int64_t total_words, const int64_t* views_host, const int64_t* views_dev,
                   int num_views, const int32_t* tables, int64_t tables_numel, const int64_t* masks_host,
                   const int64_t* masks_dev, int num_masks, int out_form, void* out, int out_h, int out_w,
                   int32_t* stats, int32_t* workspace, int64_t workspace_words, void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO RLE of the segments of label maps, and its inverse (bm2f_amd/label_rle.py): what
 * detectron2's encode_json_sem_seg, datasets/prepare_ade20k_ins_seg.py and the panoptic-to-detection conversion get
 * from pycocotools.mask.encode(map == v) once per value, without a dense mask per segment.  A label map read
 * column-major (p = x * H + y) is a sequence of runs of one label; the segment `map == v` has the transitions s and,
 * when e < H * W, e of every run [s, e) of v, and the RLE format is that of m2f_rle_* above.
 *
 *   images (B, M2F_LABEL_RLE_IMAGE_FIELDS) int64, device = 0 address of pixel (0, 0) of the plane (label_bytes 1 =
 *           uint8, 2 = int16, 4 = int32 elements, unit column stride), 1 H, 2 W (both > 0, H * W < 2^31), 3 row stride
 *           in elements, 4 col_base (running sum of W), 5 block_base (running sum of ceil(W / 256)), 6 the key of the
 *           label whose pixels belong to no segment or -1, 7 unused.  The key of (image i, label v) is
 *           (i << 32) | (uint32(v) ^ 0x80000000): int64 order is (image, signed label).  The planes are read through
 *           the addresses of the table, which the entry points cannot check: they are the caller's.
 *   m2f_label_rle_col_counts  counts (total_cols) int32: the runs that start in column col_base + x (a run starts
 *           where a label differs from the pixel before it in column-major order; pixel 0 starts one).  Grid =
 *           num_blocks = sum ceil(W / 256).
 *   m2f_label_rle_runs        col_start = exclusive scan of counts.  run_pos[o] int32 / run_key[o] int64 = start and
 *           key of run o; a slot at or beyond `capacity` is never written.
 *   The caller sorts run_key stably (sorted_key, perm): runs of one segment become adjacent, in position order.
 *   m2f_label_rle_spans       per sorted run j: start[j], end[j] (the next run of its image, run_base (B + 1) int64
 *           being the images' first runs, or H * W), ntrans[j] = 0 when the label is no segment (the ignore key, or
 *           absent from seg_key when seg_key is given), else 1 + (end < H * W); first[j] = 1 on the first run of a
 *           segment.
 *   m2f_label_rle_seg_keys    seg_rank = inclusive scan of first: seg_key[seg_rank[j] - 1] = sorted_key[j] where
 *           first[j], *num_segments = seg_rank[num_runs - 1] (both capped by seg_capacity).  Not called when the
 *           caller supplies seg_key (ascending) and *num_segments itself.
 *   m2f_label_rle_segments    tscan = inclusive scan of ntrans.  One wave per segment slot s <= seg_capacity.  For s <
 *           *num_segments: the transitions of its runs and the closing H * W go to positions[seg_start[s] + s ...],
 *           seg_start[s] = the transitions of all runs before its first; headers[s] (M2F_LABEL_RLE_HEADER_FIELDS
 *           int32) = image, label, area, xmin, ymin, xmax, ymax (0, 0, -1, -1 when empty), H * W.  A run that
 *           crosses a column boundary spans rows 0 .. H - 1.  For s >= *num_segments: seg_start[s] = tscan[last],
 *           headers zero, nothing else: with `positions` zeroed on entry these are one-entry dummies, so that
 *           m2f_rle_deltas / m2f_rle_chars run on (positions, seg_start, seg_capacity + 1, width 1, capacity) although
 *           the number of segments is known on the device only.
 *   m2f_rle_paint_labels      the inverse.  positions / total / offsets (num_segments + 1) as m2f_rle_decode_bits;
 *           values (num_segments) int32; images (B, M2F_LABEL_RLE_PAINT_FIELDS) int64 = 0 H, 1 W, 2 first segment,
 *           3 end segment, 4 element offset of the plane in out, 5 block_base (running sum of ceil(W / 64) *
 *           ceil(H / 4)).  out[offset + y * W + x] = values[s] of the last segment s of the image with an odd number
 *           of run ends <= x * H + y, else fill: later segments overwrite earlier ones.  A lane owns one pixel, a
 *           wave 64 consecutive x of one row; one launch, every element stored once, no atomics, no memset.
 * Null pointers, negative sizes, misaligned tables and a label_bytes other than 1, 2, 4 give M2F_EINVAL; more than
 * 2^31 - 1 workgroups M2F_EUNSUPPORTED; all before any HIP call.  The kernels check every index they take from a
 * device table against the sizes passed by value.
 * ------------------------------------------------------------------------------------------- */
enum { M2F_LABEL_RLE_IMAGE_FIELDS = 8, M2F_LABEL_RLE_HEADER_FIELDS = 8, M2F_LABEL_RLE_PAINT_FIELDS = 6 };
int m2f_label_rle_col_counts(const int64_t* images, int num_images, int64_t num_blocks, int label_bytes,
                             int32_t* counts, int64_t total_cols, void* stream);
int m2f_label_rle_runs(const int64_t* images, int num_images, int64_t num_blocks, int label_bytes,
                       const int64_t* col_start, int64_t total_cols, int32_t* run_pos, int64_t* run_key,
                       int64_t capacity, void* stream);
int m2f_label_rle_spans(const int64_t* sorted_key, const int64_t* perm, int64_t num_runs, const int32_t* run_pos,
                        const int64_t* run_base, const int64_t* images, int num_images, const int64_t* seg_key,
                        const int64_t* num_segments, int64_t seg_capacity, int32_t* start, int32_t* end,
                        int32_t* ntrans, int32_t* first, void* stream);
int m2f_label_rle_seg_keys(const int64_t* sorted_key, const int32_t* first, const int64_t* seg_rank, int64_t num_runs,
                           int64_t* seg_key, int64_t seg_capacity, int64_t* num_segments, void* stream);
int m2f_label_rle_segments(const int64_t* sorted_key, int64_t num_runs, const int32_t* start, const int32_t* end,
                           const int32_t* ntrans, const int64_t* tscan, const int64_t* images, int num_images,
                           const int64_t* seg_key, const int64_t* num_segments, int64_t seg_capacity,
                           int32_t* positions, int64_t capacity, int64_t* seg_start, int32_t* headers, void* stream);
int m2f_rle_paint_labels(const int32_t* positions, int64_t total, const int64_t* offsets, int64_t num_segments,
                         const int32_t* values, const int64_t* images, int num_images, int64_t num_blocks,
                         int64_t fill, int label_bytes, void* out, int64_t out_elems, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BM2F_H_ */

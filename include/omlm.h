/* libomlm_hip.so -- C ABI of the MI355X (gfx950) kernels behind the open-musiclm
 * TokenConditionedTransformer hot path.
 *
 * The reference (zhvng/open-musiclm) is pure Python/PyTorch and has NO FFI / plugin / custom-op
 * interface for this path; its only fused-operator seam is the optional
 * xformers.ops.memory_efficient_attention call at open_musiclm/transformer.py:298.  Each entry point
 * below therefore names the reference *Python* code whose arithmetic it replaces.  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add at each of those sites.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (omlm_last_error() gives the thread-local message);
 *   - all pointers are DEVICE pointers unless stated otherwise; the caller owns every buffer, including
 *     workspaces; the library never allocates device memory, never synchronises, never changes the device;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call returns at once;
 *   - dtype codes: 0 = fp32, 1 = bf16, 2 = fp16 (IEEE half).  For GEMM / attention OPERANDS, fp32 selects the "bf16x3" split
 *     (hi*hi + hi*lo + lo*hi on the bf16 matrix cores, fp32 accumulation), bf16 / fp16 the single-pass modes
 *     (v_mfma_f32_32x32x16_bf16 / _f16, same rate; precision modes "bf16x3" / "bf16" / "fp16" of the Python layer).  A call
 *     uses ONE 16-bit type: bf16 operands give fp32 or bf16 outputs, fp16 operands fp32 or fp16 outputs.  The library holds
 *     a bf16 and an fp16 copy of every 16-bit kernel; these entry points dispatch on the code;
 *   - row-major everywhere; "ld" = row pitch in elements.
 *
 * Not in this library: the data-parallel gradient exchange.  SURVEY.md 8b sketches an `omlm_allreduce_flat` export; it does not exist --
 * the exchange is ONE torch.distributed (backend "nccl" = RCCL over xGMI) SUM all-reduce of the flat fp32 gradient buffer per optimizer
 * step, issued by the Python host between the captured micro-step and omlm_adamw_clip_step (open_musiclm_amd/parallel.py:
 * DataParallel.allreduce_sum_; the reference: accelerate / DDP bucketed all-reduces on every micro-batch backward, trainer.py:154-155,439).
 * A collective is a host-side call on a communicator the host owns; nothing of it would gain from crossing this C ABI.
 */
#ifndef OMLM_H
#define OMLM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int         omlm_version(void);
const char* omlm_last_error(void);
void        omlm_set_error(const char* msg);

/* C[m,n] = alpha * sum_k A(m,k) B(n,k) (+ Cin[m,n]).  Replaces every nn.Linear / einsum contraction on the path:
 * to_q / to_kv / to_out (transformer.py:203-212,254,333), ConvFeedForward Linear layers (:144,:149), the
 * per-quantizer logit heads einsum 'q c d, b n q d -> b n q c' (open_musiclm.py:173,180), RelativePositionBias
 * Linear layers (transformer.py:48-53) and the autograd backward of each.
 * a_kmajor/b_kmajor: operand stored [K, M] / [K, N] instead of [M, K] / [N, K].
 * a_map / b_map / c_map (optional, int32): physical row of each logical row (k row for k-major operands);
 * c_map < 0 skips the row.  a_rows / b_rows: physical row counts (bounds for out-of-range zero fill).
 * workspace / workspace_bytes (optional; 16-bit operands): caller-owned scratch for the deterministic split-K of the peeled tail -- the m-tile
 * rows behind the last full round of 256 x 256 tiles have their K range cut into slices that fill the machine, each slice stores its partial
 * tile to its own plane of the workspace, a reduction kernel adds the planes in a fixed order with the residual and writes the output type.
 * omlm_gemm_tail_workspace_bytes(M, N) bounds what an M x N output needs; a smaller buffer or NULL / 0 keeps the one-launch tail.  The library
 * keeps no pointer: the buffer belongs to the call, one buffer per stream that launches GEMMs concurrently.  $OMLM_GEMM_TAIL_SPLIT=0: off. */
int omlm_gemm(const void* A, const void* B, void* C, const float* Cin,
              const int* a_map, const int* b_map, const int* c_map, long long a_rows, long long b_rows,
              int M, int N, int K, int lda, int ldb, int ldc, int ldcin,
              int a_kmajor, int b_kmajor, int in_dtype, int out_dtype, float alpha,
              void* workspace, long long workspace_bytes, void* stream);
long long omlm_gemm_tail_workspace_bytes(int M, int N);

/* LayerNorm (transformer.py:24-31: F.layer_norm, learnable gamma, beta == 0, eps 1e-5).
 * fwd: y = LN(x)*gamma in out_dtype (pitch ldy); xcast (optional) = cast(x) for the K/V projection, which the
 *      reference feeds with the UN-normalised input (kv_input bound at :228 before the pre-norm at :250).
 * bwd: dx = dx_scale * (dres + LN^T(dy)); dxcast (optional) = cast(dx); dgamma += sum_rows dy * xhat.  workspace (optional,
 *      omlm_layernorm_bwd_workspace_bytes): per-workgroup dgamma partials instead of contended atomics. */
int omlm_layernorm_fwd(const float* x, const float* gamma, void* y, void* xcast, float* mean, float* rstd,
                       int M, int D, int ldy, float eps, int out_dtype, void* stream);
/* the same forward with the result as hi/lo planes of the 16-bit type out_dtype (1 = bf16, 2 = fp16): y = rne16(v), y_lo = rne16(v - y), both
 * at pitch ldy (precision "fp16ff": the FF-in omlm_gemm_planes16 reads both, the backward reads y) */
int omlm_layernorm_fwd_planes(const float* x, const float* gamma, void* y, void* y_lo, float* mean, float* rstd,
                              int M, int D, int ldy, float eps, int out_dtype, void* stream);
/* Row segments (the `_seg` entries here and of the ConvFeedForward forward below).  A segment (n_full, p0, n_live = n_full - p0) names the rows
 * [p0, n_full) of every sample of a [B * n_full, ..] buffer, held compact as [B * n_live, ..]: compact row r is full row
 * (r / n_live) * n_full + p0 + r % n_live.  The last layer's feed-forward block runs on such a segment when the heads read only a tail of
 * every sample (engine.live_rows).  n_full == 0: no segment, the plain entry.
 * omlm_layernorm_fwd*_seg: x [B * n_full, D] is read at the segment's rows; y, the statistics and every other output are compact ([M, ..],
 *   M = B * n_live) and bit-equal to the plain entry run on a gathered copy of x; xc (optional, [M, D] fp32) receives the gathered rows of x
 *   themselves in the same pass.  16-bit outputs, statistics required, no xcast.
 * omlm_layernorm_bwd2_seg: dy, x, the statistics and dres are compact; dx / dxcast are FULL-size ([B * n_full, D]): the segment's rows receive
 *   what the plain entry computes from the compact inputs (dgamma likewise), every row in front of the segment is written as zeros by the same
 *   launch.  16-bit dy and cast type, no dres2. */
int omlm_layernorm_fwd_seg(const float* x, const float* gamma, void* y, void* xcast, float* mean, float* rstd, float* xc,
                           int M, int D, int ldy, float eps, int out_dtype, int n_full, int p0, int n_live, void* stream);
int omlm_layernorm_fwd_planes_seg(const float* x, const float* gamma, void* y, void* y_lo, float* mean, float* rstd, float* xc,
                                  int M, int D, int ldy, float eps, int out_dtype, int n_full, int p0, int n_live, void* stream);
int omlm_layernorm_bwd2_seg(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                            const float* dres, const void* dres2, float* dx, void* dxcast, float* dgamma, float* workspace, int M, int D,
                            float dx_scale, int cast_dtype, int dy_dtype, int n_full, int p0, int n_live, void* stream);
long long omlm_layernorm_bwd_workspace_bytes(int D);
/* dy_dtype: 0 fp32, 1 bf16 / 2 fp16 (GEMM epilogue output).  dres2 [M, D] (optional): a second residual-gradient term in the type
 * cast_dtype names (dxcast may be null): the K/V projection's input gradient reaches the attention LayerNorm's backward as a 16-bit GEMM
 * output instead of being added to the fp32 residual gradient by the GEMM's own epilogue (146 MB read + 146 MB written per layer at
 * B = 32). */
int omlm_layernorm_bwd2(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                        const float* dres, const void* dres2, float* dx, void* dxcast, float* dgamma, float* workspace, int M, int D,
                        float dx_scale, int cast_dtype, int dy_dtype, void* stream);

/* q/k l2-normalise * learned per-dim scale, v pass-through (transformer.py:265-271; utils.py:68-69), dim_head 64. */
int omlm_qk_norm_fwd(const float* q_raw, const float* kv_raw, const float* q_scale, const float* k_scale,
                     void* q, void* k, void* v, int M, int H, int out_dtype, void* stream);
int omlm_qk_norm_bwd(const float* dq, const float* dk, const float* dv, const float* q_raw, const float* kv_raw,
                     const float* q_scale, const float* k_scale, void* dq_raw, void* dkv_raw,
                     float* dq_scale, float* dk_scale, int M, int H, int out_dtype, void* stream);

/* Attention q / k projections with the l2-norm + learned scale of transformer.py:265-271 folded into the GEMM epilogue (16-bit modes):
   C [M, N] = per 64-wide head h < groups: (A B^T)[:, h] / max(|.|, 1e-12) * scale[0..63]; heads >= groups pass through; columns
   >= c2_col0 go to C2 (pitch ldc2) when C2 is given (v of the k | v projection); norm_out [M, ldnorm] fp32 receives the norms.
   A [M, K], B [N, K] row-major, dtype 1 = bf16 / 2 = fp16 (operands and outputs).  Replaces to_q / to_kv + l2norm + scale
   (transformer.py:254,265-271) without the fp32 pre-norm tensors. */
int omlm_gemm_qknorm(const void* A, const void* B, void* C, void* C2, int c2_col0, int ldc2, const float* scale, float* norm_out,
                     int ldnorm, int groups, long long a_rows, long long b_rows, int M, int N, int K, int lda, int ldb, int ldc,
                     int dtype, void* stream);
/* its backward, from the normalised 16-bit q / k and the saved norms (qn [M, H], kn [M]) instead of the fp32 pre-norm projections;
   outputs as omlm_qk_norm_bwd (dq_raw [M, H*64], dkv_raw [M, 128] 16-bit; dq_scale / dk_scale [64] fp32, accumulated). */
int omlm_qk_norm_bwd2(const float* dq, const float* dk, const float* dv, const void* q, const void* k, const float* qn, const float* kn,
                      const float* q_scale, const float* k_scale, void* dq_raw, void* dkv_raw, float* dq_scale, float* dk_scale,
                      int M, int H, int dtype, void* stream);

/* Multi-query attention with rel-pos bias table and key mask (transformer.py:303-331; the same logical inputs as the xformers seam at
 * :275-301, without materialising attn_bias), causal or with a non-causal prefix of P >= 0 rows (:315-322, non_causal_prefix_size).
 * With Pn = min(P, N), score (i, j) is live iff
 *   j <= i   or   (i < Pn and j < Pn)
 * and the key mask keeps j (inside the prefix too).  P = 0 is causal; P >= N: every row sees every live key.
 * q [B*N, H*64], k, v [B*N, 64] (dtype), keymask [B, N] uint8 (1 = attend) or NULL, out [B*N, H*64] (dtype), lse [B, H, N] fp32 (log2 domain).
 * dtype: 0 = fp32 ("bf16x3" forward), 1 = bf16, 2 = fp16.
 * bias: the rel-pos table [N + Pn - 1, bias_ld] fp32, column = head, row = i - j + Pn - 1 (the distances -(Pn - 1) .. N - 1 in ascending
 * order: the negative distances of the scores above the diagonal inside the prefix, then the causal table [N, bias_ld] with row = i - j, the
 * un-gathered MLP output of RelativePositionBias, :60-64), or NULL.
 * biasT: that table prepared by omlm_attn_bias_prepare_group with the same P (omlm_attn_bias_prepare for P = 0), or NULL.
 * p: attention dropout in [0, 1) (round(p * 65536) < 65536; 0: none) with the keep-mask below, seed and the optional per-forward salt seed_dev
 * (one uint64 in device memory, read by the kernels: a captured graph draws new masks when the salt is bumped).  At p = 0 seed and seed_dev are
 * not read.  P < 0 or p outside [0, 1) is refused before any launch.
 * bwd: dq [B*N, H*64], dk, dv [B*N, 64] fp32 overwritten; dbias (bias's layout) accumulated (+=) over all its rows; delta scratch [B, H, N].
 * A query row without any live score (its key mask drops every key it could see, e.g. key 0 for row 0) has no softmax: on every route its out
 * row is 0 and its lse the sentinel 1e30, and the backward handed that lse gives it dq = 0 and lets it add nothing to dk, dv or dbias; no
 * NaN or Inf is produced, and the other rows of the call are not affected.  A masked key's score never enters another row's result: it sets
 * neither sum nor the running maximum (tests/test_gpu_attn_edges.py).  dk and dv rows of masked keys are exactly 0.
 *
 * Routes: 16-bit operands with biasT (or without any bias) run the second-generation kernels -- causal up to N = 16384
 * (omlm_attn_max_positions; 4096 < N runs their long forms: the forward's liveness prologue as a loop, the dQ kernel with a byte per key and a
 * sliding window of d(bias) bins in LDS, the dK / dV kernel summing per-workgroup slots of the workspace in a fixed order), a prefix while
 * their plans fit (N >= 32, N <= 4096 and the dQ kernel's LDS, which holds 8 (ceil32(N) + Pn - 1) d(bias) bins: about N + Pn <= 4000).
 * Otherwise, and for fp32 operands, the first-generation kernels read `bias`; they keep the table in LDS, which caps ceil32(N) + Pn - 1 at
 * about 3800 for the bf16x3 dQ kernel and about 4330 for the 16-bit one.  The forward and the backward decide alike, so a backward is always
 * handed the lse its forward wrote.
 * Limits: N past what the route takes is refused (OMLM_ERR_UNSUPPORTED) before any launch, and the message says which case it is -- causal
 * 16-bit operands past omlm_attn_max_positions(dtype, 0); fp32 operands past their LDS limit; a non-causal prefix, or a raw table without
 * biasT, past N = 4096 where the first-generation kernels no longer fit.
 *
 * Dropout (transformer.py:198,211: nn.Dropout(attn_dropout) on the softmax probabilities before P V), for the prefix's extra scores as for the
 * others: out = (P o Z / (1 - p)) V with Z the keep-mask below; lse stays that of the undropped P (bit-identical to p = 0), and the backward
 * regenerates Z: dV = (P o Z / (1 - p))^T dO, dS = P o (Z o dP~ / (1 - p) - delta), delta = rowsum(dO o O) as before.
 *
 * Keep-mask of probability (b, h, i, j) -- sample b, head h, query i, key j (i < 2^17, j < 2^16):
 *   hash(x)  = lowbias32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32 arithmetic)
 *   s        = seed + (seed_dev ? *seed_dev * 0x9E3779B97F4A7C15 : 0)                                (uint64, wrapping)
 *   headkey  = hash(hash(hash(lo32(s) ^ b) ^ hi32(s)) + h)
 *   w        = hash(headkey ^ (i << 15) ^ (j >> 1))
 *   draw     = (j & 1) ? w >> 16 : w & 0xFFFF
 *   Z        = draw >= round(p * 65536)                                                            (the FF dropout's rule)
 * It depends on nothing else (not on N, the tile shapes, the dtype or the kernel).  Keys j, j + 1 share one hash (16 bits each), and
 * headkey ^ (i << 15) is a per-(b, h, i) key hoisted out of the kernels' key loops. */
int omlm_mqa_attn_fwd(const void* q, const void* k, const void* v, const float* bias, const float* biasT, const unsigned char* keymask,
                      void* out, float* lse, int B, int N, int H, float scale, int bias_ld, int dtype, int P, float p,
                      unsigned long long seed, const unsigned long long* seed_dev, void* stream);
/* biasT: the table transposed to [ceil8(H)][ld'] with 64 leading zeros per row (then the Pn - 1 negative distances), zero tail,
 * pre-multiplied by log2(e): the layout the 16-bit kernels stream per key tile (omlm_attn_bias_table_floats(N, H, P) floats; bias == NULL
 * gives an all-zero table).  Built once per forward for all layers; fp32 ("bf16x3") operands read `bias` directly and ignore biasT. */
long long omlm_attn_bias_table_floats(int N, int H, int P);
/* The causal table of one layer (P = 0).  q_scale / k_scale (64 floats each, optional: the learned scales of transformer.py:269-271) or
 * qk_bound > 0 give the bound |q.k| <= max_d |q_scale_d k_scale_d| that lets the 16-bit forward exponentiate against a fixed reference point
 * (m_h = scale log2e bound + max bias_h, subtracted from the table) instead of a running maximum; neither: online softmax.
 * p_max_log2: 0 for bf16 / fp32 attention operands; 15 for IEEE half operands -- the reference point is lowered by 15 so that the
 * probability numerators span half's normal range (2^-13 .. 2^15) and the fixed form is selected while scale log2e 2 bound + the
 * table's range < 28 (wider: the flag in the table stays 0 and the forward runs its online-softmax kernel). */
int omlm_attn_bias_prepare(const float* bias, float* biasT, int N, int H, int bias_ld, const float* q_scale,
                           const float* k_scale, float qk_bound, float scale, int p_max_log2, void* stream);
/* The tables of `layers` attention layers over ONE rel-pos table in ONE launch (transformer.py:402-405 computes the bias once per forward and
 * hands it to every layer; here each layer's copy carries that layer's reference point): biasT[l] from q_scale[l] / k_scale[l], for a
 * prefix of P >= 0 rows (bias: the [N + Pn - 1, bias_ld] table above; the reference point covers the negative distances too).
 * biasT / q_scale / k_scale: HOST arrays (length `layers`) of DEVICE pointers; q_scale and k_scale both given or both NULL (then qk_bound). */
int omlm_attn_bias_prepare_group(const float* bias, float* const* biasT, int layers, int N, int H, int bias_ld,
                                 const float* const* q_scale, const float* const* k_scale, float qk_bound, float scale,
                                 int p_max_log2, int P, void* stream);
/* Most positions per sample omlm_mqa_attn_fwd followed by omlm_mqa_attn_bwd take for operands of `dtype` and a prefix of P rows: 16384 for
 * bf16 / fp16 causal (P = 0); for fp32 operands, and for 16-bit operands with P > 0, what the first-generation kernels' LDS-resident tables
 * allow (about 3800 and 4330; with P > 0 never less than the 4096 the second-generation kernels serve while their plan fits).  0 for an
 * unknown dtype or P < 0.  A forward alone reaches further with fp32 operands (its table is half the dQ kernel's). */
int omlm_attn_max_positions(int dtype, int P);
/* dbias_ws (optional, omlm_mqa_attn_bwd_workspace_bytes(B, N, H) bytes, contents irrelevant on entry and exit): the dQ kernel leaves
 * each wave's d(bias) bins there with plain stores and a small reduction adds them into dbias; without it every wave adds its bins into
 * dbias with device-scope atomics (measured 290 us per layer slower at B = 8, N = 1817, H = 16).
 * N <= 4096: B H ceil(N / 32)^2 128 bytes.  N > 4096 (16-bit operands): the same rows, then 64 KiB per workgroup of the dK / dV kernel
 * (a few hundred MB at B N = 32768), where each workgroup leaves its dK / dV sums for a reduction in a fixed order: with the workspace dq,
 * dk, dv and (at B = 1) dbias are the same bits from run to run; without it dK / dV are added with fp32 atomics in order of arrival, as they
 * are at N <= 4096 in either form.  Size the buffer with this function, not with the formula. */
long long omlm_mqa_attn_bwd_workspace_bytes(int B, int N, int H);
int omlm_mqa_attn_bwd(const void* q, const void* k, const void* v, const float* bias, const float* biasT, const unsigned char* keymask,
                      const void* out, const void* dout, const float* lse, float* delta, float* dq, float* dk, float* dv, float* dbias,
                      float* dbias_ws, int B, int N, int H, float scale, int bias_ld, int dtype, int P, float p, unsigned long long seed,
                      const unsigned long long* seed_dev, void* stream);
/* keep [B, H, N, N] uint8 (1 = kept): the mask above, as the attention kernels apply it (a test / integration hook for small shapes). */
int omlm_attn_dropout_keep(unsigned char* keep, int B, int N, int H, float p, unsigned long long seed,
                           const unsigned long long* seed_dev, void* stream);
/* Dropout of to_out (transformer.py:211,333: Sequential(Linear, Dropout)) with the residual add: x1 = x + Z' o y / (1 - p), x, y, x1 [M, D]
 * fp32 (D even).  Z' of element (row, c): w = hash(hash(hash(lo32(s) ^ row) ^ hi32(s)) ^ (c >> 1)), draw and rule as above, s = seed +
 * *seed_dev * 0x9E3779B97F4A7C15 -- seed is the layer's own, so Z' and the attention mask are independent.
 * bwd: dy = Z' o dx1 / (1 - p) in out_dtype (0 fp32, 1 bf16, 2 fp16), dx1 [M, D] fp32. */
int omlm_dropout_residual_fwd(const float* x, const float* y, float* x1, long long M, int D, float p, unsigned long long seed,
                              const unsigned long long* seed_dev, void* stream);
int omlm_dropout_residual_bwd(const float* dx1, void* dy, long long M, int D, float p, unsigned long long seed,
                              const unsigned long long* seed_dev, int out_dtype, void* stream);

/* Middle of ConvFeedForward: CausalDSConv -> GEGLU -> LayerNorm(F) -> Dropout (transformer.py:122-148).
 * h1: [M, 2*Fp] (value half cols [0,F), gate half cols [Fp, Fp+F)); h2: [M, Fp]; convw: taps re-packed tap-major and
 * padded, [3, 2*Fp] in h1's column layout (from the reference ds_conv.weight [2F,1,3]); gamma padded to [Fp] with zeros; both in
 * the operand dtype of h1 (they are re-read by every row, so in bf16 mode they travel as bf16 like every other operand);
 * dconv is accumulated in the reference layout [2F, 3].  rows are b*nseq + t.  Dropout mask = Philox-4x32-10(seed', element
 * index / 8): one 16-bit draw per element, kept iff draw >= p * 65536; seed' = seed + *seed_dev * golden-ratio (seed_dev optional device word: lets a captured HIP graph draw a new mask
 * on every replay).  With drop_bits given (or p == 0) both operand dtypes take the second-generation kernels (csrc/ffmid2.hip: a thread owns a few
 * channel pairs and walks down a strip of rows -- conv window, taps and gamma in fp32 registers, packed fp32 arithmetic, and a
 * backward that fuses dropout^T .. conv^T in one pass behind a row-sum prepass: no du round trip); their keep-mask comes from a
 * 32-bit integer hash of (seed', element index / 8) with the same 16-bit draws, and always reaches the backward through drop_bits.  drop_bits (optional, [M, Fp/8] bytes): the forward stores the keep-mask, 1 bit per element, and the
 * backward reads it instead of regenerating it (null: the backward regenerates the mask from the same (seed, salt) pair).
 * gh (optional, [M, Fp] in the operand dtype): the forward stores the normalised GEGLU output (before gamma and dropout); handed
 * to the backward, its LayerNorm^T sums and d(gamma) are formed from it without recomputing the conv and the GELU. */
int omlm_ffmid_fwd(const void* h1, const void* convw, const void* gamma, void* h2, float* mean, float* rstd,
                   int M, int nseq, int F, int Fp, float eps, float p, unsigned long long seed,
                   const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh, int dtype, void* stream);
/* The same forward on hi/lo planes of the 16-bit type `dtype` (1 = bf16, 2 = fp16; precision "fp16ff"): h1 (what omlm_gemm_planes16 left), the
 * conv taps and gamma are read as hi + lo (each *_lo plane in its hi plane's layout), h2 leaves as planes (h2 = rne16(y), h2_lo = rne16(y - h2))
 * for the FF-out omlm_gemm_planes16; gh, statistics and keep bits as above.  Strip kernels only: Fp <= 4096, drop_bits required when p > 0.
 * The backward is omlm_ffmid_bwd on the hi planes. */
int omlm_ffmid_fwd_planes(const void* h1, const void* h1_lo, const void* convw, const void* convw_lo, const void* gamma, const void* gamma_lo,
                          void* h2, void* h2_lo, float* mean, float* rstd, int M, int nseq, int F, int Fp, float eps, float p,
                          unsigned long long seed, const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh, int dtype, void* stream);
/* The forwards on a row segment (see omlm_layernorm_fwd_seg): every buffer holds the rows [p0, n_full) of each sample compact, nseq = n_full - p0,
 * and the strip kernels draw the keep bits those rows have in a launch over the full buffer -- drop_bits row r equals the full launch's row of
 * the same token, and h2 / gh / the statistics are bit-equal from the third row of every sample on (the first two see a zero conv window in
 * place of rows p0 - 2, p0 - 1).  The backward needs no segment: it reads the keep bits (omlm_ffmid_bwd on the compact buffers, nseq = n_live).
 * Where the wave-per-row kernels serve the call the mask is a function of the compact row instead. */
int omlm_ffmid_fwd_seg(const void* h1, const void* convw, const void* gamma, void* h2, float* mean, float* rstd,
                       int M, int nseq, int F, int Fp, float eps, float p, unsigned long long seed,
                       const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh, int dtype, int n_full, int p0, void* stream);
int omlm_ffmid_fwd_planes_seg(const void* h1, const void* h1_lo, const void* convw, const void* convw_lo, const void* gamma, const void* gamma_lo,
                              void* h2, void* h2_lo, float* mean, float* rstd, int M, int nseq, int F, int Fp, float eps, float p,
                              unsigned long long seed, const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh, int dtype,
                              int n_full, int p0, void* stream);
long long omlm_ffmid_bwd_workspace_bytes(int F, int Fp);
int omlm_ffmid_bwd(const void* dh2, const void* h1, const void* convw, const void* gamma, const float* mean,
                   const float* rstd, void* du_tmp, void* dh1, float* dgamma, float* dconv, float* workspace,
                   int M, int nseq, int F, int Fp, float p, unsigned long long seed,
                   const unsigned long long* seed_dev, const unsigned char* drop_bits, const void* gh, int dtype, void* stream);
int omlm_colsum_accumulate(const float* part, float* out, int P, int C, int ldp, void* stream);
/* out_i[c] += sum_p part_i[p * ldp_i + c] for `count` problems in ONE launch: the d(gamma) partial rows of every LayerNorm of a backward
 * pass (omlm_layernorm_bwd2 with dgamma NULL and a workspace leaves its [min(M, 2048), D] partial rows there instead of summing them). */
typedef struct omlm_colsum_desc { const float* part; float* out; int P, C, ldp; } omlm_colsum_desc;
int omlm_colsum_group(const omlm_colsum_desc* problems, int count, void* stream);
/* 1 (default): the column-strip kernels where their preconditions hold (Fp <= 4096, drop_bits present when
 * p > 0, and gh present for the backward); 0: the wave-per-row kernels (A/B runs, tests). */
int omlm_ffmid_set_impl(int impl);

/* Embedding gather + start-token interleave + concat (open_musiclm.py:123-145; utils.get_embeds :126-143) and its
 * transpose with the grad_shrink factor (utils.py:60-61).  tables/starts/pos: HOST arrays of device pointers. */
/* table_rows / pos_rows (optional HOST arrays, length nseq): row counts of the tables; an id or position past its table is
 * skipped like a pad (never an out-of-bounds access) and ORed into *err_flag (optional DEVICE int: bit 0 token id, bit 1
 * position, bit 2 label >= V from the cross entropy) -- torch's embedding raises a device assert in the same situation. */
int omlm_embed_gather_fwd(const int* ids, const int* seg, const int* posidx,
                          const float* const* tables, const float* const* starts, const float* const* pos,
                          int nseq, float* out, int B, int N, int D,
                          const long long* table_rows, const long long* pos_rows, int* err_flag, void* stream);
int omlm_embed_gather_bwd(const int* ids, const int* seg, const int* posidx,
                          float* const* dtables, float* const* dstarts, float* const* dpos,
                          int nseq, const float* dx, int B, int N, int D, float alpha,
                          const long long* table_rows, const long long* pos_rows, int* err_flag, void* stream);

/* Training-batch preparation as one launch: eos append + labels + last-token drop + conditioning pad / eos masking + key mask
   (TokenConditionedTransformerWrapper.forward, open_musiclm.py:340-376), per-quantizer offsets + start markers + concatenation
   (TokenConditionedTransformer.forward, :116-130,:139-145) and the forgetful mask (generate_mask_with_prob, utils.py:49-56: the n_drop
   largest of scores[b, 1:] are dropped).  ids[s]: int64 [B, len[s]]; labels[s]: int32 [B, len[s] + 1] or null; ids32 int32 [B, N]
   (-2 = start token, offsets applied); keymask uint8 [B, N]; scores fp32 [B, N] or null (no forgetful mask);
   N = sum_s (len[s] + 1) + (nseq - 1).
   Condition drop (training side of classifier-free guidance, below): null_u fp32 [B] or null.  With null_u, sample b trains on the null
   condition iff null_u[b] < null_p: at every id position p < len[0] of sequence 0 ids32 is -1 (the pad embedding's zero row) and the key
   mask is 1 before the forgetful mask is ANDed in, whatever the raw id was; the appended eos of sequence 0, every other sequence and all
   labels are what they are without it.  null_u == NULL: null_p is not read and the launch does what it always did.  nseq >= 2 then. */
int omlm_prepare_train_batch(const long long* const* ids, int* const* labels, const int* len, const int* eos, const int* Q,
                             const int* codebook, int nseq, int B, int pad_id, const float* scores, int n_drop,
                             int* ids32, unsigned char* keymask, int N, const float* null_u, float null_p, void* stream);

/* F.cross_entropy(logits, labels) pieces (open_musiclm.py:401-405): per-row lse + NLL sum; (softmax-onehot)*coef*g. */
int omlm_cross_entropy_fwd(const float* logits, const int* labels, float* row_lse, float* nll_sum,
                           int R, int V, int ld, int* err_flag, void* stream);
int omlm_cross_entropy_bwd(const float* logits, const int* labels, const float* row_lse, const float* gscale,
                           float coef, void* dlogits, int R, int V, int ld, int ldd, int out_dtype, void* stream);
/* Label smoothing (eps = label_smoothing in [0, 1), torch's F.cross_entropy(label_smoothing=) convention) and z-loss (zeta = z_loss,
   finite and >= 0; PaLM / T5X: zeta * lse^2 per row): extensions, training mode only; no reference counterpart.
   A live row (label y in [0, V)) with logits l[0..V), lse = log sum_c exp l[c], p = exp(l - lse):
       nll    = lse - l[y]
       smooth = lse - (1 / V) sum_c l[c]        (the mean over all V entries of -log p[c]; V counts the eos entry)
       z      = lse^2
       row loss = (1 - eps) nll + eps smooth + zeta z
       d row loss / d l[c] = p[c] (1 + 2 zeta lse) - (1 - eps) [c == y] - eps / V
   The loss over all sequences is sum_s w_s ((1 - eps) NLL_s + eps S_s + zeta Z_s) / total with NLL_s, S_s, Z_s the sums of nll, smooth, z
   over the rows of sequence s and w_s, total the weights and the count of non-ignored labels of the plain loss.  Ignored rows (label < 0)
   and rows whose label is >= V (err_flag |= 4) add nothing to any sum and get exact-zero gradients; pad columns [V, ldd) are exact zeros.
   _fwd_reg: the arguments of omlm_cross_entropy_fwd with `sums`, 3 floats {nll, smooth, z}, each ACCUMULATED onto, in place of nll_sum
   (eps and zeta enter where the host combines the sums).  _bwd_reg: the arguments of omlm_cross_entropy_bwd plus eps and zeta, on every
   route of it; a value outside the ranges above (NaN and inf included) is refused by name before anything else is looked at.
   The same four kernels serve both pairs through one template flag; the plain pair is the instructions and the launches it always was, and with
   eps = zeta = 0 the _reg pair gives the same row_lse and dlogits bit for bit. */
int omlm_cross_entropy_fwd_reg(const float* logits, const int* labels, float* row_lse, float* sums,
                               int R, int V, int ld, int* err_flag, void* stream);
int omlm_cross_entropy_bwd_reg(const float* logits, const int* labels, const float* row_lse, const float* gscale,
                               float coef, void* dlogits, int R, int V, int ld, int ldd, int out_dtype,
                               float label_smoothing, float z_loss, void* stream);
/* Per-quantizer diagnostics of the cross entropy (extension, off unless called; no reference counterpart): a second, read-only pass over
   the rows the loss has just walked, and an ordered reduce that bins the rows per quantizer.  The kernels live in a translation unit of
   their own (csrc/ce_metrics.hip): the four cross-entropy kernels above, their launches and their results are what they are without it.
   Row rule (omlm_ce_metrics).  Row r has logits l[0..V) -- columns [V, ld) are never read into any result -- and label y:
       y < 0 (ignored)   row_nll = 0, row_rank = -1, row_entropy = 0
       y >= V            the same, and err_flag |= 4 as in omlm_cross_entropy_fwd
       live row          row_nll     = lse - l[y], lse formed as the forward kernels form row_lse (maximum, __expf, __logf, the same reduction
                                       order: bit for bit their row_lse on the same row)
                         row_rank    = #{c : l[c] > l[y]} + #{c < y : l[c] == l[y]}, integer counts only: 0 exactly where
                                       argmax(l) == y under the first-occurrence tie rule; rank < k: y survives a top-k filter
                         row_entropy = log s - (sum_c e_c d_c) / s with d_c = l[c] - max, e_c = exp(d_c), s = sum_c e_c: -sum_c p log p.
                                       A column with e_c == 0 (a -inf logit) adds exactly 0.  A row holding a NaN logit is unspecified.
   Any of the three outputs may be NULL: that output alone is skipped.  One wave per row while V <= 1088 (the row in registers), one
   workgroup per row above; the route is a function of V alone (csrc/ce_metrics_plan.h).
   Bin rule (omlm_ce_metrics_bins).  Rows are in [B, n] order, t = r mod n; R % n == 0.  The bin of a live row is Q where y == V - 1 (the
   eos entry) and t mod Q otherwise; ignored rows and rows with y >= V enter no bin.  bins is [Q + 1][5] doubles
   {count, nll, entropy, top1 (rank == 0), topk (rank < k_top)}, each ACCUMULATED onto: several batches cost no host read.  One workgroup
   per bin adds its rows in a fixed order in fp64 -- no float atomics -- so the same input gives the same bits on every launch and the
   three counts are exact.
   Refused by name before any launch: R < 0, V < 1, ld < V, n < 1, R % n != 0, Q < 1, k_top outside [1, V], and null pointers when
   R > 0 (the three per-row outputs of omlm_ce_metrics excepted).  R == 0 returns 0 and launches nothing. */
int omlm_ce_metrics(const float* logits, const int* labels, float* row_nll, int* row_rank, float* row_entropy,
                    int R, int V, int ld, int* err_flag, void* stream);
int omlm_ce_metrics_bins(const float* row_nll, const int* row_rank, const float* row_entropy, const int* labels,
                         int R, int n, int Q, int V, int k_top, double* bins, void* stream);

/* clip_grad_norm_ + Adam/AdamW on flat buffers (optimizer.py:10-34; trainer.py:444-447). */
/* out[0] += sum g^2; partials (optional, >= 2048 floats) selects the bit-reproducible two-pass form (identical clip on every replica). */
int omlm_sumsq_accumulate(const float* g, long long n, float* out, float* partials, void* stream);
int omlm_adamw_clip_step(float* p, float* g, float* m, float* v, void* p16, long long n,
                         float lr, float beta1, float beta2, float eps, float wd, int step,
                         float gscale, const float* gnorm_sq, float max_norm, int decoupled, int zero_grad, int p16_dtype,
                         const float* ls_state, void* stream);
/* p16 (optional): 16-bit shadow of p in p16_dtype (1 bf16 / 2 fp16); a non-finite *gnorm_sq skips the update (gradients still cleared).
   ls_state (optional, precision "fp16"): 5 floats on the device {loss scale, good steps since its last change, skipped steps, applied
   steps, scale of the last finished step}: gradients are divided by ls_state[0] and the bias corrections use step = ls_state[3] + 1
   instead of `step`; omlm_loss_scale_update copies ls_state[0] to ls_state[4] before it halves / doubles the scale. */
/* The same step with an exponential moving average of the weights riding along (no reference counterpart; off unless this entry is
   called).  e: flat fp32 like p, read and written in the same pass.  After an APPLIED step with clock t has produced the new p':
       n    = t - ema_update_after_step
       d(t) = 0                                       if n <= 0        (the EMA follows the weights)
            = min(ema_decay, (1 + n) / (10 + n))      if ema_warmup
            = ema_decay                               otherwise
       e'   = p' + d * (e - p')                       in fp32; d = 0 gives e' = p' bit for bit
   t counts from 1: `step`, or ls_state[3] + 1 where ls_state is given -- the clock of the bias corrections.  d is formed in double and
   rounded to float once per launch (per workgroup under ls_state).  A skipped step (non-finite *gnorm_sq) leaves e untouched bit for bit,
   like p, m, v.  ema_decay outside [0, 1) (NaN included) or ema_update_after_step < 0 is refused before any device work.  p, g, m, v,
   p16 come out bit-equal to omlm_adamw_clip_step's.  No 16-bit shadow of e is kept. */
int omlm_adamw_clip_step_ema(float* p, float* g, float* m, float* v, void* p16, long long n,
                             float lr, float beta1, float beta2, float eps, float wd, int step,
                             float gscale, const float* gnorm_sq, float max_norm, int decoupled, int zero_grad, int p16_dtype,
                             const float* ls_state, float* e, float ema_decay, int ema_update_after_step, int ema_warmup, void* stream);
/* after the last parameter group of a step: non-finite *gnorm_sq -> scale = max(scale * backoff, scale_min), skipped += 1; else applied += 1
   and after `interval` consecutive good steps scale = min(scale * growth, scale_max).  (No reference counterpart: the reference trains in
   fp32, trainer.py:444-447; this is torch.cuda.amp.GradScaler's rule kept on the device so that the captured step never reads the norm.) */
int omlm_loss_scale_update(float* ls_state, const float* gnorm_sq, float growth, float backoff, int interval,
                           float scale_min, float scale_max, void* stream);

/* operand casts / weight repack */
int omlm_cast_pad(const float* src, void* dst, long long R, int C, int ld_src, int ld_dst, int out_dtype, void* stream);
/* The per-step weight re-packs of a model as ONE launch: problem i casts src [R, C] (pitch ld_src) into dst [R, ld_dst] with zero pad
 * columns (omlm_cast_pad), or -- transpose != 0 -- writes dst[c, r] = cast(src[r, c]) (pad entries untouched): the k-contiguous W^T copies
 * for the input-gradient GEMMs (the autograd transpose of nn.Linear, transformer.py:203-212,144,149), refreshed once per optimizer step.
 * lo != 0: dst receives the LO PLANE of the cast, rne16(v - rne16(v)), instead of the cast itself (the hi/lo weight planes of precision
 * "fp16ff": omlm_gemm_planes16, omlm_ffmid_fwd_planes). */
typedef struct omlm_cast_pad_desc { const float* src; void* dst; int R, C, ld_src, ld_dst, transpose, lo; } omlm_cast_pad_desc;
int omlm_cast_pad_group(const omlm_cast_pad_desc* problems, int count, int out_dtype, void* stream);

/* fp32-grade GEMM ("bf16x3") on bf16 hi/lo operand planes through the bf16 LDS-DMA tile kernels: A and B point at bf16 hi planes
 * laid out as omlm_gemm takes bf16 operands, the lo plane of each lies a_plane_bytes / b_plane_bytes behind it
 * (omlm_split_planes: hi = fp32 truncated to bf16, lo = RNE(x - hi)).  One launch, k-loop three times as long:
 * hi*hi + hi*lo + lo*hi with fp32 accumulation -- the products the fp32 path of omlm_gemm forms, at the bf16 kernels' rate.
 * Row maps as in omlm_gemm; k-row maps (k-major operand with a map) are not supported. */
int omlm_gemm_planes(const void* A, long long a_plane_bytes, const void* B, long long b_plane_bytes, void* C, const float* Cin,
                     const int* a_map, const int* b_map, const int* c_map, long long a_rows, long long b_rows,
                     int M, int N, int K, int lda, int ldb, int ldc, int ldcin,
                     int a_kmajor, int b_kmajor, int out_dtype, float alpha, void* workspace, long long workspace_bytes, void* stream);
int omlm_split_planes(const float* x, void* planes, long long n, long long plane_elems, void* stream);
/* Precision "fp16ff" (round 5): the forward of the two ConvFeedForward linears (transformer.py:144,149 -- 86-88 % of the fp16 logits-error
 * variance, profiles/r05_error_budget.md) on hi/lo planes of the 16-bit operand type `dtype` (1 = bf16, 2 = fp16).  C = A B^T (+ Cin), A [M, K]
 * and B [N, K] row-major, every *_lo plane in its hi plane's layout (separate allocations are fine); one launch, hi*hi + hi*lo + lo*hi with
 * fp32 accumulation.  C_lo NULL: C is fp32 (Cin optional).  C_lo given: C = rne16(v) and C_lo = rne16(v - C) in `dtype` (no Cin) -- the next
 * forward kernel reads the un-rounded value hi + lo, the 16-bit backward reads C alone.  a_map / c_map (optional): row maps as in omlm_gemm
 * (the logit heads of the same mode, open_musiclm.py:163-186). */
int omlm_gemm_planes16(const void* A, const void* A_lo, const void* B, const void* B_lo, void* C, void* C_lo, const float* Cin,
                       const int* a_map, const int* c_map, long long a_rows, long long b_rows, int M, int N, int K,
                       int lda, int ldb, int ldc, int ldcin, int dtype, void* workspace, long long workspace_bytes, void* stream);
/* Round 6: the same contraction for IEEE-half planes with the two CORRECTION products on fp8 at twice the matrix rate (csrc/gemm_mx.hip):
 *   C = A_hi B_hi^T (v_mfma_f32_32x32x16_f16)  +  2^(ea + eb - 11) (A_hi8 B_lo8^T + A_lo8 B_hi8^T)  (v_mfma_scale_f32_32x32x64_f8f6f4)
 * A [M, K] / B [N, K]: the half hi planes (pitch lda / ldb elements).  A8 / B8: the operand's two fp8 (e4m3) planes [hi8 | lo8] at the half plane's
 * row pitch in BYTES (2 lda / 2 ldb; element k of a row at byte k; bytes [K, ceil128(K)) zero), the lo8 plane a8_stride / b8_stride bytes behind
 * the hi8 plane, rows padded to a multiple of 256 (both planes readable in full).  a_scale / b_scale: one E8M0 byte per row,
 * hi8 = fp8(hi 2^-(byte - 127)), lo8 = fp8(lo 2^-(byte - 127 - 11)) (omlm_layernorm_fwd_mx / omlm_ffmid_fwd_mx / omlm_quant_rows_mx write all
 * of it).  2 x the k-tiles of a plain GEMM instead of omlm_gemm_planes16's 3 x; what the fp8 corrections leave in the logits:
 * profiles/r06_error_budget_fp8corr.md.  C_lo given: planes out (no Cin) -- C the half hi plane rne16(v), C_lo the remainder v - C as half
 * (c_lo_bf8 == 0) or as bf8 (e5m2) BYTES at the same element pitch ldc (c_lo_bf8 != 0: the upper byte of a half, same exponent range, no
 * scale; C + C_lo ~ v to 2^-14 -- h1 of the ConvFeedForward forward, read back by omlm_ffmid_fwd_mx: half the lo plane's bytes written and
 * read); else fp32 (+ Cin).  workspace as in omlm_gemm (omlm_gemm_mx16_workspace_bytes(M, N, K)).  K % 64 == 0. */
int omlm_gemm_mx16(const void* A, const void* A8, long long a8_stride, const unsigned char* a_scale,
                   const void* B, const void* B8, long long b8_stride, const unsigned char* b_scale,
                   void* C, void* C_lo, int c_lo_bf8, const float* Cin, long long a_rows, long long b_rows,
                   int M, int N, int K, int lda, int ldb, int ldc, int ldcin,
                   void* workspace, long long workspace_bytes, void* stream);
long long omlm_gemm_mx16_workspace_bytes(int M, int N, int K);
/* Producers of omlm_gemm_mx16's operand form (fp16 only).  Each writes the half hi plane exactly as its plain / planes sibling does, plus the fp8
 * planes [hi8 | lo8] (row pitch = 2 x the half plane's pitch in elements, in bytes; lo8 plane `*_stride` bytes behind hi8; bytes behind the row's
 * last element zero up to the next multiple of 128) and one E8M0 scale byte per row, 2^e >= 2^-8 x a bound of the row's largest entry:
 *   omlm_layernorm_fwd_mx : transformer.py:24-31 in front of FF-in; bound = sqrt(D) max|gamma| (what a LayerNorm output cannot exceed)
 *   omlm_ffmid_fwd_mx     : omlm_ffmid_fwd_planes with h2 in this form; bound = sqrt(F) max|gamma / keep| the same way.  h1_lo: the lo plane
 *                           of h1 as bf8 BYTES at h1's element pitch (what omlm_gemm_mx16 writes with c_lo_bf8 != 0)
 *   omlm_quant_rows_mx    : fp32 weights (all problems of a model in one launch); hi = rne_half(w), exact row maximum; rows' tails untouched
 *                           (zero-fill the buffer once) */
int omlm_layernorm_fwd_mx(const float* x, const float* gamma, void* y, void* y8, long long y8_stride, unsigned char* scale8,
                          float* mean, float* rstd, int M, int D, int ldy, float eps, void* stream);
int omlm_ffmid_fwd_mx(const void* h1, const void* h1_lo, const void* convw, const void* convw_lo, const void* gamma, const void* gamma_lo,
                      void* h2, void* h2_8, long long h2_8_stride, unsigned char* scale8, float* mean, float* rstd, int M, int nseq, int F, int Fp,
                      float eps, float p, unsigned long long seed, const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh, void* stream);
/* the same two on a row segment (omlm_layernorm_fwd_seg / omlm_ffmid_fwd_seg) */
int omlm_layernorm_fwd_mx_seg(const float* x, const float* gamma, void* y, void* y8, long long y8_stride, unsigned char* scale8,
                              float* mean, float* rstd, float* xc, int M, int D, int ldy, float eps, int n_full, int p0, int n_live, void* stream);
int omlm_ffmid_fwd_mx_seg(const void* h1, const void* h1_lo, const void* convw, const void* convw_lo, const void* gamma, const void* gamma_lo,
                          void* h2, void* h2_8, long long h2_8_stride, unsigned char* scale8, float* mean, float* rstd, int M, int nseq, int F, int Fp,
                          float eps, float p, unsigned long long seed, const unsigned long long* seed_dev, unsigned char* drop_bits, void* gh,
                          int n_full, int p0, void* stream);
typedef struct omlm_quant_rows_desc { const float* src; unsigned char* dst8; long long lo_stride; unsigned char* scale8; int R, C, ld_src, ld8; } omlm_quant_rows_desc;
int omlm_quant_rows_mx(const omlm_quant_rows_desc* problems, int count, void* stream);
/* All weight-gradient contractions of a backward pass in one launch (autograd of nn.Linear, transformer.py:203-212,144,149:
 * dW += dY^T X).  Problem i: C_i [M_i, N_i] fp32 (accumulated, +=; c_map optional: physical row of logical row m, < 0 skips)
 * from 16-bit k-major operands A_i [K_i, M_i] (pitch lda) and B_i [K_i, N_i] (pitch ldb); pitches are multiples of 8 elements.
 * splits: K-splits per output tile (0: chosen for whole machine rounds; > 1 accumulates with fp32 atomics). */
typedef struct omlm_gemm_wgrad_desc {
    const void* A; const void* B; float* C; const int* c_map;
    int M, N, K, lda, ldb, ldc;
} omlm_gemm_wgrad_desc;
int omlm_gemm_wgrad_group(const omlm_gemm_wgrad_desc* problems, int count, int splits, int dtype, void* stream);   /* dtype: operands of ALL problems, 1 bf16 / 2 fp16 */

/* RelativePositionBias MLP helpers (transformer.py:55-64): SiLU layers around omlm_gemm, over the distances x0 .. x0 + n - 1 (row r is
 * distance x0 + r; x0 = 0: the causal table, x0 = -(min(P, N) - 1): the non-causal prefix's). */
int omlm_relpos_first_fwd(const float* w0, const float* b0, float* pre, float* z, int n, int Hd, int x0, void* stream);
int omlm_relpos_first_bwd(const float* ds, float* dw0, int n, int Hd, int x0, void* stream);
int omlm_bias_silu_fwd(const float* a, const float* b, float* pre, float* z, long long R, int C, void* stream);
int omlm_silu_bwd(const float* dz, const float* pre, float* ds, long long total, void* stream);
int omlm_bias_add(const float* a, const float* b, float* out, int R, int C, int ld, void* stream);
/* The whole MLP as ONE forward launch and TWO backward launches (round 5; Hd = 256 or 512, H <= 16: every shipped config), replacing the
 * 21 launches of the layer-by-layer path above.  RelativePositionBias.forward (transformer.py:55-64) restricted to the n distances
 * x0 .. x0 + n - 1: table[r, h] = net(x0 + r)[h].  w0 = net.0.0.weight viewed [Hd]; W1 / W2 = net.1.0 / net.2.0 weights [Hd, Hd]; W3 = net.3.weight
 * [H, Hd].  pre* / z* [n, Hd] are the layers' pre-activations / SiLU outputs, written by the forward when non-null (all or none) and
 * read by the backward; table / dtable are [n, ldb] (ldb <= 16, pad columns zero).  The backward ACCUMULATES into the g* buffers
 * (deterministic: one owner thread per element, rows summed in ascending order); scratch holds 3 * n * Hd floats. */
int omlm_relpos_mlp_fwd(const float* w0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* W3, const float* b3, float* pre0, float* z0, float* pre1, float* z1, float* pre2, float* z2,
                        float* table, int n, int Hd, int H, int ldb, int x0, void* stream);
int omlm_relpos_mlp_bwd(const float* dtable, const float* W1, const float* W2, const float* W3, const float* pre0, const float* z0,
                        const float* pre1, const float* z1, const float* pre2, const float* z2, float* scratch, float* gw0, float* gb0,
                        float* gW1, float* gb1, float* gW2, float* gb2, float* gW3, float* gb3, int n, int Hd, int H, int ldb, int x0,
                        void* stream);

/* Nearest-codeword kernels: ClapQuantized.quantize -> ResidualVQ eval path (clap_quantized.py:75-87) and
 * HfHubertWithKmeans assign (hf_hubert_kmeans.py:87).  codebooks_T: [nstage][D][C] (transposed); indices int32 [n, nstage] -- idx_stride
 * 0 or nstage -- or, with nstage == 1 only, row i's index at indices[i * idx_stride] (a column of an [n, stages] table: the fit step).
 * omlm_rvq_encode uses the distance form of vector-quantize-pytorch's EuclideanCodebook -- argmax(-cdist(x, embed)),
 * first maximum: dist = sqrt(max((|x|^2 + |e|^2) - 2 x.e, 0)) in fp32, IEEE root (distances whose roots round equal are a tie for
 * the lowest index); pinned bit for bit against torch.cdist on exactly representable inputs (tests/rvq_cases.py).
 * omlm_nearest_centroid uses sum_d (x_d - c_d)^2 (pinned against sklearn.MiniBatchKMeans.predict).  Ties -> lowest index. */
int omlm_rvq_encode(const float* x, const float* codebooks_T, int* indices, float* residual_out,
                    int n, int D, int C, int nstage, int idx_stride, void* stream);
int omlm_nearest_centroid(const float* x, const float* centroids_T, int* indices, int n, int D, int C, void* stream);
/* Fitting side of the residual VQ (reference call sites: trainer.py:689-736 -> clap_quantized.py:75-84 with rq.train(True); the
 * arithmetic is vector-quantize-pytorch's EuclideanCodebook, un-vendored: oracle.rvq_fit_step restates the published update rules;
 * the assignment inside it is the -cdist form above).
 * accumulate: counts[k] += #rows assigned to k, sums[k, :] += those rows (caller zeroes both; indices[i * idx_stride]).
 * kmeans_update: means[k] = sums[k] / counts[k] where counts[k] > 0 (Lloyd step), means_T [D, K] refreshed.
 * ema_update: cluster_size = d cs + (1-d) counts; embed_avg = d avg + (1-d) sums; embed = embed_avg / Laplace-smoothed sizes
 * ((cs + eps) / (sum cs + K eps) * sum cs); embed_T [D, K] refreshed; total_scratch: one device float. */
int omlm_vq_accumulate(const float* x, const int* indices, int idx_stride, float* counts, float* sums, int n, int D, int K, void* stream);
int omlm_vq_kmeans_update(float* means, float* means_T, const float* counts, const float* sums, int K, int D, void* stream);
int omlm_vq_ema_update(float* cluster_size, float* embed_avg, float* embed, float* embed_T, const float* counts, const float* sums,
                       float* total_scratch, int K, int D, float decay, float eps, void* stream);

/* Fitting the semantic k-means codebook (reference: hf_hubert_kmeans.py:95-149, sklearn's MiniBatchKMeans on the host; these entry
 * points run the published MiniBatchKMeans rules on the device, csrc/kmeans_fit.hip, driven by open_musiclm_amd/kmeans_fit.py).
 * k-means++ on rows [m, D] (16-byte aligned): pick number *pick_counter (a device int, advanced by the call) draws `trials` (<= 16)
 * candidates from uniforms[pick * trials + t] by inverse CDF over closest [m]: cum_i = sum_{j <= i} closest_j in fp64, candidate =
 * the first row with cum_i > u * cum_{m-1} (rows of weight zero are never drawn), clipped to m - 1; pick 0 takes row
 * min(floor(uniforms[0] * m), m - 1) and resets closest.  The candidate with the lowest potential sum_i min(closest_i, d_i) (fp64,
 * fixed order; ties: first) becomes centres[pick] (and column `pick` of centres_T [D, K]); chosen[pick] / pots[pick] record its row and
 * potential; closest takes the minimum.  Three launches per pick, no host round trip; omlm_kmeans_pp_seed zeroes the counter and queues
 * all K picks.  workspace: omlm_kmeans_pp_workspace_bytes(m, trials) bytes, 16-byte aligned.  Same draws -> same bits. */
long long omlm_kmeans_pp_workspace_bytes(int m, int trials);
int omlm_kmeans_pp_pick(const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres, float* centres_T,
                        int* chosen, double* pots, void* workspace, long long workspace_bytes, int m, int D, int K, int trials,
                        void* stream);
int omlm_kmeans_pp_seed(const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres, float* centres_T,
                        int* chosen, double* pots, void* workspace, long long workspace_bytes, int m, int D, int K, int trials,
                        void* stream);
/* One mini-batch step on rows x[idx[0 .. B)] of x [n, D] (out-of-range indices take no part): assignment in the arithmetic of
 * omlm_nearest_centroid, then for every centre that received m_k rows: counts_k += m_k; c_k += (sum_k - m_k c_k) / counts_k (centres_T
 * refreshed).  bcounts [K] and sums [K, D] are scratch that is zero on entry and zero again on return; rowmin [B], move_partial [K]
 * (fp64) scratch.  state: 8 fp64 on the device, zero before the first step: [0] ewa inertia, [1] its minimum, [2] this batch's mean
 * inertia (centres before the update), [3] squared centre movement, [4] steps done, [5] steps without improvement, [6] stopped (1: no
 * improvement for max_no_improvement steps, 2: movement <= tol_abs; tol_abs = 0 / max_no_improvement = 0 switch a rule off), [7]
 * internal.  The rules are sklearn's _mini_batch_convergence (alpha = min(1, 2 B / (n + 1)) is the caller's).  A step that finds
 * state[6] != 0 changes nothing, so steps may be queued ahead of the host's look at the state. */
int omlm_kmeans_minibatch_step(const float* x, const int* idx, float* centres, float* centres_T, float* counts, float* bcounts,
                               float* sums, float* rowmin, double* move_partial, double* state, int n, int B, int D, int K,
                               double alpha, double tol_abs, int max_no_improvement, void* stream);
/* out[0] += sum_i min_k |x_i - c_k|^2 over x [n, D] (fp64 on the device, one atomic per workgroup; the caller zeroes out); labels
 * (int32 [n], may be NULL) receives the assignment, equal to omlm_nearest_centroid's. */
int omlm_kmeans_inertia(const float* x, const float* centres_T, double* out, int* labels, int n, int D, int K, void* stream);

/* AR sampler: eos suppression + top_k(thres) + gumbel_sample (open_musiclm.py:309-316; utils.py:65-84).
 * Kept set: every logit strictly above the k-th largest value, then of the logits equal to it the lowest indices until exactly k are
 * kept.  Id: the first maximum of l / T + Gumbel(u) over the kept set (0 when every kept logit is -inf).  The same rule holds for
 * omlm_sample_topk_gumbel_at and omlm_sample_embed_at below.
 * Limit: 0 < V <= 65536 (V = codebook size + 1, so codebooks of up to 65535 entries sample; the uint16 token stores end there too),
 * 1 <= k <= V, temperature > 0; anything else is refused before the launch.  V <= 2048 runs one wave per row, 2048 < V <= 65536 one
 * workgroup per row; both are the same function of (logits, uniform, k, temperature, forbid_last), id for id. */
int omlm_sample_topk_gumbel(const float* logits, const float* uniform, long long* out, int B, int V, int ld,
                            int k, float temperature, int forbid_last, void* stream);

/* The same sampler in graph-replayable form: uniform_base [steps, B, V] and hist [steps, B] (optional) are indexed by the
 * DEVICE counter *step_dev; out [B] is the fixed buffer the next decode step embeds from. */
int omlm_sample_topk_gumbel_at(const float* logits, const float* uniform_base, const int* step_dev, long long* out,
                               long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last, void* stream);

/* Sampler + embedding gather of the sampled id, x[b, :] = emb_table[id_b + emb_row_offset] (rows clamped to [0, emb_rows);
 * open_musiclm.py:123-134): the decode step's first launch folded into the sampler (omlm_decode_step then runs with
 * emb_table == NULL). */
int omlm_sample_embed_at(const float* logits, const float* uniform_base, const int* step_dev, long long* out, long long* hist,
                         int B, int V, int ld, int k, float temperature, int forbid_last,
                         const float* emb_table, long long emb_row_offset, long long emb_rows, float* x, int D, void* stream);

/* The three sampler entry points on a counter-based uniform stream: no uniform buffer, u is computed in registers.  Everything else --
 * kept set, tie rule, l / T + Gumbel(u), first maximum, the all -inf rule, the embedding gather, hist -- is the rule above, and an id equals
 * the buffer form's when that is fed the stream's values.
 * Stream -- uniform of step t, sample b, logit index c (c < 65536), from a 64-bit seed = seed_hi * 2^32 + seed_lo; uint32 arithmetic:
 *   h(x)      = lowbias32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (the dropout masks' hash)
 *   s0        = h(h(seed_lo) ^ seed_hi)
 *   key(t, b) = h(h(s0 + t * 0x9E3779B9) ^ (b * 0x85EBCA6B))
 *   r(t,b,c)  = h(key(t, b) ^ (c * 0x9E3779B9))
 *   u(t,b,c)  = (r >> 8) * 2^-24                                  (the 24-bit grid in [0, 1) that torch.rand draws from)
 * t is `step` (host) or *step_dev: the index of the sampled id within the generate() call.  b = row0 + (row of this call): the GLOBAL
 * sample index, so ids do not depend on how a batch is cut into calls.  The seed is hashed before t is added: with key = h(t ^ seed_lo) ...
 * seeds s and s ^ 1 would be one stream with steps swapped pairwise.  It depends on nothing else (not on B, V, ld or the kernel).
 * Seed halves and row0 are plain arguments (a captured step stays valid for a whole call); same argument checks and limits as above. */
int omlm_sample_topk_gumbel_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, int step, int row0, long long* out,
                                int B, int V, int ld, int k, float temperature, int forbid_last, void* stream);
int omlm_sample_topk_gumbel_at_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0,
                                   long long* out, long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last,
                                   void* stream);
int omlm_sample_embed_at_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0, long long* out,
                             long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last,
                             const float* emb_table, long long emb_row_offset, long long emb_rows, float* x, int D, void* stream);

/* The sampler with a nucleus (top-p), and one entry point over all six forms above.  For a row of V logits, forbid_last, k, T > 0 and
 * 0 < top_p < 1:
 *   1. the last logit becomes -inf if forbidden;
 *   2. S = the top-k kept set above, tie rule unchanged (strictly above the k-th value, then the lowest indices among the equals);
 *   3. m = the largest logit in S; if m is -inf the id is 0, as above.  Otherwise w_c = exp((l_c - m) / T) for c in S (0 for -inf) and
 *      W = sum of w_c;
 *   4. rank S by logit descending, then index ascending: entry c is in the nucleus iff the mass of the entries ranked strictly before
 *      it is < top_p W (the first-ranked entry is therefore always kept);
 *   5. the id is the first maximum of l_c / T + Gumbel(u_c) over the nucleus -- the score, the 1e-20 guards and the first-maximum rule
 *      of the sampler above, u_c the uniform of index c (uniform[row, c], or u(t, b, c) of the counter stream, unchanged).
 * Equal logits have equal weights and are ranked by index, so the nucleus is every key above a threshold plus the first n entries by
 * index among the keys equal to it: a second selection of the kind the top-k is.  The kernels form the masses in fixed point,
 * q_c = floor(w_c 2^40) as 64-bit integers with w_c in fp32, and cut at mass-before < ceil(top_p sum of q): integer sums do not depend
 * on order, so one row gives one id in every launch and in both kernels.  Against exact arithmetic the cut moves by less than 2^-18 of W.
 * top_p == 1: no nucleus, the launch of the six entry points above.  top_p <= 0, > 1 or NaN is refused before the launch.
 * Block: uniform non-null selects the buffer ([B, V], or [steps, B, V] with step_dev), null the counter stream (seed_lo, seed_hi, row0
 * and step, or *step_dev); step_dev non-null selects the graph-replayable form (hist [steps, B], optional, is indexed by it; without
 * step_dev hist is [B]); emb_table non-null adds the embedding gather into x [B, D] (D % 4 == 0).  Limits and checks as above. */
typedef struct omlm_sample_args {
    const float* logits;
    int B, V, ld;
    const float* uniform;
    unsigned seed_lo, seed_hi;
    int step, row0;
    const int* step_dev;
    long long* out;
    long long* hist;
    int k;
    float temperature, top_p;
    int forbid_last;
    const float* emb_table;
    long long emb_row_offset, emb_rows;
    float* x;
    int D;
} omlm_sample_args;
int omlm_sample(const omlm_sample_args* args, void* stream);

/* The log-probabilities of the sampled id.  For a row of V fp32 logits l_c as the head wrote them, forbid_last, k, T > 0 and
 * 0 < top_p <= 1, with s the id the sampler returns for the row (natural logarithms):
 *   lp_model   = l_s - log sum_{c < V} exp(l_c): the model's own distribution -- T = 1, all V entries, the last one included even when
 *                it is forbidden;
 *   lp_sampled = l_s / T - log sum_{c in N} exp(l_c / T), N the set s was drawn from: the top-k kept set, cut to the nucleus when
 *                top_p < 1, the last logit at -inf when forbidden.  It is the log of the probability with which the Gumbel-max rule picks s.
 * A -inf logit contributes 0.  When the largest kept logit m is -inf (the "id 0" rule) both values are -inf.  When N has one entry
 * (k == 1, a tiny top_p, V == 1) lp_sampled is exactly 0.0f: the value is formed as (l_s - m) / T - log(sum of exp((l_c - m) / T)).
 * lp_model is formed as (l_s - M) - log(sum of exp(l_c - M)), M the larger of m and the forbidden last logit.  Rows with +inf or NaN
 * logits are unspecified, as they are for the id.
 * Arithmetic: fp32, weights by the precise expf that forms the nucleus masses; the sums run in a fixed order (a lane's slots in order,
 * the wave's shuffle tree, in the workgroup kernel the waves' partials in wave order), without floating-point atomics: one row gives the
 * same bits in every launch.  The wave kernel (V <= 2048) and the workgroup kernel may differ from each other in the last bits.
 *
 * omlm_sample plus the log-probabilities of the id it returns.  lp_model / lp_sampled: [B] floats, or [steps, B]
 * indexed by *step_dev when args->step_dev is given (like hist); either may be NULL; both NULL: exactly omlm_sample. */
int omlm_sample_lp(const omlm_sample_args* args, float* lp_model, float* lp_sampled, void* stream);

/* Per-row sampling parameters: omlm_sample_lp with k, temperature, top_p, the stream's seed and the stream's sample index of every row
 * taken from [B] device arrays.  Row r of the call is the function stated above evaluated with k_r, T_r and top_p_r: tie rule,
 * fixed-point nucleus masses, first maximum, the all -inf rule, both log-probabilities (at T_r), hist, step_dev, the embedding gather --
 * id for id and bit for bit what omlm_sample_lp gives row r with those three as its scalars.  forbid_last stays one value per call (it
 * belongs to the quantizer phase).  On the counter stream row r draws u(t, sample_r, c) from seed_r (seed_r = seed_hi * 2^32 + seed_lo
 * of the stream above): a row's uniforms then depend on its own pair alone, not on its place in the call.
 * A NULL member leaves the block's scalar in force for every row (seed: seed_lo / seed_hi; sample: row0 + row).  The arrays are indexed
 * by the row alone, also with step_dev (one value per row for the whole call).  top_p_r == 1: no nucleus for that row -- it takes the
 * path of a call with top_p == 1, beside rows that run one.
 * Checks, all before the launch: rows == NULL or every member NULL is exactly the launch of omlm_sample_lp; seed or sample together
 * with args->uniform is refused by name (they belong to the counter stream); a scalar whose array is given is neither read nor
 * checked; everything else keeps the checks above.  The library sees pointers, not values: k_r is clamped into [1, V]; a temperature that
 * is not > 0 or a top_p outside (0, 1] (NaN included) gives an unspecified id in [0, V) and unspecified log-probabilities for that row,
 * never an out-of-range access.  One launch; lp_model / lp_sampled as for omlm_sample_lp, either or both NULL. */
typedef struct omlm_sample_row_params {
    const int*   k;                    /* [B] device, or NULL: args->k           */
    const float* temperature;          /* [B] device, or NULL: args->temperature */
    const float* top_p;                /* [B] device, or NULL: args->top_p       */
    const unsigned long long* seed;    /* [B] device, or NULL: args->seed_lo/hi  (counter stream only) */
    const int*   sample;               /* [B] device, or NULL: args->row0 + row  (counter stream only) */
} omlm_sample_row_params;
int omlm_sample_rows(const omlm_sample_args* args, const omlm_sample_row_params* rows,
                     float* lp_model, float* lp_sampled, void* stream);

/* Classifier-free guidance on the condition (token sequence 0, the CLAP tokens).  The null condition is the pad embedding at every id
 * position of that sequence: raw id -1 - codebook (p mod Q) at position p, which is -1 after the per-quantizer offset and therefore the
 * zero row of the gather; the appended eos, the start tokens and every other sequence are unchanged.  A guided call of P prompts decodes
 * 2P rows: rows [0, P) conditional, rows [P, 2P) their null twins.  For one row, with l the conditional logits, n the null twin's and
 * s = scale, in fp32 with exactly three roundings and no contraction:
 *     g_c = n_c + (s * (l_c - n_c))        i.e. __fadd_rn(n_c, __fmul_rn(s, __fsub_rn(l_c, n_c)))
 * so float32 arithmetic in that order reproduces it bit for bit (s = 1 does not return l_c bit for bit; callers do not launch for s = 1).
 * Everything downstream is the sampler above applied to g: forbidden eos, top-k, nucleus, Gumbel, lp_sampled -- and lp_model, which
 * on a guided row is therefore the log-softmax of g at T = 1, not of the model's conditional logits.
 * cond / null / out: [rows, ld] fp32, columns V .. ld - 1 are not written; out may alias cond.  16-byte loads where ld % 4 == 0 and the
 * three bases are 16-byte aligned, scalar loads otherwise and on the tail of a row.  One launch; scale finite and >= 0, V <= 2^24. */
int omlm_guide_logits(const float* cond, const float* null, float* out, int rows, int V, int ld, float scale, void* stream);
/* The same with one scale per row: g_c = n_c + (s_r * (l_c - n_c)) in row r, the same three roundings, loads, aliasing and untouched
 * columns.  scale: fp32 [rows] on the device; its values are not checked -- a non-finite scale gives non-finite g in its own row and
 * nothing out of range. */
int omlm_guide_logits_rows(const float* cond, const float* null, float* out, int rows, int V, int ld,
                           const float* scale /* [rows] device */, void* stream);

/* The twin copy of a guided decode cycle, one launch: ids_twin[r] = ids[r] and x_twin[r, :] = x[r, :] for r < rows -- the ids the sampler
 * picked for the conditional rows and the embedding rows it gathered, handed to the null twins.  Either pair of pointers may be NULL
 * (both NULL: no launch); a source without its twin is refused.  x / x_twin: [rows, D] fp32. */
int omlm_decode_twin(const long long* ids, long long* ids_twin, const float* x, float* x_twin, int rows, int D, void* stream);

/* KV-cached AR decode step: ONE new row (index *pos_dev) per sample through all L layers and the logit head of the quantizer
 * that row predicts -- replaces the reference's full re-forward per sampled id (wrapper.generate, open_musiclm.py:301-321;
 * the trunk is strictly causal, so the logits are the same).  State owned by the caller:
 *   Kc/Vc[l]  [B, Nmax, 64]   l2-normalised keys / values of rows < pos (row `pos` is appended by this call): fp32, or with kv16 != 0
 *                             the 16-bit operand type of w_dtype (bf16 / fp16), the pointers then cast to float*
 *   hist[l]   [B, 2, 2*Fp]    fp32 FF-in outputs of rows pos-2, pos-1 (conv state; advanced by this call)
 * With 16-bit weights and round_bf16 = 1 the step rounds every key (after its l2 normalisation) and every value to the operand type before
 * it stores them, so the 16-bit cache holds the fp32 cache's numbers in half the bytes: same logits, bit for bit.  The one number that
 * must not pass through 16 bits is the step's RAW key: with kv16 it waits in k_new [B, 64] fp32 until the attention kernel has normalised
 * it.  kv16 is refused (an argument error, before any launch) with w_dtype == 0, with round_bf16 == 0 or without k_new.
 * Pointer-array members are HOST arrays of L device pointers.  w_dtype 0: fp32 weights, 1: bf16 operand copies (then
 * round_bf16 = 1 rounds the activations the batched path keeps in bf16).  W1p [2*Fp, D] / W2p [D, Fp] / convw [3, 2*Fp] /
 * mid_gamma [Fp] are the padded layouts of omlm_ffmid_fwd.  emb_table (optional): x = emb_table[ids[b] + emb_row_offset]
 * first (open_musiclm.py:123-134); otherwise x must already hold the new row.  head_W (optional) [V1, D]: logits
 * [B, ldV] = LN(x_L) head_W^T.  B <= 8; 16-bit weights with D = 1024 and ln_parts given: B <= 16 (matrix-core step kernels); with
 * splitk_ws and splitk_cnt as well: B <= 64.
 * A call of more than 16 samples runs as G = OMLM_DECODE_GROUPS(B) groups of 16 consecutive samples (the last one possibly partial)
 * carried through ONE launch of every phase: a group is computed exactly as a call of its own sample count would be (same kernels'
 * branches, same summation order, same bits), and the G workgroups that read the same weight rows share an XCD.  The scratch grows with
 * G -- sizes for a call of B samples (for B <= 16 they are the per-group sizes named at the members):
 *   ln_parts    OMLM_DECODE_LN_PARTS_B(B, D, Fp) floats   = 3 * G * OMLM_DECODE_LN_PARTS(D, Fp)
 *   splitk_ws   OMLM_DECODE_SPLITK_FLOATS_B(B, D) floats  = G * OMLM_DECODE_SPLITK_FLOATS(D)
 *   splitk_cnt  OMLM_DECODE_SPLITK_CNT_B(B, D) ints       = max(G * ceil(D / 16), B, 16): FF-out takes its tickets per (group, tile), the
 *               attention combine per sample, in the same array; all zero before the first step, every step leaves them zero.
 * The library sees pointers only and cannot check these sizes; it checks that the scratch a batch needs is given.
 * Every refusal of omlm_decode_step (an argument error with its reason in omlm_last_error) is decided from the sizes and from which pointers
 * are given, and returned BEFORE anything is launched: a refused call leaves x, the caches, hist and every scratch buffer untouched -- the
 * lo-plane argument checks and the head's missing-partials check included, which used to come after the embedding gather or the row sums
 * had run. */
typedef struct omlm_decode_args {
    int B, D, H, L, F, Fp, Nmax, w_dtype, round_bf16, nsplit;     /* nsplit >= ceil(Nmax / 64): attention key ranges */
    float eps, scale;
    const int* pos_dev;                                            /* DEVICE int: index of the row computed by this step */
    const void* const* Wq; const void* const* Wkv; const void* const* Wo; const void* const* W1p; const void* const* W2p;
    const float* const* attn_gamma; const float* const* q_scale; const float* const* k_scale;
    const float* const* ffin_gamma; const float* const* convw; const float* const* mid_gamma;
    float* const* Kc; float* const* Vc; float* const* hist;
    const float* bias_table; int bias_ld;
    const float* final_gamma; const void* head_W; int V1; int ldV;
    const float* emb_table; long long emb_row_offset; long long emb_rows;
    float* x; float* x1; float* q; float* parts; float* u; float* logits;   /* scratch: parts [B, nsplit, H, 66] */
    int* advance_pos; int* advance_step;   /* optional DEVICE counters (+= 1) bumped by the step's last kernel: pass pos_dev (and the
                                            * sampler's step counter) here instead of launching omlm_decode_advance */
    float* ln_parts;                       /* optional scratch, 3 * OMLM_DECODE_LN_PARTS(D, Fp) floats: the batched matrix-core kernels
                                            * (B >= 2; B > 16: OMLM_DECODE_LN_PARTS_B floats) leave per-workgroup partial sums of their outputs there, and the kernel that
                                            * applies the next LayerNorm adds them up instead of re-reducing every sample's row; null:
                                            * every consumer reduces the rows itself */
    /* precision "fp16ff" (optional; all NULL: the plain 16-bit step): lo planes of the FF-in / FF-out / head weights in the layout of
     * W1p / W2p / head_W.  With them those three launches read W = hi + lo and keep LayerNorm outputs and h1 un-rounded -- the arithmetic of
     * the batched forward's omlm_gemm_planes16 (open_musiclm.py:299-319 evaluated fp32-grade where the error budget puts the error).
     * B >= 2: needs the matrix-core kernels (16-bit weights, D = 1024, ln_parts given, L >= 1), Fp <= 3072. */
    const void* const* W1p_lo; const void* const* W2p_lo; const void* head_W_lo;
    /* optional scratch of the batched FF-out launch (2 <= B <= 64, matrix-core kernels, ln_parts given; required for B > 16): with it a tile of 16 output rows
     * is cut into four k-slices (256 workgroups instead of 64) that meet through fp32 slabs, added in slice order by the last to arrive.
     * splitk_ws: OMLM_DECODE_SPLITK_FLOATS(D) floats, contents irrelevant; splitk_cnt: max(ceil(D / 16), 16) ints (the attention kernel's combine
     * counts per sample in the same array; B > 16: OMLM_DECODE_SPLITK_FLOATS_B / OMLM_DECODE_SPLITK_CNT_B), ZERO before the first step
     * (every step leaves them zero).  One decode stream at a time per scratch pair.  NULL: one workgroup per tile walks the whole row. */
    float* splitk_ws; int* splitk_cnt;
    /* kv16 != 0: Kc[l] / Vc[l] hold the 16-bit operand type (see above); k_new: fp32 scratch [B, 64] for the step's raw key, contents
     * irrelevant between steps.  kv16 == 0: fp32 caches, k_new unused (may be NULL). */
    int kv16; float* k_new;
} omlm_decode_args;
#define OMLM_DECODE_SPLITK_FLOATS(D) (4 * (((D) + 15) / 16) * 256)
#define OMLM_DECODE_LN_PARTS(D, Fp) ((((D) + 15) / 16 > ((Fp) + 7) / 8 ? ((D) + 15) / 16 : ((Fp) + 7) / 8) * 32)
#define OMLM_DECODE_MAX_BATCH 64
#define OMLM_DECODE_GROUPS(B) (((B) + 15) / 16)
#define OMLM_DECODE_LN_PARTS_B(B, D, Fp) (3 * OMLM_DECODE_GROUPS(B) * OMLM_DECODE_LN_PARTS(D, Fp))
#define OMLM_DECODE_SPLITK_FLOATS_B(B, D) (OMLM_DECODE_GROUPS(B) * OMLM_DECODE_SPLITK_FLOATS(D))
#define OMLM_DECODE_SPLITK_CNT_B(B, D) \
    (OMLM_DECODE_GROUPS(B) * (((D) + 15) / 16) > ((B) > 16 ? (B) : 16) ? OMLM_DECODE_GROUPS(B) * (((D) + 15) / 16) : ((B) > 16 ? (B) : 16))
int omlm_decode_step(const omlm_decode_args* args, const long long* ids, void* stream);
/* omlm_decode_step under a key mask: the same step, its attention launches replaced by their masked forms (same grids, same LDS, every
 * other launch the same), so the new row attends only to the keys the training forward attends to
 * (TokenConditionedTransformerWrapper._prepare: conditioning positions that hold a pad or an eos id are no keys).
 *   key_live  [B, Nmax] bytes on the device, row-major; byte (b, j) nonzero: sample b attends to cache row j.  Bytes of rows > *pos_dev
 *             are not read.  Byte *pos_dev of EVERY sample must be 1: the new key is always attended, and it is what guarantees a
 *             nonzero softmax sum.  That is the caller's duty -- the library sees a pointer only.  The buffer is read by every layer's
 *             attention launch and never written; it may stay the same over a captured graph's replays.
 * A masked key has score -3.0e38f and weight 0 exactly, like a key past *pos_dev.  A 64-key range whose keys are all masked leaves the
 * partial {max = -3.0e38f, sum = 0, o = 0} in parts, which every combine weighs with exp(-3.0e38f - live max) = 0; such ranges still
 * load their K / V and count in the per-sample tickets, so splitk_cnt is zero again after the step.  A mask of all ones gives
 * omlm_decode_step's logits bit for bit.  The refusals are omlm_decode_step's, made before any launch, plus "null key_live". */
int omlm_decode_step_masked(const omlm_decode_args* args, const unsigned char* key_live, const long long* ids, void* stream);
/* *pos_dev += 1, *step_dev += 1 (either may be null): keeps the row / sampler-step counters on the device so that a
 * captured step can be replayed. */
int omlm_decode_advance(int* pos_dev, int* step_dev, void* stream);

/* hardware probe (tests only): raw ds_read_b64_tr_b16 result for a linear LDS image, 64 lanes x 4 int16 */
int omlm_probe_tr16(short* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

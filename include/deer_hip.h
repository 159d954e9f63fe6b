/* deer_hip.h - C ABI of libdeer_hip.so: the MI355X (gfx950) kernels behind DeeR-VLA's early-exit forward path.
 *
 * The reference (yueyang130/DeeR-VLA) has no C ABI: its "plugin interface" for this path is a Python object
 * protocol whose compute is implicit vendor kernels reached through torch ops.  Each entry
 * point below replaces one such implicit op and cites the reference call site it stands for (paths relative
 * to the reference repo).  The Python host in deer_vla_amd/ binds these with ctypes (deer_vla_amd/_abi.py)
 * and keeps the reference's Python surface (create_model_and_transforms / MPTFlamingo.forward / the
 * mosaic_gpt multi-exit lang_encoder.forward / ExitController) on top - see INTEGRATION.md.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless noted; `stream` is a hipStream_t passed as void*
 *   - bf16 data is passed as `const void*` (uint16 storage); f32 as float*
 *   - every function only ENQUEUES work on `stream` (graph-capturable, no allocation, no sync) and
 *     returns 0 on success, DEER_ERR_SHAPE (1) for an invalid argument, DEER_ERR_LAUNCH (2) if the launch failed
 *   - `ctl` is the device control block array (int32[DEER_CTL_WORDS] per environment); kernels on the early-exit path
 *     return at entry once ctl[DEER_CTL_ALL_EXITED] != 0 (device-side termination, no host round trip per layer); the
 *     exit checks also publish their verdict into a pinned host mirror (DEER_CTL_HOST_PTR) so that the host can stop
 *     enqueueing the remaining graph pieces of the step without the device ever waiting for it
 */
#ifndef DEER_HIP_H
#define DEER_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define DEER_OK 0
#define DEER_ERR_SHAPE 1
#define DEER_ERR_LAUNCH 2

/* control block layout (32-bit words); one block per environment of the batch (env b at ctl + b*DEER_CTL_WORDS);
 * SHADOW and ALL_EXITED are batch-global (block 0); HOLD is per environment: deer_ctl_begin_step spreads bit b of step_info[0] into block b */
#define DEER_CTL_EXIT_FLAG 0
#define DEER_CTL_EXIT_LAYER 1
#define DEER_CTL_CUR_EXIT_ID 2
#define DEER_CTL_HOLD 3
#define DEER_CTL_N_EVALS 4
#define DEER_CTL_SHADOW 5      /* calibration: evaluate every exit, commit at the first that fires, never stop */
#define DEER_CTL_COMMITTED 6
#define DEER_CTL_ALL_EXITED 7  /* block 0: every environment of the batch has exited */
#define DEER_CTL_PREV_ACTION 8   /* float[8] */
#define DEER_CTL_OUT_ACTION 16   /* float[8]: pose[6], gripper prob, gripper logit */
#define DEER_CTL_DELTAS 24       /* float[16] */
#define DEER_CTL_N_EXITED 40   /* block 0: environments exited so far in this step */
#define DEER_CTL_SEQ 41        /* block 0: sequence number of the current control step (from step_info) */
#define DEER_CTL_HOST_PTR 42   /* block 0, 2 words: pinned host mirror the verdicts are published to, or 0 */
#define DEER_CTL_EVALS_DONE 44 /* block 0: environments that finished the current exit check */
#define DEER_CTL_PREV_REAL 45  /* PREV_ACTION is an exit-check action of this step (member of value_net.action_list), not the pseudo action */
#define DEER_CTL_ENS_ACTION 48 /* float[8]: ActionValueNet.get_ensemble_action (value_net.py:92-95): mean of the last two exit-check actions
                                * of this step - pose[6], gripper prob, number of actions averaged (1 or 2) */
/* host mirror (int32 words, pinned + system-coherent): [0] = seq*64 + exit checks completed this step, [1] = seq once every
 * environment exited, [64*(1+b), +64) = environment b's control block at its exit.  Lets the host stop enqueueing the
 * remaining graph segments of a step without the device ever waiting for the host. */
#define DEER_HOSTM_PROGRESS 0
#define DEER_HOSTM_DONE 1
#define DEER_CTL_WORDS 64

/* GEMM epilogues (deer_gemm_bf16_nt) */
#define DEER_EPI_BF16 0
#define DEER_EPI_F32 1
#define DEER_EPI_QGELU_BF16 2
#define DEER_EPI_GELU_BF16 3
#define DEER_EPI_RESADD_F32 4
#define DEER_EPI_BF16OUT 5   /* bf16 store whatever the operand format (deer_gemm_f16_nt: fp16 tower -> bf16 media K/V for the trunk's x-attn) */
/* skinny-GEMM A operand sources */
#define DEER_A_BF16 0
#define DEER_A_SLABS_GELU 1
#define DEER_A_SLABS 2
#define DEER_A_F32 3
/* head input modes / prologues / evaluation kinds / delta types */
#define DEER_X_RAW 0
#define DEER_X_POOL_MAX 1
#define DEER_X_POOL_AVG 2
#define DEER_X_LN 3
#define DEER_PRO_RAW 0
#define DEER_PRO_LN 1
#define DEER_PRO_GROUP_LN_RELU 2
#define DEER_PRO_GROUP_RELU 3
#define DEER_KIND_PSEUDO 0
#define DEER_KIND_CHECK 1
#define DEER_KIND_COMMIT 2
#define DEER_THR_L2 0
#define DEER_THR_MEAN 1
#define DEER_THR_MAX 2
#define DEER_THR_COSINE 3
/* epilogues of deer_head_seq_gemm */
#define DEER_SEQ_EPI_NONE 0
#define DEER_SEQ_EPI_RELU 1
#define DEER_SEQ_EPI_TANH 2
#define DEER_SEQ_EPI_SIGMOID_LOGIT 3

/* ---- MFMA GEMM, large M:  C = epi(A[M,K] * W[N,K]^T + bias) -----------------------------------------------
 * Replaces the nn.Linear / nn.Conv2d(patch embed) calls inside open_clip's ViT-L/14 (called at
 * robot_flamingo/models/flamingo_mpt.py:580), PerceiverAttention/FeedForward (open_flamingo/src/helpers.py:47-52,
 * 15-22) and MaskedCrossAttention.to_kv (helpers.py:190).  A, W bf16; bias f32 or NULL; C bf16 or f32 per `epi`;
 * DEER_EPI_RESADD_F32: C(f32) += tanh(*gate or 1) * (A W^T + bias).  batch: A += z*strideA, C += z*strideC.
 * tile: 0 auto (the selector of csrc/gemm_tiled.hip: by M, N, K and the epilogue), 1 64x64, 2 64x128, 3 128x128; 4..79 name one kernel
 * instantiation each for tests and microbenchmarks (LDS-ring tiles 4-46, 16-wave 32-column rings 51-62, frame tiles = one 257-row camera
 * frame per row tile: 63-73 on 16 waves, 74 / 75 on 8, 76-79 on 4 waves (whole frames only, K % 64 == 0, no erf-GELU epilogue); a tile
 * that does not take the shape / epilogue returns DEER_ERR_SHAPE).  Needs K%8==0, N%16==0. */
int deer_gemm_bf16_nt(const void* A, int lda, long strideA, const void* W, int ldw, const float* bias, void* C, int ldc,
                      long strideC, int M, int N, int K, int batch, int epi, const float* gate, int tile, const int* ctl,
                      void* stream);

/* Batched form with one weight matrix per batch entry: C[z] = epi(A[z] W[z]^T) (Perceiver to_kv of every layer applied to
 * that layer's norm_media(x), helpers.py:47-55: the media tokens do not change across layers). */
int deer_gemm_bf16_nt_wbatch(const void* A, int lda, long strideA, const void* W, int ldw, long strideW, const float* bias,
                             void* C, int ldc, long strideC, int M, int N, int K, int batch, int epi, int tile, const int* ctl,
                             void* stream);
/* Split-K form of deer_gemm_bf16_nt for the latency-bound ViT / Perceiver projections that end in a residual add
 * (open_clip c_proj / out_proj, helpers.py:71 to_out, :22 FeedForward out): slab[s][M][N] (f32) = A[:, Ks] W[:, Ks]^T;
 * the consumer (deer_resadd_ln) sums the slabs, adds the bias and applies the residual + following LayerNorm. */
int deer_gemm_bf16_nt_splitk(const void* A, int lda, const void* W, int ldw, float* slab, int M, int N, int K, int splitk,
                             int tile, const int* ctl, void* stream);

/* ---- the vision tower's fp16 arithmetic (round 6) --------------------------------------------------------------------------------
 * The reference's evaluation runs fp32 weights under fp16 autocast (robot_flamingo/eval/eval_utils.py:333 `torch.cuda.amp.autocast(enabled=
 * self.amp)`, README.md:161-167 `--precision fp32 --amp 1`): every nn.Linear / conv of open_clip's ViT-L/14 and of the PerceiverResampler
 * computes on fp16 operands and returns fp16, LayerNorm / softmax / residual adds run in f32.  The same kernels as the bf16 family above,
 * instantiated on v_mfma_f32_16x16x32_f16 (same issue rate): A, W IEEE fp16; DEER_EPI_BF16 / QGELU_BF16 / GELU_BF16 store FP16 here,
 * DEER_EPI_BF16OUT stores bf16; f32 accumulation and f32 epilogue arithmetic as before.  Same arguments, same tile codes. */
int deer_gemm_f16_nt(const void* A, int lda, long strideA, const void* W, int ldw, const float* bias, void* C, int ldc,
                     long strideC, int M, int N, int K, int batch, int epi, const float* gate, int tile, const int* ctl,
                     void* stream);
int deer_gemm_f16_nt_wbatch(const void* A, int lda, long strideA, const void* W, int ldw, long strideW, const float* bias,
                            void* C, int ldc, long strideC, int M, int N, int K, int batch, int epi, int tile, const int* ctl,
                            void* stream);
int deer_gemm_f16_nt_splitk(const void* A, int lda, const void* W, int ldw, float* slab, int M, int N, int K, int splitk,
                            int tile, const int* ctl, void* stream);
/* deer_attn_mfma_hd64 / _2seg on fp16 q / k / v with an fp16 result (P rounded to fp16 for the P V MFMA; scores, softmax, O in f32) */
int deer_attn_f16_hd64(const void* Q, const void* K, const void* V, void* O, int batch, int heads, int q_len, int kv_len,
                       int ldq, int ldk, int ldv, int ldo, long q_bstride, long k_bstride, long v_bstride, long o_bstride,
                       float scale, void* stream);
int deer_attn_f16_hd64_2seg(const void* Q, const void* K1, const void* V1, const void* K2, const void* V2, void* O, int batch,
                            int heads, int q_len, int kv1, int kv2, int ldq, int ld1, int ld2, int ldo, long q_bstride, long bstride1,
                            long bstride2, long o_bstride, float scale, void* stream);
/* deer_layernorm_rows / _multi / deer_resadd_ln with the 16-bit LayerNorm output in fp16 (the A operand of deer_gemm_f16_nt) */
int deer_layernorm_rows_f16(const float* x, long in_rstride, long in_bstride, int rows_per_batch, int batch, const float* gamma,
                            const float* beta, void* out_f16, float* out_f32, long out_rstride, long out_bstride, int C, float eps,
                            void* stream);
int deer_layernorm_rows_multi_f16(const float* x, long in_rstride, long in_bstride, int rows_per_batch, int batch,
                                  const float* gamma, const float* beta, int n_sets, long param_stride, void* out_f16,
                                  long out_set_stride, long out_rstride, long out_bstride, int C, float eps, void* stream);
int deer_resadd_ln_f16(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias,
                       const float* gamma, const float* beta, void* out_f16, float* out_f32, float* x_copy, int T, int d, float eps,
                       const int* ctl, void* stream);
/* im2col with fp16 patches; img_kind: 0 = f32 frames, 1 = bf16, 2 = fp16 (copied bit for bit) */
int deer_vit_im2col_f16(const void* img, int img_kind, int N, int S, int patch, void* out_f16, int Kpad, void* stream);

/* ---- MFMA GEMM, M <= 128 (weight-streaming): part[ks][Mpad][N] = A[:, Kslice ks] * W[:, Kslice ks]^T ------
 * Replaces the bias-free nn.Linear calls of the MPT GPTBlock (EXTERNAL; constructed mosaic_gpt_3b.py:104-106,
 * called :413-417) and of GatedCrossAttentionBlock (helpers.py:188,231,15-22) at T<=32 text tokens.
 * Wp = deer_pack_weight_mfma16(W).  Mpad = M rounded up to a multiple of 16.  a_mode: DEER_A_BF16 reads A (bf16 [M,lda]);
 * DEER_A_F32 reads A (f32 [M,lda]); DEER_A_SLABS(_GELU) reads sum_s Aslab[s*slab_stride_in + m*K + k] (optionally
 * through exact GELU).  f32 sources are fed to the MFMA as bf16 hi + bf16 lo (two MFMAs per weight fragment; free
 * on this HBM-bound kernel), so the activation keeps ~16 mantissa bits.
 * Partials are reduced by the consumer (deer_resadd_ln / deer_*_attn_small / next deer_gemm_skinny). */
int deer_gemm_skinny(const void* A, int lda, const float* Aslab, int s_in, long slab_stride_in, int a_mode, const void* Wp,
                     float* part, int M, int N, int K, int splitk, const int* ctl, void* stream);
int deer_skinny_splitk(int M, int N, int K);                       /* host helper: suggested split-K */
/* The same Linears for an ENV BATCH of 4-8 environments (49..128 rows), where MFMA time, LDS-read time and the weight stream are
 * the same order: the activation arrives pre-split as two bf16 planes A_hi = bf16(a), A_lo = bf16(a - A_hi), each [>= M rows, lda]
 * (written by deer_resadd_ln_split / deer_mpt_attn_small_hl / deer_slab_gelu_split), and is staged - together with the packed
 * weight fragments - by LDS-DMA into a ring (counted vmcnt + one raw barrier per 64 K-columns).  128-column workgroups:
 * splitk = deer_skinny_hl_splitk(M, N, K) slabs, half as many as deer_gemm_skinny.  K % (64 * splitk) == 0.  part[ks][Mpad][N];
 * rows M..Mpad-1 are written as zeros. */
int deer_gemm_skinny_hl(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk,
                        const int* ctl, void* stream);
int deer_skinny_hl_splitk(int M, int N, int K);
/* the same for up to 512 rows (8 environments x 32-token instructions, data.py:905-919): row blocks of <= 128 rows, one launch each,
 * part[ks][slab_rows][N] with slab_rows >= 16 * ceil(M / 16) */
int deer_gemm_skinny_hl_rows(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk,
                             int slab_rows, const int* ctl, void* stream);
/* hi / lo planes [rows, C] of act(sum_s slab[s]) (act = exact GELU when gelu != 0): the activation of the down-projections
 * (GELU between mlp_up / mlp_down of the MPT block and ff.1 / ff.3 of the gated x-attn block, helpers.py:15-22), computed ONCE
 * instead of once per column group of the consumer. */
int deer_slab_gelu_split(const float* slab, int s_in, long slab_stride, int gelu, void* out_hi, void* out_lo, int rows, int C,
                         const int* ctl, void* stream);
int deer_pack_weight_mfma16(const void* W, void* Wp, int N, int K, void* stream);  /* [N,K] -> [N/16][K/32][64][8] */

/* ---- attention ----------------------------------------------------------------------------------------------
 * deer_attn_mfma_hd64: softmax(scale * Q K^T) V per (batch, head), head_dim 64, kv_len <= 320 (<= 576 through a 36-key-tile instantiation of the same
 * kernel, one workgroup per CU: pre fusion's two-segment call over 2 x 256 patch tokens + 64 latents).  Replaces
 * nn.MultiheadAttention inside the open_clip ViT blocks and the einsum/softmax of PerceiverAttention
 * (helpers.py:53-63).  Q,K,V,O bf16 with row strides ld* and batch strides *_bstride (elements); head h lives at
 * column h*64. */
int deer_attn_mfma_hd64(const void* Q, const void* K, const void* V, void* O, int batch, int heads, int q_len, int kv_len,
                        int ldq, int ldk, int ldv, int ldo, long q_bstride, long k_bstride, long v_bstride, long o_bstride,
                        float scale, void* stream);
/* Same with the keys/values in two segments ([0,kv1) from K1/V1 with row stride ld1, [kv1,kv1+kv2) from K2/V2 with ld2):
 * PerceiverAttention's kv = [media ; latents] (helpers.py:51) without materialising the concatenation. */
int deer_attn_mfma_hd64_2seg(const void* Q, const void* K1, const void* V1, const void* K2, const void* V2, void* O, int batch,
                             int heads, int q_len, int kv1, int kv2, int ldq, int ld1, int ld2, int ldo, long q_bstride,
                             long bstride1, long bstride2, long o_bstride, float scale, void* stream);
/* deer_xattn_mfma: MaskedCrossAttention core (helpers.py:192-232) on the MFMA attention kernel: q = sum of f32 split-K slabs
 * [batch*T, ldqs], kv bf16 [batch*n_kv, ldkv] (k at col h*64, v at col inner+h*64), key j visible iff
 * text_time[t] == j/n_per_media + 1, rows with text_time == 0 zeroed; out f32 or bf16 [batch*T, ldo]. */
int deer_xattn_mfma(const float* qslab, int s_in, long slab_stride, int ldqs, const void* kv, int ldkv, int inner,
                    const int* text_time, int n_per_media, void* out, int out_is_f32, int ldo, int T, int n_kv, int heads,
                    int batch, float scale, const int* ctl, void* stream);
/* deer_xattn_fused: to_q -> masked cross-attention -> to_out of MaskedCrossAttention (helpers.py:184-233) as ONE launch.  xn: f32
 * [batch*T, d] (= attn.norm(x)); Wq_p / Wo_p: to_q [inner,d] / to_out [d,inner] packed by deer_pack_weight_mfma16; kv as above;
 * out: f32 [heads][slab_stride]: slab h = head h's contribution to y = Attn(x) for all rows (the consumer deer_resadd_ln sums
 * the `heads` slabs, s_in = heads).  T <= 32, n_kv <= 128, d % 128 == 0. */
int deer_xattn_fused(const float* xn, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time,
                     int n_per_media, int n_kv, const void* Wo_p, float* out, long slab_stride, int T, int heads, int batch,
                     float scale, const int* ctl, void* stream);
/* deer_xattn_small: the same op as fp32 VALU code (kept as a second implementation for cross-checks) (helpers.py:192-232): q from split-K slabs (x scale), kv bf16
 * [n_kv, ldkv] (k at col h*64, v at col inner+h*64), mask text_time[t] == j/n_per_media + 1, rows with
 * text_time == 0 zeroed; out bf16 or f32 [T, ldo]. */
int deer_xattn_small(const float* qslab, int s_in, long slab_stride, int ldqs, const void* kv, int ldkv, int inner,
                     const int* text_time, int n_per_media, void* out, int out_is_f32, int ldo, int T, int n_kv, int heads,
                     int batch, float scale, const int* ctl, void* stream);
/* deer_mpt_attn_small: MPT attention core (attn bias built at mosaic_gpt_3b.py:158-219): qkv from
 * split-K slabs [T,3d]; optional q/k LayerNorm over d_model (weights f32 or NULL); ALiBi slope
 * 2^(-alibi_bias_max*(h+1)/H); causal; key_mask (uint8[T], 0 = padded) or NULL; qkv_ws = f32 [T,3d] workspace;
 * out bf16 or f32 [T, ldo].  Two launches: slab reduce + q/k LayerNorm (one workgroup per row and q|k|v), then one
 * workgroup per head. */
int deer_mpt_attn_small(const float* qkvslab, int s_in, long slab_stride, int d_model, int n_heads, const float* q_ln_w,
                        const float* k_ln_w, float eps, const unsigned char* key_mask, float alibi_bias_max, float* qkv_ws,
                        void* out, int out_is_f32, int ldo, int T, int batch, const int* ctl, void* stream);
/* the same op, output as two bf16 planes hi = bf16(o), lo = bf16(o - hi), each [batch*T, ldo] (operand of deer_gemm_skinny_hl) */
int deer_mpt_attn_small_hl(const float* qkvslab, int s_in, long slab_stride, int d_model, int n_heads, const float* q_ln_w,
                           const float* k_ln_w, float eps, const unsigned char* key_mask, float alibi_bias_max, float* qkv_ws,
                           void* out_hi, void* out_lo, int ldo, int T, int batch, const int* ctl, void* stream);

/* ---- the trunk at ONE environment, <= 16 text rows (csrc/trunk_r16.hip) ----
 * deer_trunk_wide_gemm: the wide bias-free Linears of a layer (helpers.py:15-22 ff.1; MPT block, SURVEY App. B.1: Wqkv, mlp_up) with the K
 * split INSIDE the workgroup, so the result leaves final.  a_hi / a_lo: the LayerNorm output as bf16 planes in MFMA-fragment order
 * [K/32][64][8] (deer_resadd_ln_packed); Wp = packed [N, K] (deer_pack_weight_mfma16); N % 32 == 0, K = 256 or 2048, T <= 16.
 * epi 0: out_f32 [T, ldo]; 1: exact GELU (helpers.py:19 / the MPT MLP) -> row-major bf16 hi / lo planes [T, ldo] (operand of
 * deer_gemm_skinny_hl for ff.3 / mlp_down); 2: out_f32 + stats [N/32][16][2] = (mean, centred sum of squares) of every row over each
 * 32-column group (combined by deer_trunk_mpt_attn into the q / k LayerNorm over d_model). */
int deer_trunk_wide_gemm(const void* a_hi, const void* a_lo, const void* Wp, int N, int K, int epi, float* out_f32, void* out_hi, void* out_lo,
                         int ldo, float* stats, int T, const int* ctl, void* stream);
/* deer_trunk_mpt_attn: MPT attention core like deer_mpt_attn_small on FINAL f32 q|k|v [T, 3 d_model] (no slabs); the q / k LayerNorm over
 * d_model (attn_qk_ln, weights or NULL) from the 32-column moments `stats` of deer_trunk_wide_gemm(epi 2); out as row-major bf16 hi / lo
 * planes [T, ldo].  d_model % 256 == 0, T <= 16. */
int deer_trunk_mpt_attn(const float* qkv, const float* stats, int d_model, int n_heads, const float* q_ln_w, const float* k_ln_w, float eps,
                        const unsigned char* key_mask, float alibi_bias_max, void* out_hi, void* out_lo, int ldo, int T, const int* ctl,
                        void* stream);
/* deer_resadd_ln_split with the two planes in MFMA-fragment order [d/32][64 lanes][8], lane = 16 * (k % 32 / 8) + row (T <= 16): the operand
 * of deer_trunk_wide_gemm / deer_xattn_fused_packed reads back as one contiguous 1 KiB per k-tile and plane. */
int deer_resadd_ln_packed(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias, const float* gamma,
                          const float* beta, void* out_hi, void* out_lo, float* out_f32, float* x_copy, int T, int d, float eps, const int* ctl,
                          void* stream);
/* deer_xattn_fused for ONE environment of <= 16 rows with LN(x) as fragment-ordered bf16 hi / lo planes (deer_resadd_ln_packed) */
int deer_xattn_fused_packed(const void* x_hi, const void* x_lo, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time,
                            int n_per_media, int n_kv, const void* Wo_p, float* out, long slab_stride, int T, int heads, float scale,
                            const int* ctl, void* stream);

/* deer_resadd_ln for the env-batch vision tower (d == 1024, bf16 LayerNorm output, no control block): rows_per_wg = 2 or 4 rows per workgroup,
 * all loads of all rows in flight before the first use, one pair of block reductions for the R rows.  Per row bit-identical to deer_resadd_ln,
 * which selects it from 2048 rows on (open_clip ResidualAttentionBlock residual + ln_1 / ln_2 of the next op). */
int deer_resadd_ln_multirow(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias, const float* gamma,
                            const float* beta, void* out_bf16, int T, int d, float eps, int rows_per_wg, void* stream);

/* ---- env batch with COMPACTION of exited environments (the reference stops every environment at its own layer,
 * mosaic_gpt_3b.py:438-443): the rows of the still-active environments stay packed at the front of the trunk's buffers.  Row map `cmap`
 * (int32, CMAP_WORDS = 64 per copy): [0] = active slots, [1 + s] = environment of slot s, [17 + e] = slot of environment e or -1 (up to 16 environments).  The
 * *_active / *_rows entry points are the kernels above restricted to the active slots (rows_per_env rows each); per-environment inputs
 * (media K/V, text_time, key mask, control blocks) stay in environment order and are reached through the map. ---- */
int deer_resadd_ln_rows(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* gamma, const float* beta, void* out_bf16,
                        void* out_lo, float* out_f32, float* x_copy, int T_rows, int d, float eps, const int* ctl, const int* cmap, int rows_per_env,
                        const float* x_in, const int* cmap_old, int B, int drop_upto, void* stream);   /* x_in != NULL: gather the surviving rows (first row op of a compaction layer: environments that exited at a layer <= drop_upto leave), publish the new map into cmap */
int deer_gemm_skinny_hl_active(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk, int slab_rows,
                               const int* ctl, const int* cmap, int rows_per_env, void* stream);
int deer_slab_gelu_split_active(const float* slab, int s_in, long slab_stride, int gelu, void* out_hi, void* out_lo, int rows, int C, const int* ctl,
                                const int* cmap, int rows_per_env, void* stream);
int deer_mpt_attn_small_hl_active(const float* qkvslab, int s_in, long slab_stride, int d_model, int n_heads, const float* q_ln_w, const float* k_ln_w,
                                  float eps, const unsigned char* key_mask, float alibi_bias_max, float* qkv_ws, void* out_hi, void* out_lo, int ldo, int T,
                                  int batch, const int* ctl, const int* cmap, void* stream);
int deer_xattn_fused_active(const float* xn, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time, int n_per_media, int n_kv,
                            const void* Wo_p, float* out, long slab_stride, int T, int heads, int batch, float scale, const int* ctl, const int* cmap,
                            void* stream);
int deer_head_pool_active(const float* feats, float* pooled, int T, int d, int avg, int B, const unsigned char* key_mask, const int* ctl, int kind,
                          int layer, const int* cmap, void* stream);
int deer_ctl_begin_step_map(int* ctl, const int* step_info, int B, int* cmap, void* stream);   /* deer_ctl_begin_step + both map copies := identity */

/* (deer_head_*: w_is_f32 = 1 when the weight pointers are f32 - the fp32 arithmetic keeps the head's weights in f32) */

/* ---- fp32-activation arithmetic (csrc/precise.hip; deer_config.precision = 1): the second arithmetic of the path, for
 * north_star's "1e-3 fp32" clause.  Activations AND weights stay f32 end to end (the arena keeps f32 / hi+lo copies in this mode). */
/* every nn.Linear / conv of the ViT, the Perceiver and the media K/V projection: C f32 [M,N] (op)= A f32 [M,K] * W[N,K]^T + bias with
 * the exact-f32 MFMA.  epi: 0 store, 1 QuickGELU, 2 exact GELU, 3 C += (residual add).  K % 4 == 0, N % 4 == 0. */
int deer_gemm_f32_nt(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N, int K,
                     int epi, void* stream);
/* open_clip MHA core / PerceiverAttention core (helpers.py:47-73) in fp32: q [batch][q_len][ldq] (head h at column h*64), keys and
 * values in one or two segments ([batch][kv_s][ld_s], pointers at the K / V column offset), out f32 [batch][q_len][ldo].
 * head_dim 64, kv1 + kv2 <= 352 with the keys of a head resident in LDS; up to 664 keys (pre fusion: 576) through a chunked form (its 156 KB of LDS). */
int deer_attn_f32(const float* Q, const float* K1, const float* V1, const float* K2, const float* V2, float* O, int batch, int heads,
                  int q_len, int kv1, int kv2, int ldq, int ld1, int ld2, int ldo, long q_bstride, long bstride1, long bstride2,
                  long o_bstride, float scale, void* stream);
/* MaskedCrossAttention core (helpers.py:192-232) with f32 K/V: q from split-K slabs, kv f32 [batch][n_kv][ldkv] (k at column h*64, v at
 * inner + h*64), media-time mask from text_time, out f32 [batch][T][ldo]. */
int deer_xattn_f32(const float* qslab, int s_in, long slab_stride, int ldqs, const float* kv, int ldkv, int inner, const int* text_time,
                   int n_per_media, float* out, int ldo, int T, int n_kv, int heads, int batch, float scale, const int* ctl, void* stream);

/* deer_embed_tokens with an f32 table */
int deer_embed_tokens_f32(const long long* ids, const float* wte, float* x, int* text_time, int T, int batch, int d, int vocab,
                          int media_id, void* stream);
/* im2col of the camera frames in f32 (deer_vit_im2col keeps bf16): out f32 [N*P, Kpad] */
int deer_vit_im2col_f32(const float* img, int N, int S, int patch, float* out, int Kpad, void* stream);

/* ---- row ops ------------------------------------------------------------------------------------------------
 * deer_layernorm_rows: nn.LayerNorm (ViT ln_1/ln_2, helpers.py:32-33,17,132), f32 in, bf16 and/or f32 out. */
int deer_layernorm_rows(const float* x, long in_rstride, long in_bstride, int rows_per_batch, int batch, const float* gamma,
                        const float* beta, void* out_bf16, float* out_f32, long out_rstride, long out_bstride, int C,
                        float eps, void* stream);
/* deer_layernorm_rows_multi: one pass of statistics, n_sets affine outputs out[s] = LN(x)*gamma[s]+beta[s] (Perceiver
 * norm_media of all layers on the same media tokens, helpers.py:32,47). */
int deer_layernorm_rows_multi(const float* x, long in_rstride, long in_bstride, int rows_per_batch, int batch,
                              const float* gamma, const float* beta, int n_sets, long param_stride, void* out_bf16,
                              long out_set_stride, long out_rstride, long out_bstride, int C, float eps, void* stream);
/* deer_resadd_ln: x += tanh(*gate or 1) * (sum_s slab[s] + bias or 0); optional copy of x (hidden_states[i], mosaic_gpt_3b.py:424-427);
 * optional LayerNorm -> bf16 and/or f32 (helpers.py:267-279 gated residuals; MPT block residuals + ln_1/ln_2). */
int deer_resadd_ln(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias,
                   const float* gamma,
                   const float* beta, void* out_bf16, float* out_f32, float* x_copy, int T, int d, float eps, const int* ctl,
                   void* stream);
/* deer_resadd_ln with the LayerNorm output ALSO as two bf16 planes hi = bf16(y), lo = bf16(y - hi) (operand of deer_gemm_skinny_hl);
 * out_f32 optional. */
int deer_resadd_ln_split(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias,
                         const float* gamma, const float* beta, void* out_hi, void* out_lo, float* out_f32, float* x_copy, int T,
                         int d, float eps, const int* ctl, void* stream);
/* ViT patch embedding (open_clip conv1 + class/positional embedding + ln_pre) */
int deer_vit_im2col(const void* img, int img_is_bf16, int N, int S, int patch, void* out_bf16, int Kpad, void* stream);
int deer_vit_embed_lnpre(const float* patch, const float* cls, const float* pos, const float* ln_w, const float* ln_b,
                         float* x, int N, int P, int W, float eps, void* stream);
/* wte lookup (mosaic_gpt_3b.py:341) + text_time = cumsum(ids == media_token_id) (flamingo_lm.py:211, helpers.py:208) */
int deer_embed_tokens(const long long* ids, const void* wte_bf16, float* x, int* text_time, int T, int batch, int d, int vocab,
                      int media_id, void* stream);
int deer_broadcast_rows(const float* src, float* dst, long n, int batch, void* stream);   /* helpers.py:128 */

/* ---- action head + exit gate (robot_flamingo/models/action_head.py:499-611, value_net.py:105-133,277-297) -----
 * All three evaluate a BATCH of B <= 16 independent environments (weights read once per 8 environments: batches above 8 run in two halves): features [B][T][d],
 * LSTM state tensors [L][B][H], control blocks ctl + b*DEER_CTL_WORDS, exit decision per environment. */
int deer_head_pool(const float* feats, float* pooled, int T, int d, int avg, int B, const unsigned char* key_mask, const int* ctl,
                   int kind, int layer, void* stream);
/* DeterministicDecoder(use_state=True) (action_head.py:443-453,524-536): deer_head_state_embed computes, per environment, the embedding
 * W_state [relu(W_arm arm + b_arm) ; relu(E_grip[(g + 1) / 2])] + b_state of the robot state (state [B][8] f32: arm pose robot_obs[:6],
 * gripper opening robot_obs[-1], pad); deer_head_pool_state is deer_head_pool with that embedding added to the pooled feature. */
int deer_head_state_embed(const float* state, const float* w_arm, const float* b_arm, const float* e_grip, const void* w_state,
                          const float* b_state, float* out, int d, int B, int w_is_f32, void* stream);
int deer_head_pool_state(const float* feats, float* pooled, int T, int d, int avg, int B, const unsigned char* key_mask,
                         const float* state_emb, const int* ctl, int kind, int layer, void* stream);   /* AdaptiveMax/AvgPool1d over the text tokens (action_head.py:480-483,
                   519-520); key_mask (uint8 [B][T], 0 = right-padding of an env batch, data.py:905-919) or NULL */
int deer_head_lstm_layer(const float* x_src, long x_bstride, int x_mode, int T, int in_dim, const float* ln_w, const float* ln_b,
                         const void* w_ih, const void* w_hh, const float* b_ih, const float* b_hh, const float* h_prev,
                         const float* c_prev, float* h_out, float* c_out, int H, int B, float eps, const int* ctl, int kind,
                         int layer, int w_is_f32, void* stream);
/* The recurrent half of all LSTM layers once per control step: ghh[l][b][q*H + j] = W_hh^l[q*H + j, :] . h_state[l][b] + b_hh^l (L <= 8 layers in
 * one launch; h_state [L][B][H]).  Every head evaluation of a step (pseudo / exit checks / committing call) starts from the state the previous
 * step committed (action_head.py:560-575, update_hidden_state=False until the committing call), so this half is common to all of them. */
int deer_head_lstm_hh(const void* const* w_hh, const float* const* b_hh, int L, const float* h_state, float* ghh, int H, int B, int w_is_f32,
                      void* stream);
/* deer_head_lstm_layer with its recurrent half taken from ghh ([B][4H] of this layer): streams W_ih only. */
int deer_head_lstm_layer_pre(const float* x_src, long x_bstride, int x_mode, int T, int in_dim, const float* ln_w, const float* ln_b,
                             const void* w_ih, const float* b_ih, const float* ghh, const float* c_prev, float* h_out, float* c_out, int H, int B,
                             float eps, const int* ctl, int kind, int layer, int w_is_f32, void* stream);
int deer_head_fc(const float* src, int src_stride, int in_dim, int pro, const float* lnw0, const float* lnb0, const float* lnw1,
                 const float* lnb1, const void* W0, const float* b0, const void* W1, const float* b1, int out_dim, float* dst,
                 int B, float eps, const int* ctl, int kind, int layer, int w_is_f32, void* stream);
int deer_head_final(const float* src, int src_stride, int in_dim, int pro, const float* lnw0, const float* lnb0, const float* lnw1,
                    const float* lnb1, const void* Wa, const float* ba, const void* Wg, const float* bg, int* ctl, int kind,
                    int layer, int slot, const float* thresholds, int force, int thr_type, int leq, const float* h_tmp,
                    const float* c_tmp, float* h_state, float* c_state, int L, int H, int B, float* action_dbg, float eps,
                    int w_is_f32, void* stream);
/* the same with multi_step_action = A (action_head.py:458,472-473: Wa [6 A, in_dim], Wg [A, in_dim]; the criterion's delta over all 6 A pose
 * values; ModelWrapper executes the first multi_execution of the A actions, eval_utils.py:466-475).  action_dbg: [B][64] f32 = pose 6 A |
 * gripper A | logit A.  A > 1 with a control block: act_ext [B][4][64] f32 holds the previous / committed / ensemble action (the 8-float
 * fields of the control block then carry the FIRST action), and a host mirror carries [B][128] f32 (committed | ensemble) behind its
 * (1 + B) * 64 words. */
int deer_head_final_multi(const float* src, int src_stride, int in_dim, int pro, const float* lnw0, const float* lnb0, const float* lnw1,
                          const float* lnb1, const void* Wa, const float* ba, const void* Wg, const float* bg, int* ctl, int kind,
                          int layer, int slot, const float* thresholds, int force, int thr_type, int leq, const float* h_tmp,
                          const float* c_tmp, float* h_state, float* c_state, int L, int H, int B, float* action_dbg, float eps,
                          int w_is_f32, int multi_step_action, float* act_ext, void* stream);
/* the same with a per-environment operating point (several exit ratios / layer caps side by side in one env batch): env_exit is the table
 * [DEER_MAX_ENVS * 16 + DEER_MAX_ENVS] words of csrc/common.h (ENV_EXIT_*): f32 threshold row of environment b at b * 16, int32 layer cap of
 * environment b at word 256 + b.  Environment b's check compares with its own row and is forced at layer >= its cap (or when `force` is
 * set); everything else is deer_head_final_multi's. */
int deer_head_final_env(const float* src, int src_stride, int in_dim, int pro, const float* lnw0, const float* lnb0, const float* lnw1,
                        const float* lnb1, const void* Wa, const float* ba, const void* Wg, const float* bg, int* ctl, int kind,
                        int layer, int slot, const float* env_exit, int force, int thr_type, int leq, const float* h_tmp,
                        const float* c_tmp, float* h_state, float* c_state, int L, int H, int B, float* action_dbg, float eps,
                        int w_is_f32, int multi_step_action, float* act_ext, void* stream);
/* writes n_envs rows (f32 [n_envs][16], device memory when rows_on_device, else host memory copied into the launch) and n_envs caps (host
 * int32) into an env_exit table, as one launch on `stream`. */
int deer_env_exit_write(float* env_exit, const float* rows, int rows_on_device, const int* caps, int n_envs, void* stream);
/* ---- window mode of the head (csrc/head_seq.hip): DeterministicDecoder.forward on N sequences of L steps, action_head.py:499-611 ----
 * Layer-major pieces that deer_head_sequence (deer_model.h) chains; w_kind: 0 bf16, 1 f32, 2 fp16 weight rows (nn.Linear layout [N][K]).
 * deer_head_seq_pool        AdaptiveMax/AvgPool1d over the T rows of each of M (sequence, step) rows (action_head.py:519-520; no key mask
 *                           reaches the head), + emb[M][d] (the robot-state embedding, :536) when emb != NULL.  feats [M][T][d] -> X [M][d].
 * deer_head_seq_state_u     u [M][2d] = [relu(embed_arm_state(state[:6])) ; relu(embed_gripper_state((state[6] + 1) / 2))] (:526-532),
 *                           state [M][8] f32; embed_state (:533) is then deer_head_seq_gemm on u.
 * deer_head_seq_gemm        out[m][n] = epi(X[m] . W[n] + bias[n]) (nn.Linear, :86-136): MFMA, 16-bit weights against the hi + lo
 *                           planes of the f32 activations, f32 weights on the f32 MFMA.  DEER_SEQ_EPI_SIGMOID_LOGIT also stores the
 *                           logit at out[m][N + n].  K % 8 == 0, ldx % 8 == 0.
 * deer_head_seq_lstm_step   one step of one nn.LSTM layer over N rows (torch gate order i, f, g, o): gates = pre[m] + h_prev[m] W_hh^T + b_hh,
 *                           c_state [N][H] updated in place, h to h_out (row stride ld_out), (h_n, c_n) [N][H] too when not NULL;
 *                           h_prev NULL = zero state.  H % 16 == 0.
 * deer_head_seq_ln          LayerNorm of M rows of n values (LayerNormLSTM :44-53, MLP LayerNorm :97-103), ReLU when relu != 0; in place allowed. */
int deer_head_seq_pool(const float* feats, const float* emb, float* X, int M, int T, int d, int avg, void* stream);
int deer_head_seq_state_u(const float* state, const float* w_arm, const float* b_arm, const float* e_grip, float* u, int M, int d,
                          void* stream);
int deer_head_seq_gemm(const float* X, long ldx, const void* W, int w_kind, const float* bias, float* out, long ldo, int M, int N, int K,
                       int epi, void* stream);
int deer_head_seq_lstm_step(const float* pre, long ld_pre, const float* h_prev, long ld_h, const void* w_hh, int w_kind, const float* b_hh,
                            float* c_state, float* h_out, long ld_out, float* h_n, float* c_n, int N, int H, void* stream);
int deer_head_seq_ln(const float* src, long ld_src, float* dst, long ld_dst, const float* w, const float* b, int M, int n, float eps, int relu,
                     void* stream);
/* ---- threshold calibration as one device pass (csrc/calib.hip): ActionValueNet.forward(mode='generate'), value_net.py:134-160 ----
 * Pieces that deer_pool_exit_layers / deer_calibrate_values (deer_model.h) chain with the window-mode GEMM / LayerNorm above.
 * deer_calib_pool_layers    P[frame][k][d] = max / mean over the T rows of frame `frame` of hidden[layers[k]] (action_head.py:519-520, all T
 *                           rows); hidden + layer * layer_stride + (frame * T + t) * d.  layers: HOST int[NL], NL <= DEER_CALIB_MAX_NL.  d % 4 == 0.
 * deer_calib_gather         rows of a chunk of bc windows from P [bc][W][NL][d]: X[(b, t)] = P[b][t][slot_of_layer[rand_layers[b][t]]] for
 *                           t < W - 1 (the history, flamingo_mpt.py:486-490), then X[bc (W - 1) + (k, b, s)] = P[b][W/2 - 1 + s][k] for
 *                           s < W - W/2 (the candidates, value_net.py:139-153), and idx[(k, b, s)] = history row (b, W/2 - 2 + s) or -1.
 *                           rand_layers: DEVICE int32 [bc][W]; slot_of_layer: HOST int[n_layers] (-1: no slot -> NaN row).
 * deer_calib_lstm_step      launches the sequence head's step kernel (deer_head_seq_lstm_step's, csrc/head_seq.hip) with a read-only previous
 *                           state: row m continues from row idx[m] (idx NULL: m) of h_prev / c_prev (row strides ld_h / ld_c); a negative
 *                           index or h_prev NULL = the zero state (zero_row: H zeros).  c to c_out (or dropped when NULL), h to h_out.
 * deer_calib_delta          values[e][r] = get_delta(actions[e][r], actions[e + 1][r]) (value_net.py:105-117) over the first NP values of
 *                           each action row; actions [NL][rows][ld_act], values [NL - 1][ld_val]; thr_type 0 L2, 1 mean, 2 max, 3 cosine. */
#define DEER_CALIB_MAX_NL 17
#define DEER_CALIB_MAX_LAYERS 64
int deer_calib_pool_layers(const float* hidden, long layer_stride, const int* layers, int NL, float* P, int n_frames, int T, int d, int avg,
                           void* stream);
int deer_calib_gather(const float* P, const int* rand_layers, const int* slot_of_layer, int n_layers, float* X, int* idx, int bc, int W,
                      int NL, int d, void* stream);
int deer_calib_lstm_step(const float* pre, long ld_pre, const float* h_prev, long ld_h, const float* c_prev, long ld_c, const int* idx,
                         const float* zero_row, const void* w_hh, int w_kind, const float* b_hh, float* c_out, long ld_co, float* h_out,
                         long ld_out, int N, int H, void* stream);
int deer_calib_delta(const float* actions, long ld_act, int NL, int rows, int NP, int thr_type, float* values, long ld_val, void* stream);
/* ---- per-exit demonstration loss (csrc/exit_eval.hip): the all-exits window forward and the forward half of the multi-exit step ----
 * Pieces that deer_exit_outputs (deer_model.h) chains with deer_calib_pool_layers (the pooling of an arbitrary host list of layers: reused,
 * there is no second pooling kernel) and the window-mode head above.
 * deer_window_gather_layers  the layer mixing of the two sampling strategies (robot_flamingo/models/flamingo_mpt.py:485-490 and :499-505)
 *                            on POOLED rows (pooling, action_head.py:519-520, commutes with the per-step layer choice):
 *                            X[s][(b, t)] = P[(b, t)][slot_of_layer[sel[s][b][t]]], all S selections in one launch.  P [bs W][NL][d];
 *                            sel: DEVICE int32 [S][bs][W] exit layers; slot_of_layer: HOST int[n_layers] (-1: no slot -> NaN row, as
 *                            deer_calib_gather).  d % 4 == 0 (16-byte loads and stores).
 * deer_exit_losses           robot_flamingo/train/train_utils.py:519-540 for Hn heads over R = bs W rows: actions [Hn][R][8 A] = [pose 6 A |
 *                            prob A | logit A], labels pose [R][6 A] and grip01 [R][A] ->
 *                              num[h][r]  = F.huber_loss(pose, label, reduction='none').mean(-1), delta = 1           (:520)
 *                              bin[h][r]  = F.binary_cross_entropy_with_logits(logit, grip01, reduction='none').mean(-1), computed as
 *                                           max(x, 0) - x y + log1p(exp(-|x|))                                         (:529)
 *                              loss[h]    = mean over r of num + w_bin bin (w_bin 0.01, or 0.05 for real data)          (:534-540)
 *                            No atomics: per head one workgroup sums its rows in a fixed order.  The exit weighting (get_exit_weights,
 *                            :541) is the caller's, from loss[h]. */
int deer_window_gather_layers(const float* P, const int* sel, const int* slot_of_layer, int n_layers, float* X, int S, int bs, int W, int NL,
                              int d, void* stream);
int deer_exit_losses(const float* actions, const float* pose, const float* grip01, int Hn, long R, int A, float w_bin, float* num, float* bin,
                     float* loss, void* stream);
/* ---- exit-only fine-tuning of one head (csrc/head_grad.hip): the backward half of the multi-exit step with a frozen trunk
 * (only_train_head / no_backbone_grad, robot_flamingo/train/train_utils.py:487-543) and its optimizer (train_calvin_post_strategy.py:535) ----
 * Pieces that deer_head_loss_grad (deer_model.h) chains with deer_head_seq_gemm on f32 weight rows.  f32 arithmetic, fixed summation
 * orders, no atomics (two runs give identical bits); no dropout.
 * deer_head_grad_ln            launches the sequence head's LayerNorm kernel (deer_head_seq_ln's, csrc/head_seq.hip: LayerNormLSTM
 *                              action_head.py:44-53, MLP LayerNorm :97-103) and also keeps stats [M][2] = (mean, rstd) of every row for the backward
 * deer_head_grad_lstm_step     launches the sequence head's step kernel (deer_head_seq_lstm_step's: one nn.LSTM step over N rows, gate order
 *                              i, f, g, o) on f32 W_hh [4H][H] with a tape:
 *                              gates [N rows, pitch ld_g][4H] holds x W_ih^T + b_ih on entry and the ACTIVATED gates on return; c_out / h_out
 *                              receive c_t and the raw h_t; h_prev / c_prev both NULL at t = 0 (zero state).  H % 16 == 0.
 * deer_head_grad_loss          loss = mean_rows( mean_6A Huber_1(pose - label) + w_bin mean_A BCEwithlogits(logit, target) ) of one head
 *                              (train_utils.py:519-540): launches deer_exit_losses' two kernels (csrc/exit_eval.hip) for one head (num, bin [R], loss [1]), with
 *                              dz [R][8 A] = d (scale loss) / d [pre-tanh pose 6 A | gripper logit A | 0 A] (autograd of :519-543; scale =
 *                              exit weight x accumulation share).  actions [R][8 A] = [pose 6 A | prob A | logit A].
 * deer_head_grad_gemm          C[M][N] (+)= sum_k opA(m, k) opB(n, k), exact-f32 MFMA (v_mfma_f32_16x16x4_f32): ta / tb = 0 operand stored
 *                              [rows][K], 1 stored [K][rows].  Linear backward: dX = dY W is (dY, ta 0; W, tb 1), dW = dY^T X is (dY, ta 1;
 *                              X, tb 1) (torch.nn.Linear's autograd).  Any M, N, K; 16-byte accesses where pointer, pitch and extent allow.
 * deer_head_grad_colsum        out_sum[c] (and out_sum2[c]) (+)= sum_m dy[m][c] (bias gradient, LayerNorm d beta); with x / stats:
 *                              out_xhat[c] (+)= sum_m dy[m][c] (x[m][c] - mean_m) rstd_m (LayerNorm d gamma)
 * deer_head_grad_relu_mask     dz[i] = act[i] > 0 ? dz[i] : 0 (ReLU backward from its output), n % 4 == 0 contiguous values
 * deer_head_grad_ln_bwd        LayerNorm d input of M rows: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dx may be dy
 * deer_head_grad_lstm_bwd_step one step of the LSTM's backward through time over N rows: dh_t = dh_ext + dG_{t+1} W_hh (dg_next NULL at the
 *                              last step: no recurrent term and dc taken as zero), dG_t [.., pitch ld_g][4H] = the pre-activation gate
 *                              gradients, dc [N][H] <- dc_{t-1}; gates / c_t / c_prev (NULL at t = 0) from the tape.  H % 16 == 0.
 * deer_adamw_step              torch.optim.AdamW (_single_tensor_adamw) over flat f32 buffers: p <- p (1 - lr wd) on decaying segments,
 *                              m, v moments, bias corrections 1 - beta^step, p <- p - lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  seg_end /
 *                              seg_decay: DEVICE int32 [n_seg] ascending exclusive segment ends and decay flags (norms and biases: 0);
 *                              n_seg = 0: every element decays; elements past the last end take no decay.  hyper: HOST double[5] = {lr,
 *                              beta1, beta2, eps, weight_decay} - doubles, because torch forms 1 - beta and the bias corrections in
 *                              Python floats before its f32 kernels see them (1 - 0.999f is off by 1.3e-5).  step >= 1. */
int deer_head_grad_ln(const float* src, long ld_src, float* dst, long ld_dst, const float* w, const float* b, float* stats, int M, int n, float eps,
                      int relu, void* stream);
int deer_head_grad_lstm_step(float* gates, long ld_g, const float* h_prev, long ld_h, const float* w_hh, const float* b_hh, const float* c_prev,
                             float* c_out, long ld_c, float* h_out, long ld_out, int N, int H, void* stream);
int deer_head_grad_loss(const float* actions, const float* pose, const float* grip01, long R, int A, float w_bin, float scale, float* dz, float* num,
                        float* bin, float* loss, void* stream);
int deer_head_grad_gemm(const float* A, long lda, int ta, const float* B, long ldb, int tb, float* C, long ldc, int M, int N, int K, int accumulate,
                        void* stream);
int deer_head_grad_colsum(const float* dy, long ld, const float* x, long ldx, const float* stats, float* out_sum, float* out_sum2, float* out_xhat,
                          int M, int n, int accumulate, void* stream);
int deer_head_grad_relu_mask(float* dz, const float* act, long n, void* stream);
int deer_head_grad_ln_bwd(const float* dy, long ld_dy, const float* x, long ld_x, const float* stats, const float* gamma, float* dx, long ld_dx,
                          int M, int n, void* stream);
int deer_head_grad_lstm_bwd_step(const float* dh_ext, long ld_dh, const float* dg_next, const float* gates, float* dg, long ld_g, const float* w_hh,
                                 const float* c_t, const float* c_prev, long ld_c, float* dc, int N, int H, void* stream);
int deer_adamw_step(float* param, const float* grad, float* m, float* v, long numel, const int* seg_end, const int* seg_decay, int n_seg,
                    const double* hyper, int step, void* stream);
/* ---- exit thresholds of many operating points from one calibration matrix (csrc/thresholds.hip): the solver of
 * ExitController.set_threshold, value_net.py:242-262 ----
 * values [n_stage][ld] f32 (n_sample deltas per row); out_n: DEVICE int32 [n_points][n_exit], the counts floor(n_sample * probs[e]) of
 * every point, computed on the host in the reference's f32 arithmetic (deer_vla_amd.value_net.exit_counts).  For point p every sample
 * starts alive; for e = 0 .. n_exit - 2, with c = out_n[p][e] and a alive samples: thresholds[p][e] = the c-th order statistic of
 * values[e] over the alive samples (ascending for leq, descending otherwise) when 1 <= c <= a, else the sentinel -1e8 (leq) / +1e8; then
 * every alive sample with v <= T (>= T) leaves and exit_counts[p][e] is their number.  The last exit gets +1e8 (-1e8) and the samples
 * still alive.  status[p] = NaNs met in rows 0 .. n_exit - 2 (non-zero: do not trust point p).  One workgroup per point, radix select
 * (four 8-bit passes) per exit; integer counting only, so the result is deterministic.  alive_scratch: n_points * n_sample bytes.
 * n_exit <= 16, n_exit <= n_stage, ld >= n_sample. */
int deer_solve_thresholds(const float* values, int n_stage, int n_sample, int ld, const int* out_n, int n_points, int n_exit, int leq,
                          unsigned char* alive_scratch, float* thresholds, int* exit_counts, int* status, void* stream);
/* On-policy exit values (csrc/value_log.hip): after a SHADOW step (DEER_CTL_SHADOW: every exit evaluated, its delta of
 * ActionValueNet.forward(mode='infer'), value_net.py:120-133, in ctl[b][DEER_CTL_DELTAS + e]) append one column per environment of
 * active_mask (bit b = environment b, ascending b) to values [n_exit][ld] f32: column count + (active environments below b) receives the
 * n_exit deltas of environment b bit for bit, taken[column] its DEER_CTL_EXIT_LAYER - the sample of the "average exit layer" that
 * bayesian_optimization.py:75-79 takes as its budget.  state: device int32[3] = {count, dropped, nonfinite}: columns in use, columns that
 * found no room (columns at or beyond capacity are not written), non-finite deltas written.  One workgroup, no atomics: appends are
 * ordered by their stream.  Does not consult ALL_EXITED.  n_envs 1..DEER_MAX_ENVS, n_exit 1..16, capacity >= 1, ld >= capacity, no bit
 * of active_mask at or above n_envs. */
int deer_value_log_append(const int* ctl, int n_envs, int n_exit, int active_mask, float* values, int ld, int capacity, int* taken,
                          int* state, void* stream);
/* ExitController.set_timestep (eval_utils.py:662-663) + per-step reset. step_info: device int32[4] = {hold, step sequence
 * number, host mirror pointer lo, hi} or NULL (no stage hold, no mirror). */
int deer_ctl_begin_step(int* ctl, const int* step_info, int B, void* stream);

/* ---- camera-frame preprocessing (robot_flamingo/data/data.py:898-902 + open_clip eval transform, factory.py:109-112) ----------
 * uint8 frames [N][H][W][3] -> Resize(S, bicubic, shorter side) -> CenterCrop(S) -> /255 -> Normalize(mean, std) as [N][3][S][S] bf16
 * and/or f32, bit-exact w.r.t. PIL's two-pass fixed-point resampler (the reference runs PIL on the host).  tmp: device scratch of
 * deer_preprocess_scratch_bytes(N, H, W, S) bytes; mean / std_: HOST float[3]. */
int deer_preprocess_frames(const unsigned char* src, int N, int H, int W, int S, const float* mean, const float* std_,
                           unsigned char* tmp, void* out_bf16, float* out_f32, void* stream);
/* deer_preprocess_frames with the 16-bit output in IEEE fp16 (the frame format of a fp16 engine) */
int deer_preprocess_frames_f16(const unsigned char* src, int N, int H, int W, int S, const float* mean, const float* std_,
                           unsigned char* tmp, void* out_bf16, float* out_f32, void* stream);
long deer_preprocess_scratch_bytes(int N, int H, int W, int S);

/* keeps `stream` busy for ~us microseconds (profiling aid: lets the host enqueue ahead of the GPU) */
int deer_spin_us(int us, void* stream);

/* library identification: returns the gfx arch string the kernels were compiled for ("gfx950") */
const char* deer_hip_arch(void);
int deer_hip_abi_version(void);

/* ---- the LLM trunk and the head on IEEE fp16 operands (round 6) ------------------------------------------------------------------------
 * The reference's evaluation arithmetic is fp32 weights under fp16 autocast (robot_flamingo/eval/eval_utils.py:333, README.md:161-167):
 * every nn.Linear of the MPT blocks (mosaic_gpt_3b.py:413-417), of GatedCrossAttentionBlock (helpers.py:188,231,15-22) and of the action
 * head multiplies fp16-ROUNDED weights.  bf16-rounded weights are 2.6e-2 from that on the action at the full 3B size, fp16-rounded ones
 * 9e-4 (tools/amp_difference.py full --parts, profiles/r06_*).  Every trunk entry point above therefore has a twin that reads weights
 * packed as fp16 (deer_model_load_tensor with deer_config.operands_f16) and activation planes fp16 hi / lo on v_mfma_f32_16x16x32_f16 -
 * same arguments, same kernels, same speed (the trunk is HBM-bound; same bytes).  K / V of the gated x-attn arrive as fp16
 * (deer_gemm_f16_nt with DEER_EPI_BF16 = "the family's 16-bit format").  The head entry points take the weight kind in their
 * `w_is_f32` argument: 0 = bf16 rows, 1 = f32 rows, 2 = fp16 rows. */
int deer_gemm_skinny_f16(const void* A, int lda, const float* Aslab, int s_in, long slab_stride_in, int a_mode, const void* Wp,
                     float* part, int M, int N, int K, int splitk, const int* ctl, void* stream);
int deer_gemm_skinny_hl_f16(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk,
                        const int* ctl, void* stream);
int deer_gemm_skinny_hl_rows_f16(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk,
                             int slab_rows, const int* ctl, void* stream);
int deer_gemm_skinny_hl_active_f16(const void* A_hi, const void* A_lo, int lda, const void* Wp, float* part, int M, int N, int K, int splitk, int slab_rows,
                               const int* ctl, const int* cmap, int rows_per_env, void* stream);
int deer_slab_gelu_split_f16(const float* slab, int s_in, long slab_stride, int gelu, void* out_hi, void* out_lo, int rows, int C,
                         const int* ctl, void* stream);
int deer_slab_gelu_split_active_f16(const float* slab, int s_in, long slab_stride, int gelu, void* out_hi, void* out_lo, int rows, int C, const int* ctl,
                                const int* cmap, int rows_per_env, void* stream);
int deer_resadd_ln_split_f16(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias,
                         const float* gamma, const float* beta, void* out_hi, void* out_lo, float* out_f32, float* x_copy, int T,
                         int d, float eps, const int* ctl, void* stream);
int deer_resadd_ln_rows_f16(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* gamma, const float* beta, void* out_bf16,
                        void* out_lo, float* out_f32, float* x_copy, int T_rows, int d, float eps, const int* ctl, const int* cmap, int rows_per_env,
                        const float* x_in, const int* cmap_old, int B, int drop_upto, void* stream);
int deer_resadd_ln_packed_f16(float* x, const float* slab, int s_in, long slab_stride, const float* gate, const float* bias, const float* gamma,
                          const float* beta, void* out_hi, void* out_lo, float* out_f32, float* x_copy, int T, int d, float eps, const int* ctl,
                          void* stream);
int deer_trunk_wide_gemm_f16(const void* a_hi, const void* a_lo, const void* Wp, int N, int K, int epi, float* out_f32, void* out_hi, void* out_lo,
                         int ldo, float* stats, int T, const int* ctl, void* stream);
int deer_trunk_mpt_attn_f16(const float* qkv, const float* stats, int d_model, int n_heads, const float* q_ln_w, const float* k_ln_w, float eps,
                        const unsigned char* key_mask, float alibi_bias_max, void* out_hi, void* out_lo, int ldo, int T, const int* ctl,
                        void* stream);
int deer_xattn_fused_f16(const float* xn, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time,
                     int n_per_media, int n_kv, const void* Wo_p, float* out, long slab_stride, int T, int heads, int batch,
                     float scale, const int* ctl, void* stream);
int deer_xattn_fused_active_f16(const float* xn, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time, int n_per_media, int n_kv,
                            const void* Wo_p, float* out, long slab_stride, int T, int heads, int batch, float scale, const int* ctl, const int* cmap,
                            void* stream);
int deer_xattn_fused_packed_f16(const void* x_hi, const void* x_lo, int d, const void* Wq_p, const void* kv, int ldkv, int inner, const int* text_time,
                            int n_per_media, int n_kv, const void* Wo_p, float* out, long slab_stride, int T, int heads, float scale,
                            const int* ctl, void* stream);
int deer_xattn_mfma_f16(const float* qslab, int s_in, long slab_stride, int ldqs, const void* kv, int ldkv, int inner,
                    const int* text_time, int n_per_media, void* out, int out_is_f32, int ldo, int T, int n_kv, int heads,
                    int batch, float scale, const int* ctl, void* stream);
int deer_mpt_attn_small_hl_f16(const float* qkvslab, int s_in, long slab_stride, int d_model, int n_heads, const float* q_ln_w,
                           const float* k_ln_w, float eps, const unsigned char* key_mask, float alibi_bias_max, float* qkv_ws,
                           void* out_hi, void* out_lo, int ldo, int T, int batch, const int* ctl, void* stream);
int deer_mpt_attn_small_hl_active_f16(const float* qkvslab, int s_in, long slab_stride, int d_model, int n_heads, const float* q_ln_w, const float* k_ln_w,
                                  float eps, const unsigned char* key_mask, float alibi_bias_max, float* qkv_ws, void* out_hi, void* out_lo, int ldo, int T,
                                  int batch, const int* ctl, const int* cmap, void* stream);
int deer_embed_tokens_f16(const long long* ids, const void* wte_bf16, float* x, int* text_time, int T, int batch, int d, int vocab,
                      int media_id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEER_HIP_H */

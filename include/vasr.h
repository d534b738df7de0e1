/*
 * vasr.h — C ABI of libvasr_hip.so, the MI355X (gfx950) kernels behind the
 * VELOCITY-ASR inference path.
 *
 * The reference (shaderko/velocity-asr) has no native layer at all: its hot path is
 * implicit ATen ops under Python modules.  Each entry point below replaces one of
 * those op groups; the reference file:line it stands in for is cited per function.
 * The one native-operator contract the reference itself defines is
 * `selective_scan_fn(u, delta, A, B, C, D, z, ...)` (velocity_asr/ssm.py:20-26,
 * call site ssm.py:326-332); vasr_ssm_scan_f32 is its replacement and also covers
 * the reference's default pure-PyTorch tree scan (ssm.py:173-295).
 *
 * Conventions (all functions):
 *   - All pointers are DEVICE pointers owned by the caller; the library never
 *     allocates or frees on these paths (graph-capturable).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is
 *     enqueued, never synchronised.
 *   - Matrices are row-major float32; `ld*` are row strides in ELEMENTS, `stride_*`
 *     are batch strides in elements.
 *   - Return 0 on success, a negative VASR_E* code for invalid arguments, or a
 *     positive hipError_t if a launch failed.  vasr_last_error() returns a
 *     thread-local description of the last failure.  No C++ exception crosses
 *     this boundary.
 *   - Functions are stateless and re-entrant.
 */
#ifndef VASR_H_
#define VASR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VASR_ABI_VERSION 21

#define VASR_OK 0
#define VASR_EINVAL (-1)
#define VASR_EUNSUPPORTED (-2)

/* ABI version (== VASR_ABI_VERSION) and last-error text. */
int vasr_version(void);
const char* vasr_last_error(void);

/* Tuning options of the launchers (process-wide; not numerics: every setting computes the same
 * results).  Defaults are read once from the environment variable named per key; 0 = automatic.
 * vasr_set_option returns the previous value (value < 0 only queries), VASR_EINVAL otherwise. */
enum vasr_option {
    VASR_OPT_SCAN_LANES = 0, /* state indices per lane of vasr_ssm_scan_f32: 0, 2, 4 (VASR_SCAN_NPL)       */
    VASR_OPT_SCAN_CHUNK = 1, /* time steps per staged chunk of the streaming scan: 0, 16, 32 (VASR_SCAN_T) */
    VASR_OPT_TAIL_ROWS = 2,  /* token rows per fused-SSMBlock-tail workgroup: 0, 16, 32 (VASR_TAIL_ROWS)   */
    VASR_OPT_GEMM_ENGINE = 3, /* split-bf16 GEMM main loop: 0 auto, 1 LDS-ring tiles, 2 A-rows-stationary
                                 (K = 128 / 192, batch 1, unpaired epilogues) (VASR_GEMM_ENGINE)         */
    VASR_OPT_TAIL_WAVES = 4,  /* waves per fused-SSMBlock-tail workgroup: 0, 4, 6, 12 (VASR_TAIL_WAVES)    */
    VASR_OPT_SCAN_SPLIT = 5,  /* form of vasr_ssm_scan_chunked_f32: 0 auto, 1 three launches, 2 one launch
                                 (time split inside the workgroup) (VASR_SCAN_SPLIT)                     */
    VASR_OPT_DW_ROWS = 6      /* output rows per vasr_ln_dwconv_f32 workgroup: 0 auto, 4, 8, 16 (VASR_DW_ROWS) */
};
int vasr_set_option(int key, int value);

/* Diagnostics (no reference counterpart; bench.py's machine-state record).  A `blocks`-workgroup
 * launch of 256 threads, each running a dependent VALU chain of `iters` steps; per workgroup b:
 * out[3b] = the XCD (XCC_ID hardware register) it ran on, out[3b + 1] / out[3b + 2] = the shader
 * clock (s_memtime) / 100-MHz constant (s_memrealtime) ticks its wave 0 spent in the chain.  The
 * clock is out[3b+1] / out[3b+2] * 100 MHz; out[3b] == b % 8 checks the round-robin XCD dispatch
 * the kernels' XCD-aware block maps assume.  out: device, 3 * blocks int64. */
int vasr_probe_clock(int64_t* out, int blocks, int iters, void* stream);

/* ------------------------------------------------------------------ GEMM
 * C[b] = epilogue(A[b] (M x K) * W^T (K x N) + bias), W row-major [N][K] as in
 * nn.Linear, fp32 in / fp32 out (vasr_linear_x3_f32), or bf16 weights (vasr_linear_bf16).
 * Replaces every nn.Linear / Conv1d-as-GEMM on the path: in_proj, x_proj+dt_proj
 * (ssm.py:72-79, :105-113), out_proj (:90, :130), FFN (:394-400), temporal conv
 * (model.py:156-162), pool_proj (attention.py:35, :76), q/k/v/out (:107-110),
 * gated fusion (:183-218), CTC head (model.py:218-227), and the STFT as a
 * windowed-DFT GEMM (audio.py:104-115).
 */
enum vasr_epilogue {
    VASR_EPI_NONE = 0,          /* C = acc + bias                                      */
    VASR_EPI_GELU = 1,          /* C = gelu_erf(acc + bias)                            */
    VASR_EPI_SOFTPLUS_FROM = 2, /* C = acc + bias; softplus on columns >= n_out        */
    VASR_EPI_RESIDUAL = 3,      /* C = (acc + bias) + aux[b][row][col]                 */
    VASR_EPI_GELU_PE = 4,       /* C = gelu_erf(acc + bias) + aux[row][col] (pos. enc.) */
    VASR_EPI_PAIR_POWER = 5,    /* W rows paired in 32s (re|im): C[row][k] = re^2+im^2 */
    VASR_EPI_PAIR_FUSION = 6,   /* W rows paired (gate|global): gated fusion, see doc  */
    VASR_EPI_ARGMAX = 7,        /* row argmax of acc + bias (after qparams), no logits write:
                                   C is (rows, ldc) uint64 partial keys, one per 32 columns
                                   (ldc >= ceil(N/32)), every slot written; decode with
                                   vasr_argmax_keys (ties -> first index, decode.py:46) */
    VASR_EPI_ARGMAX_LSE = 11,   /* ARGMAX and LSE in one pass over the accumulators, for a greedy
                                   decode with confidences and no logits write (fp32 GEMM only, no
                                   qparams; it runs where ARGMAX runs at that shape).  C is
                                   (rows, ldc) 8-byte slots, ldc >= 2 * ceil(N/32), 8-byte aligned:
                                   for group g of 32 columns slot 2g is the ARGMAX key and slot
                                   2g + 1 the LSE pair, or the neutral key 0 and pair {-inf, 0};
                                   the 2 * ceil(N/32) slots of every row are all written with
                                   plain stores, slots past them are not touched.  Columns >= N are
                                   skipped for the key and count as -inf for the pair; a -inf bias
                                   entry is allowed.  On the tile kernels each key is bitwise
                                   ARGMAX's and each pair bitwise LSE's.  Consume with
                                   vasr_ctc_collapse_keys_conf */
    VASR_EPI_LSE = 9            /* (8 and 10 are unassigned and refused.)
                                   row log-sum-exp of acc + bias, no logits write (fp32 GEMM
                                   only, no qparams; it runs on the engine the plain epilogue
                                   gets at that shape, vasr_gemm_tile): C is (rows, ldc) 8-byte slots
                                   as ARGMAX, each a float pair {m, s}: m the maximum of a group
                                   of the row's columns, s the sum of exp(v - m) over them, or
                                   the neutral {-inf, 0}; every slot written with plain stores;
                                   columns >= N count as -inf, a -inf bias entry is allowed.
                                   Fold a row's pairs with vasr_lse_combine_f32 */
};

typedef struct vasr_gemm_args {
    const float* A;
    int64_t lda, stride_a;
    const float* W;
    int64_t ldw;
    const float* bias;      /* [N] or NULL */
    float* C;
    int64_t ldc, stride_c;
    int32_t batch, M, N, K; /* M rows per batch */
    int32_t epilogue;       /* enum vasr_epilogue */
    const float* aux;       /* residual / positional table / paired partial product */
    int64_t ld_aux, stride_aux;
    const float* aux2;      /* PAIR_FUSION: local_proj bias [n_out] */
    int32_t n_out;          /* PAIR_*: output columns; SOFTPLUS_FROM: first softplus column */
    const float* qparams;   /* NULL, or per-column activation fake-quant {scale, zero_point,
                               qmin, qmax} (4 floats per column) applied to acc + bias before
                               the epilogue's function (QuantizedLinear / QuantizedConv1d
                               activation_quantizer, quantize.py:177-191, :252-266).
                               PAIR_FUSION: N entries in the paired column layout (gate |
                               global_proj) followed by n_out entries for local_proj.
                               A column whose scale is 0 is not quantized.  Not allowed
                               with PAIR_POWER. */
} vasr_gemm_args;

/* The fp32 GEMM (fp32 results to within accumulation order) on the bf16 matrix cores: fp32
 * operands are split exactly into three bf16 terms (x = hi + mid + lo, all 24 significant
 * bits) and the six products larger than 2^-25 |a||b| are accumulated in fp32 on
 * v_mfma_f32_32x32x16_bf16 — 2.67x the f32-input MFMA rate.  `w_split` holds W pre-split by
 * vasr_split_weights_bf16x3 (args->W is not read).
 */
int vasr_linear_x3_f32(const vasr_gemm_args* args, const uint16_t* w_split, void* stream);

/* Split W (N x K fp32, row stride ldw) into bf16 terms (hi, mid, lo) in the fragment-native
 * layout out[NT][KS][3][64][8] (NT = ceil(N/32), KS = Kp/16, Kp = K rounded up to 32):
 * element (n, k) of plane p is out[n/32][k/16][p][32*((k%16)/8) + n%32][k%8]; padding is
 * zero.  vasr_split_weights_elems(N, K) = 3 * 32*NT * Kp. */
int vasr_split_weights_bf16x3(const float* W, int64_t ldw, int N, int K, uint16_t* out, void* stream);
int64_t vasr_split_weights_elems(int N, int K);

/* The GEMM of a bf16 model (BASELINE config C3, `model.to(torch.bfloat16)`): W is bf16,
 * packed once by vasr_pack_weights_bf16 into the same fragment-native layout with one plane
 * (out[NT][KS][64][8], vasr_pack_weights_bf16_elems(N, K) = 32*NT * Kp elements); A stays
 * fp32 in HBM and is rounded to bf16 (round-to-nearest-even) as it enters the MFMA
 * (v_mfma_f32_32x32x16_bf16), accumulation and epilogues in fp32 — the reference's bf16
 * Linear (ssm.py, attention.py, model.py nn.Linear under bf16 parameters) with fp32
 * accumulation.  Same args and epilogues as vasr_linear_x3_f32. */
int vasr_linear_bf16(const vasr_gemm_args* args, const uint16_t* w_packed, void* stream);
int vasr_pack_weights_bf16(const uint16_t* W, int64_t ldw, int N, int K, uint16_t* out, void* stream);
int64_t vasr_pack_weights_bf16_elems(int N, int K);

/* Which kernel the matching vasr_linear_x3_f32 (bf16 = 0) or vasr_linear_bf16 (bf16 = 1) call
 * would launch under the current options, for a dense C (ABI 21).  Host only, launches nothing;
 * the launchers take their decision from the same rule.  Returns 128128, 128064 or 64064 for the
 * 128 x 128, 128 x 64 and 64 x 64 tile kernels, 1 for the A-rows-stationary engine
 * (VASR_OPT_GEMM_ENGINE), VASR_EINVAL for M, N, K or batch < 1 (a call with M = 0 launches
 * nothing), K % 4 != 0, an unknown epilogue, a paired epilogue with N % 64 != 0, bf16 not 0 / 1. */
int vasr_gemm_tile(int M, int N, int K, int batch, int epilogue, int bf16);

/* ------------------------------------------------------------------ norms / conv
 * nn.LayerNorm over the last dim (C <= 1024), biased variance.  y may alias x.
 * Replaces every LayerNorm on the path (26 per forward).
 */
int vasr_layer_norm_f32(const float* x, int64_t ldx, const float* w, const float* b,
                        float* y, int64_t ldy, int rows, int C, float eps, void* stream);

/* Two LayerNorms in a row, one launch: y1 = LN(x; w1, b1, eps1), y2 = LN(y1; w2, b2, eps2), each
 * bitwise what vasr_layer_norm_f32 gives (y2 from y1's registers, not re-read).  Replaces the
 * local stack's final norm (LocalSSMProcessor.norm, reference ssm.py:504) followed by the
 * global context's query norm (HierarchicalGlobalContext.norm2, attention.py:307), which the
 * reference runs as two nn.LayerNorm calls.  y1 != y2; C <= 1024. */
int vasr_layer_norm_pair_f32(const float* x, int64_t ldx, const float* w1, const float* b1, float eps1,
                             float* y1, int64_t ldy1, const float* w2, const float* b2, float eps2,
                             float* y2, int64_t ldy2, int rows, int C, void* stream);

/* out[b][l][c] = x[b][l][c] + table[l][c] for x (B, L, C) contiguous (standalone
 * PositionalEncoding2D.forward, model.py:106-127; the model fuses it into the conv GEMM). */
int vasr_add_table_f32(const float* x, const float* table, float* out, int B, int L, int C,
                       void* stream);

/* SSMBlock pre-norm + causal depthwise conv (ssm.py:409-414, :377-383):
 * y[b,t,c] = bias[c] + sum_j conv_w[c][j] * LN(x)[b, t-(Kc-1)+j, c]  (zero for t<0).
 * x, y: (B, L, C) contiguous; conv_w: (C, Kc) contiguous; Kc <= 8.
 */
int vasr_ln_dwconv_f32(const float* x, const float* ln_w, const float* ln_b,
                       const float* conv_w, const float* conv_b, float* y,
                       int B, int L, int C, int Kc, float eps, void* stream);

/* vasr_ln_dwconv_f32 on LN0(x) without the LN0 launch: xo = LN0(x; pre_w, pre_b, pre_eps) (the
 * temporal binding's LayerNorm, reference model.py:200, applied to its conv + GELU + PE rows) is
 * formed in registers, stored once (the first SSM block's residual input) and fed to norm1 + the
 * causal conv: xo and y bitwise vasr_layer_norm_f32 followed by vasr_ln_dwconv_f32.  C = 192,
 * Kc = 4 (the model's); x, xo, y distinct. */
int vasr_ln_dwconv_prenorm_f32(const float* x, const float* pre_w, const float* pre_b, float pre_eps, float* xo,
                               const float* ln_w, const float* ln_b, const float* conv_w, const float* conv_b,
                               float* y, int B, int L, int C, int Kc, float eps, void* stream);

/* ------------------------------------------------------------------ selective scan
 * SelectiveSSM scan + D skip + SiLU gate (ssm.py:119-129):
 *   dA = exp(dt*A), dBx = x*(dt*B)
 *   mode 0 (scan_mode="parallel", the reference default): the reference's exclusive,
 *          mis-combined Blelloch tree prefix h (ssm.py:216-295), streamed in its exact
 *          float-operation order with an O(log L) block stack per state lane;
 *   mode 1 (scan_mode="sequential"): the true recurrence h_t = dA_t h_{t-1} + dBx_t
 *          (ssm.py:134-171);
 *   mode 2: the tree of mode 0 with each a*b + c as one fused multiply-add and
 *          dBx = (x*dt)*B (one rounding fewer per op; the model's default for
 *          scan_mode="parallel", VASR_SCAN_FMA=0 selects mode 0);
 *   out[b,t,d] = (sum_n h[b,t,d,n] C[b,t,n] + x[b,t,d] D[d]) * silu(z[b,t,d]).
 * x = xz[:, :, 0:Di], z = xz[:, :, Di:2Di]; B = bc[:, :, 0:N], C = bc[:, :, N:2N].
 * A2 = A * log2(e) (A = -exp(A_log), shared across Di).  N in {16, 32, 64, 128}: any other
 * state dim N' < 128 runs as the next size up with B and C zero-padded (columns N'..N-1 of each
 * half of bc) and A2 padded with 0 -- the padded states then stay exactly 0 and add nothing to
 * y, so the outputs are those of N' states (velocity_asr.ssm pads the projection weights with
 * zero rows, so the GEMM writes that layout).  Di a multiple of 4 * 64 * NPL / N channels per
 * workgroup (16 at N = 64, 8 at N = 128; host checks); L <= 8192.
 */
int vasr_ssm_scan_f32(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt,
                      const float* bc, int64_t ld_bc, const float* A2, const float* D,
                      float* out, int64_t ld_out, int B, int L, int Di, int N, int mode,
                      void* stream);

/* The ungated form of the tree modes (0, 2) for the z-in-tail SSMBlock (ABI 15):
 *   out[b,t,d] = sum_n h[b,t,d,n] C[b,t,n] + x[b,t,d] D[d]
 * with x = x[:, :, 0:Di] (row stride ld_x >= Di; no z is read) and the other operands as
 * vasr_ssm_scan_f32; the same kernels and lane layout, so out * silu(z) (gate.h) is bitwise
 * vasr_ssm_scan_f32's output.  vasr_ssm_block_tail_gated_f32 applies the gate. */
int vasr_ssm_scan_ungated_f32(const float* x, int64_t ld_x, const float* dt, int64_t ld_dt,
                              const float* bc, int64_t ld_bc, const float* A2, const float* D,
                              float* out, int64_t ld_out, int B, int L, int Di, int N, int mode,
                              void* stream);

/* Chunk-parallel form of modes 0 and 2 for small launches (one utterance at a time, as
 * scripts/transcribe.py:69-78 and evaluate.py:91-98 run the model): time is cut at the
 * streaming kernel's 16-step chunks; pass 1 forms each chunk's up-sweep composite, pass 2
 * the composites of aligned blocks of 2^k chunks (the entries of the streaming kernel's
 * chunk-level stack), pass 3 folds each chunk's prefix from them and runs the chunk's tree
 * with the y reduction and gate.  Launches whose workgroups fit the CUs once (N <= 64, B * Di * N
 * / 128 <= 256; VASR_OPT_SCAN_SPLIT) run the same passes in ONE launch instead: a workgroup
 * owns one wave's channels and its waves split time into ranges of aligned 8-step chunk blocks
 * (2 state indices per lane; the workspace is then unused).  Same float operations as
 * vasr_ssm_scan_f32 with the same lane layout: bitwise equal outputs.
 * workspace: >= vasr_ssm_scan_workspace_floats(B, L, Di, N) floats, 16-byte aligned. */
int vasr_ssm_scan_chunked_f32(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt,
                              const float* bc, int64_t ld_bc, const float* A2, const float* D,
                              float* out, int64_t ld_out, int B, int L, int Di, int N, int mode,
                              float* workspace, int64_t workspace_floats, void* stream);
int64_t vasr_ssm_scan_workspace_floats(int B, int L, int Di, int N);
/* 1 when vasr_ssm_scan_chunked_f32 runs this shape as the one-launch time-split form under the
 * current options (VASR_OPT_SCAN_SPLIT / VASR_OPT_SCAN_LANES), else 0: the launcher's own rule,
 * for hosts that choose between the streaming and chunked entry points (ABI 15). */
int vasr_ssm_scan_split_selected(int B, int L, int Di, int N);

/* ------------------------------------------------------------------ selective scan, backward (added to ABI 20)
 * Training through the true recurrence (mode 1; reference ssm.py:134-171 under autograd, the
 * operator mamba_ssm.selective_scan_fn differentiates, ssm.py:297-337).  With g = d loss / d out,
 * s = sigmoid(z), gy = g silu(z) (gy = g without z), a_t = exp(dt_t A), and walking t down from
 * L - 1 with gh_L = 0:
 *   dz_t  = g_t y_t s (1 + z (1 - s)),          gh_t[d][n] = gy_t[d] C_t[n] + a_{t+1} gh_{t+1},
 *   dC_t[n] = sum_d gy_t h_t,                   dB_t[n] = sum_d gh_t dt_t x_t,
 *   dx_t  = gy_t D + dt_t sum_n gh_t B_t,       ddt_t = x_t sum_n gh_t B_t + sum_n gh_t a_t h_{t-1} A[n],
 *   dA[n] = sum_{b,t,d} gh_t a_t h_{t-1} dt_t,  dD[d] = sum_{b,t} gy_t x_t.
 * Limits are vasr_ssm_scan_f32's: fp32, N in {16, 32, 64, 128} (pad as there), L <= 8192, whole
 * batches; Di a multiple of 1024 / N.  The scan is causal, so zero rows of g on padded frames give
 * the exact gradients of a ragged batch.
 *
 * vasr_ssm_scan_save_f32: the forward.  Operands as vasr_ssm_scan_f32 at mode 1; gated = 0 reads
 * no z (xz holds x alone, ld_xz >= Di) and writes out = y + x D.  out is bitwise
 * vasr_ssm_scan_f32(mode 1)'s (gated = 0: that kernel's value before the gate).  ckpt receives the
 * state h every 16-step chunk starts from, (B, ceil(L / 16), Di, N) floats =
 * vasr_ssm_scan_checkpoint_floats(B, L, Di, N), 16-byte aligned.
 *
 * vasr_ssm_scan_bwd_f32: the reverse-time walk from those checkpoints.  x, z, dt, g: (B L, Di) row
 * views with row strides ld_*; z and dz are both NULL for the ungated form; A = -exp(A_log) and
 * A2 = A log2(e), N floats each.  Outputs, all contiguous and every element written: dx, ddt, dz
 * (B L, Di); dB, dC (B L, N); dA_part (B, Di, N) and dD_part (B, Di), whose sums over (b, d) and
 * over b are dA and dD.  workspace: vasr_ssm_scan_bwd_workspace_floats(B, L, Di, N) floats (the
 * per-workgroup dB / dC partial sums, 2 (B L) (Di N / 1024) N).  No floating-point atomics: every
 * sum runs in a fixed order, so the gradients are run-to-run bitwise, and an utterance's rows do
 * not depend on the rest of the batch. */
int vasr_ssm_scan_save_f32(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt,
                           const float* bc, int64_t ld_bc, const float* A2, const float* D,
                           float* out, int64_t ld_out, int B, int L, int Di, int N, int gated,
                           float* ckpt, int64_t ckpt_floats, void* stream);
int64_t vasr_ssm_scan_checkpoint_floats(int B, int L, int Di, int N);
int vasr_ssm_scan_bwd_f32(const float* x, int64_t ld_x, const float* z, int64_t ld_z,
                          const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
                          const float* A, const float* A2, const float* D,
                          const float* g, int64_t ld_g, const float* ckpt,
                          float* dx, float* ddt, float* dz, float* dB, float* dC,
                          float* dA_part, float* dD_part, float* workspace, int64_t workspace_floats,
                          int B, int L, int Di, int N, void* stream);
int64_t vasr_ssm_scan_bwd_workspace_floats(int B, int L, int Di, int N);

/* ------------------------------------------------------------------ tree scan, backward (added to ABI 20)
 * Training through the default scan (modes 0 / 2: the reference's _parallel_scan under autograd,
 * ssm.py:173-295), a different function of its inputs from the recurrence.  Per (utterance,
 * channel, state n): a_t = exp(dt_t A[n]), b_t = x_t dt_t B_t[n], P_e = prod_{r <= e} a_r, and for
 * an aligned block S of 2^k steps ending at e_S, R_S = its local inclusive scan.  The state is
 *   h_t = sum over the set bits k of t of P_{e_S} R_S,  S = [t with bits 0..k cleared, + 2^k),
 * and with gh_t = gy_t C_t[n], w_S = P_{e_S} sum_{t in the right sibling of S} gh_t and
 * lambda_S(s) = w_S prod_{s < r <= e_S} a_r the gradients are
 *   d/db_s = sum_{S containing s} lambda_S(s),
 *   d/d(dt_r A[n]) = sum_{S : e_S >= r} w_S R_S + sum_{S containing r} lambda_S(r - 1) rho^S_{r-1}
 * (rho^S_r: the local scan of S up to r; nothing divides by a_r), from which dx, ddt, dz, dB, dC,
 * dA, dD follow as for the recurrence.  The forward is vasr_ssm_scan_f32 / vasr_ssm_scan_ungated_f32
 * itself (only the inputs are kept); modes 0 and 2 round differently and share this gradient.
 *
 * vasr_ssm_tree_bwd_f32: operands, outputs, limits and guarantees as vasr_ssm_scan_bwd_f32, without
 * checkpoints: x, z, dt, g (B L, Di) row views, z and dz both NULL for the ungated form, bc
 * (B L, 2N) [B | C], A and A2 = A log2(e); dx, ddt, dz (B L, Di), dB, dC (B L, N), dA_part
 * (B, Di, N), dD_part (B, Di), every element written; N in {16, 32, 64, 128}, Di a multiple of
 * 1024 / N, L <= 8192.  workspace: vasr_ssm_tree_bwd_workspace_floats(B, L, Di, N) floats, 16-byte
 * aligned: B ceil(L / 16) Di (7 N + 1), seven floats per 16-step chunk, channel and state plus the
 * chunk's dD partial -- no (B, L, Di, N) array is formed.  No atomics: run-to-run bitwise, and an
 * utterance's rows do not depend on the rest of the batch. */
int vasr_ssm_tree_bwd_f32(const float* x, int64_t ld_x, const float* z, int64_t ld_z,
                          const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
                          const float* A, const float* A2, const float* D,
                          const float* g, int64_t ld_g,
                          float* dx, float* ddt, float* dz, float* dB, float* dC,
                          float* dA_part, float* dD_part, float* workspace, int64_t workspace_floats,
                          int B, int L, int Di, int N, void* stream);
int64_t vasr_ssm_tree_bwd_workspace_floats(int B, int L, int Di, int N);

/* ------------------------------------------------------------------ SSMBlock tail, fused
 * The tail of SSMBlock._forward_impl (ssm.py:415-425) in one launch for d_model D = 192 and
 * FFN width / d_inner E = 384:
 *   x1 = g @ Wo^T + x;  h = LayerNorm(x1; ln_w, ln_b, ln_eps);  f = gelu(h @ W1^T + b1);
 *   out = f @ W2^T + b2 + x1
 * with g (M, E) the gated scan output (row stride ldg), x (M, D) the block input, Wo = out_proj
 * (D x E, ssm.py:90), W1 = ffn.0 (E x D), W2 = ffn.3 (D x E) (ssm.py:394-400), each given as
 * vasr_split_weights16_bf16x3 planes.  x1 and f never leave the chip.  fp32-accurate (split
 * bf16 products, as vasr_linear_x3_f32). */
int vasr_ssm_block_tail_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, const uint16_t* wo16,
                            const float* ln_w, const float* ln_b, float ln_eps, const uint16_t* w1_16,
                            const float* b1, const uint16_t* w2_16, const float* b2, float* out, int64_t ldo,
                            int M, int D, int E, void* stream);
/* The tail of the z-in-tail block (ABI 15): z = u @ W_z^T (W_z = in_proj rows Di..2Di-1 as
 * vasr_split_weights_bf16x3 planes; u (M, D) the in_proj input, row stride ldu) with the split
 * GEMM's exact product, g = yd * silu(z) with the gate of scan mode `mode` (0 or 2; yd = the
 * vasr_ssm_scan_ungated_f32 output, row stride ldy), then the tail above on g.  Bitwise the
 * output of vasr_ssm_scan_f32 + vasr_ssm_block_tail_f32 on the full projection; the projection
 * GEMM no longer writes z (E floats per token).  32-row workgroups of 12 waves. */
int vasr_ssm_block_tail_gated_f32(const float* yd, int64_t ldy, const float* u, int64_t ldu, const uint16_t* wz,
                                  int mode, const float* x, int64_t ldx, const uint16_t* wo16,
                                  const float* ln_w, const float* ln_b, float ln_eps, const uint16_t* w1_16,
                                  const float* b1, const uint16_t* w2_16, const float* b2, float* out, int64_t ldo,
                                  int M, int D, int E, void* stream);
/* The same tail for the bf16 model (C3): weights as one bf16 plane (vasr_pack_weights16_bf16 of
 * the bf16 parameters), activations rounded to bf16 at the MFMA input, fp32 accumulation and
 * fp32 LayerNorm / bias / GELU / residual -- the arithmetic of vasr_linear_bf16. */
int vasr_ssm_block_tail_bf16(const float* g, int64_t ldg, const float* x, int64_t ldx, const uint16_t* wo16,
                             const float* ln_w, const float* ln_b, float ln_eps, const uint16_t* w1_16,
                             const float* b1, const uint16_t* w2_16, const float* b2, float* out, int64_t ldo,
                             int M, int D, int E, void* stream);
/* The z-in-tail tail for the bf16 model (ABI 16): z = u @ W_z^T with W_z as one
 * vasr_pack_weights_bf16 plane (the bf16 in_proj rows Di..2Di-1) and u rounded to bf16 at the MFMA
 * input -- vasr_linear_bf16's exact product --, g = yd * silu(z) rounded to bf16 as the tail
 * above stages it, then that tail (Wo, W1, W2 as vasr_pack_weights16_bf16 planes).  Bitwise the
 * output of vasr_ssm_scan_f32 + vasr_ssm_block_tail_bf16 on vasr_linear_bf16's [x | z]. */
int vasr_ssm_block_tail_gated_bf16(const float* yd, int64_t ldy, const float* u, int64_t ldu, const uint16_t* wz,
                                   int mode, const float* x, int64_t ldx, const uint16_t* wo16,
                                   const float* ln_w, const float* ln_b, float ln_eps, const uint16_t* w1_16,
                                   const float* b1, const uint16_t* w2_16, const float* b2, float* out, int64_t ldo,
                                   int M, int D, int E, void* stream);
int vasr_pack_weights16_bf16(const uint16_t* W, int64_t ldw, int N, int K, uint16_t* out, void* stream);
int64_t vasr_pack_weights16_bf16_elems(int N, int K);
/* Split-bf16 planes of a (N, K) fp32 weight in the fragment layout of v_mfma_f32_16x16x32_bf16
 * ([ceil(N/16)][ceil(K/32)][3][64][8] bf16), vasr_split_weights16_elems(N, K) uint16 elements. */
int vasr_split_weights16_bf16x3(const float* W, int64_t ldw, int N, int K, uint16_t* out, void* stream);
int64_t vasr_split_weights16_elems(int N, int K);

/* ------------------------------------------------------------------ gated fusion + head LayerNorm, fused
 * (added to ABI 21: a new symbol, nothing existing changed)
 * GatedFusion.forward_attention (attention.py) and the CTC head's LayerNorm (model.py) in one launch
 * for d_model D = 192 and attention dim A = 48:
 *   t = local @ w_local^T;  g = o @ w_glob^T                  (both (M, 2D), columns in 32-wide pairs
 *                                                              [gate | branch] as VASR_EPI_PAIR_FUSION)
 *   gate = sigmoid((t_gate + g_gate) + b_glob_gate)
 *   fused = gate * (t_branch + b_local) + (1 - gate) * (g_branch + b_glob_branch)
 *   out = fused @ w_out^T + b_out;  y = LayerNorm(out; ln_w, ln_b, ln_eps)
 * local (M, D) and o (M, A) are row views (strides ldl, ldo, multiples of 4, 16-byte aligned);
 * w_local (2D x D), w_glob (2D x A) and w_out (D x D) are vasr_split_weights_bf16x3 planes, b_glob
 * (2D) the paired bias, b_local (D).  y (M, D) is always written; out (M, D) only when non-NULL.
 * t, g and fused never leave the chip.  y and out are bitwise what vasr_linear_x3_f32 (EPI_NONE,
 * then EPI_PAIR_FUSION with aux = t, then EPI_NONE with bias) and vasr_layer_norm_f32 give.
 * rows: token rows per workgroup, 32 (6 waves) or 64 (12 waves); 0 chooses by M. */
int vasr_fusion_tail_f32(const float* local, int64_t ldl, const float* o, int64_t ldo, const uint16_t* w_local,
                         const uint16_t* w_glob, const float* b_glob, const float* b_local, const uint16_t* w_out,
                         const float* b_out, const float* ln_w, const float* ln_b, float ln_eps, float* y,
                         int64_t ldy, float* out, int64_t ldout, int M, int D, int A, int rows, void* stream);

/* ------------------------------------------------------------------ audio I/O (host)
 * load_audio (audio.py:22-62) without torchaudio.  Host functions on host memory (the only
 * entry points here that are not device work): they produce the waveform the front end reads.
 * vasr_flac_decode: a FLAC stream (torchaudio.load's FLAC path, audio.py:47) -> channel-major
 *   (channels, samples) float32 scaled by 2^(bits-1); out = NULL queries the sizes.  Frame
 *   CRCs are checked; errors return VASR_EINVAL with vasr_last_error().
 * vasr_resample_f32: torchaudio.transforms.Resample(orig, new) defaults (sinc_interp_hann,
 *   lowpass_filter_width 6, rolloff 0.99; audio.py:54-56), vasr_resample_length() outputs. */
int vasr_flac_decode(const uint8_t* data, int64_t n, float* out, int64_t out_cap, int* channels,
                     int* sample_rate, int* bits, int64_t* samples);
int64_t vasr_resample_length(int64_t n, int orig_sr, int new_sr);
int vasr_resample_f32(const float* x, int channels, int64_t n, int64_t ld_x, int orig_sr, int new_sr,
                      float* y, int64_t ld_y);
/* The resampler's kernel, exported for the device path (host functions).
 * vasr_resample_plan: the geometry after reducing the rates by their gcd: a frame of `orig`
 *   inputs gives `nw` outputs, each through klen = 2 * width + orig taps.  VASR_EINVAL for rates
 *   <= 0 and for tables over 2^24 taps (44101 -> 16000), as vasr_resample_f32.
 * vasr_resample_taps_f32: the row-major (nw, klen) float32 table (built in float64, rounded once)
 *   that vasr_resample_f32 applies; cap >= nw * klen floats. */
int vasr_resample_plan(int orig_sr, int new_sr, int* orig, int* nw, int* width, int* klen);
int vasr_resample_taps_f32(int orig_sr, int new_sr, float* taps, int64_t cap);

/* ------------------------------------------------------------------ resampling (device)
 * vasr_resample_mix_f32: channel downmix + sample-rate conversion of a zero-padded batch in one
 * launch, bit-identical to a fp32 downmix followed by vasr_resample_f32.  Clip b, channel c,
 * sample i is x[b*ld_clip + c*ld_chan + i] (1 <= C <= 8); samples (device, optional): clip b has
 * samples[b] in [1, S_in] samples, all S_in when NULL.  taps (device): the vasr_resample_taps_f32
 * table of the pair whose vasr_resample_plan gave (orig, nw, width).
 *   m[i]    = (x_0[i] + ... + x_{C-1}[i]) / C in float32, ascending channels, 0 outside the clip
 *   y[b][o] = (float) sum_{k ascending} (double)taps[o % nw][k] * (double)m[(o / nw)*orig - width + k]
 *             for o < vasr_resample_length(samples[b]): one float64 chain per output, the host
 *             resampler's order, so the float32 results are its results bit for bit;
 *   y[b][o] = 0 up to S_out (>= the output count of S_in samples; ld_y >= S_out); nothing is
 *             written at or past S_out, so mel_on_device(lengths=) reads y as its padded batch.
 * orig == nw (equal rates) is a downmix-and-copy and reads no taps.  No allocation, no
 * synchronisation, no host read: the launch can be captured in a graph.  Argument errors return
 * VASR_EINVAL before any device call, as does a geometry whose input span does not fit in LDS
 * (callers then resample on the host).
 * vasr_resample_tile_outputs: consecutive outputs one workgroup produces for (orig, nw); 0 when
 * the geometry is refused. */
int vasr_resample_mix_f32(const float* x, int64_t ld_clip, int64_t ld_chan, int B, int C, int S_in,
                          const int32_t* samples, const float* taps, int orig, int nw, int width,
                          float* y, int64_t ld_y, int S_out, void* stream);
int vasr_resample_tile_outputs(int orig, int nw);

/* ------------------------------------------------------------------ long-form segmentation (device)
 * A recording longer than the model accepts is cut at its quietest points.  A block is 320 samples
 * (vasr_segment_block(): one token row, two mel hops); recording b is x[b*ld_x + i], i < samples[b]
 * (device, optional; all S when NULL; values are clamped to [0, S]).
 * vasr_block_energy_f64: E[b][k] = sum_{i ascending} (double)x[320k+i]^2 for the full blocks
 *   k < samples[b] / 320, one float64 chain from 0 per block (a float32 product is exact in float64, so
 *   the chain is the only rounding); 0 for the other k < S / 320.  Nothing at or past samples[b] is
 *   read.  A workgroup owns vasr_segment_tile_blocks() consecutive blocks of one recording.
 * vasr_segment_plan: the greedy rule on E, one workgroup per recording.  mB = ceil(min_samples / 320),
 *   MB = max_samples / 320, nB = samples[b] / 320; p = 0; while samples[b] - 320 p > max_samples: among
 *   the candidates c in [p + mB, min(p + MB, nB - mB)] take the smallest (score, c), score(c) =
 *   E[c - W/2] + ... + E[c + W/2 - 1] summed ascending into one float64 from 0 (NaN counts as +inf);
 *   cuts[b][n_cuts[b]++] = 320 c; p = c.  W = window_blocks is even and >= 2, mB >= W/2, MB >= 2 mB.
 *   cuts is (B, max_cuts) int64 with row stride ld_cuts; max_cuts >= max(1, vasr_segment_max_cuts(S,
 *   min_samples)) or the call is refused, and the kernel's loop stops at max_cuts.
 * vasr_segment_max_cuts: the most cuts the rule can make in n samples, (n / 320) / mB; -1 for bad
 *   arguments.
 * vasr_segment_gather_f32: table (device) is (n_seg, 3) int64 rows (recording, start, length);
 *   y[g][o] = x[recording][start + o] for o < length, 0 for length <= o < S_seg: the zero-padded batch
 *   the front end reads, in one launch.  A row that does not lie inside its recording or has
 *   length > S_seg is written as zeros.
 * All sample offsets are 64-bit.  No allocation, no synchronisation, no host read; everything is
 * enqueued on `stream`.  Argument errors return VASR_EINVAL before any device call. */
int vasr_segment_block(void);
int vasr_segment_tile_blocks(void);
int64_t vasr_segment_max_cuts(int64_t n, int64_t min_samples);
int vasr_block_energy_f64(const float* x, int64_t ld_x, int B, int S, const int32_t* samples, double* E,
                          int64_t ld_e, void* stream);
int vasr_segment_plan(const double* E, int64_t ld_e, int B, int S, const int32_t* samples, int64_t max_samples,
                      int64_t min_samples, int window_blocks, int64_t* cuts, int64_t ld_cuts, int max_cuts,
                      int32_t* n_cuts, void* stream);
int vasr_segment_gather_f32(const float* x, int64_t ld_x, int B, int S, const int64_t* table, int n_seg,
                            float* y, int64_t ld_y, int S_seg, void* stream);

/* ------------------------------------------------------------------ WER / CER scoring (device)
 * Substitution, deletion and insertion counts of P independent pairs of int32 id sequences, the rule
 * velocity_asr.training.edit_counts_host states: c[0][0] = (0,0,0), c[i][0] = i insertions,
 * c[0][j] = j deletions; for i, j >= 1, c[i][j] = c[i-1][j-1] when hyp[i-1] == ref[j-1], otherwise the
 * candidate of the smallest S + D + I among substitution (c[i-1][j-1], S + 1), deletion (c[i][j-1],
 * D + 1) and insertion (c[i-1][j], I + 1), ties to the first in that order.  The counts travel with
 * the cost: no table, no backtrace.  Integer only, so the result equals the host rule bit for bit.
 * vasr_edit_counts_i32: pair p is hyp[p*ld_hyp + i], i < min(hyp_len[p], max_hyp), against
 *   ref[p*ld_ref + j], j < min(ref_len[p], max_ref) (negative lengths count as 0); nothing past a
 *   pair's length reaches the result.  counts is (P, 3) int32: S, D, I.  1 <= P <= 65535 and
 *   0 <= max_hyp, max_ref <= 65535, so every count fits 16 bits and a cell is one 64-bit word
 *   (cost, S, D, I).  The reference lies on the columns.  A pair of at most vasr_edit_wave_cols()
 *   reference items is swept by one wave (several pairs per workgroup, no barrier); a wider one by
 *   one workgroup, in passes of vasr_edit_tile_cols() columns whose last column is kept in the
 *   workspace between passes.  One call takes any mix of the two.
 * vasr_edit_workspace_bytes: bytes vasr_edit_counts_i32 needs at `workspace` (0 when max_ref fits one
 *   pass; workspace may then be NULL); -1 for arguments outside the limits above.  The workspace is
 *   written before it is read.
 * All arrays are on the device.  No allocation, no synchronisation, no host read; everything is
 * enqueued on `stream`.  Argument errors return VASR_EINVAL before any device call. */
int vasr_edit_counts_i32(const int32_t* hyp, int64_t ld_hyp, const int32_t* hyp_len, int max_hyp,
                         const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, int max_ref,
                         int P, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int64_t vasr_edit_workspace_bytes(int P, int max_hyp, int max_ref);
int vasr_edit_wave_cols(void);
int vasr_edit_tile_cols(void);

/* ------------------------------------------------------------------ WER / CER alignment (device)
 * The edit path behind the counts above, the rule velocity_asr.training.edit_alignment_host states:
 * cell (0, j > 0) is a deletion, cell (i > 0, 0) an insertion, hyp[i-1] == ref[j-1] a hit, otherwise
 * the smallest of c[i-1][j-1], c[i][j-1], c[i-1][j], ties to the first of substitution, deletion,
 * insertion; the path walks back from (hyp_len, ref_len) along those choices.  Operation codes:
 * 0 hit, 1 substitution, 2 deletion (a reference item with no counterpart), 3 insertion (a hypothesis
 * item with no counterpart).
 * vasr_edit_align_i32: the arguments up to `counts` are vasr_edit_counts_i32's, with the same limits,
 *   and counts receives the same integers.  The same two sweeps also keep each cell's choice, 2 bits,
 *   eight columns to a 16-bit word, in the pair's part of `table`; a third kernel walks the choices
 *   back with one wave per pair and writes ops[p*ld_ops + k], k < ops_len[p] = ref_len + I, in
 *   forward order (I is in the counts by then, so nothing is reversed).  Nothing is written in ops[p]
 *   at or past ops_len[p]; ld_ops >= max_hyp + max_ref.
 *   Table.  Pair p of m x n clamped items uses vasr_edit_align_table_bytes(m, n) =
 *   2 * m * ceil(n / 8) bytes from table + table_offset[p] (device int64, (P,)).  The word of row i,
 *   strip s lies at ((i - 1 + s) mod m) * ceil(n / 8) + s: a sweep's wave stores one step's words side
 *   by side.  The kernels work the extent out from the device lengths themselves; a pair whose offset
 *   is negative or odd, or whose offset + extent exceeds table_bytes, is skipped: ops_len[p] = -1, its
 *   counts are still written, and neither the table nor ops is touched for it.  `table` is not NULL
 *   and 2-byte aligned; it is written before it is read.  (Environment VASR_EDIT_ALIGN_STAGE=1 runs
 *   the sweeps only, =2 the walk only over what an earlier call left in the same buffers: a timing aid.)
 * vasr_edit_align_table_bytes: one pair's extent; -1 for a length outside 0..65535.
 * workspace: as vasr_edit_workspace_bytes(P, max_hyp, max_ref) states.  All arrays are on the device.
 * Integer only, no atomics.  No allocation, no synchronisation, no host read; everything is enqueued
 * on `stream`.  Argument errors return VASR_EINVAL before any device call. */
int vasr_edit_align_i32(const int32_t* hyp, int64_t ld_hyp, const int32_t* hyp_len, int max_hyp,
                        const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, int max_ref, int P,
                        int32_t* counts, uint8_t* ops, int64_t ld_ops, int32_t* ops_len,
                        const int64_t* table_offset, void* table, int64_t table_bytes, void* workspace,
                        int64_t workspace_bytes, void* stream);
int64_t vasr_edit_align_table_bytes(int hyp_len, int ref_len);

/* ------------------------------------------------------------------ mel front end
 * compute_mel_spectrogram (audio.py:65-143) is three launches:
 *  1. vasr_reflect_pad_f32: xp[b][0:S+2*pad] = reflect-padded audio (audio.py:100-101),
 *     rows of stride ld_out (>= S + 2*pad + n_fft); the tail is zero-filled.
 *  2. vasr_linear_x3_f32 with VASR_EPI_PAIR_POWER on rows of stride `hop` of xp against the
 *     Hann-windowed DFT matrix -> power[b][f][k] = |X_k|^2 (audio.py:104-115).
 *  3. vasr_mel_log_norm_f32: mel = fb @ power (audio.py:126), log(mel + 1e-10) (:129),
 *     per-(b, mel bin) (x - mean)/(std_unbiased + 1e-10) over frames (:132-135), written
 *     to out[b][frame_off + f][m] with batch stride out_stride.  The other frames of each
 *     utterance's padded slab of out_stride / n_mels frames are written as 0: the zero-framed
 *     (B, F + 2, n_mels) layout the stride-2 temporal conv GEMM reads as plain strided rows
 *     (model.py:156-162, padding 1), with no separate padding pass.  fb is passed in CSR form
 *     (rows = mel bins).
 */
int vasr_reflect_pad_f32(const float* audio, int64_t ld_audio, float* xp, int64_t ld_out,
                         int B, int S, int pad, void* stream);
int vasr_mel_log_norm_f32(const float* power, int64_t ld_power, int64_t stride_power,
                          const int32_t* fb_rowptr, const int32_t* fb_col, const float* fb_val,
                          float* out, int64_t out_stride, int frame_off, int B, int F, int n_mels,
                          int normalize, float* workspace, void* stream);
/* Utterances of different lengths in one zero-padded batch (the _var entry points below and
 * vasr_stft_power_400_var_f32, vasr_adaptive_pool_var_f32, vasr_pooled_attention_var_f32,
 * vasr_ctc_collapse_var): a device int32 array gives each utterance's own size, and every
 * value an utterance keeps is the one it gets alone (the reference runs one file at a time,
 * scripts/evaluate.py:91-98).  Here frames[b] <= F is utterance b's frame count: its
 * statistics cover its own frames only and its later frames are written as 0.  Needs
 * ld_power <= 256 and n_mels <= 85 (the chunked pass). */
int vasr_mel_log_norm_var_f32(const float* power, int64_t ld_power, int64_t stride_power,
                              const int32_t* fb_rowptr, const int32_t* fb_col, const float* fb_val,
                              float* out, int64_t out_stride, int frame_off, int B, int F, int n_mels,
                              int normalize, const int32_t* frames, float* workspace, void* stream);
/* workspace size of vasr_mel_log_norm_f32 in floats (log-mel rows + per-chunk fp64 partials) */
int64_t vasr_mel_workspace_floats(int B, int F, int n_mels);

/* Steps 1 + 2 in one launch for n_fft = 400, hop = 160 (the reference defaults, audio.py:15-18):
 * power[b][f][k] = |X_k|^2, k = 0..200, frame f of the reflect-padded audio (pad 200, computed
 * on the fly, no padded copy) times window[0:400], by a 400-point real FFT in LDS (200-point
 * complex FFT as 8 x 5 x 5 + real unpack).  F = S / 160 + 1 frames; power rows of stride ldp
 * (>= 201), batch stride stride_power (>= F * ldp).  Needs S > 200 (torch's reflect-pad rule). */
int vasr_stft_power_400_f32(const float* audio, int64_t ld_audio, int B, int S, const float* window,
                            float* power, int64_t ldp, int64_t stride_power, void* stream);
/* samples[b] (device, 200 < samples[b] <= S): utterance b's length inside the zero-padded
 * (B, S) batch; its reflect padding is taken at its own end, so its first samples[b]/160 + 1
 * frames equal those of the utterance alone (later frames: ignored by the _var mel pass). */
int vasr_stft_power_400_var_f32(const float* audio, int64_t ld_audio, int B, int S, const int32_t* samples,
                                const float* window, float* power, int64_t ldp, int64_t stride_power,
                                void* stream);
/* Write (B, F, C) rows into a zero-padded frame layout: out[b][off + f][c] = x[b][f][c]
 * and zero for the other out_frames - F frames (batch stride out_frames * C).  Feeds mel
 * to the stride-2 temporal conv, whose im2col rows are then plain strided rows (the public
 * model(mel) path; the device pipeline has vasr_mel_log_norm_f32 write the padded layout). */
int vasr_pad_frames_f32(const float* x, float* out, int out_frames, int off,
                        int B, int F, int C, void* stream);

/* ------------------------------------------------------------------ global context
 * F.adaptive_avg_pool1d over time (attention.py:71-73): bin i = [floor(iL/K), ceil((i+1)L/K)).
 * x: (B, L, C), out: (B, K, C).
 */
int vasr_adaptive_pool_f32(const float* x, float* out, int B, int L, int C, int K, void* stream);
/* Per utterance (device): its first lens[b] rows pooled into ks[b] bins (1 <= ks[b] <= lens[b]
 * <= L, ks[b] <= K), bins past ks[b] written as 0; x and out keep the strides L and K. */
int vasr_adaptive_pool_var_f32(const float* x, float* out, int B, int L, int C, int K, const int32_t* lens,
                               const int32_t* ks, void* stream);

/* LayerNorm(x; w, b, eps) of every row, then vasr_adaptive_pool_f32 (lens / ks null) or
 * vasr_adaptive_pool_var_f32 (both given) of the normalised rows, in one launch without the
 * normalised rows in memory: bitwise vasr_layer_norm_f32 followed by the pooling.  Replaces the
 * global SSM stack's final norm (reference ssm.py:555) followed by the second pooling level's
 * average pool (attention.py:303, AdaptivePool.forward :69-73).  C <= 1024. */
int vasr_ln_adaptive_pool_f32(const float* x, const float* w, const float* b, float eps, float* out, int B, int L,
                              int C, int K, const int32_t* lens, const int32_t* ks, void* stream);

/* Pooled multi-head cross attention core (attention.py:143-160), no mask:
 * out[b,t,h*hd:(h+1)*hd] = softmax(q_bth . k_bh^T / sqrt(hd)) v_bh over the Kp pooled keys.
 * q: (B, L, A) with row stride ld_q; kv: (B, Kp, 2A) [k | v]; out: (B, L, A) contiguous.
 * Kp <= 64, hd <= 64.
 */
int vasr_pooled_attention_f32(const float* q, int64_t ld_q, const float* kv, float* out,
                              int B, int L, int Kp, int heads, int head_dim, void* stream);
/* kps[b] (device, 1 <= kps[b] <= Kp): utterance b attends over its own first kps[b] keys. */
int vasr_pooled_attention_var_f32(const float* q, int64_t ld_q, const float* kv, float* out,
                                  int B, int L, int Kp, int heads, int head_dim, const int32_t* kps,
                                  void* stream);

/* ------------------------------------------------------------------ global context, backward (added to ABI 21)
 * Training through HierarchicalGlobalContext (reference attention.py under autograd): the
 * gradients of the two kernels above; the forwards are those kernels themselves (only their
 * inputs are kept).
 *
 * vasr_pooled_attention_bwd_f32: with s_k = q . k_k / sqrt(hd), p = softmax(s) over the utterance's
 * keys (recomputed with the forward's operations), g = d loss / d out, dP_k = g . v_k and
 * delta = sum_k p_k dP_k (= g . out), per (utterance, head):
 *   dS_k = p_k (dP_k - delta),           dq   = sum_k dS_k k_k / sqrt(hd),
 *   dK_k = sum_t dS_tk q_t / sqrt(hd),   dV_k = sum_t p_tk g_t.
 * q: (B L, A) rows with stride ld_q, kv: (B Kp, 2A) [k | v], dout: (B L, A) contiguous, kps: NULL or
 * as vasr_pooled_attention_var_f32.  Outputs, contiguous and every element written: dq (B L, A) and
 * dkv (B Kp, 2A) [dK | dV], rows k >= kps[b] as 0 (L = 0: dkv all 0).  Limits are the forward's:
 * Kp <= 64, head_dim <= 32, A = heads head_dim <= 256 and a multiple of 4, kv 16-byte aligned,
 * Kp 2A floats <= 64 KiB.  workspace: vasr_pooled_attention_bwd_workspace_floats(B, L, Kp, heads,
 * head_dim) floats = B ceil(L / 64) Kp 2A, the [dK | dV] partial of every 64-token tile, and 0 for
 * L <= 64, where the one tile writes dkv itself (workspace may then be NULL).  No floating-point
 * atomics: dq has no reduction, a tile's tokens are added in token order and the tiles in tile
 * order, so the gradients are run-to-run bitwise and an utterance's rows do not depend on the rest
 * of the batch.  Work is only enqueued on stream. */
int vasr_pooled_attention_bwd_f32(const float* q, int64_t ld_q, const float* kv, const float* dout,
                                  float* dq, float* dkv, float* workspace, int64_t workspace_floats,
                                  int B, int L, int Kp, int heads, int head_dim, const int32_t* kps,
                                  void* stream);
int64_t vasr_pooled_attention_bwd_workspace_floats(int B, int L, int Kp, int heads, int head_dim);
/* vasr_adaptive_pool_bwd_f32: g (B, K, C) = d loss / d out of vasr_adaptive_pool_f32 (lens, ks
 * NULL) or vasr_adaptive_pool_var_f32 (both given) -> dx (B, L, C), every element written once:
 *   dx[b,t,c] = sum over the bins i with s_i <= t < e_i, ascending, of g[b,i,c] / (e_i - s_i),
 * s_i = floor(i L_b / K_b), e_i = ceil((i + 1) L_b / K_b): a gather, at most two bins for K <= L.
 * Rows t >= lens[b] are written as 0; bins i >= ks[b] of g are never read. */
int vasr_adaptive_pool_bwd_f32(const float* g, float* dx, int B, int L, int C, int K,
                               const int32_t* lens, const int32_t* ks, void* stream);

/* ------------------------------------------------------------------ INT8 fake quantisation (C5)
 * FakeQuantize.forward in eval with calibrated buffers (quantize.py:79-97, :118-133):
 *   q = clamp(round_half_even(x / scale + zp), qmin, qmax); x_dq = (q - zp) * scale;
 *   y = x + (x_dq - x)
 * every operation IEEE-rounded in that order (bit-identical to torch's CPU evaluation).
 * x, y: (rows, cols) with row strides ldx, ldy (y may alias x).  scale / zero_point are
 * device arrays of `rows` entries if per_row != 0 (per-output-channel weights,
 * channel_dim 0) or of one entry (per-tensor).
 */
int vasr_fakequant_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int cols,
                       const float* scale, const float* zero_point, int per_row, float qmin,
                       float qmax, void* stream);

/* Per-row min and max of x (rows, cols), NaN-propagating like torch.amin / amax: the
 * statistics FakeQuantize._update_scale_zp observes (quantize.py:99-116).  A per-tensor
 * range is two calls (rows of x, then the row results as one row). */
int vasr_minmax_f32(const float* x, int64_t ldx, int rows, int cols, float* out_min,
                    float* out_max, void* stream);

/* ------------------------------------------------------------------ CTC decode
 * argmax over V per row, ties -> first index (decode.py:46).
 */
int vasr_argmax_f32(const float* logits, int64_t ld, int rows, int V, int32_t* out, void* stream);

/* Partial keys of a VASR_EPI_ARGMAX GEMM ((rows, ld), `slots` = ceil(N/32) used) -> int32
 * argmax indices.  Keys are order-preserving (float bits, ~column) pairs, so the largest is
 * the largest logit with the smallest index.  The fused CTC head (model.py:223-227 +
 * decode.py:46) never writes the (rows, V) logits. */
int vasr_argmax_keys(const uint64_t* keys, int64_t ld, int slots, int rows, int32_t* out, void* stream);

/* CTC prefix beam search (decode.py:128-217, lm_scorer = None), one workgroup per utterance.
 * logits: (B, L, V) with row stride ld_row and utterance stride ld_utt; W <= 32 beams.
 * Outputs per utterance b, beam r < out_nbeams[b] (sorted as the reference returns them):
 * out_tokens[(b*W + r)*L + 0 .. out_len[b*W + r]), out_score[b*W + r] (float64 sum of the
 * float32 log-softmax values, as the reference's Python floats).  trie: caller workspace of
 * B * vasr_ctc_beam_workspace_elems(L, W) int32. */
int vasr_ctc_beam_search(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                         int W, int blank, int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                         double* out_score, int32_t* out_nbeams, void* stream);
int64_t vasr_ctc_beam_workspace_elems(int L, int W);

/* The same search for padded batches and with a bigram language model; same
 * outputs, layout ((B, W, L) token rows) and workspace.  With frames and lm_table both NULL it is
 * vasr_ctc_beam_search.
 * frames (B, device int32, or NULL = all L): utterance b is searched over its first
 *   min(max(frames[b], 0), L) rows and no row at or past that count is read; a count of 0 gives
 *   the single empty beam with score 0.0 (the reference on seq_len = 0).
 * lm_table ((V + 1, V) float32 with row stride ld_lm >= V, device, or NULL): row 0 holds
 *   log p(tok | sentence start), row 1 + p holds log p(tok | previous token p); column `blank` and
 *   row 1 + blank are never read.  Active when lm_table != NULL and lm_weight > 0 (decode.py:188):
 *   a non-blank candidate whose collapsed prefix is k then scores
 *   (score + lp[tok]) + lm_weight * S(k), S(k) the float64 left-to-right sum of k's table entries
 *   -- in every frame, a repeat of the last token included; the blank extension gets no term
 *   (decode.py:174-193).  lm_weight must not be NaN. */
int vasr_ctc_beam_search_lm(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                            int W, int blank, const int32_t* frames, const float* lm_table,
                            int64_t ld_lm, double lm_weight, int32_t* trie, int32_t* out_tokens,
                            int32_t* out_len, double* out_score, int32_t* out_nbeams, void* stream);

/* Per-frame shortlist for vasr_ctc_beam_search_shortlist, one launch for all B * L
 * rows.  logits, ld_row, ld_utt, frames as vasr_ctc_beam_search_lm; V up to 2^20 (the row is staged
 * in LDS up to V = 16384 and re-read from global memory above).  Each row's log-probabilities are
 * bitwise those vasr_ctc_beam_search forms: the same operations and the same summation order.
 * 1 <= K <= 64 (V >= 2; K above V - 1 is taken as V - 1, which then is the arrays' last extent):
 *   out_tok, out_lp (B, L, K): the K non-blank tokens with the largest log-probabilities, ordered by
 *   (log-probability descending, token ascending), and those log-probabilities; out_blank_lp (B, L):
 *   the blank's.  Rows at or past min(max(frames[b], 0), L) are not read; they are filled with token
 *   -1 and -inf.
 * K == 0 (complete mode): out_lp (B, L, V) receives the whole log-probability rows, out_tok and
 *   out_blank_lp are not used (may be NULL), and rows at or past the count are left unwritten. */
int vasr_ctc_beam_shortlist_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                int K, int blank, const int32_t* frames, int32_t* out_tok, float* out_lp,
                                float* out_blank_lp, void* stream);

/* vasr_ctc_beam_search's frame step (lm_scorer = None) over the blank and each frame's K shortlisted
 * tokens: nb * (K + 1) candidates per frame instead of nb * V, one wave per utterance.  tok, lp
 * (B, L, K) and blank_lp (B, L) contiguous, as vasr_ctc_beam_shortlist_f32 writes them (1 <= K <=
 * min(64, V - 1)); V is the vocabulary the tokens come from (insertion positions are those of the
 * full search); W, blank, frames, trie and the four outputs as vasr_ctc_beam_search_lm.
 * out_uncertified (B): the number of frames of utterance b whose step is not proved equal to the
 * full search's.  A frame is certified when K == V - 1, or when it yields W survivors and the W-th
 * survivor's score is strictly above s_i + (double)theta for every live beam score s_i, theta the
 * shortlist's smallest log-probability (a comparison with NaN fails).  With out_uncertified[b] == 0
 * utterance b's outputs are bitwise vasr_ctc_beam_search_lm's on the same logits; otherwise they
 * are the pruned search's and the caller searches b again.
 * tok == NULL (complete): lp is (B, L, V) log-probabilities (vasr_ctc_beam_shortlist_f32 with K = 0),
 * looked up by token; K and blank_lp are ignored, no certificate is evaluated, out_uncertified is
 * 0, and the result is vasr_ctc_beam_search_lm's for any V up to 2^20. */
int vasr_ctc_beam_search_shortlist(const int32_t* tok, const float* lp, const float* blank_lp, int B, int L,
                                   int K, int V, int W, int blank, const int32_t* frames, int32_t* trie,
                                   int32_t* out_tokens, int32_t* out_len, double* out_score,
                                   int32_t* out_nbeams, int32_t* out_uncertified, void* stream);

/* The standard CTC prefix beam search (not the reference's, which the entries above
 * restate): a prefix carries the summed log-probability of all its alignments, pb over those ending
 * in the blank and pnb over those ending in its tail token (float64, joined by logaddexp, start
 * pb = 0, pnb = -inf for the empty prefix).  Per frame, live beam i (tot = pb (+) pnb) gives
 * tot + lp[blank] to its own pb, pnb + lp[tail] to its own pnb, pb + lp[tail] to prefix + (tail) and
 * tot + lp[tok] to prefix + (tok) for every other non-blank token; contributions to one prefix are
 * summed, a contribution of -inf is not made.  The W prefixes of largest
 *   rank = ((pb (+) pnb) + alpha * S(prefix)) + beta * len(prefix)
 * survive (ties: the reference's insertion order, position i (V + 1) + tok + 1, the blank's at
 * i (V + 1), and at the position of a repeated tail the prefix's own key before the extension); S is the bigram table's left-to-right float64 sum, so a token's language-model score is
 * added once, when it is appended, and beta is a per-token length bonus.
 * logits, ld_row, ld_utt, B, L, V <= 16384, W <= 32, blank, frames, lm_table, ld_lm, trie, out_tokens,
 * out_len and out_nbeams as vasr_ctc_beam_search_lm; the table is active when lm_table != NULL and
 * alpha > 0; alpha and beta must not be NaN.  out_score[b*W + r] = rank, out_logp[b*W + r] =
 * pb (+) pnb, the log-probability of the prefix given the frames (under the beam's pruning).  A frame
 * count of 0 gives the single empty beam with out_logp = out_score = 0.0. */
int vasr_ctc_prefix_beam_search(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                int W, int blank, const int32_t* frames, const float* lm_table,
                                int64_t ld_lm, double alpha, double beta, int32_t* trie, int32_t* out_tokens,
                                int32_t* out_len, double* out_score, double* out_logp, int32_t* out_nbeams,
                                void* stream);

/* The same search with token pruning: the frame's candidates are the blank and the K tokens of
 * vasr_ctc_beam_shortlist_f32's arrays (tok, lp (B, L, K), blank_lp (B, L), 1 <= K <= min(64, V - 1));
 * every other token counts as -inf, while the log-probabilities stay those of the full softmax.  An
 * approximation: no certificate, no fallback.  V (up to 2^20) is the vocabulary the tokens come from;
 * an entry that is the blank or outside 0 .. V - 1 is skipped.  Everything else as above. */
int vasr_ctc_prefix_beam_search_shortlist(const int32_t* tok, const float* lp, const float* blank_lp, int K,
                                          int V, int B, int L, int W, int blank, const int32_t* frames,
                                          const float* lm_table, int64_t ld_lm, double alpha, double beta,
                                          int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                                          double* out_score, double* out_logp, int32_t* out_nbeams,
                                          void* stream);

/* Greedy CTC collapse per utterance (decode.py:51-69, :89-123): drop blank (and reset
 * prev), skip repeats of prev if collapse != 0.  out_tokens (B, L) holds each
 * utterance's kept tokens left-aligned, out_len (B) their counts.  If out_start /
 * out_end are non-NULL they receive the (start_frame, end_frame) of each kept token
 * with the semantics of ctc_greedy_decode_with_timestamps (collapse must be 1).
 */
int vasr_ctc_collapse(const int32_t* pred, int B, int L, int blank, int collapse,
                      int32_t* out_tokens, int32_t* out_len, int32_t* out_start,
                      int32_t* out_end, void* stream);
/* frames[b] (device): utterance b collapses its own first frames[b] rows; values outside [0, L]
 * are clamped to it (no row past L is read or written). */
int vasr_ctc_collapse_var(const int32_t* pred, int B, int L, const int32_t* frames, int blank, int collapse,
                          int32_t* out_tokens, int32_t* out_len, int32_t* out_start, int32_t* out_end,
                          void* stream);
/* Greedy decode straight from a VASR_EPI_ARGMAX GEMM's keys (B * L rows, `slots` used, row
 * stride ld): vasr_argmax_keys then vasr_ctc_collapse[_var] in ONE launch, one workgroup per
 * utterance (the predictions stay in LDS; the fused CTC head + decode.py:46-69 of the
 * reference's greedy path).  frames: NULL or device int32[B] as in vasr_ctc_collapse_var;
 * pred: NULL or device int32[B * L] to also receive the per-frame argmax.  L <= 8192. */
int vasr_ctc_collapse_keys(const uint64_t* keys, int64_t ld, int slots, int B, int L, const int32_t* frames,
                           int blank, int collapse, int32_t* pred, int32_t* out_tokens, int32_t* out_len,
                           int32_t* out_start, int32_t* out_end, void* stream);

/* Greedy decode with confidences.  The log-probability of frame (b, t)'s argmax
 * k* is lp[b,t] = (z[k*] - Ms) - lse, {Ms, lse} the row statistics as vasr_lse_combine_f32 defines
 * them.  For kept token j of utterance b, whose run is frames [start, end) as vasr_ctc_collapse
 * reports them with collapse = 1: out_logp_sum[b*L + j] = the sum of lp over the run (added left to
 * right), out_logp_min[b*L + j] = its minimum; the run length is end - start.  out_path_logp[b] = the
 * sum of lp over the utterance's frames, blank ones included (the log-probability of the greedy
 * path; 0.0 for no frames): lane l of one wave adds frames l, l + 64, ... in order, then a fixed tree
 * over the 64 lanes.  Every value depends on the utterance's own frames alone: bitwise repeatable
 * and independent of B and of the other utterances.  All float32.
 *
 * vasr_argmax_logp_f32: out_idx bitwise vasr_argmax_f32, out_logp[row] = lp from an fp32
 * max-subtracted log-sum-exp of the row; any V >= 1, any alignment. */
int vasr_argmax_logp_f32(const float* logits, int64_t ld, int rows, int V, int32_t* out_idx, float* out_logp,
                         void* stream);
/* Collapse (B, L) predictions with their lp: one workgroup per utterance.  out_tokens, out_len,
 * out_start, out_end are bitwise those of vasr_ctc_collapse[_var] with collapse = 1 (all required here).
 * frames: NULL (all L rows) or device int32[B], clamped to [0, L]; no row at or past the clamped
 * count is read.  1 <= L <= 8192 (VASR_EINVAL otherwise); only the first out_len[b] entries of an
 * output row are written. */
int vasr_ctc_collapse_conf(const int32_t* pred, const float* logp, int B, int L, const int32_t* frames, int blank,
                           int32_t* out_tokens, int32_t* out_len, int32_t* out_start, int32_t* out_end,
                           float* out_logp_sum, float* out_logp_min, float* out_path_logp, void* stream);
/* The same straight from a VASR_EPI_ARGMAX_LSE GEMM's slots (B * L rows of row stride ld, nslots =
 * 2 * ceil(N/32) used: key, pair, key, pair, ...), in ONE launch: per row the keys fold as
 * vasr_argmax_keys folds them and the pairs as vasr_lse_combine_f32 does, the maximum logit is read
 * back out of the largest key's float bits, then the collapse above.  The per-frame values stay in
 * LDS; pred / logp: NULL or device int32 / float [B * L] to also receive them (rows at or past an
 * utterance's count are neither read nor written). */
int vasr_ctc_collapse_keys_conf(const uint64_t* slots, int64_t ld, int nslots, int B, int L, const int32_t* frames,
                                int blank, int32_t* pred, float* logp, int32_t* out_tokens, int32_t* out_len,
                                int32_t* out_start, int32_t* out_end, float* out_logp_sum, float* out_logp_min,
                                float* out_path_logp, void* stream);

/* ------------------------------------------------------------------ CTC loss and forced alignment
 * Forward-only scoring of a KNOWN transcript (training.py:47-104: F.log_softmax + nn.CTCLoss as
 * Trainer.eval_step, training.py:273-299, uses them for eval_loss), and the Viterbi form of the
 * same lattice: per-token frame spans, the companion of ctc_greedy_decode_with_timestamps
 * (decode.py:74-125), which only timestamps the model's own guess.  The gradient of the loss is
 * the next section.
 *
 * Common arguments: targets (B, Smax) int32 (may be NULL if Smax == 0); frames[B] and tlen[B]
 * device int32, clamped to [0, L] and [0, Smax]; rows t >= frames[b] and target slots
 * j >= tlen[b] are neither read nor used.  1 <= L <= 8192 (VASR_EINVAL otherwise), Smax <= 2048
 * (VASR_EUNSUPPORTED above).
 *
 * Stage 1, the only pass over the logits ((B, L, V), row stride ld_row >= V, utterance stride
 * ld_utt, as vasr_ctc_beam_search; any V, any alignment): emis (B, L, Smax + 1) contiguous,
 *   emis[b][t][0]     = logit[b,t,blank]         - lse[b,t]
 *   emis[b][t][1 + j] = logit[b,t,targets[b][j]] - lse[b,t]      (j < tlen[b])
 * with lse the fp32 max-subtracted log-sum-exp of the row; entries of padding rows and slots are
 * left unwritten.  A target id outside [0, V) (within tlen[b]) is never used as an index: its
 * emission is -inf, so that utterance scores as an infeasible target (nll +inf, align score -inf). */
int vasr_ctc_emissions_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                           const int32_t* targets, int Smax, const int32_t* frames, const int32_t* tlen,
                           int blank, float* emis, void* stream);

/* Stage 2a: out_nll[b] = -log p(targets[b] | logits[b]) over the extended label sequence of
 * S' = 2 tlen + 1 states (blanks interleaved): a state is reached from s, s - 1, and from s - 2
 * only when s is a non-blank that differs from state s - 2 (the recursion of
 * torch.nn.functional.ctc_loss); nll = -logsumexp(alpha[T-1][S'-1], alpha[T-1][S'-2]), all in
 * fp32 log space with the maximum subtracted.  An infeasible target gives +inf (zero_infinity is
 * the caller's); tlen = 0 sums the blank emissions; frames = 0 gives 0 for tlen = 0, else +inf.
 * One workgroup per utterance; each value depends on its own utterance only. */
int vasr_ctc_loss_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                      const int32_t* frames, const int32_t* tlen, float* out_nll, void* stream);

/* Stage 2b, the Viterbi form: the best path through the same lattice.
 *   frame_state (B, L): the target index frame t emits, -1 for blank and for t >= frames[b];
 *   out_start / out_end (B, Smax): first frame and one past the last frame of token j's run
 *     (the convention of ctc_greedy_decode_with_timestamps), -1 for j >= tlen[b];
 *   out_score[b]: the path's log-probability.
 * An infeasible target gives out_score = -inf and -1 everywhere.  Ties go to the smaller source
 * state (s before s - 1 before s - 2), and to S' - 2 over S' - 1 at the end.
 * workspace (4-byte aligned) holds a 2-bit back-pointer per (t, s), 4 states per byte, rows padded
 * to 32-bit words: vasr_ctc_align_workspace_bytes(B, L, Smax) = B * L * 4 * ceil((2 Smax + 1) / 16);
 * workspace_bytes below that is VASR_EINVAL. */
int vasr_ctc_align_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                       const int32_t* frames, const int32_t* tlen, void* workspace, int64_t workspace_bytes,
                       int32_t* frame_state, int32_t* out_start, int32_t* out_end, float* out_score,
                       void* stream);
int64_t vasr_ctc_align_workspace_bytes(int B, int L, int Smax);

/* ------------------------------------------------------------------ CTC loss, backward
 * The gradient of vasr_ctc_loss_f32's nll with respect to the logits, in three launches, with the
 * common arguments and limits above.  These three symbols were ADDED to ABI 20 without a bump:
 * they are purely additive (no existing symbol, argument or result changed), so every caller of
 * ABI 20 keeps working unchanged, and a caller that needs them finds out by looking the symbols up.
 *
 * For utterance b with T = frames[b], n = tlen[b], S' = 2 n + 1 and e[t][s] the emission of state s
 * (emis[b][t][0] for a blank, emis[b][t][1 + j] for label j), all in fp32 log space:
 *   alpha as vasr_ctc_loss_f32;
 *   beta[T-1][s] = e[T-1][s] for s in {S'-1, S'-2}, -inf otherwise;
 *   beta[t][s]   = e[t][s] + lse(beta[t+1][s], beta[t+1][s+1], beta[t+1][s+2]), the last term only
 *                  for a label s whose successor label differs (both include the emission at t, the
 *                  convention of torch.nn.functional.ctc_loss);
 *   gamma[t][s]  = exp(alpha[t][s] + beta[t][s] - e[t][s] + nll).
 *
 * Stage 2a': vasr_ctc_loss_f32 that also keeps alpha (B, L, 2 Smax + 1): alpha[b][t][s] for t < T,
 * s < S'; the other entries are left unwritten.  out_nll is bitwise vasr_ctc_loss_f32's.
 * alpha_elems (floats available at alpha) below B * L * (2 Smax + 1) is VASR_EINVAL. */
int vasr_ctc_loss_alpha_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                            const int32_t* frames, const int32_t* tlen, float* out_nll, float* alpha,
                            int64_t alpha_elems, void* stream);

/* Stage 3: the posterior occupancy occ (B, L, Smax + 1), linear space, from emis, the alpha and the
 * nll of vasr_ctc_loss_alpha_f32:
 *   occ[b][t][0]     = sum of gamma[t][s] over the blank states (even s),
 *   occ[b][t][1 + j] = gamma[t][2 j + 1]                                   (t < T, j < n),
 * and exact zeros in every other entry: rows t >= T, slots past n, and all of an utterance whose
 * nll is +inf.  Every entry of occ is written, and lies in [0, 1]: a value that fp32 rounding
 * (alpha + beta at magnitudes in the thousands) puts above 1 is clamped to it, which only moves it
 * towards the exact posterior.  One workgroup per utterance; the blank sum is
 * reduced in a fixed order (within a wave, then over the waves in wave order), so each value
 * depends on its own utterance only and repeats bitwise. */
int vasr_ctc_occupancy_f32(const float* emis, const float* alpha, int64_t alpha_elems, const float* nll, int B,
                           int L, int Smax, const int32_t* targets, const int32_t* frames, const int32_t* tlen,
                           float* occ, void* stream);

/* Stage 4: the gradient, grad (B, L, V) contiguous fp32, from the logits (strides as
 * vasr_ctc_emissions_f32; any V, any alignment) and occ:
 *   grad[b][t][v] = scale[b] * (softmax(logits[b][t])[v] - sum of occ[b][t][slot] over the slots
 *                   whose token is v)            (t < T; slot 0 is `blank`, slot 1 + j targets[b][j]),
 *   grad[b][t][:] = 0                            (t >= T; those logit rows are not read).
 * scale[B] (device fp32) is the upstream gradient of nll_b.  The row's log-sum-exp is recomputed as
 * in stage 1, so no (B, L, V) log-softmax and no (B, L) side buffer exists.  Slots that share a
 * token are summed in ascending slot order and every column has one writer of its final value (no
 * floating-point atomics): the result repeats bitwise.  A token id outside [0, V) is never used as
 * an index.  workspace: B * (Smax + 1) int32 (the per-utterance chain of slots with the same token,
 * built by a first small launch); workspace_elems below that is VASR_EINVAL. */
int vasr_ctc_grad_logits_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                             const int32_t* targets, int Smax, const int32_t* frames, const int32_t* tlen,
                             int blank, const float* occ, const float* scale, int32_t* workspace,
                             int64_t workspace_elems, float* grad, void* stream);

/* ------------------------------------------------------------------ CTC loss on the head, no logits
 * The loss of logits = xn W^T + bias (the CTC head: xn (B * L, K) its normalised rows, W (V, K))
 * without a (B, L, V) tensor.  Forward: vasr_linear_x3_f32 with VASR_EPI_LSE, vasr_lse_combine_f32,
 * vasr_ctc_head_emissions_f32, then vasr_ctc_loss[_alpha]_f32 / vasr_ctc_align_f32 as before.
 * Backward: vasr_ctc_occupancy_f32 once, then per chunk of whole utterances the plain GEMM into a
 * (rows, V) buffer and vasr_ctc_grad_logits_stats_f32 in place on it.
 *
 * vasr_lse_combine_f32: the pairs of a VASR_EPI_LSE GEMM ((M, ld) 8-byte slots, `slots` =
 * ceil(N/32) used, ld >= slots) -> stats (M, 2) contiguous fp32 {Ms, lse}: Ms the row maximum (0 if
 * the whole row is -inf), lse = log(sum exp(x - Ms)), so log_softmax(x) = (x - Ms) - lse. */
int vasr_lse_combine_f32(const float* pairs, int64_t ld, int slots, int M, float* stats, void* stream);

/* emis (B, L, Smax + 1) with vasr_ctc_emissions_f32's meaning from xn (row b * L + t at xn +
 * (b * L + t) * ld_x), W (row stride ldw), bias ([V] or NULL) and stats (B * L, 2):
 *   emis[b][t][j] = ((xn[b][t] . W[tok_j] + bias[tok_j]) - Ms) - lse, tok_0 = blank, tok_j = targets[b][j-1];
 * -inf for a token outside [0, V).  Rows t >= frames[b] are not read; they and slots j > tlen[b] are
 * left unwritten.  The dot products are accumulated in fp64 and the emission rounded once; they equal
 * the GEMM's logits to the GEMM's own tolerance, not bitwise.  One workgroup per (utterance, 64 frames) holds its
 * rows of xn in LDS, 65 * K * 4 bytes: a K that needs more than 64 KiB is VASR_EUNSUPPORTED. */
int vasr_ctc_head_emissions_f32(const float* xn, int64_t ld_x, const float* W, int64_t ldw, const float* bias,
                                const float* stats, int B, int L, int V, int K, const int32_t* targets, int Smax,
                                const int32_t* frames, const int32_t* tlen, int blank, float* emis, void* stream);

/* vasr_ctc_grad_logits_f32 in place, with the rows' {Ms, lse} read from stats (B * L, 2) instead of
 * recomputed: `logits` holds the logits on entry and the gradient on return (rows t >= T: exact
 * zeros, never read).  A target column ends as fma(-scale, summed occupancy, scale * softmax), one
 * rounding of scale * softmax away from vasr_ctc_grad_logits_f32's scale * (softmax - sum).
 * workspace as vasr_ctc_grad_logits_f32. */
int vasr_ctc_grad_logits_stats_f32(float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                   const float* stats, const int32_t* targets, int Smax, const int32_t* frames,
                                   const int32_t* tlen, int blank, const float* occ, const float* scale,
                                   int32_t* workspace, int64_t workspace_elems, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VASR_H_ */

/*
 * mst_hip.h — C-ABI of libmst_hip.so: the MI355X (gfx950) kernels behind the
 * VarAutoEncoder training step of slyforce/MusicStyleTransfer.
 *
 * Every entry point takes raw DEVICE pointers, explicit sizes / leading
 * dimensions and a hipStream_t (passed as void*), returns 0 on success or a
 * negative mst_status, never allocates, never synchronises, and may be
 * captured into a hipGraph. mst_last_error() returns a thread-local message
 * for the last non-zero status.
 *
 * The reference has no native code (it is Python on MXNet 1.3); each function
 * below replaces the MXNet operator call site(s) cited next to it. Paths are
 * relative to /root/reference/music_style_transfer/.
 *
 * Conventions
 *   - "act" tensors (activations) are 16-bit: MST_BF16 or MST_F16, selected by
 *     the `dtype` argument. Parameters / gradients / optimizer state are fp32.
 *   - Row-major everywhere. ld* are leading dimensions in ELEMENTS.
 *   - Dense weights keep MXNet's [units, in_units] layout (y = x W^T + b).
 */
#ifndef MST_HIP_H
#define MST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mst_stream_t; /* hipStream_t */

enum mst_status {
  MST_OK = 0,
  MST_ERR_INVALID = -1, /* bad argument (shape/alignment/dtype)             */
  MST_ERR_LAUNCH = -2,  /* hip launch / runtime error (see mst_last_error)  */
  MST_ERR_UNSUPPORTED = -3
};

enum mst_dtype { MST_BF16 = 0, MST_F16 = 1, MST_F32 = 2 };

/* epilogue activation for mst_gemm_nt */
enum mst_act { MST_ACT_NONE = 0, MST_ACT_RELU = 1 };

int mst_version(void);
const char* mst_last_error(void);

/* ---- stream-capture helpers (hipGraph instead of a tracing compiler) ---- */
int mst_graph_begin(mst_stream_t stream);
int mst_graph_end(mst_stream_t stream, void** graph_exec_out);
/* mst_graph_end that also reports what was captured: the graph's node count and how many of them are kernel launches
 * (either pointer may be NULL). Host-side queries of the captured graph only; the executable graph is the same. */
int mst_graph_end_counted(mst_stream_t stream, void** graph_exec_out, int32_t* nodes_out, int32_t* kernel_nodes_out);
int mst_graph_launch(void* graph_exec, mst_stream_t stream);
int mst_graph_destroy(void* graph_exec);

/* ---- hip events on an explicit stream (bench.py times kernels with these) ---- */
int mst_event_create(void** ev_out);
int mst_event_record(void* ev, mst_stream_t stream);
int mst_event_sync(void* ev);
int mst_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out);
int mst_event_destroy(void* ev);

/* ------------------------------------------------------------------------
 * K3/K7/K8/K10/K12 + piano-roll in/out Dense: C[M,N] = epi(A[M,K] · B[N,K]^T)
 * Replaces gluon.nn.Dense(flatten=False) at transformer.py:36-40,65-68,
 * model.py:70-71,214-227 and, with B = W^T shadow, their dgrad.
 *
 *   A, B      : act dtype; K must be a multiple of 8; lda, ldb multiples of 8
 *   C         : act dtype (c_f32 = 0) or fp32 (c_f32 = 1); ldc multiple of 4.
 *               Columns N..min(roundup4(N),ldc) are written as exact zeros.
 *   bias      : fp32 [N] or NULL
 *   resid     : act dtype [M, ldr] or NULL (residual branch, added after dropout)
 *   act       : mst_act applied to alpha*(acc+bias+grpadd)
 *   gate      : act dtype [M, ldg] or NULL; result is zeroed where gate <= 0
 *               (ReLU backward fused into the FFN2 dgrad, transformer.py:36-38)
 *   alpha     : scalar applied to (acc + bias + grpadd)  (sqrt(D), transformer.py:237,270)
 *   rowadd    : fp32 [rowadd_period, ldra] or NULL; rowadd[(m % rowadd_period)] added
 *               AFTER alpha·(acc+bias+grpadd) (positional table, transformer.py:204-211)
 *   grpadd    : fp32 table [*, ldga] gathered by grp_index[m / rowadd_period] (int32) or NULL;
 *               added BEFORE alpha (class embedding, model.py:89-91)
 *   a_rows_per_group/a_group_stride/a_group_offset : if a_rows_per_group > 0, logical row m of A
 *               lives at physical row (m / rpg)*stride + offset + (m % rpg)   (model.py:253 drops row 0)
 *   c_rows_per_group/...: same remap for C rows (model.py:244 concat after the initial state)
 *   dropout   : p in [0,1); if p > 0 the epilogue applies inverted dropout with the
 *               counter-based mask keep(seed, site, row*N+n), row = PHYSICAL output row (transformer.py:35,149,182)
 *   self_resid: out = t + dropout(t) (decoder LN3(ff + dropout(ff)), transformer.py:199-200)
 * Epilogue order: t = alpha*(acc + bias + grpadd) -> act -> [u = dropout(t); self_resid: u += t]
 *                 -> + rowadd -> + resid -> gate.
 * ------------------------------------------------------------------------ */
typedef struct mst_gemm_args {
  int32_t dtype;
  int32_t c_f32;
  int64_t M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  const float* bias;
  const void* resid; int64_t ldr;
  int32_t act;
  const void* gate; int64_t ldg;
  float alpha;
  const float* rowadd; int64_t ldra; int64_t rowadd_period;
  const float* grpadd; int64_t ldga; const int32_t* grp_index;
  int64_t a_rows_per_group, a_group_stride, a_group_offset;
  int64_t c_rows_per_group, c_group_stride, c_group_offset;
  float dropout_p; uint64_t dropout_seed; uint32_t dropout_site;
  int32_t self_resid;
  const uint64_t* dropout_seed_ptr; /* optional DEVICE word XORed into dropout_seed (per-step seed under graph replay) */
  int32_t a_u8; /* 1: A is uint8 [M, lda bytes] (piano-roll frames as they arrive from the batcher), widened to the
                 * activation type while the tile is staged into LDS: the frames are never stored in 16 bits. Offered
                 * for the embedding GEMMs' form: 16-bit C, no dropout / self_resid, lda % 8 == 0. */
  int32_t resid_phys; /* 1: the residual shares C's PHYSICAL rows (it follows the C row remap); 0: it is indexed by the logical row m,
                       * as a strided view would be */
} mst_gemm_args;

int mst_gemm_nt(const mst_gemm_args* args, mst_stream_t stream);
/* Which kernel mst_gemm_nt(args) launches, decided on the host from the arguments alone (no HIP call, no device needed; the
 * pointers are looked at for NULL and alignment only). The launch code calls the same decision and nothing else.
 * Returns tile * 16 + variant:
 *   tile    0  64 x 64 tiles, 64-deep K stages
 *           1  64 x 64 tiles, 256-deep K stages (M <= 64, K >= 512, K % 256 == 0: the decoder's skinny GEMMs)
 *           2  128 x 128 tiles, 64-deep K stages
 *           3  128 x 128 tiles at three workgroups per CU, 32-deep K stages (513..768 tiles; variant is 0)
 *   variant 0  fast epilogue (whole tiles, whole K stages, 16-byte friendly operands), 16-bit C
 *           1  fast epilogue with dropout / self_resid
 *           2  general (guarded) epilogue, 16-bit C
 *           3  general epilogue, fp32 C
 *           4..7  the same four with row ops (rowadd / grpadd / an A or C row remap)
 *           8, 9  uint8 A with row ops, fast / general
 * Invalid arguments: what mst_gemm_nt returns for them (MST_ERR_INVALID, or MST_ERR_UNSUPPORTED for the dtype), same message. */
int mst_gemm_nt_form(const mst_gemm_args* args);

/* Two mst_gemm_nt problems in ONE launch: the piano-roll ends' two embedding GEMMs (model.py:81-91 encoder input and
 * model.py:241-245 decoder input, transformer.py:237,270: the same uint8 frames against two tables), whose outputs and epilogues
 * differ but whose kernel form is the same. Both problems uint8-A, 16-bit C, whole 64 x 64 tiles, row-indexed adds / C row
 * remap only: one launch; anything else: exactly mst_gemm_nt(args0) followed by mst_gemm_nt(args1). */
int mst_gemm_nt_pair(const mst_gemm_args* args0, const mst_gemm_args* args1, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K12 + K14 in one launch: the decoder's output layer Dense[D -> P] (model.py:253-256) with sigmoid + BinaryCrossEntropy
 * (loss.py:27-80) in its epilogue, for P = 128 or 256 (a 64-row x P tile holds whole rows of pitches, and — T a multiple
 * of 64 — rows of one sample). `args` is the output layer's GEMM (A = decoder output with its row remap, B = weight, bias,
 * alpha); its C receives the LOGIT GRADIENT d(sum_b loss_b)/dlogit * gscale (NULL: forward only). The logits themselves
 * are not stored (unless `logits` is set); they are rounded to the activation type before the loss arithmetic, so the
 * result equals mst_gemm_nt followed by mst_sigmoid_bce. loss[b] must be zero on entry (mst_step_begin's zero list).
 * ------------------------------------------------------------------------ */
typedef struct mst_bce_args {
  const uint8_t* labels;      /* {0,1} [M, N] */
  int64_t T;                  /* rows per sample */
  float label_smoothing;
  int32_t downweight;         /* loss.py:50-54,58-81 negative-label down-weighting */
  float* loss;                /* fp32 [M / T], accumulated */
  void* probs; int64_t ldp;   /* optional act dtype [M, ldp]: sigmoid output */
  void* logits; int64_t ldl;  /* optional act dtype [M, ldl] */
  float gscale;
  uint64_t* counts;           /* optional [MST_ROLL_SLOTS][4], 16-byte aligned: the piano-roll counts below, ADDED to */
} mst_bce_args;
/* Piano-roll counts (ABI 114), kept on the device by every launch that computes the BCE: each (frame, pitch) cell a launch computes a
 * loss term for (row m < M, column < P; padded frames count as the loss counts them, pad columns never) adds to four integers
 *   [0] tp    label == 1 and predicted      [1] pred  predicted      [2] pos  label == 1      [3] cells  every cell counted
 * where "predicted" is: the 16-bit logit the loss arithmetic uses is strictly greater than 0 (+0, -0 and NaN are not). Label
 * smoothing, down-weighting and gscale play no part. A workgroup sums its cells exactly (integers) and one thread adds the four
 * numbers to slot (linear workgroup id % MST_ROLL_SLOTS) with 64-bit atomics: the totals over the slots are bit-reproducible, and
 * the 256 slots keep same-address serialisation away. Launches ADD; the caller clears the buffer when it reads (as tok_parts) and
 * sums the slots: precision = tp / pred, recall = tp / pos, F1 = 2 tp / (pred + pos). With counts == NULL a launch stores exactly
 * what it stored before (mst_gemm_sigmoid_bce, mst_gemm_sigmoid_bce_dgrad_ln — also as its two launches — and mst_dec_tail_step
 * read the field; their form queries do not depend on it). */
#define MST_ROLL_SLOTS 256
int mst_gemm_sigmoid_bce(const mst_gemm_args* args, const mst_bce_args* bce, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense + LayerNorm in one launch (transformer.py:155,158,197,200 forward; their autograd backward): the GEMM's tile
 * spans the whole output row (N = 128 or 256), so the row statistics are available in its epilogue.
 *   mode 1, forward : C = h = epi(A B^T) as mst_gemm_nt (bias, alpha, dropout / self_resid, resid, C row remap);
 *                     out = LayerNorm(h; gamma, beta, eps); mean[r], rstd[r] with r = PHYSICAL C row.
 *                     Equals mst_gemm_nt followed by mst_layernorm_fwd on C.
 *   mode 2, backward: dy = epi(A B^T) (bias, alpha, resid) is NOT stored; C = dx = LayerNorm backward of dy with
 *                     x (the forward's pre-norm tensor), mean, rstd all taken at the PHYSICAL C row r (the forward
 *                     wrote them there), gamma; out = dropout-masked copy of dx (mask_mode 1) at the LOGICAL row m;
 *                     dgamma / dbeta accumulated into — or, with `partials` set, NOT touched: workgroup w (one per
 *                     64 output rows; mst_gemm_nt_ln_parts(M) of them) stores its column sums at
 *                     partials[w * 2N + 0..N) (dgamma) and [N..2N) (dbeta) with plain stores, and the caller adds
 *                     them up later with mst_partial_sums (256 same-address fp32 atomics per column cost ~5 us of
 *                     serialisation per launch at configs[1]).
 *                     mask modes and the dropout counter (p / seed / site in the mst_gemm_args dropout fields) are
 *                     those of mst_layernorm_bwd. Equals mst_gemm_nt followed by mst_layernorm_bwd on its result.
 * ------------------------------------------------------------------------ */
typedef struct mst_ln_args {
  int32_t mode;
  const float* gamma;
  const float* beta;
  float eps;
  void* out; int64_t ld_out;
  float* mean; float* rstd;
  const void* x; int64_t ld_x;
  float* dgamma; float* dbeta;
  int32_t mask_mode;
  float* partials;        /* mode 2, optional: [mst_gemm_nt_ln_parts(M)][2N] fp32, 16-byte aligned */
} mst_ln_args;

int mst_gemm_nt_ln(const mst_gemm_args* args, const mst_ln_args* ln, mst_stream_t stream);
/* mst_gemm_sigmoid_bce(args, bce) and mst_gemm_nt_ln(dgrad, ln) in ONE launch where `dgrad` is the output layer's input gradient
 * (model.py:253-256 backward): A = the logit gradient `args` has just produced (dgrad->A == args->C), 128 pitches, row width 128,
 * ln->mode 2 — the workgroup that holds a 64-row tile of logit gradients contracts it with W_out and runs the last decoder layer's
 * LayerNorm backward on the result; the logit gradient is still stored (the weight-gradient launch reads it). Any other shape:
 * exactly the two launches. */
int mst_gemm_sigmoid_bce_dgrad_ln(const mst_gemm_args* args, const mst_bce_args* bce, const mst_gemm_args* dgrad,
                                  const mst_ln_args* ln, mst_stream_t stream);
int64_t mst_gemm_nt_ln_parts(int64_t M);
/* What mst_gemm_sigmoid_bce(args, bce) launches (dgrad = ln = NULL), or mst_gemm_sigmoid_bce_dgrad_ln(args, bce, dgrad, ln): decided on the
 * host from the arguments alone, no HIP call, no device needed (pointers are looked at for NULL, alignment and dgrad->A == args->C
 * only). The launches take the same decisions through the same code. form is a host array of 4 entries:
 *   form[0]  BN, the width of a column tile: 128 (128 pitches) or 256
 *   form[1]  column tiles per 64-row block, N / BN (above 1: the tiles of a row block share the sample's loss atomic)
 *   form[2]  0 without dgrad / ln; 1: mst_gemm_sigmoid_bce_dgrad_ln is one launch; 2: it is the two launches
 * Returns 0; invalid arguments: what the launch returns for them, same message. */
int mst_gemm_sigmoid_bce_form(const mst_gemm_args* args, const mst_bce_args* bce, const mst_gemm_args* dgrad, const mst_ln_args* ln,
                              int64_t* form);

/* The whole feed-forward block of a Transformer layer in one launch (transformer.py:38-40 with :152-158 or :194-200):
 *     mst_gemm_nt(ff1)              a  = dropout(relu(x W1^T + b1))       — written (the backward pass needs it), never re-read
 *     mst_gemm_nt_ln(ff2, ln) mode 1 h2 = epi(a W2^T + b2), y = LayerNorm(h2), mean, rstd
 * with identical results (same MFMA order per output element, same epilogues). ff2->A must be ff1->C; the model width
 * (ff1 K = ff2 N) is 128 or 256 and divides the hidden width; no remaps, gates or row-indexed adds. */
int mst_ffn_ln_fwd(const mst_gemm_args* ff1, const mst_gemm_args* ff2, const mst_ln_args* ln, mst_stream_t stream);
/* The block's backward pass, same kernel skeleton (autograd of the above):
 *     mst_gemm_nt(ff2_dgrad)               d(pre) = ((dff W2) * alpha) gated by a > 0     — written (the weight-gradient launch reads it)
 *     mst_gemm_nt_ln(ff1_dgrad, ln) mode 2 dx = LayerNorm-backward(d(pre) W1 + resid), masked copy, dgamma / dbeta (or partials:
 *                                          mst_gemm_nt_ln_parts(M) rows)
 * ff2_dgrad->gate is the forward's hidden activation; ff1_dgrad->A must be ff2_dgrad->C. */
int mst_ffn_ln_bwd(const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad, const mst_ln_args* ln, mst_stream_t stream);
/* The same with the layer's LEADING LayerNorm backward (the one whose output gradient the block receives: LayerNorm-2 of an
 * encoder layer, transformer.py:158) computed in the kernel's prologue instead of by an mst_layernorm_bwd launch in front:
 * dx = LayerNorm-backward(dy; x, mean, rstd, gamma) on the workgroup's 64 rows, dx and (mask_mode 1) its dropout-masked copy
 * stored for the residual branch / the weight gradients, the masked copy (or dx) handed to the first GEMM on chip —
 * ff2_dgrad->A must be that buffer. dgamma / dbeta as in mst_gemm_nt_ln (partials: mst_gemm_nt_ln_parts(M) rows). */
typedef struct mst_ln_bwd_in {
  const void* dy; int64_t ld_dy;
  const void* x;  int64_t ld_x;
  const float* gamma; const float* mean; const float* rstd;
  void* dx; int64_t ld_dx;
  void* dx_masked; int64_t ld_dxm;
  float* dgamma; float* dbeta; float* partials;
  int32_t mask_mode;     /* 0 or 1 */
  float dropout_p; uint64_t dropout_seed; const uint64_t* dropout_seed_ptr; uint32_t dropout_site;
} mst_ln_bwd_in;
int mst_ffn_ln_bwd_lead(const mst_ln_bwd_in* lead, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                        const mst_ln_args* ln, mst_stream_t stream);
/* mst_ffn_ln_bwd_lead with the gradient it starts from computed in the launch too (ABI 116): the K | Q | V input gradient of the encoder
 * layer ABOVE (MultiHeadDotAttention's three input Dense layers, transformer.py:57-64, backward) —
 *     mst_gemm_nt(kqv_dgrad)               dy = d(qkv) W_kqv + d(h1 of the layer above)   [M, width], K = 3 width, residual
 *     mst_ffn_ln_bwd_lead(lead, ...)       with lead->dy = that result
 * as ONE launch where mst_kqv_ffn_ln_bwd_form says so: the workgroup that owns a 64-row tile computes its dy tile first, with
 * mst_gemm_nt's arithmetic (same MFMA order per element, the residual added in fp32, one rounding), and every tensor the two launches
 * store comes out bit for bit. kqv_dgrad->C (= lead->dy, which is not read) is OPTIONAL there: NULL, the gradient is never stored;
 * set, it receives dy. Every other valid shape runs exactly the two launches inside the call and needs kqv_dgrad->C.
 * mst_kqv_ffn_ln_bwd_form: that decision, on the host from the arguments alone (no HIP call, no device; pointers are looked at for NULL
 * and alignment only; ff2_dgrad / ff1_dgrad for M, the width and row groups). form is a host array of 1 entry:
 *   form[0]  1: one launch — width 128 or 256, N = width, K = 3 width, M and dtype the block's, a residual, no other epilogue feature
 *               of mst_gemm_nt (bias, alpha, gate, activation, dropout, row-indexed adds, remaps, fp32 C, uint8 A), no row groups on
 *               the block, A / B / residual / C 16-byte aligned with leading dimensions that are multiples of 8 and hold a row
 *            0: the two launches
 * Returns 0; a head without operands or of another M / width than the block: MST_ERR_INVALID, as the launch. */
int mst_kqv_ffn_ln_bwd(const mst_gemm_args* kqv_dgrad, const mst_ln_bwd_in* lead, const mst_gemm_args* ff2_dgrad,
                       const mst_gemm_args* ff1_dgrad, const mst_ln_args* ln, mst_stream_t stream);
int mst_kqv_ffn_ln_bwd_form(const mst_gemm_args* kqv_dgrad, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                            int64_t* form);
/* The attention output projection joins the block (MultiHeadDotAttention's W_proj Dense, transformer.py:65-68,105-106, and the
 * residual LayerNorm behind it, transformer.py:154-156 / 191-193):
 * in FRONT of mst_ffn_ln_fwd —
 *     mst_gemm_nt_ln(proj, ln1) mode 1     h1 = epi(att Wp^T + bp) (+ dropout, + residual), x1 = LayerNorm(h1), mean1, rstd1
 * with x1 (= ln1->out, which must be ff1->A) handed to the block on chip and stored, with h1 and the statistics, for backward.
 * The projection is width x width (N = K = the model width) on the same M rows. Same results as the separate launches. */
int mst_proj_ffn_ln_fwd(const mst_gemm_args* proj, const mst_ln_args* ln1, const mst_gemm_args* ff1, const mst_gemm_args* ff2,
                        const mst_ln_args* ln2, mst_stream_t stream);
/* The last decoder layer's row-wise block, the loss and their backward in ONE launch — three consecutive launches of a training
 * step whose 64-row tiles coincide, as consecutive phases of one workgroup:
 *     mst_proj_ffn_ln_fwd(proj, ln1, ff1, ff2, ln3)
 *     mst_gemm_sigmoid_bce_dgrad_ln(out, bce, out_dgrad, ln3_bwd)
 *     mst_ffn_ln_bwd(ff2_dgrad, ff1_dgrad, ln1_bwd)
 * with bit-identical results in every tensor they store (the per-sample loss sums are atomics, as there). Each phase hands its tile
 * to the next on chip. Accepted: model width 128, hidden width 512, 128 pitches, T % 64 == 0, whole 64-row tiles, row groups
 * (T, T + 1, 1) on all three parts, ln3_bwd->mask_mode 2, out->A == ln3->out, out_dgrad->A == out->C, ff2_dgrad->A == out_dgrad->C.
 * Anything else is an error (MST_ERR_INVALID before any HIP call): the caller issues the three launches. */
int mst_dec_tail_step(const mst_gemm_args* proj, const mst_ln_args* ln1, const mst_gemm_args* ff1, const mst_gemm_args* ff2,
                      const mst_ln_args* ln3, const mst_gemm_args* out, const mst_bce_args* bce, const mst_gemm_args* out_dgrad,
                      const mst_ln_args* ln3_bwd, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                      const mst_ln_args* ln1_bwd, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * Deferred column sums: dst[0..len) += scale * sum_{p < n_parts} src[p*stride + 0..len), parts added in index order
 * (deterministic). The LayerNorm-backward launches leave per-workgroup partial sums of dgamma / dbeta (`partials`
 * above and in mst_layernorm_bwd); one launch of this adds all of a backward pass's sites into the gradient bucket.
 * len % 4 == 0, stride % 4 == 0, src and dst 16-byte aligned; up to 20 jobs (host array) per launch.
 * ------------------------------------------------------------------------ */
typedef struct mst_partial_sum {
  const float* src; int64_t n_parts; int64_t stride; int64_t len;
  float* dst; float scale;
} mst_partial_sum;
int mst_partial_sums(const mst_partial_sum* jobs, int n, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * Weight gradient: dW[N,K] (+)= sum_m A[m,n] * B[m,k]   (A = dY [M,N], B = X [M,K])
 * plus optional bias gradient db[n] += sum_m A[m,n].
 * Autograd counterpart of the Dense call sites above (trainer.py:176).
 * dW, db are fp32 and are ACCUMULATED INTO (callers zero the flat gradient
 * bucket once per step); ldw in elements. lda, ldb multiples of 8 and >= roundup8(N) / roundup8(K)
 * (pad columns must hold zeros).
 * Row remaps as in mst_gemm_args apply to A (a_*) and B (b_*).
 * beta_scale multiplies the contribution (sqrt(D) for embedding-side GEMMs).
 * ------------------------------------------------------------------------ */
typedef struct mst_wgrad_args {
  int32_t dtype;
  int64_t M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  float* dW; int64_t ldw;
  float* db;
  float scale;
  int64_t a_rows_per_group, a_group_stride, a_group_offset;
  int64_t b_rows_per_group, b_group_stride, b_group_offset;
  int32_t a_u8; /* 1: A is uint8 [M, lda bytes] (the embedding tables' gradient contracts the piano-roll frames), widened on
                 * the way into LDS; lda % 8 == 0 */
} mst_wgrad_args;

/* Deferred batch outer products: out[j, i] += sum_b L[b, j] * R[b, i] (out fp32 [J, I] contiguous, accumulated into) and, with
 * obias, obias[j] += sum_b L[b, j]. L fp32 [B, J] contiguous; R [B, >= I] of r_dtype (MST_F32 / MST_BF16 / MST_F16) with row stride
 * r_stride elements. The parameter gradients of a layer that sees one row per sample — the latent block's latent_proj and
 * latent2hid (model.py:97-103,229-232; computed from mst_latent_bwd_vec's `scratch`) — which nothing downstream but the optimizer
 * reads. Up to 2 jobs per call. */
typedef struct mst_outer_job {
  const float* L; const void* R; int32_t r_dtype; int64_t r_stride;
  int64_t B, J, I;
  float* out; float* obias;
} mst_outer_job;
int mst_outer_jobs(const mst_outer_job* jobs, int n, mst_stream_t stream);
/* The weight gradients of a backward pass in ONE call: up to 16 problems (host array) in one launch — one resident round of
 * workgroups, the M-split (and with it the fp32-atomic traffic) as small as it gets.
 *   scratch (optional, NULL / 0: none): a caller-owned fp32 buffer (16-byte aligned). When the batch is large enough for 256x256
 *     tiles and the buffer holds tiles * split * 256 KiB, the M-slabs' partial tiles are written there with plain stores and summed
 *     in slab order by a second launch: no fp32 atomics on dW (deterministic gradients, and 62 MB of atomic traffic less at
 *     configs[1]). 64 MiB covers configs[1].
 *   sums (optional, NULL / 0: none): up to 20 column-sum jobs (mst_partial_sum above: the LayerNorm-backward launches'
 *     per-workgroup dgamma / dbeta rows), executed by extra workgroups of the reduction pass when there is one, else by one
 *     mst_partial_sums launch after the weight gradients.
 *   outers (optional, NULL / 0: none): up to 2 outer-product jobs: extra workgroups of the reduction pass when there is one, else
 *     one mst_outer_jobs launch after the weight gradients. */
int mst_gemm_wgrad_batch_flush(const mst_wgrad_args* list, int n, float* scratch, int64_t scratch_bytes,
                               const mst_partial_sum* sums, int n_sums, const mst_outer_job* outers, int n_outers,
                               mst_stream_t stream);
/* The decoder class table's gradient, dcls[classes[b], j] += tvec[b, j] (b < B in batch order, j < Dd), as a launch of its own:
 * classes int32 [B], tvec fp32 [B, Dd] contiguous (scratch[0 .. B*Dd) of mst_latent_bwd_vec), dcls fp32 [n_classes, ld_cls >= Dd],
 * accumulated into. No atomics: a 256-thread workgroup owns 64 columns, its four waves take a quarter of the batch each and the
 * quarters are added in order. What mst_latent_bwd_vec launches behind its own kernel when it is given dcls_d. */
int mst_class_table_grad(const int32_t* classes, const float* tvec, float* dcls, int64_t ld_cls, int64_t B, int64_t Dd,
                         mst_stream_t stream);
/* mst_gemm_wgrad_batch_flush (ABI 115) with that class-table job taken along, for a caller that passed mst_latent_bwd_vec no table
 * (dcls_d NULL): nothing but the optimizer reads the table's gradient, so it need not be a launch inside the backward pass's dependent
 * chain. cls_classes, cls_tvec, cls_dcls, cls_ld, cls_B, cls_Dd: mst_class_table_grad's arguments (all NULL / 0: no job, and the
 * call is mst_gemm_wgrad_batch_flush). With a reduction pass, cdiv(cls_Dd, 64) more workgroups of it run the job behind the
 * column-sum and outer-product jobs; else it is one mst_class_table_grad launch after the weight gradients (and after the sums' and
 * outers' launches). Either way the same workgroups in the same order: bit-identical to the launch. mst_gemm_wgrad_plan's plan[3]
 * bit 0 says which. The job is validated before any HIP call. */
int mst_gemm_wgrad_batch_flush_cls(const mst_wgrad_args* list, int n, float* scratch, int64_t scratch_bytes,
                                   const mst_partial_sum* sums, int n_sums, const mst_outer_job* outers, int n_outers,
                                   const int32_t* cls_classes, const float* cls_tvec, float* cls_dcls, int64_t cls_ld,
                                   int64_t cls_B, int64_t cls_Dd, mst_stream_t stream);
/* What mst_gemm_wgrad_batch_flush(list, n, scratch, scratch_bytes, ...) launches, decided on the host from the arguments alone (no
 * HIP call, no device needed; the pointers are looked at for NULL and alignment only, and a scratch buffer is present when
 * scratch_bytes > 0). The flush calls the same decision and nothing else. plan is a host array of 4 + 16 entries:
 *   plan[0]      tile form of the launch, by the batch's total output size (sum of N * K):
 *                0  64 x 64 tiles       (fewer than 393,216 outputs)
 *                1  128 x 128 tiles     (fewer than 1,179,648)
 *                2  256 x 128 tiles     (fewer than 1,572,864)
 *                3  256 x 256 tiles
 *   plan[1]      narrow mask: bit p set when problem p (K <= 128) runs the 256 x 128 body inside form 3
 *   plan[2]      work items (tiles x M slabs over all problems) of the main launch
 *   plan[3]      bit 0: the tiles go through the scratch buffer and the reduction pass (form 3, scratch_bytes >= items * 256 KiB);
 *                bit 1: the bias rows too (1 KiB more per item); 0: fp32 atomics
 *   plan[4 + p]  M split of problem p: its rows go to that many slabs of roundup64(ceil(M / split)) rows (0 for p >= n)
 * Returns 0. Invalid arguments: what the flush returns for them (MST_ERR_INVALID, or MST_ERR_UNSUPPORTED for the dtype), same
 * message. */
int mst_gemm_wgrad_plan(const mst_wgrad_args* list, int n, int64_t scratch_bytes, int64_t* plan);

/* ------------------------------------------------------------------------
 * K1/K2: token path input. out[b, s_off + t, :] = alpha*(table[tok[b,t]] + cls[classes[b]]) + pos[s_off+t]
 * (model.py:86-91, transformer.py:270; decoder: model.py:241-245 with cls = NULL, s_off = 1).
 * Also emits keymask[b, s_off + t] = (tok != 0) if keymask != NULL (model.py:81-83).
 * table, cls, pos fp32; tokens/classes int32; out act dtype [B, S_out, ld].
 * keep (uint8 [B * T] or NULL; ABI 118): the decoder-input dropout mask of mst_step_begin_args.in_keep. Position (b, t) with
 * keep[b * T + t] == 0 takes a zero row in place of table[tok] (the table row is not read): out = alpha*(0 + cls) + pos. keymask is
 * emitted from the token as before. NULL: the launch as it was.
 * ------------------------------------------------------------------------ */
int mst_embed_fwd(int dtype, int64_t B, int64_t T, int64_t D,
                  const int32_t* tokens, const float* table, int64_t ldt,
                  const int32_t* classes, const float* cls_table, int64_t ldc,
                  const float* pos, int64_t ldp, float alpha,
                  void* out, int64_t ld_out, int64_t S_out, int64_t s_off,
                  uint8_t* keymask, const uint8_t* keep, mst_stream_t stream);

/* scatter-add of alpha*dX rows into dtable (fp32, accumulated) and dcls (fp32, accumulated). keep (as above, or NULL): a dropped
 * position adds nothing to dtable; dcls gets every row either way. With dcls the column sums are mst_group_colsum's, and its
 * checks (D a multiple of 8, ...) are made with this call's own before the first launch: a refused call adds nothing anywhere.
 * The sums are fp32 atomics in no fixed order: equal calls may differ in the last bits. */
int mst_embed_bwd(int dtype, int64_t B, int64_t T, int64_t D,
                  const int32_t* tokens, float* dtable, int64_t ldt,
                  const int32_t* classes, float* dcls, int64_t ldc, float alpha,
                  const void* dX, int64_t ld_dx, int64_t S_out, int64_t s_off,
                  const uint8_t* keep, mst_stream_t stream);

/* dst[idx[b], :] += alpha * sum_{t<T} X[b, s_off+t, :]  (fp32 dst, accumulated): gradient of the class
 * embedding that the piano-roll input GEMM's epilogue added to every frame (model.py:89-91) */
int mst_group_colsum(int dtype, int64_t B, int64_t T, int64_t D, const void* X, int64_t ldx,
                     int64_t S_out, int64_t s_off, const int32_t* idx, float* dst, int64_t ldd,
                     float alpha, mst_stream_t stream);

/* The thread map and launch of mst_group_colsum for T frames of width D (ABI 121; also mst_embed_bwd's dcls part): no launch, no
 * HIP call, `form` is 4 int64. A workgroup of 256 threads takes 64 frames of one sample; a thread owns one 16-byte chunk (8 columns)
 * of every RG-th frame.
 *   form[0]  cpr = D / 8: chunks per row        form[1]  RG = 256 / cpr: row groups (threads cpr * RG .. 255 idle)
 *   form[2]  grid.x = ceil(T / 64) (grid.y = B)  form[3]  dynamic LDS bytes, 4 * RG * D
 * Returns 0; T, D refused as mst_group_colsum refuses them (MST_ERR_INVALID, same message). */
int mst_group_colsum_form(int64_t T, int64_t D, int64_t* form);

/* key-validity mask from lengths: keymask[b,s] = s < lens[b] + add (model.py:246-247 SequenceMask) */
int mst_mask_from_lengths(int64_t B, int64_t S, const int32_t* lens, int32_t add,
                          uint8_t* keymask, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K4/K11: MultiHeadDotAttention with the reference's key-row softmax
 * (transformer.py:85-126): logits[k,q] = K[k]·Q[q]/sqrt(dh) + (keymask[k] ? 0 : -1e9),
 * P = softmax over q, O[q] = sum_k P[k,q] V[k].
 *   qkv   : act dtype [B*S, ld_qkv]; K at column k_off + h*dh, Q at q_off + h*dh, V at v_off + h*dh
 *   lse   : fp32 [2, B, H, S] softmax row statistics (written by fwd, read by bwd): plane 0 = row max,
 *           plane 1 = log(row sum). Kept apart because a padded key row has max -1e9, where a single
 *           fp32 logsumexp would round log(S) away.
 *   out   : act dtype [B*S, ld_out], head h at column h*dh
 * dh in {16, 32, 64}.
 * ------------------------------------------------------------------------ */
int mst_attn_keysoftmax_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh,
                            const void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                            const uint8_t* keymask, float* lse,
                            void* out, int64_t ld_out,
                            int64_t q_limit /* produce only queries [0, q_limit); <= 0 or >= S: all. The row statistics
                                               always cover every query (they normalise over the query axis) */,
                            mst_stream_t stream);

/* dqkv has the same layout as qkv; delta is fp32 scratch [B, H, S]. */
/* The layer's K | Q | V projection AND its attention in one call (transformer.py:88-104): qkv = x W^T + bias with
 * W [3 D, ld_w] (row c = output column c of the qkv layout, D = H * dh) and bias fp32 [3 D] is computed, written to `qkv`
 * (the backward pass reads it) and attended to as mst_attn_keysoftmax_fwd does. For head size 32 and sequences that take the
 * resident attention kernel the projection runs INSIDE the attention launch — every (batch, head) workgroup forms its own
 * [S, 3 * 32] tile of the product — which saves a launch and the re-read of qkv; other shapes run mst_gemm_nt followed by
 * mst_attn_keysoftmax_fwd. Same results either way up to the summation order of the fp32 accumulation. */
int mst_attn_qkv_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* x, int64_t ld_x, const void* w,
                     int64_t ld_w, const float* bias, void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                     const uint8_t* keymask, float* lse, void* out, int64_t ld_out, int64_t q_limit, mst_stream_t stream);
int mst_attn_keysoftmax_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh,
                            const void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                            const uint8_t* keymask, const float* lse,
                            const void* dout, int64_t ld_dout,
                            void* dqkv, int64_t ld_dqkv, float* delta,
                            int64_t q_limit /* the caller's promise that rows [q_limit, S) of every sample of dout are ZERO
                                               (the mirror of the forward's q_limit; <= 0 or >= S: dense). With
                                               q_limit <= 32 the resident kernel skips the work that multiplies those
                                               zeros — results are bit-identical to the dense computation; the
                                               streaming kernels read dout in full, so the rows must really be zero */,
                            mst_stream_t stream);
/* The layer's W_proj INPUT GRADIENT and its attention backward in one call, the mirror of mst_attn_qkv_fwd:
 * dO = dproj wt^T with dproj [B*S, ld_dproj] the gradient behind the projection and wt [D, ld_wt] the TRANSPOSED 16-bit weights
 * (row c = column c of dO, contiguous over the contraction; D = H * dh), then mst_attn_keysoftmax_bwd on that dO (dense). Where
 * mst_attn_bwd_form reports form[7] = 1 every (batch, head) workgroup forms its own [S, dh] tile of dO INSIDE the resident launch,
 * with the arithmetic of mst_gemm_nt (same instruction, same K order, one rounding): dqkv and delta are bit-identical to the two
 * calls. dout_out (may be null there) then also receives dO, the bits mst_gemm_nt stores. Other shapes run mst_gemm_nt into
 * dout_out (required) followed by the launches of mst_attn_keysoftmax_bwd. */
int mst_attn_proj_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv, int64_t k_off,
                      int64_t q_off, int64_t v_off, const uint8_t* keymask, const float* lse, const void* dproj, int64_t ld_dproj,
                      const void* wt, int64_t ld_wt, void* dout_out, int64_t ld_dout, void* dqkv, int64_t ld_dqkv, float* delta,
                      mst_stream_t stream);

/* What mst_attn_keysoftmax_fwd (fused = 0) or mst_attn_qkv_fwd (fused = 1; ld_x and ld_w are looked at then only) launches for these
 * arguments, and what mst_attn_keysoftmax_bwd launches: decided on the host from the shape alone (and the MST_ATTN_PATH=stream
 * override), no HIP call, no device needed. The launches call the same decision and nothing else. The arguments are validated as
 * the launch validates them, pointers apart (same status, same message). form is a host array of 8 entries.
 * mst_attn_fwd_form:
 *   form[0]  path: 0  resident, Q | K | V tiles together in LDS            (one launch, one workgroup per (batch, head))
 *                  1  resident, two tiles: K and V staged over Q between the phases
 *                  2  resident, one tile: the output phase over two chunks of keys (head sizes 32 and 64, an even number of blocks)
 *                  3  resident with the K | Q | V projection inside the launch (fused = 1, head size 32, 6..16 row blocks)
 *                  4  streaming: the statistics launch, then the output launch (fused = 1 and path != 3: mst_gemm_nt comes first)
 *   form[1]  waves per workgroup (streaming: 4)
 *   form[2]  dynamic LDS bytes (streaming: 0)
 *   form[3]  1 when the last row of a 32 n + 1 sequence is handled apart (head size 16, every query produced; resident paths)
 *   form[4]  grid.x of the streaming statistics launch, ceil(S / 128) (resident: 0)
 *   form[5]  grid.x of the streaming output launch, ceil(min(q_limit, S) / 128) (resident: 0)
 * mst_attn_bwd_form:
 *   form[0]  path: 0  resident (one launch)
 *                  1  streaming dV / dK launch, then dQ by one workgroup per (batch, head) with the keys in form[5] chunks
 *                  2  streaming dV / dK launch, then the streaming dQ launch
 *   form[1]  waves per workgroup of the first launch (streaming: 4)
 *   form[2]  dynamic LDS bytes: of the resident launch (path 0), of the chunked dQ launch (path 1), else 0
 *   form[3]  1: the sparse kernels (0 < q_limit <= 32: only those rows of dout are read), 0: dense
 *   form[4]  1 when the last row of a 32 n + 1 sequence is handled apart (head size 16, dense, resident)
 *   form[5]  key chunks of the chunked dQ launch (path 1: 1, 2 or 4; else 0)
 *   form[6]  waves per workgroup of the chunked dQ launch (path 1: 8; else 0)
 *   form[7]  1 when mst_attn_proj_bwd forms dO inside the resident launch for this shape (path 0, dense, head sizes 16 and 32, a wave
 *            per 32-row owner block, D a multiple of 64, two workgroups' LDS per CU), 0 when it runs mst_gemm_nt first. That launch
 *            takes max(form[2], 144 * 32 * ceil(S / 32) + 2 * dh * (D + 8)) bytes of LDS. mst_attn_keysoftmax_bwd does not look at it
 * Entries not listed are 0. Returns 0; invalid arguments: MST_ERR_INVALID, or MST_ERR_UNSUPPORTED for the dtype. */
int mst_attn_fwd_form(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, int64_t ld_qkv, int64_t k_off, int64_t q_off,
                      int64_t v_off, int64_t ld_out, int64_t q_limit, int fused, int64_t ld_x, int64_t ld_w, int64_t* form);
int mst_attn_bwd_form(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, int64_t ld_qkv, int64_t k_off, int64_t q_off,
                      int64_t v_off, int64_t ld_dout, int64_t ld_dqkv, int64_t q_limit, int64_t* form);

/* ------------------------------------------------------------------------
 * Causal self-attention with a conventional softmax over the KEY axis (the decoder's opt-in causal mode; the
 * model mst_attn_decode mode 1 samples from). Per (batch b, head h), with keymask[b,k] the decoder's mask:
 *   logit[q,k] = Q[q]·K[k]/sqrt(dh) for k <= q and keymask[b,k], excluded (probability exactly 0) otherwise;
 *   P[q,:] = softmax over k; O[q] = sum_k P[q,k] V[k].
 * Same layouts as mst_attn_keysoftmax_fwd/bwd: lse fp32 [2, B, H, S] now holds per-QUERY statistics (plane 0 =
 * row max, plane 1 = log row sum of the non-excluded logits); the backward writes delta fp32 [B, H, S] =
 * rowsum(dO * O) and dQ | dK | dV into dqkv (the qkv layout). Key blocks above the diagonal are skipped,
 * nothing S x S reaches HBM, no atomics: identical calls give identical bits. dh in {16, 32, 64}; qkv, out,
 * dout and dqkv 16-byte aligned with leading dimensions that are multiples of 8.
 * A query without an admissible key (key 0 masked, or every key up to it) gets out = 0, lse = -inf in both planes
 * and delta = 0, and contributes to no gradient: its dQ row is 0 (a contract, held by tests/causal_refs.py).
 * ------------------------------------------------------------------------ */
int mst_attn_causal_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh,
                        const void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                        const uint8_t* keymask, float* lse, void* out, int64_t ld_out, mst_stream_t stream);
int mst_attn_causal_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh,
                        const void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                        const uint8_t* keymask, const float* lse, const void* dout, int64_t ld_dout,
                        void* dqkv, int64_t ld_dqkv, float* delta, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K6: y = LayerNorm(x) * gamma + beta over the last axis (eps, biased variance;
 * gluon.nn.LayerNorm at transformer.py:142,147,175,180). The residual add is fused
 * into the producing GEMM's epilogue, so x is the pre-norm sum.
 *   x, y : act dtype [M, ld]; mean, rstd : fp32 [M] (saved for backward)
 * bwd: dx (act dtype) and dgamma/dbeta (fp32, ACCUMULATED INTO). The gradient arriving through the
 *   residual branch is added by the consuming dgrad GEMM's `resid` epilogue, not here.
 *   mask_mode 0: dx only. 1: also dx_masked = dx * keep/(1-p), the gradient of the dropped-out
 *   GEMM output feeding this norm (transformer.py:155,158,197). 2: dx <- dx * (1 + keep/(1-p)),
 *   the decoder's LN3(ff + dropout(ff)) (transformer.py:200). The keep mask is regenerated from
 *   (dropout_seed, dropout_site, m*D + d), the same counter RNG the forward GEMM epilogue used.
 * ------------------------------------------------------------------------ */
int mst_layernorm_fwd(int dtype, int64_t M, int64_t D, const void* x, int64_t ldx,
                      const float* gamma, const float* beta, float eps,
                      void* y, int64_t ldy, float* mean, float* rstd,
                      int64_t row_id_stride /* statistics of row m are stored at index m*row_id_stride (1 = dense) */,
                      mst_stream_t stream);

int mst_layernorm_bwd(int dtype, int64_t M, int64_t D, const void* x, int64_t ldx,
                      const float* gamma, const float* mean, const float* rstd,
                      const void* dy, int64_t ldy, void* dx, int64_t ld_dx,
                      void* dx_masked, int64_t ld_dxm, float* dgamma, float* dbeta,
                      int mask_mode, float dropout_p, uint64_t dropout_seed, uint32_t dropout_site,
                      const uint64_t* dropout_seed_ptr,
                      int64_t row_id_stride /* row m here is row m*row_id_stride of the forward (mean/rstd index and
                                               dropout counter); 1 for a dense pass */,
                      float* partials /* optional [mst_layernorm_bwd_parts(M, D)][2D] fp32: per-workgroup column sums
                                         (dgamma | dbeta) stored instead of atomics on dgamma / dbeta; add them
                                         with mst_partial_sums */,
                      mst_stream_t stream);
int64_t mst_layernorm_bwd_parts(int64_t M, int64_t D);

/* What mst_layernorm_fwd (backward = 0) or mst_layernorm_bwd (backward != 0) instantiates and launches for M rows of width D
 * (ABI 121): no launch, no HIP call, no pointer followed but `form` (5 int64). The launch and this query share one host function, so
 * they cannot disagree.
 *   form[0]  NV: 64-lane groups of 4 elements per row: 1 for D <= 256, 2 for D <= 512, 4 for D <= 1024
 *   form[1]  R: rows a wave has in flight. Forward: 2 when M > 4 grid.x (grid.x is capped at 2048, so M > 8192), else 1.
 *            Backward: 2 when NV = 1 and ceil(M / (grid.x * waves)) > 1, else 1
 *   form[2]  grid.x (backward: the rows of `partials`, what mst_layernorm_bwd_parts returns)
 *   form[3]  waves per workgroup (forward: 4; backward: min(16, 4096 / D), at least 1)
 *   form[4]  dynamic LDS bytes (forward: 0; backward: 8 * waves * D)
 * Returns 0; M, D refused as the launches refuse them (MST_ERR_INVALID, same message), MST_ERR_UNSUPPORTED for the dtype. */
int mst_layernorm_form(int backward, int dtype, int64_t M, int64_t D, int64_t* form);

/* ------------------------------------------------------------------------
 * K8/K9/K10 latent block (model.py:97-103,292,229-232; loss.py:8-12), fp32 math:
 *   fwd: h0 = enc_out[b, 0, :]                     (act dtype, row stride ld_enc*S)
 *        [mu | sigma] = h0 · Wl^T + bl              (Wl fp32 [2Z, De])
 *        z = mu + eps * sigma ; kl[b] = 0.5 * sum_z (sigma^2 + mu^2 - 1 - log(sigma^2))
 *        dec_in[b, 0, :] = alpha_d*(z · Wh^T + bh + cls_d[classes[b]]) + pos_d[0]   (Wh fp32 [Dd, Z])
 *   bwd: given d(dec_in[b,0,:]) and beta (KL weight): all parameter grads (accumulated, fp32),
 *        d(enc_out[b,0,:]) written (act dtype) into denc row 0 of each sample.
 * ------------------------------------------------------------------------ */
int mst_latent_fwd(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd,
                   const void* enc_out, int64_t enc_sample_stride,
                   const float* Wl, const float* bl, const float* eps,
                   const float* Wh, const float* bh,
                   const int32_t* classes, const float* cls_d, int64_t ld_cls,
                   const float* pos_d, float alpha_d,
                   float* mu, float* sigma, float* z, float* kl,
                   void* dec_in, int64_t dec_sample_stride, mst_stream_t stream);
/* ... and, on the same launch, the decoder's first K | Q | V projection of THAT row (transformer.py:88-93 on position 0):
 * qkv0[b * qkv_sample_stride + j] = dec_in[b, 0, :] . Wq[j, :] + bq[j], j < nq (Wq: the 16-bit weight, [nq, ld_wq]; fp32 dot products
 * over the row as stored). The other B T rows of that projection do not depend on the latent block: the step computes them as a
 * rider of the forward position-0 tail (mst_row_tail_fwd_ride). Dd must be 64, 128 or 256. */
int mst_latent_fwd_proj(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd,
                        const void* enc_out, int64_t enc_sample_stride,
                        const float* Wl, const float* bl, const float* eps,
                        const float* Wh, const float* bh,
                        const int32_t* classes, const float* cls_d, int64_t ld_cls,
                        const float* pos_d, float alpha_d,
                        float* mu, float* sigma, float* z, float* kl,
                        void* dec_in, int64_t dec_sample_stride,
                        const void* Wq, int64_t ld_wq, const float* bq, void* qkv0, int64_t qkv_sample_stride, int64_t nq,
                        mst_stream_t stream);
/* Decoder row 0 from a latent RECIPE — generation from the latent space (prior draws, posterior draws, interpolation between two
 * melodies, a blend of two class embeddings). For every output row n < N, fp32 math, one rounding to the act dtype at the store:
 *   base  = interp(zsrc[a[n]], zsrc[b[n]], w[n])                a[n] < 0 (or M = 0): base = 0, scale = 1 — a draw from the prior
 *   scale = ssrc ? (1 - w[n]) * ssrc[a[n]] + w[n] * ssrc[b[n]] : 1
 *   z     = base + tau * eps(seed, site, (row0 + n) * Z + k) * scale            (tau = 0: no random number is made)
 *   dec_in[n * dec_stride + :] = alpha_d * (z . Wh^T + bh + (1 - cw[n]) * cls_d[ca[n]] + cw[n] * cls_d[cb[n]]) + pos_d[0 .. Dd)
 *   z_out[n, :] = z
 * zsrc / ssrc: fp32 [M, Z] (the mu / sigma of an encode, or any vectors); a, b, ca, cb: int32 [N]; w, cw: fp32 [N]; z_out fp32 [N, Z].
 * mode 0: interp is linear, (1 - w) * za + w * zb. mode 1: spherical, sin((1 - w) om) / sin(om) * za + sin(w om) / sin(om) * zb with
 * om the angle between the two; w <= 0 and w >= 1 return za / zb themselves, and where either vector is zero or |cos om| >= 1 - 2^-16
 * the linear form is used (never a NaN from a vanishing sine).
 * eps: the Gaussian of mst_randn / mst_step_begin (Box-Muller over the counter hash; element g is the cosine (g even) or sine (g odd)
 * branch of pair g >> 1) at the GLOBAL element index (row0 + n) * Z + k, effective seed = seed ^ (seed_ptr ? *seed_ptr : 0): N rows in
 * one call, or in chunks that pass their first row number as row0, are the same vectors.
 * The identity recipe (a = b = n, w = cw = tau = 0 on an encode's mu, ca = the batch's classes) is mst_latent_fwd's row 0.
 * Indices are clamped into their tables (source rows to M - 1, classes to n_classes - 1): validate a recipe where it is built. */
int mst_latent_rows(int dtype, int64_t N, int64_t M, int64_t Z, int64_t Dd,
                    const float* zsrc, const float* ssrc, const int32_t* a, const int32_t* b, const float* w, int mode,
                    float tau, uint64_t seed, const uint64_t* seed_ptr, uint32_t site, int64_t row0,
                    const float* Wh, const float* bh,
                    const int32_t* ca, const int32_t* cb, const float* cw, const float* cls_d, int64_t ld_cls, int64_t n_classes,
                    const float* pos_d, float alpha_d,
                    float* z_out, void* dec_in, int64_t dec_stride, mst_stream_t stream);

/* The latent block's backward pass: the per-sample vectors, then the decoder class table's gradient (dcls_d[classes[b], :] += t[b, :]).
 * gscale is the encoder-side loss scale, enc_scale = gscale / the decoder-side loss scale. Leaves t = alpha_d * d(dec_in[b, 0, :]) at
 * scratch[0 .. B*Dd) and d[mu | sigma] at scratch[B*Dd .. B*(Dd + 2Z)) (fp32), writes d(enc_out) row 0. The remaining parameter
 * gradients are two mst_outer_job of the caller's weight-gradient flush:
 *   dWl[2Z, De] += dlat^T enc_out[:, 0, :], dbl += sum_b dlat;   dWh[Dd, Z] += t^T z, dbh += sum_b t.
 * dcls_d may be NULL (ABI 115; in all four forms): the class table's gradient is then not computed here (one launch less) and the
 * caller takes it from scratch later, as the class-table job of mst_gemm_wgrad_batch_flush_cls or by mst_class_table_grad. */
int mst_latent_bwd_vec(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd, const float* Wl, const float* eps, const float* Wh,
                       const int32_t* classes, const float* mu, const float* sigma, const void* d_dec_in, int64_t dec_sample_stride,
                       float alpha_d, float kl_weight, float gscale, float enc_scale, float* dcls_d, int64_t ld_cls,
                       void* d_enc_out, int64_t denc_sample_stride, float* scratch, mst_stream_t stream);
/* mst_latent_bwd_vec with d(dec_in[b, 0, :]) COMPUTED instead of read: dq0[b * dq_sample_stride + k] (k < nq: the gradient of the
 * decoder's first K | Q | V projection at position 0) against Wt [Dd, ld_wt >= nq] (the TRANSPOSED 16-bit weight, the operand of the
 * input-gradient GEMM) plus resid0[b * resid_sample_stride + :] (the residual branch's gradient row, may be NULL), rounded to the
 * activation type as that GEMM rounds it — whose other B T rows the step computes as a rider of the backward position-0 tail
 * (mst_row_tail_bwd_ride). nq must be 384 or 768 (decoder width 128 or 256). */
int mst_latent_bwd_vec_proj(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd, const float* Wl, const float* eps, const float* Wh,
                            const int32_t* classes, const float* mu, const float* sigma,
                            const void* dq0, int64_t dq_sample_stride, const void* Wt, int64_t ld_wt, int64_t nq,
                            const void* resid0, int64_t resid_sample_stride,
                            float alpha_d, float kl_weight, float gscale, float enc_scale, float* dcls_d, int64_t ld_cls,
                            void* d_enc_out, int64_t denc_sample_stride, float* scratch, mst_stream_t stream);

/* The scheduled forms of the two launches above: the scalar kl_weight is replaced by the device schedule block of mst_step_begin
 * (sched[0] = beta_t, sched[1] = tau, the per-sample KL allowance in nats: "free bits") and the forward pass's per-sample kl [B]:
 * the KL part of d mu / d sigma of sample b is multiplied by beta_t where kl[b] > tau (strictly) and by exactly 0.f otherwise; the
 * loss these are the gradients of is recon_b + beta_t * max(kl_b - tau, 0). The test is per SAMPLE, so a data-parallel shard computes
 * what the whole batch computes. Everything else — and, for a sample above the allowance, every bit of the result — as the
 * unscheduled launch called with kl_weight = beta_t. */
int mst_latent_bwd_vec_sched(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd, const float* Wl, const float* eps, const float* Wh,
                             const int32_t* classes, const float* mu, const float* sigma, const void* d_dec_in, int64_t dec_sample_stride,
                             float alpha_d, const float* sched, const float* kl, float gscale, float enc_scale, float* dcls_d,
                             int64_t ld_cls, void* d_enc_out, int64_t denc_sample_stride, float* scratch, mst_stream_t stream);
int mst_latent_bwd_vec_proj_sched(int dtype, int64_t B, int64_t De, int64_t Z, int64_t Dd, const float* Wl, const float* eps,
                                  const float* Wh, const int32_t* classes, const float* mu, const float* sigma,
                                  const void* dq0, int64_t dq_sample_stride, const void* Wt, int64_t ld_wt, int64_t nq,
                                  const void* resid0, int64_t resid_sample_stride,
                                  float alpha_d, const float* sched, const float* kl, float gscale, float enc_scale, float* dcls_d,
                                  int64_t ld_cls, void* d_enc_out, int64_t denc_sample_stride, float* scratch, mst_stream_t stream);

/* What the latent block's launches above take for a shape, from the two host functions the launches themselves decide with; no HIP
 * call, and Wl is looked at for its alignment only (never followed). nq: outputs of the fused projection (mst_latent_fwd_proj's nq,
 * mst_latent_bwd_vec_proj's nq), 0 for the plain launches. form: eight entries,
 *   [0] forward preloaded (1) / general (0)       [1] loader of the h0 . Wl product: 0 registers (preloaded), 1 wave_dots_pre, 2 wave_dots
 *   [2] the same for z . Wh                        [3] elements per lane of the forward projection (1, 2 or 4; 0: no projection)
 *   [4] forward dynamic LDS bytes                  [5] backward preloaded (1) / general (0)
 *   [6] dh0 path: 0 preloaded, 1 four columns per thread, 2 one column per thread                 [7] backward dynamic LDS bytes
 * The shape is validated as the launches validate it, the forward launch's checks first: same status, same message. [0 .. 4] are
 * written before the backward launch's checks run, so they are valid for a shape only the backward launch refuses (a forward
 * projection of a width the backward one does not take: form[5] stays as the caller left it). */
int mst_latent_form(int64_t De, int64_t Z, int64_t Dd, int64_t nq, const void* Wl, int64_t* form);

/* Per-dimension statistics of the posterior (ABI 120): what the logs need to tell "a few dimensions carry everything" from "every
 * dimension carries a little", and whether z separates the classes. mu, sigma: fp32 [B, ld >= Z] as mst_latent_fwd leaves them;
 * classes int32 [B]; acc: double [C][5][Z], ADDED to by every launch. Plane k of class c, dimension d, over the counted samples b
 * with classes[b] == c:
 *   0: n (the number of terms)   1: sum mu   2: sum mu^2   3: sum sigma^2   4: sum kl_d, kl_d = 0.5 * (sigma^2 + mu^2 - 1 - log(sigma^2))
 * fp64 arithmetic on the fp32 values widened (loss.py:8-12 per element, no epsilon). A (sample, dimension) term whose mu or sigma is
 * not finite, or whose sigma == 0, is in none of the five planes; neither is a sample whose class is outside [0, C) (the class is
 * compared, never used as an index). Every cell of acc is owned by one thread — (class, plane, dimension), consecutive threads on
 * consecutive dimensions — which adds its column's terms in ascending batch order from zero, then adds that sum to the cell: no
 * atomics, nothing summed across threads, so launches ordered on one stream give the same bits every time. (The terms themselves, an
 * fp64 logarithm each, are evaluated by the whole workgroup, 64 rows x 16 dimensions at a time through LDS.) Classes go four at a
 * time; C > 4 takes more passes over the batch. Grid cdiv(Z, 16), 1024 threads. */
int mst_latent_dim_stats(int64_t B, int64_t Z, int64_t C, const float* mu, int64_t ld_mu, const float* sigma, int64_t ld_sigma,
                         const int32_t* classes, double* acc, mst_stream_t stream);

/* The class-conditional MMD penalty on z and its gradient (ABI 123; the Variational Fair Autoencoder's remedy, Louizos et al.): pulls the
 * distribution of z within every class onto the pooled one, so that z itself does not tell the class (what mst_latent_dim_stats'
 * class_leak measures). For the n = B rows z_i = mu_i + eps_i * sigma_i (fp32 [B, ld_z >= Z] as mst_latent_fwd leaves them) with classes
 * c_i (int32 [B]) and the kernel k_ij = exp(-|z_i - z_j|^2 / (2 s2)):
 *   L = sum_c (n_c / n) * MMD^2(q_c, q_pooled) = sum_ij w_ij k_ij,     w_ij = [c_i == c_j] / (n * n_{c_i}) - 1 / n^2
 * n_{c_i}: the number of rows with row i's class. Classes are compared, never used as an index: any int32 value is a class and no class
 * count is needed. One class in the batch: every w_ij is exactly 0, so L and every gradient are exactly 0. (With the linear kernel
 * z_i . z_j the same weights give sum_c (n_c / n) |m_c - m|^2, the numerator of class_leak's eta^2 summed over the dimensions.)
 *   g_i = dL/dz_i = sum_j c_ij (z_j - z_i),   c_ij = 2 w_ij k_ij / s2;     dL/dmu_i = g_i,   dL/dsigma_i = g_i * eps_i
 * Arithmetic: q_ij = |z_i - z_j|^2 in fp32 by fmaf in ascending d on the fp32 differences; k_ij the fp32 exponential of -q_ij / (2 s2),
 * exactly 1 for i == j; the counts, w_ij, c_ij, the differences z_j - z_i and every sum over j in fp64, in ascending j.
 * VALUE. rows[i] = L_i = sum_j w_ij k_ij (i < B, plain stores). acc: double [3], ADDED to: with L = sum_i L_i, added by one thread in
 * ascending i (the same bits on every run), {L, 1, 0} when L is finite and {0, 0, 1} when it is not. A non-finite z is not
 * special-cased: NaN in, NaN out, as in the latent backward; only acc sorts such a launch into its third cell.
 * GRADIENT, when dlat is non-NULL (then Wl, d_enc_out and eps must be non-NULL too; all four NULL: the value alone). dlat: the fp32
 * [B, 2Z] d[mu | sigma] block mst_latent_bwd_vec* leaves at scratch + B * Dd; Wl: the fp32 [2Z, De] latent projection; eps fp32
 * [B, ld_eps >= Z]; d_enc_out: the 16-bit d(enc_out) of that launch, row i at d_enc_out + i * denc_sample_stride.
 *   dlat[i, d] += add_i[d] = (float)(coef * g_i[d]);       dlat[i, Z + d] += add_i[Z + d] = (float)(coef * g_i[d] * eps[i, d])
 *   d_enc_out[i * stride + e] = round_act(float(old) + sum_{j < 2Z} add_i[j] * Wl[j, e]),   e < De (fp32 fmaf, ascending j)
 * The latent backward is linear in dlat, so this is its own result for the summed gradient up to one more rounding to the activation
 * type; the outer-product jobs of the weight-gradient flush read dlat later and pick up dWl and dbl unchanged. coef carries the
 * caller's scaling: the gradient bucket holds sums over samples that the optimizer rescales by 1 / (global_batch * gscale), so a step
 * with objective mean_b(recon_b + beta kl_b) + lambda * L passes coef = lambda * B * gscale (the encoder-side scale).
 * One wave per row, sixteen rows per workgroup, grid cdiv(B, 16); z goes through LDS in 64 x 64 tiles. ticket: one word, zero before
 * the launch and left at zero: the workgroup that draws the last ticket adds the rows. Z at most 256 (a row's sums live in registers).
 * Before any HIP call a status for: a null pointer; B, Z or De not positive; ld_z (ld_eps) < Z; s2 not finite or not > 0; coef not
 * finite; an inconsistent NULL set among the four gradient pointers; dtype not bf16 / fp16 when the gradient runs (value only: dtype is
 * not looked at). */
int mst_class_mmd(int dtype, int64_t B, int64_t Z, int64_t De,
                  const float* z, int64_t ld_z, const float* eps, int64_t ld_eps, const int32_t* classes,
                  float s2, float coef,
                  const float* Wl, float* dlat, void* d_enc_out, int64_t denc_sample_stride,
                  double* rows, uint32_t* ticket, double* acc, mst_stream_t stream);

/* The importance-weighted bound on log p(x) from K posterior draws (ABI 122; Burda et al.):
 *   log p(x) ~= log (1/K) sum_k p(x | z_k) p(z_k) / q(z_k | x)
 * folded one draw at a time on the device, so that K decoder passes and a whole validation set need one read at the end.
 *
 * mst_iw_fold — one draw. eps, sigma, z: fp32 [B, ld >= Z] as mst_step_begin / mst_latent_fwd leave them; recon: the fp32 [B] the loss
 * launch leaves (the project's MEAN reconstruction loss of sample b); recon_scale turns that mean back into nats: T * P for the
 * piano-roll ends (padded frames count as the loss counts them), T for the token ends. state: double [B][6] =
 * {m, s, s2, sum_lw, n, n_bad}, zeroed by the caller before the first draw. The log-weight of sample b in this draw, in fp64 on the
 * fp32 inputs widened:
 *   lw = -recon_scale * recon[b] + sum_d (0.5 eps_d^2 - 0.5 z_d^2 + log|sigma_d|)
 * (log p(z) - log q(z | x) written through eps: z = mu + eps sigma, so (z - mu) / sigma = eps and the 2 pi terms cancel; sigma is a raw
 * linear output and may be negative, hence |sigma|). The sum over d: lane l of the sample's wave adds its terms d = l, l + 64, ... in
 * ascending order from zero, then the 64 partial sums go through xor butterflies of 32, 16, 8, 4, 2, 1 lanes — a fixed order.
 * Each sample is one wave, a workgroup holds four samples; lane 0 then does the online update of its sample's six cells:
 *   lw not finite (a non-finite input, sigma_d == 0, an infinite recon): a BAD draw — n_bad += 1 and no other cell changes
 *   n == 0:   m = lw, s = s2 = 1
 *   lw > m:   s = s * exp(m - lw) + 1, s2 = s2 * exp(2 (m - lw)) + 1, m = lw
 *   else:     r = exp(lw - m), s += r, s2 += r * r
 *   then      sum_lw += lw, n += 1
 * so that s = sum_k exp(lw_k - m) and s2 = sum_k exp(2 (lw_k - m)) with m the largest log-weight so far. No atomics; every cell of
 * state is owned by one lane: launches ordered on a stream give the same bits each time.
 * Checked before any HIP call: null pointers; B, Z > 0; leading dimensions >= Z; state 16-byte aligned; recon_scale finite and > 0. */
int mst_iw_fold(int64_t B, int64_t Z, const float* eps, int64_t ld_eps, const float* sigma, int64_t ld_sigma, const float* z, int64_t ld_z,
                const float* recon, double recon_scale, double* state, mst_stream_t stream);
/* mst_iw_finish — the bound from the folded state. out: double [B][4] =
 *   {log_px = m + log(s) - log(n),  elbo = sum_lw / n,  ess = s^2 / s2,  n}
 * A sample with n == 0 or n_bad > 0 is INVALID: its out row is NaN except the n entry. acc: double [6], ADDED to —
 *   {sum log_px, sum elbo, sum ess, sum n, pieces counted, pieces invalid}
 * over the valid samples (an invalid one adds 1 to acc[5] only), in ascending sample order, by one thread: a validation set
 * accumulates on the device and is read once. One workgroup; plain stores. log_px >= elbo (Jensen) and 1 <= ess <= n up to rounding. */
int mst_iw_finish(int64_t B, const double* state, double* out, double* acc, mst_stream_t stream);

/* standalone reparameterisation + KL (loss.VariationalKLLoss, loss.py:4-12; model.py:292) */
int mst_reparam_kl_fwd(int64_t B, int64_t Z, const float* mu, const float* sigma, const float* eps,
                       float* z, float* kl, mst_stream_t stream);
int mst_reparam_kl_bwd(int64_t B, int64_t Z, const float* mu, const float* sigma, const float* eps,
                       const float* dz, float kl_weight, float* dmu, float* dsigma, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * The position-0 tail of the top encoder layer in one launch (the model reads the encoder at position 0 only, model.py:97):
 *   h1 = resid + dropout(att Wp^T + bp);  x1 = LN1(h1);  a = dropout(relu(x1 W1^T + b1));  h2 = x1 + dropout(a W2^T + b2);
 *   x2 = LN2(h2)                                            (transformer.py:42-46,154-158 on B rows, B <= 64, D = 128 | 256)
 * = mst_gemm_nt (+resid) · mst_layernorm_fwd · mst_gemm_nt (ReLU) · mst_gemm_nt (+resid) · mst_layernorm_fwd on those rows,
 * same rounding points and dropout counters (sites site0, site0+1, site0+2; counter row = row * phys_stride), as D / 16
 * workgroups that own output-column slices and meet at three grid barriers. Row r of every tensor sits at element offset
 * r * (its row stride); statistics at index r * stat_stride. `sync`: THREE zeroed device words (mst_step_begin's zero list): barrier counter, claimed XCD, roles handed out — the launch oversubscribes the grid and keeps the workgroups of one XCD (one L2).
 * ------------------------------------------------------------------------ */
typedef struct mst_row_tail_args {
  int32_t dtype;
  int64_t B, D;
  const void* att; int64_t rs_att;
  const void* resid; int64_t rs_res;
  const void* Wp; int64_t ldwp; const float* bp;
  const float* g1; const float* be1;
  const void* W1; int64_t ldw1; const float* b1;
  const void* W2; int64_t ldw2; const float* b2;
  const float* g2; const float* be2;
  void* h1; void* x1; void* h2; void* x2; int64_t rs_d;
  void* a; int64_t rs_a;
  float* mean1; float* rstd1; float* mean2; float* rstd2; int64_t stat_stride;
  float eps;
  float dropout_p; uint64_t dropout_seed; const uint64_t* dropout_seed_ptr; uint32_t site0;
  int64_t phys_stride;
  uint32_t* sync;    /* THREE zeroed device words: [0] barrier counter (3 * D/16 after a complete launch), [1] claimed XCD + 1, [2] roles */
  uint32_t* status;  /* optional sticky device word: MST_TAIL_* flags are OR-ed into it when the launch could not do its work */
} mst_row_tail_args;
int mst_row_tail_fwd(const mst_row_tail_args* args, mst_stream_t stream);
/* RIDERS: the chain above keeps ONE XCD busy for ~26 us while seven idle. mst_row_tail_*_ride launch the same kernel with enough
 * workgroups for every CU; those that land on another XCD than the chain's compute the 128 x 128 tiles of `rider` — ONE
 * mst_gemm_nt problem that nothing in the chain reads (M, N multiples of 128, K of 64; 16-bit C; bias, alpha, a residual and
 * row remaps in whole tiles only) — from a work queue (`queue`: ONE zeroed device word, in another cache line than `sync`);
 * the chain's own workgroups pass by the queue when they are done, so every tile is computed by the end of the launch wherever
 * the workgroups land. The training step rides the decoder's K | Q | V projection of rows 1..T (transformer.py:88-93; its input
 * rows exist since the step's first launch) on the forward tail and that projection's input gradient on the backward tail:
 * two launches (12 + 10 us) less in the step's dependent chain. Same results as mst_gemm_nt, bit for bit. */
int mst_row_tail_fwd_ride(const mst_row_tail_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream);
/* ... with the step's transposed-shadow refresh (mst_transpose_shadows' list, in the tail's activation type) BEHIND the rider's tiles in
 * the same queue, sixteen 32 x 32 tiles per ticket: the 16-bit transposed copies that only the backward pass reads (nothing in this launch
 * does) are rebuilt on compute units that idle until the chain ends, instead of 4.9 us on the step's first launch
 * (mst_step_begin_args.sh_*). The weights they are built from must be final (the previous step's optimizer launch precedes). */
int mst_row_tail_fwd_ride_shadows(const mst_row_tail_args* args, const mst_gemm_args* rider, uint32_t* queue, int sh_dtype,
                                  const float* sh_w, void* sh_wt16, const int64_t* sh_desc, const int64_t* sh_prefix, int64_t sh_n_mat,
                                  int64_t sh_tiles, mst_stream_t stream);
/* The same rows on the way back: autograd of mst_row_tail_fwd's chain for the gradient `dy` of the layer's output rows —
 *     mst_layernorm_bwd (LayerNorm-2; dh, its dropout-masked copy dhm, dgamma2 / dbeta2 +=)
 *  -> mst_gemm_nt(dhm, W2t, gate = a, alpha = 1 / (1 - p))   d(pre)                 [B, 4 D]
 *  -> mst_gemm_nt(d(pre), W1t, resid = dh)                   dx1
 *  -> mst_layernorm_bwd (LayerNorm-1; dh1 rows, masked copy dh1m, dgamma1 / dbeta1 +=)
 *  -> mst_gemm_nt(dh1m, Wpt)                                 datt rows
 * in one launch (same results to rounding of the LayerNorm sums). W2t [4 D, D], W1t [D, 4 D], Wpt [D, D]: the transposed
 * 16-bit weights (K-contiguous dgrad operands). dh / dhm / dx1 / dh1m: compact [B, >= D] scratch rows (row stride rs_c);
 * dh1 / datt: rows of the strided full-size buffers the following launches read. `sync`: three zeroed device words (as above). */
typedef struct mst_row_tail_bwd_args {
  int32_t dtype;
  int64_t B, D;
  const void* dy; int64_t rs_dy;
  const void* h2; const void* h1; int64_t rs_d;
  const void* a; int64_t rs_a;
  const float* mean1; const float* rstd1; const float* mean2; const float* rstd2; int64_t stat_stride;
  const float* g1; const float* g2;
  const void* W2t; int64_t ldw2t;
  const void* W1t; int64_t ldw1t;
  const void* Wpt; int64_t ldwpt;
  void* dh; void* dhm; void* dx1; void* dh1m; int64_t rs_c;
  void* dpre; int64_t rs_dpre;
  void* dh1; int64_t rs_dh1;
  void* datt; int64_t rs_datt;
  float* dg1; float* db1; float* dg2; float* db2;
  float dropout_p; uint64_t dropout_seed; const uint64_t* dropout_seed_ptr; uint32_t site0;
  int64_t phys_stride;
  uint32_t* sync;    /* three zeroed device words, as above ([0] ends at 2 * D/16) */
  uint32_t* status;  /* optional, as above */
} mst_row_tail_bwd_args;
int mst_row_tail_bwd(const mst_row_tail_bwd_args* args, mst_stream_t stream);
int mst_row_tail_bwd_ride(const mst_row_tail_bwd_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream);
/* What the five tail launches above take for a width and a rider, from the host functions the launches themselves decide with; no
 * HIP call, no pointer of `rider` is followed (they are looked at for null and alignment, as the launch does). backward: 0 the
 * forward tail, 1 the backward one; rider: NULL for the plain launches; sh_tiles: the shadow list's 32 x 32 tiles behind the rider
 * (mst_row_tail_fwd_ride_shadows' sh_tiles; 0: none; forward with a rider only). form: six entries,
 *   [0] kernel index: (D == 256 ? 0 : 1) + (no rider 0, 128-row rider tiles 2, 256-row rider tiles 4)
 *   [1] rider tile rows: 0 (no rider), 128, or 256 (more than 208 tiles of 128 rows, M and the row-remap groups multiples of 256)
 *   [2] rider tiles of that height        [3] workgroups launched (D / 16 of them on one XCD run the chain)
 *   [4] dynamic LDS bytes                 [5] shadow tickets (sixteen tiles each) queued behind the rider's tiles
 * D, the activation type and the rider are validated as the launches validate them: same status, same message. */
int mst_row_tail_form(int backward, int dtype, int64_t D, const mst_gemm_args* rider, int64_t sh_tiles, int64_t* form);

/* ------------------------------------------------------------------------
 * Incremental decode (inference; model.py:259-272, transformer.py:70-77,242-249): the new position's query against the
 * K | Q | V rows cached so far. cache: act dtype [B, t_max, ld] with the training layout (k_off / q_off / v_off, head h at
 * columns h*dh); the new row is row n_keys - 1 and is already cached. out: act dtype [B, ld_out].
 *   mode 0: the reference's arithmetic — softmax over the QUERY axis, which holds the one new query: P = 1, out = sum of
 *           the cached value rows;   mode 1: softmax over the cached keys.
 * ------------------------------------------------------------------------ */
int mst_attn_decode(int dtype, int64_t B, int64_t H, int64_t dh, int64_t n_keys, int64_t t_max, const void* cache,
                    int64_t ld, int64_t k_off, int64_t q_off, int64_t v_off, int mode, void* out, int64_t ld_out,
                    mst_stream_t stream);

/* ------------------------------------------------------------------------
 * Beam search on the device (sampler.py:198-257, token ends), one position per call pair — capturable with the decode step.
 * mst_beam_step: B samples x K hypotheses (K <= 16); probs fp32 [B*K, ldp] = the decoder's distribution of position i; a
 *   hypothesis whose last token (seqs_in[., i-1]) is EOS — or PAD from position 2 on — is finished and continues with PAD only,
 *   at no cost (sampler.py:218-221); every other continuation costs -log max(p, 1e-30). Per sample the K candidates with the
 *   smallest (score, hypothesis * V + word) are kept: new hypothesis r of sample b gets scores_out, its source hypothesis in
 *   hyp_src (a row index into the B*K hypotheses), its word in word[] (int32, the next position's input) and its token row
 *   seqs_out[., 0..i] (int32 rows of L). active[i] (optional, zeroed by the caller) += hypotheses still running after position i.
 * mst_beam_gather: out[j, r, :] = in[src[j], r, :] for r < n_rows — the K | Q | V cache rows ([N, t_max, row_bytes]) of the
 *   re-ranked hypotheses (sampler.py:236-238); in and out are distinct buffers (the decode plan alternates between two).
 * ------------------------------------------------------------------------ */
int mst_beam_step(int64_t B, int64_t K, int64_t V, int64_t i, int64_t L, const float* probs, int64_t ldp, const float* scores_in,
                  float* scores_out, const int32_t* seqs_in, int32_t* seqs_out, int32_t* hyp_src, int32_t* word, int32_t* active,
                  int32_t eos, int32_t pad, mst_stream_t stream);
int mst_beam_gather(const void* in, void* out, const int32_t* src, int64_t N, int64_t n_rows, int64_t row_bytes, int64_t t_max,
                    mst_stream_t stream);
/* ... the same with bytes [skip_begin, skip_begin + skip_bytes) of every row left alone (whole 16-byte pieces): the Q third of the
 * cache rows, which no later position reads (a decode step takes its query from the newest row only) — a third less traffic. */
int mst_beam_gather_cols(const void* in, void* out, const int32_t* src, int64_t N, int64_t n_rows, int64_t row_bytes, int64_t t_max,
                         int64_t skip_begin, int64_t skip_bytes, mst_stream_t stream);
/* Ancestral sampling on the device (sampler.py:155-190): every sequence n of N draws token i from probs[n, :V] (fp32, need not be
 * normalised) by inverse CDF with u = counter hash of (seed, i, n); written to seqs[n, i] (int32 rows of L) and word[n] (the next
 * position's input); scores[n] += -log p; a finished sequence (EOS, or PAD from position 2 on) continues with PAD at no cost;
 * active[i] (optional, zeroed by the caller) += sequences still running. Capturable: the draw depends on device data and on the
 * host constants (seed, i) only. */
int mst_sample_step(int64_t N, int64_t V, int64_t i, int64_t L, const float* probs, int64_t ldp, int32_t* seqs, float* scores,
                    int32_t* word, int32_t* active, uint64_t seed, int32_t eos, int32_t pad, mst_stream_t stream);
/* The same for the piano-roll ends: position i's frame of every sequence n of N from the position's LOGITS (act dtype, [N, ldl >= P]),
 * with x = logit / tau and p = sigmoid(x) in fp32.
 *   mode 0 (draw)     : frame[n, j] = u < p, u = (counter hash of (*seed_ptr, i, n * P + j) >> 8) * 2^-24 in [0, 1)
 *   mode 1 (threshold): frame[n, j] = x > log(thr / (1 - thr)), thr in (0, 1) — no random number; thr = 0.5 is logit > 0
 * frame -> frames[n, :P] (uint8 rows of ldf: the next position's input; columns >= P are not touched) and roll[n, i - 1, :P] (uint8
 * [N, L, ldr]: the piece stays on the device); scores[n] += -sum_j log max(frame ? p : 1 - p, 1e-30); probs_out (optional, fp32
 * [N, L, P]) gets p at [n, i - 1, :]. 1 <= i < L. The seed is read through a device pointer (one 8-byte word the host rewrites
 * between runs), so a graph captured with this launch replays unchanged for every seed; tau, mode and thr are launch constants. */
int mst_frame_step(int dtype, int64_t N, int64_t P, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int mode, float thr,
                   const uint64_t* seed_ptr, uint8_t* frames, int64_t ldf, uint8_t* roll, int64_t ldr, float* scores, float* probs_out,
                   mst_stream_t stream);
/* The token ends' draw with a temperature, a top-k and a nucleus (top-p) cut, from the position's LOGITS (act dtype, [N, ldl >= V]:
 * DecodePlan.logits) — mst_frame_step's counterpart, one launch per position, capturable: the seed is a device word. Per sequence,
 * over columns 0..V-1:
 *   x_j = logit_j / tau (fp32); s = softmax(x) is the sampling distribution, p = softmax(logit) the model's own. x is non-decreasing
 *   in the stored 16-bit logit, so every cut is a cut on the stored value (as an order-preserving 16-bit integer key):
 *   top-k : c_k = the k-th largest stored logit with multiplicity; logit_j >= c_k survives (tie groups at the cut survive whole: the
 *           kept set is a function of the values, never of the column order); top_k = 0 or >= V keeps everything;
 *   top-p : among the survivors, mass measured by s: c_p = the largest stored value c with mass{logit_j >= c} >= top_p *
 *           mass{survivors}; logit_j >= c_p is kept — the smallest set of most likely tokens, in whole tie groups, that reaches
 *           top_p (the arg-max group always); top_p = 1 is off;
 *   draw  : inverse CDF over the kept tokens in column order, u = ((counter hash of (*seed_ptr, i, n) >> 8) + 1) * 2^-24 times the
 *           kept mass (mst_sample_step's rule); if rounding leaves no owner the LAST KEPT token takes the draw, never one outside.
 * Bookkeeping is mst_sample_step's: a finished sequence (seqs[n, i-1] EOS, or PAD from position 2 on) gets PAD at no cost; otherwise
 * seqs[n, i] = word[n] = token and scores[n] += -log max(p_token, 1e-30) — the MODEL's probability, unfiltered at temperature 1, so
 * the scores of every decoder are the same quantity; active[i] (optional) += running sequences; kept_out[n] (optional, int32 [N]) =
 * the number of kept tokens (finished sequences too). tau > 0 finite; top_k >= 0; 0 < top_p <= 1; 1 <= i < L; all launch constants. */
int mst_token_step(int dtype, int64_t N, int64_t V, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int32_t top_k,
                   float top_p, const uint64_t* seed_ptr, int32_t* seqs, float* scores, int32_t* word, int32_t* active,
                   int32_t* kept_out, int32_t eos, int32_t pad, mst_stream_t stream);
/* Constrained decoding: the two draws above with some cells GIVEN. The decoder is fed a held cell as if it had drawn it, and only the
 * free cells are drawn; the held cells' -log p is kept apart from the drawn cells', in held_scores (fp32 [N], ADDED to: the caller
 * zeroes it before a piece). Same launch shape (one wave per sequence, no atomics on the sums, a fixed order), capturable: the mask
 * and the piece are device data, so one captured graph serves every mask and piece.
 *
 * mst_frame_step_held: given and hold are uint8 [N, L, ldg] / [N, L, ldh] in the roll's indexing — row (n, i - 1) belongs to
 *   position i, columns >= P are never read. Cell (n, j) is held where hold != 0; its frame is given != 0, stored as 0 or 1. A free
 *   cell is mst_frame_step's, random number (*seed_ptr, i, n * P + j) included: what it draws does not depend on which other cells
 *   are held. frames, roll and probs_out are written for every cell as above; scores[n] += the sum over the FREE cells,
 *   held_scores[n] += -sum over the HELD cells of log max(frame ? p : 1 - p, 1e-30) — what the model thinks of what it was given.
 *   With hold all zero every output is bitwise mst_frame_step's and held_scores is unchanged. Refuses what mst_frame_step refuses,
 *   a null given, hold or held_scores, and ldg or ldh below P. */
int mst_frame_step_held(int dtype, int64_t N, int64_t P, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int mode,
                        float thr, const uint64_t* seed_ptr, uint8_t* frames, int64_t ldf, uint8_t* roll, int64_t ldr, float* scores,
                        float* probs_out, const uint8_t* given, int64_t ldg, const uint8_t* hold, int64_t ldh, float* held_scores,
                        mst_stream_t stream);
/* mst_token_step_held: given int32 [N, L] and hold uint8 [N, L] in seqs' indexing. Where hold[n, i] != 0: seqs[n, i] = word[n] =
 *   given[n, i] whatever the sequence's state; unless the sequence is finished, held_scores[n] += -log max(softmax(logit)[given],
 *   1e-30) (the model's distribution: temperature 1, uncut); active[i] counts the token by the usual rule (neither EOS nor PAD);
 *   kept_out[n] = 0 (nothing was drawn; the cuts are not evaluated). A given token outside [0, V) never indexes the row: PAD is
 *   written and nothing is charged (callers refuse such input). Where hold[n, i] == 0 the position is mst_token_step's bit for bit
 *   (seqs, scores, word, active, kept_out). Refuses what mst_token_step refuses and a null given, hold or held_scores. */
int mst_token_step_held(int dtype, int64_t N, int64_t V, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int32_t top_k,
                        float top_p, const uint64_t* seed_ptr, int32_t* seqs, float* scores, int32_t* word, int32_t* active,
                        int32_t* kept_out, int32_t eos, int32_t pad, const int32_t* given, const uint8_t* hold, float* held_scores,
                        mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K12/K13: softmax over V + SoftmaxCrossEntropy (model.py:256; loss.py:15-23).
 *   logits : act dtype [M = B*T, ld]; labels int32 [M]
 *   loss[b] = (1/T) * sum_t -log p[b,t,label] * (label != 0)     (fp32 [B], written)
 *   probs  : optional fp32 [M, ldp] output (reconstruction)
 *   dlogits: optional act dtype [M, ld]: (p - onehot) * (label != 0) / T * gscale; pad cols zero
 *   tok_parts: optional fp32 [MST_CE_MAX_WORKGROUPS, 4], the masked token metrics of trainer.py:107-113 kept on the
 *            device: every workgroup ADDS {sum -log max(p[label], 1e-10), #(label is the arg-max), #(label among
 *            the top_k), #(label != 0)} of its rows to its own row (no atomics; the caller clears the buffer when it
 *            reads the metrics and sums the rows): ppl = exp([0]/[3]), acc = [1]/[3], topk = [2]/[3].
 * ------------------------------------------------------------------------ */
#define MST_CE_MAX_WORKGROUPS 4096
int mst_softmax_ce(int dtype, int64_t B, int64_t T, int64_t V,
                   const void* logits, int64_t ld, const int32_t* labels,
                   float* loss, float* probs, int64_t ldp,
                   void* dlogits, int64_t ldd, float gscale,
                   int pre_zeroed /* 1: loss[] is already zero (mst_step_begin's zero list), skip the memset node */,
                   float* tok_parts, int top_k, mst_stream_t stream);

/* The reference's own call forms of the two reconstruction losses, on PROBABILITIES (what Model(...) returns):
 *   SoftmaxCrossEntropy()(probs, labels)                  loss.py:16-23: -log(pick(pred, label)) * (label != 0), / padded T
 *   BinaryCrossEntropy(from_sigmoid=True)(probs, labels)  loss.py:40-56 without the sigmoid
 * probs: dtype MST_F32 / MST_BF16 / MST_F16, [B*T, ldp] resp. contiguous [B, n_per_sample]; loss fp32 [B], written.
 * Forward only (the training step differentiates the fused logit forms above). */
int mst_ce_from_probs(int dtype, int64_t B, int64_t T, int64_t V, const void* probs, int64_t ldp,
                      const int32_t* labels, float* loss, mst_stream_t stream);
int mst_bce_from_probs(int dtype, int64_t B, int64_t n_per_sample, const void* probs, const uint8_t* labels,
                       float label_smoothing, int downweight, float* loss, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K14: sigmoid + BinaryCrossEntropy (loss.py:27-80), piano-roll head.
 *   logits : act dtype [B, T*P] viewed as [B*T, ld] with P valid columns
 *   labels : uint8 {0,1} [B*T, P]
 *   loss[b] = mean_{t,p} bce ; bce = -(s log(1e-12+p) + (1-s) log(1e-12+1-p)), s = (1-ls)*y + 0.5*ls
 *   negative down-weighting (downweight != 0): where y == 0, bce <- w_b * bce^2,
 *   w_b = n_pos_b / (n_neg_b + 1e-12) (loss.py:50-54,58-81); npos is int32 [B] scratch.
 *   probs  : optional act dtype [B*T, ldp] (sigmoid output = reconstructed piano-roll)
 *   dlogits: optional act dtype, d(sum_b loss_b)/dlogit * gscale
 *   Columns P..roundup4(P) of probs and dlogits are written as zeros; the pad columns of logits may hold anything.
 * ------------------------------------------------------------------------ */
int mst_sigmoid_bce(int dtype, int64_t B, int64_t T, int64_t P,
                    const void* logits, int64_t ld, const uint8_t* labels,
                    float label_smoothing, int downweight, int32_t* npos,
                    float* loss, void* probs, int64_t ldp,
                    void* dlogits, int64_t ldd, float gscale,
                    int pre_zeroed /* as in mst_softmax_ce */, mst_stream_t stream);
/* The same launch (mst_sigmoid_bce is this call with counts = NULL) which also ADDS the piano-roll counts of its cells — see
 * mst_bce_args — to counts: uint64 [MST_ROLL_SLOTS][4], 16-byte aligned, slot = (sample * grid.x + workgroup) % MST_ROLL_SLOTS.
 * Pad columns P..ld are not counted. The launch form is the one mst_sigmoid_bce_form reports. */
int mst_sigmoid_bce_counts(int dtype, int64_t B, int64_t T, int64_t P,
                           const void* logits, int64_t ld, const uint8_t* labels,
                           float label_smoothing, int downweight, int32_t* npos,
                           float* loss, void* probs, int64_t ldp,
                           void* dlogits, int64_t ldd, float gscale,
                           int pre_zeroed, uint64_t* counts, mst_stream_t stream);
/* What mst_sigmoid_bce launches for the same arguments: decided on the host, no HIP call, no device needed (the pointers are looked at
 * for NULL and alignment only). The kernel's choice of the vector width is the same function. form is a host array of 8 entries:
 *   form[0]  pitches a thread sweeps at a time: 8 (P, ld, ldp, ldd multiples of 8, logits / probs / dlogits on 16-byte and labels on
 *            8-byte boundaries) or 4
 *   form[1]  bytes of a label load: 8 (with form[0] = 8), 4 (P % 4 == 0) or 1
 *   form[2]  how sample 0's positives are counted: 8 bytes at a time (its labels start on an 8-byte boundary) or 1; 0 without down-weighting
 *   form[3]  the same for sample 1 (0 when B = 1): the samples' labels are T * P bytes apart
 *   form[4]  workgroups per sample, grid.x: min(ceil(512 / B), ceil(T * ceil(P / 4) / 1024)). At 1 a sample's loss is a single atomic
 *            and the launch is bit-reproducible in loss too
 * Entries not listed are 0. Returns 0; invalid arguments: what mst_sigmoid_bce returns for them, same message. */
int mst_sigmoid_bce_form(int dtype, int64_t B, int64_t T, int64_t P,
                         const void* logits, int64_t ld, const uint8_t* labels,
                         float label_smoothing, int downweight, int32_t* npos,
                         float* loss, void* probs, int64_t ldp,
                         void* dlogits, int64_t ldd, float gscale,
                         int pre_zeroed, int64_t* form);

/* ------------------------------------------------------------------------
 * K15/K21: total[b] = recon[b] + kl_weight * kl[b]; metric_acc[0] += sum_b kl, [1] += sum_b total,
 * [2] += B (running sums kept on device: trainer.py:107-120,172,181-186).
 * ------------------------------------------------------------------------ */
int mst_loss_combine(int64_t B, const float* recon, const float* kl, float kl_weight,
                     float* total, float* metric_acc, mst_stream_t stream);

/* ------------------------------------------------------------------------
 * K16: multi-tensor Adam over one flat fp32 bucket with MXNet's update rule
 * (gluon.Trainer.step → optimizer.Adam → adam_update; trainer.py:94-101,177):
 *   g = clip(grad * rescale + wd * w, ±clip)  (clip < 0: no clipping)
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g² ; w -= lr_t * m / (sqrt(v) + eps)
 *   lr_t = lr * sqrt(1-b2^t)/(1-b1^t), evaluated in double like the Python reference (lr, b1, b2 are doubles for
 *   that reason: 1 - 0.999f is already 1.3e-5 off); t lives in step_state[0] on the device and is advanced by a
 *   1-thread kernel issued ahead of the update in the same stream, so a captured graph replays
 *   with the right bias correction.
 * Also refreshes the 16-bit shadow copy w16 (act dtype, same offsets; may be NULL).
 * ONE entry point, mst_adam_flat, over ONE argument block, mst_adam_args (below, where every optional group is stated).
 * ------------------------------------------------------------------------ */
typedef struct mst_step_metrics {
  int64_t B; const float* recon; const float* kl; float kl_weight; float* total; float* metric;
  /* Step guard (all optional). status: two sticky device words {flags, number of skipped steps}. A step COUNTS only if
   * status[0] == 0 and every given *expect_ptr holds expect_val (the barrier counters of the one-launch position-0 tails,
   * mst_row_tail_*: a tail that could not finish leaves its counter short). Otherwise mst_adam_flat leaves parameters,
   * moments and the step count as they were, the metric sums are not touched, flag MST_STEP_INCOMPLETE is added to
   * status[0] when an expectation failed and status[1] is incremented: the batch is skipped, not mis-learned. The host reads
   * the words with the metrics, takes its fallback and clears them. */
  uint32_t* status; const uint32_t* expect_ptr0; uint32_t expect_val0; const uint32_t* expect_ptr1; uint32_t expect_val1;
  /* Non-finite guard (optional; needs status, which then has a third word): fin_recon / fin_kl = the step's fin_B per-sample
   * losses. If one of them is not finite — an activation overflowed (fp16 at long sequences: the key-row softmax lets a query
   * collect up to T key masses, attention outputs of several thousand), or sigma reached 0 under log(sigma^2) — the gradients
   * are NaN too and an update would destroy every parameter: mst_adam_flat then leaves parameters, moments and the step count
   * alone, adds nothing to the metric sums and increments status[2]. NOT sticky: the next batch is tried again. Every optimizer
   * launch of the step gets the same pointers (a second range without `recon` skips with the first). */
  const float* fin_recon; const float* fin_kl; int64_t fin_B;
} mst_step_metrics;
#define MST_TAIL_SPIN_FWD 1u     /* a grid barrier of mst_row_tail_fwd gave up waiting */
#define MST_TAIL_SPIN_BWD 2u     /* ... of mst_row_tail_bwd */
#define MST_STEP_INCOMPLETE 16u  /* an expect_ptr of the step guard did not hold its value at the end of the step */
/* The argument block of mst_adam_flat: ONE launch over w[0..n), behind — with advance_step — the 1-thread launch that advances
 * the step count. The first three lines of fields state the update rule above; each optional group below is off while its
 * pointer is NULL, and the launch is then exactly the one without the group. Every check named here is made before any HIP call.
 *
 * dtype is the act dtype of w16 and wt16. w, grad, m, v: fp32, n > 0 elements, 16-byte aligned. step_state: device int32[2] =
 * {t, bits(lr_t)}. advance_step = 1 (standalone use): t and lr_t are advanced here from lr, beta1, beta2; 0: the launch reuses
 * the lr_t that mst_step_begin, or the previous launch of the step (a second range of one step), left there. advance_step = 1
 * goes with none of sched, emb, parts and ema, whose step count is mst_step_begin's.
 *
 * metrics: the end-of-step bookkeeping of mst_loss_combine (total[b] = recon[b] + kl_weight * kl[b] and the running metric
 * sums; trainer.py:107-120,172,181-186) done by the first workgroup of this launch instead of a launch of its own, and the two
 * guards of mst_step_metrics. The launch given `recon` carries the step's bookkeeping; a second range of the step gets the guards'
 * fields alone.
 *
 * sched: the bookkeeping reads the device schedule block of mst_step_begin (which exists only behind an mst_step_begin of the
 * same step) instead of metrics->kl_weight, which is ignored:  total[b] = recon[b] + sched[0] * max(kl[b] - sched[1], 0)  (the KL
 * charged beyond the free bits, at this step's weight); metric[0] += sum_b kl[b] — the RAW KL, comparable across schedules —,
 * metric[1] += sum_b total, metric[2] += B. The guards work on the raw per-sample losses as without a schedule; a step they skip
 * takes the step count back, and the schedule — a function of that count alone — with it. lr_t is read from step_state as
 * always: the learning-rate warm-up is already in it.
 *
 * base, emb, n_emb, wt16: the launch also keeps the transposed 16-bit shadow of n_emb = 0..2 matrices current (the piano-roll
 * embedding tables, which the step's first launch reads). emb is a HOST array, emb[4j..4j+3] = {source offset in the flat bucket,
 * offset in wt16, rows, cols} (rows, cols > 0, rows * cols < 2^31, the offset in wt16 >= 0); for an element of matrix j the new weight is
 * also stored at wt16[dst + c * roundup8(rows) + r]. base >= 0 is the flat offset of `w` itself (a launch over a sub-range of the
 * bucket); a matrix outside [base, base + n) simply never matches. n_emb = 0: emb and wt16 are ignored.
 *
 * parts, n_parts, max_norm, gstat: the gradient is clipped by its global L2 norm (gluon.utils.clip_global_norm's rule), which the
 * per-workgroup sums of squares that mst_grad_sumsq left in parts state:
 *   S    = sum of parts[0..n_parts) in double, formed by every wave alike: lane l adds parts[4l..4l+3] as (p0 + p1) + (p2 + p3),
 *          then six pairwise levels across the 64 lanes (partners 1 and 2 apart, mirrored within 8 and within 16, 16 and 32
 *          apart; each level the commutative sum of two lanes' values) — the same instructions on the same words in every wave
 *          of every launch of the step, so all of them apply the same factor
 *   norm = sqrtf((float)S);  c = max_norm / (norm + 1e-8f) in fp32, and c = 1 unless c < 1
 *   g    = grad * fl32(rescale * c) + wd * w, then the per-element clip and the update as above
 * The norm is that of the batch-mean, loss-scale-free gradient, before weight decay: pass mst_grad_sumsq the rescales of the
 * Adam launches. gstat (NULL on every launch but the one that carries the step's bookkeeping) receives, on a step that counts,
 * gstat[0..6) = {norm, c, running sum of norms, largest norm, steps, steps with c < 1}; the host clears the running fields.
 * Checked: parts 16-byte aligned, n_parts == mst_grad_sumsq_parts(), 0 < max_norm < inf; and with parts NULL, that n_parts,
 * max_norm and gstat are 0 / NULL too.
 *
 * ema, decay: the averaging form. Every thread also folds each weight it has just written into ema[0..n) (fp32, 16-byte aligned,
 * the flat offsets of `w`), an exponential moving average of the weights:
 *   t    = step_state[0], Adam's step count after the step's increment (1-based)
 *   d_t  = fminf(decay, (1.f + t) / (10.f + t))      fp32, t converted to fp32 first, a correctly rounded division: the usual
 *          warm-up, so the first steps do not average in the initial weights
 *   omd  = 1.f - d_t
 *   e_i <- fl(fl(d_t * e_i) + fl(omd * w_i'))        w_i' the fp32 weight this thread stores: two rounded products and one
 *          rounded sum, in this order, never contracted into an FMA (engine.ema_decay_at / engine.ema_update state the same in
 *          np.float32; the result is theirs bit for bit)
 * w, m, v, w16 and the transposed shadows are exactly what the launch without `ema` writes. Reading t is race-free: in this
 * launch only the bookkeeping thread ever writes step_state, and only to take the count back on a skipped step, where every
 * thread returns before the read; on a step that counts nobody writes it (the increment is mst_step_begin's, earlier in the
 * stream). Both ranges of a two-range fp16 step read the same t, hence the same d_t. Checked: ema 16-byte aligned and
 * 0 < decay < 1 (a NaN fails); and with ema NULL, that decay is 0.
 *
 * Skipped steps. Three guards, asked in this order, each uniform over the launch and over the launches of a step: the step guard
 * and the non-finite guard of mst_step_metrics, then — with parts — a norm that is not finite (a NaN or inf somewhere in the
 * bucket). A launch that a guard skips leaves parameters, moments, w16, the transposed shadows, ema and the metric sums as they
 * were. The launch that carries the step's bookkeeping (metrics->recon for the first two guards, gstat for the third) takes the
 * step count back — once per step, for any number of ranges and ranks — and counts the skip: the step guard in metrics->status[0]
 * and [1] as stated at mst_step_metrics, either non-finite guard by incrementing status[2] (the third only if metrics->status is
 * given). gstat is not written on a skipped step. */
typedef struct mst_adam_args {
  int32_t dtype; int64_t n; float* w; const float* grad; float* m; float* v; void* w16;
  double lr, beta1, beta2; float eps, wd, rescale, clip;
  int32_t* step_state; int32_t advance_step;
  const mst_step_metrics* metrics;
  const float* sched;
  int64_t base; const int64_t* emb; int64_t n_emb; void* wt16;
  const float* parts; int64_t n_parts; float max_norm; float* gstat;
  float* ema; float decay;
} mst_adam_args;
int mst_adam_flat(const mst_adam_args* args, mst_stream_t stream);
/* What mst_adam_flat launches for a block: no HIP call, no device pointer followed, the launch's own checks with its status and
 * message. form[0..5) = {scheduled bookkeeping, clipping, averaging (each 0/1: the three switches of the kernel), transposed
 * shadows kept (0..2), the step-count launch ahead (0/1)}. */
int mst_adam_flat_form(const mst_adam_args* args, int64_t* form);
/* mst_loss_combine with the step guard of mst_step_metrics (validation steps: a step whose position-0 tail failed adds
 * nothing to the running sums) */
int mst_loss_combine_v(const mst_step_metrics* metrics, mst_stream_t stream);

/* mst_grad_sumsq, for the clipping group of mst_adam_args: ONE launch of mst_grad_sumsq_parts() workgroups (a fixed count,
 * <= 256) over the flat fp32 gradient bucket grad[0..n) (16-byte aligned). Element i is multiplied by rescale_lo if i < cut, else
 * by rescale_hi (0 <= cut <= n, any residue mod 4: the two loss-scale ranges of an fp16 step), and squared; workgroup j stores the
 * sum over its elements at parts[j]. Order: per thread an fp32 chain over its grid-stride 4-vectors (the up-to-three tail
 * elements on the last workgroup), a DPP wave sum, the four waves through LDS in wave order. No atomics: the same data gives the
 * same bits in every launch. A NaN or inf in the bucket — or an element whose square overflows fp32, |g r| > 1.8e19 — makes a
 * part non-finite. */
int64_t mst_grad_sumsq_parts(void);
int mst_grad_sumsq(int64_t n, const float* grad, int64_t cut, float rescale_lo, float rescale_hi, float* parts, mst_stream_t stream);

/* mst_ema_swap, for the averaging group of mst_adam_args: ONE launch that exchanges w[i] <-> ema[i] over the bucket (16-byte loads
 * and stores, a grid-stride loop, the up-to-three tail elements on the last workgroup) and writes w16[i] (may be NULL) from the
 * new w[i], the cast the Adam launch writes. Contents move, pointers do not: captured graphs stay valid. Exact: two calls restore
 * every bit of w and ema. The transposed shadows are the caller's to refresh (mst_transpose_shadows). */
int mst_ema_swap(int dtype, int64_t n, float* w, float* ema, void* w16, mst_stream_t stream);

/* 16-bit shadow + transposed shadow refresh for a list of matrices.
 * desc: int64 [n_mat, 4] on device = {src_offset, dst_offset, rows, cols}; dst is [cols, ld_t] with
 * ld_t = roundup8(rows), pad columns zeroed. tiles: int64 prefix sums [n_mat+1] of 32x32 tile counts. */
int mst_transpose_shadows(int dtype, const float* w, void* wt16, const int64_t* desc,
                          const int64_t* tile_prefix, int64_t n_mat, int64_t total_tiles,
                          mst_stream_t stream);

/* out[i] = sum of squares of x[ranges[2i] .. ranges[2i+1]) (device int64 [n_segments, 2]): the per-parameter gradient
 * norms of the reference's periodic gradient log (trainer.py:257-270) in one launch over the flat bucket */
int mst_segment_sumsq(const float* x, const int64_t* ranges, int64_t n_segments, float* out, mst_stream_t stream);

/* fp32 -> act dtype cast of a flat range (initial shadow fill) */
int mst_cast_f32_to_act(int dtype, int64_t n, const float* src, void* dst, mst_stream_t stream);

/* counter-based dropout keep-mask materialisation (for the oracle comparison): keep[i] in {0,1}; 0 <= p <= 1 (p = 1 keeps nothing: the
 * layer dropouts stay below 1, the decoder-input dropout of mst_step_begin_args.in_* may reach it) */
int mst_dropout_mask(int64_t n, float p, uint64_t seed, uint32_t site, uint8_t* keep, mst_stream_t stream);

/* stream-ordered memset to zero (gradient bucket, metric sums) */
int mst_zero(void* ptr, int64_t bytes, mst_stream_t stream);
/* device-resident per-step RNG seed: state = uint64[4] {seed for this step, step counter, base seed, 0};
 * one launch per step advances it, so dropout masks and eps differ on every replay of a captured graph
 * (word 3 is the workgroup arrival counter of mst_step_begin and is zero between launches) */
int mst_rng_advance(uint64_t* state, mst_stream_t stream);
/* Top-of-step bookkeeping in ONE launch (every kernel in the captured graph costs ~4.7 us): mst_rng_advance, Adam's
 * step counter / bias-corrected lr (then call mst_adam_flat with advance_step = 0), mst_randn into eps_out, and the two
 * mst_mask_from_lengths masks (model.py:246-247), and two optional buffers to clear (16-byte aligned, sizes multiples
 * of 16: the per-sample loss sums and the gradient bucket, instead of two memset nodes). Any pointer may be NULL to
 * skip that part. rng_state is the uint64[4] state of mst_rng_advance.
 * eps_index0 (even): eps_out[i] is draw number eps_index0 + i of the step's stream, so a data-parallel rank that
 * passes its first global sample index times Z draws exactly what a single process draws for those samples. */
typedef struct mst_step_begin_args {
  uint64_t* rng_state; int32_t* adam_state; double lr, beta1, beta2;
  float* eps_out; int64_t n_eps; uint32_t eps_site; int64_t eps_index0;
  const int32_t* lens; int64_t B; uint8_t* mask_e; int64_t Se; int32_t add_e; uint8_t* mask_d; int64_t Sd; int32_t add_d;
  void* zero_a; int64_t zero_a_bytes; void* zero_b; int64_t zero_b_bytes;
  /* Optional transposed-shadow refresh riding on the same launch (mst_transpose_shadows' arguments; sh_w == NULL: none): the
   * 16-bit transposed copies of matrices that only the BACKWARD pass reads can be rebuilt from the fp32 weights at the start
   * of the next step instead of in a launch of their own behind the optimizer. Matrices the launch itself reads (the
   * piano-roll embedding tables of mst_gemm_nt_pair_begin) must not be listed: mst_adam_flat keeps those current (mst_adam_args.emb). */
  int32_t sh_dtype; const float* sh_w; void* sh_wt16; const int64_t* sh_desc; const int64_t* sh_prefix; int64_t sh_n_mat, sh_tiles;
  /* Optional training schedules (sched == NULL: none, the launch is exactly the one without these fields; needs adam_state). With t =
   * adam_state[0] AFTER this launch's increment (1-based) and all arithmetic in double:
   *   f_lr   = sched_lr_warmup > 0 ? min(1, t / sched_lr_warmup) : 1;      lr_t = (float)((lr * f_lr) * sqrt(1-b2^t) / (1-b1^t))
   *   u      = sched_kl_cycle > 0 ? ((t - 1) mod sched_kl_cycle) + 1 : t;  ramp = sched_kl_warmup > 0 ? min(1, u / sched_kl_warmup) : 1
   *   beta_t = (float)((double)sched_kl_weight * ramp)
   * and the thread that advances Adam's step count writes the fp32 schedule block sched[0..3] = {beta_t, sched_kl_free_bits, f_lr, t},
   * which the scheduled launches of the same step read (mst_latent_bwd_vec_sched, mst_adam_flat with mst_adam_args.sched). A pure function of the step
   * count: it replays inside a captured graph, resumes with the optimizer state and is the same on every data-parallel rank; a
   * step the optimizer's guards take back (mst_step_metrics) takes the schedule back with the count.
   * Lengths and free bits must be >= 0; a cycle needs 0 < sched_kl_warmup <= sched_kl_cycle. */
  float* sched; float sched_kl_weight, sched_kl_free_bits; int32_t sched_kl_warmup, sched_kl_cycle, sched_lr_warmup;
  /* Optional decoder-input dropout (ABI 118; in_keep == NULL: none, the launch is exactly the one without these fields; needs
   * rng_state). "Word dropout" for the teacher-forced decoder: with probability p = in_p (0 <= p <= 1) the decoder does not see a
   * previous frame / token and has to predict the next one through the latent. THE SEMANTICS, stated here once:
   *   - Decoder input position k (k = 0..T-1) of sample b is the input of decoder row k + 1; r = b * T + k indexes in_keep, in_n = B * T.
   *   - in_keep[r] = dropout_keep(s, in_site, in_index0 + r, in_p) (the function of the layer dropouts and of mst_dropout_mask), s
   *     being this step's NEW seed — the value eps is drawn from, rng_state[0] after the launch. 1: kept, 0: dropped. The realised
   *     keep probability is (65536 - floor(65536 p)) / 65536 as for the other masks; p = 1 drops every position.
   *   - in_index0 = (the plan's first GLOBAL sample index) * T, as eps_index0, and in_site is ONE constant for all data-parallel ranks
   *     (not offset per rank): a shard draws exactly what a single process draws for those samples.
   *   - A dropped position contributes a ZERO EMBEDDING: its decoder input row is sqrt(D) * 0 + pos[k + 1], rounded to the activation
   *     type. Piano-roll ends: the frame is all zeros (in_src / in_dst below). Token ends: no table row is gathered (mst_embed_fwd's
   *     keep). No rescaling by 1 / (1 - p) — word dropout has none — and no UNK symbol: a zero row is the same thing for both kinds.
   *   - Backward is the autograd of exactly that: a dropped position adds nothing to the decoder embedding's weight gradient (the
   *     weight-gradient problem reads in_dst; mst_embed_bwd's keep); every other gradient follows from the changed forward values.
   *   - Not affected: the encoder (it sees the intact piece), labels, loss, key masks, decoder row 0 (the latent block's). The draw
   *     does not look at the sequence lengths: padded positions are drawn like any other and are masked as before.
   *   - Inference passes carry no job: they are the launches, and the bits, of a step without these fields.
   * With in_src (optional; in_src and in_dst come together) the bookkeeping workgroups also write the masked copy of the uint8 frames:
   *   in_dst[r, 0..in_row_bytes) = in_keep[r] ? in_src[r, 0..in_row_bytes) : 0    (leading dimensions in_ld_src / in_ld_dst, in bytes)
   * and touch no byte of a dst row beyond in_row_bytes. in_row_bytes and both leading dimensions are multiples of 8, the leading
   * dimensions >= in_row_bytes, both pointers 8-byte aligned. in_n > 0, in_index0 >= 0, in_index0 + in_n < 2^31. */
  uint8_t* in_keep; int64_t in_n; float in_p; uint32_t in_site; int64_t in_index0;
  const uint8_t* in_src; int64_t in_ld_src; uint8_t* in_dst; int64_t in_ld_dst; int64_t in_row_bytes;
} mst_step_begin_args;
int mst_step_begin(const mst_step_begin_args* args, mst_stream_t stream);
/* mst_step_begin and mst_gemm_nt_pair in ONE launch: nothing in the piano-roll ends' embedding GEMMs (the first arithmetic of the
 * step) reads what the bookkeeping writes, so its workgroups ride in front of the tiles of that launch. Where mst_gemm_nt_pair
 * would fall back to two launches this is exactly mst_step_begin(begin) followed by mst_gemm_nt_pair(args0, args1).
 * When `begin` carries a decoder-input dropout job (in_keep != NULL) the decoder's problem reads what the bookkeeping writes (in_dst),
 * so the call is ALWAYS mst_step_begin(begin) followed by mst_gemm_nt_pair(args0, args1): the bookkeeping is a launch of its own in
 * front (a requested shadow refresh stays behind the tiles of the GEMM launch, which neither reads nor writes what it touches). The
 * rule lives here, in the library: the race cannot be constructed from outside. */
int mst_gemm_nt_pair_begin(const mst_gemm_args* args0, const mst_gemm_args* args1, const mst_step_begin_args* begin,
                           mst_stream_t stream);
/* eps ~ N(0,1) (replaces mx.nd.random_normal, model.py:292): Box-Muller over the counter hash;
 * effective seed = seed ^ (seed_ptr ? *seed_ptr : 0) */
int mst_randn(int64_t n, float* out, uint64_t seed, const uint64_t* seed_ptr, uint32_t site, mst_stream_t stream);

/* elementwise act-dtype helpers used on gradient joins: y = a + b */
int mst_add_act(int dtype, int64_t n, const void* a, const void* b, void* y, mst_stream_t stream);

/* hardware layout self-test (MFMA fragment maps + ds_read_tr16_b64); out: int32[4] pass flags */
int mst_selftest(int32_t* out_flags_device, mst_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MST_HIP_H */

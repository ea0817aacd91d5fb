// attention.hip — MultiHeadDotAttention with the reference's KEY-ROW softmax, forward and backward.
//
// Reference arithmetic (VarAutoEncoder/transformer.py:85-126), per (batch b, head h):
//   L[k,q] = K[k]·Q[q] / sqrt(dh) + (keymask[k] ? 0 : -1e9)        :96-99,106-126
//   P[k,:] = softmax over q (the LAST axis of [B,H,T_K,T_Q])        :100
//   O[q]   = sum_k P[k,q] V[k]                                      :102 (transpose_a)
// Quirks reproduced on purpose: normalisation runs over queries, not keys; the padding mask adds
// the same -1e9 to a whole softmax row, so in fp32 a padded key row collapses to a (near-)uniform
// 1/S row instead of being excluded. The kernels add -1e9 in fp32 to the fp32 MFMA accumulator
// exactly as the reference does, in 16-bit modes too (no -inf, no NaN).
//
// Nothing S x S ever reaches HBM. Four kernels, all on v_mfma_f32_32x32x16 with the softmax axis
// chosen per kernel so reductions stay in-lane:
//   fwd_stats (key-owner, key on the lane)   : lse[k] = logsumexp_q L[k,q]        (online, in-lane)
//   fwd_out   (query-owner, query on the lane): O[q] += P^T V, P tile reused straight from the
//                                               accumulator registers as the next MFMA's A operand
//   bwd_kv    (key-owner)  : dV[k] = sum_q P dO[q];  delta[k] = sum_q P dP;  dK[k] = s * sum_q dL Q[q]
//   bwd_q     (query-owner): dQ[q] = s * sum_k dL[k,q] K[k],  dL = P * (dP - delta[k]),  dP = dO[q]·V[k]
// Operands that a product needs "transposed" (V, dO, Q, K as the B operand of an X^T·B product) are
// staged row-major in LDS and read with ds_read_tr16_b64.
//
// The code is cut by launch family. attention.hpp: the tile arithmetic every kernel shares. attention_fwd.hip / attention_bwd.hip: the
// launches of one direction each — the two kernels above as launches of their own (streaming, any sequence length) and as phases of
// one resident launch with the sequence held in LDS, with the fused projection prologues and the chunked dQ kernel.
// This unit: the argument checks, the form rules (every decision between kernels), the C entry points and the decode kernel.
// attention_forms.hpp: the forms and the launchers' declarations.
#include <math.h>
#include <stdlib.h>
#include "attention_forms.hpp"

namespace mst {

// Waves per workgroup for the resident kernels, or 0 when the sequence does not fit: maximise (resident waves per CU)
// x (balance of the 32-row owner blocks over the waves); 128 VGPRs per lane (launch bounds 1024) allow 16 waves per CU,
// the 96 of the head-size-16 instantiations 20 (two 9-wave workgroups of a 257-row sequence: the decoder of configs[1]).
static int choose_resident(int64_t S, int64_t n_wg, size_t lds_bytes, int waves_cu = 16, bool lone = false, int max_nw = 16) {
  const char* force = getenv("MST_ATTN_PATH");  // "stream" / "resident": pin the path (tests cover both)
  if (force && force[0] == 's') return 0;
  const size_t LDS_CU = 160 * 1024;
  if (lds_bytes > LDS_CU - 1024) return 0;
  const int NB = (int)cdiv(S, 32) - (lone ? 1 : 0);  // owner blocks
  const int by_grid = (int)cdiv(n_wg, 256);
  int best = 0;
  double best_score = 0.0;
  for (int nw = 1; nw <= max_nw && nw <= NB; ++nw) {
    int wgs = waves_cu / nw;
    if ((size_t)wgs * lds_bytes > LDS_CU) wgs = (int)(LDS_CU / lds_bytes);
    if (wgs > by_grid) wgs = by_grid;
    if (wgs < 1) continue;
    const double eff = (double)NB / (double)(nw * cdiv(NB, nw));
    const double score = (double)(wgs * nw) * eff;
    if (score >= best_score) { best_score = score; best = nw; }
  }
  return best;
}
// dynamic LDS of the resident kernels: the staged tiles ([SP][dh + 8] 16-bit each, LdsLd), the per-key fp32 arrays, the lone row's scratch
static size_t res_lds_fwd(int dh, int64_t S, int tiles) { const size_t SP = (size_t)cdiv(S, 32) * 32; return (size_t)tiles * SP * (dh + 8) * 2 + 5 * SP * 4 + LONE_RED * 4; }
static size_t res_lds_bwd(int dh, int64_t S) { const size_t SP = (size_t)cdiv(S, 32) * 32; return 2 * SP * (dh + 8) * 2 + 6 * SP * 4 + LONE_RED * 4; }
// ... of dout_prologue's staged operands: a 64-deep slice of dproj for every row, the head's weight panel
static size_t res_lds_bwd_proj(int dh, int64_t S, int64_t Dm) { const size_t SP = (size_t)cdiv(S, 32) * 32; return SP * DOP_LDS * 2 + (size_t)dh * (Dm + 8) * 2; }
static int res_max_waves(int dh) { return dh == 64 ? RES_MAX_WAVES<64> : RES_MAX_WAVES<32>; }

static int attn_check(int64_t B, int64_t S, int64_t H, int64_t dh, int64_t ld, int64_t k_off, int64_t q_off, int64_t v_off) {
  MST_CHECK_ARG(B > 0 && S > 0 && H > 0, "attention: B,S,H must be positive");
  MST_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "attention: head size must be 16, 32 or 64 (got %lld)", (long long)dh);
  MST_CHECK_ARG(ld % 8 == 0 && k_off % 8 == 0 && q_off % 8 == 0 && v_off % 8 == 0, "attention: ld and offsets must be multiples of 8");
  MST_CHECK_ARG(B * H <= 65535, "attention: B*H too large for grid.y");
  return MST_OK;
}
// the leading-dimension checks of each entry point, made after attn_check (the form queries make the same ones)
static int attn_check_fwd_ld(int64_t H, int64_t dh, int64_t ld_out) { MST_CHECK_ARG(ld_out >= H * dh, "mst_attn_keysoftmax_fwd: ld_out < H*dh"); return MST_OK; }
static int attn_check_qkv_ld(int64_t H, int64_t dh, int64_t ld_x, int64_t ld_w, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                             int64_t ld_out) {
  const int64_t Dm = H * dh;
  MST_CHECK_ARG(ld_x % 8 == 0 && ld_x >= Dm && ld_w % 8 == 0 && ld_w >= Dm && ld_qkv >= 3 * Dm && ld_out >= Dm,
                "mst_attn_qkv_fwd: leading dimensions must be multiples of 8 and cover the model width");
  MST_CHECK_ARG(k_off + Dm <= 3 * Dm && q_off + Dm <= 3 * Dm && v_off + Dm <= 3 * Dm, "mst_attn_qkv_fwd: section offsets beyond the 3 D weight rows");
  return MST_OK;
}
static int attn_check_bwd_ld(int64_t H, int64_t dh, int64_t ld_dout, int64_t ld_dqkv) {
  MST_CHECK_ARG(ld_dout % 8 == 0 && ld_dout >= H * dh && ld_dqkv % 8 == 0, "mst_attn_keysoftmax_bwd: bad leading dims");
  return MST_OK;
}
static int check_act_dtype(int dtype) { return dispatch_act(dtype, [](auto) -> int { return MST_OK; }); }
// the q_limit the kernels see: forward, queries [0, q_limit) are produced; backward, 0 = dense dO
static int64_t fwd_q_limit(int64_t q_limit, int64_t S) { return (q_limit > 0 && q_limit < S) ? q_limit : S; }
static int64_t bwd_q_limit(int64_t q_limit, int64_t S) { return (q_limit > 0 && q_limit < S) ? q_limit : 0; }
// the fields the four launching entry points fill the same way (q_limit: fwd_q_limit's / bwd_q_limit's)
static AttnArgs attn_args(int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                          const uint8_t* keymask, const float* lse, int64_t q_limit) {
  AttnArgs a = {};
  a.B = B; a.S = S; a.H = H; a.qkv = qkv; a.ld_qkv = ld_qkv; a.k_off = k_off; a.q_off = q_off; a.v_off = v_off;
  a.keymask = keymask; a.lse = const_cast<float*>(lse);
  a.q_limit = q_limit;
  a.scale = 1.f / sqrtf((float)dh);
  return a;
}

// ---- What a valid call launches: the codes of mst_attn_fwd_form / mst_attn_bwd_form (include/mst_hip.h; AttnFwdForm / AttnBwdForm,
// attention_forms.hpp). Every decision between kernels is made HERE, from the shape (and the MST_ATTN_PATH override inside
// choose_resident) alone; the launchers of the kernel units (attn_launch_fwd / attn_launch_bwd) switch on the result and decide
// nothing themselves, and the form queries report it.

// q_limit: fwd_q_limit's. fused_call: mst_attn_qkv_fwd (the projection inside the launch where the shape takes it, else the
// GEMM and one of the plain forms)
static AttnFwdForm attn_fwd_form(int dh, int64_t S, int64_t H, int64_t n_wg, int64_t q_limit, bool fused_call) {
  AttnFwdForm f = {};
  const int NB = (int)cdiv(S, 32);
  if (fused_call && dh == 32) {
    const int64_t Dm = H * dh;
    const size_t lds = res_lds_fwd(32, S, 3);  // (the projection's slices borrow the Q / K / V tiles)
    const int nw = choose_resident(S, n_wg, lds, 16, false);
    // every owner block needs its own wave (one pass over the weight slices); the staging pattern is laid out for 512 threads
    // (four x pieces and two weight pieces per thread; the weight slice must fit the V tile: NB >= 6)
    if (nw >= NB && nw >= 6 && Dm % QKV_KC == 0) { f.path = ATT_FWD_FUSED; f.waves = nw; f.lds = lds; return f; }
  }
  const bool lone = lone_row_shape(S, dh) && q_limit >= S;
  const int waves_cu = dh == 16 ? 4 * ATT16_WAVES : 16;
  f.lone = lone;
  for (int tiles = 3; tiles >= 2; --tiles) {
    // three tiles: Q | K | V together. Two (restage = 1): they do not fit, K and V are staged over Q between the phases (configs[4]'s
    // decoder: S 1025, dh 16)
    const size_t lds = res_lds_fwd(dh, S, tiles);
    if (const int nw = choose_resident(S, n_wg, lds, waves_cu, lone)) {
      f.path = tiles == 3 ? ATT_FWD_RES3 : ATT_FWD_RES2; f.waves = nw; f.lds = lds; f.restage = tiles == 3 ? 0 : 1;
      return f;
    }
  }
  if (!lone && dh >= 32 && NB % 2 == 0) {
    // ... nor K | V alone: one tile (restage = 2), the output phase in two chunks of keys (configs[4]'s encoder: S 1024, head size 32)
    const size_t lds = res_lds_fwd(dh, S, 1);
    const int maxw = res_max_waves(dh);  // (the chunked instantiation's launch bounds)
    const int nw = choose_resident(S, n_wg, lds, maxw, false, maxw);
    if (nw && NB <= 2 * nw) { f.path = ATT_FWD_CHUNKED; f.waves = nw; f.lds = lds; f.restage = 2; return f; }
  }
  f.path = ATT_FWD_STREAM; f.waves = 4; f.lone = 0;
  f.grid_stats = cdiv(S, ATT_WG_ROWS); f.grid_out = cdiv(q_limit, ATT_WG_ROWS);
  return f;
}
// q_limit: bwd_q_limit's
static AttnBwdForm attn_bwd_form(int dh, int64_t S, int64_t n_wg, int64_t q_limit) {
  AttnBwdForm f = {};
  f.sparse = q_limit > 0 && q_limit <= 32;
  const bool lone = lone_row_shape(S, dh) && !f.sparse;
  const size_t lds = res_lds_bwd(dh, S);
  if (const int nw = choose_resident(S, n_wg, lds, dh == 16 ? 4 * ATT16_WAVES : res_max_waves(dh), lone, res_max_waves(dh))) {
    f.path = ATT_BWD_RES; f.waves = nw; f.lds = lds; f.lone = lone;
    return f;
  }
  f.path = ATT_BWD_STREAM; f.waves = 4;
  // dQ: one workgroup per (batch, head) with the keys staged in chunks where the constants and two chunk tiles fit LDS
  // (head size 32: at 64 four blocks' accumulators and fragments do not fit 256 registers)
  const int NB = (int)cdiv(S, 32);
  if (dh == 32 && NB <= ATT_DQ_OBM * ATT_DQ_NW) {
    for (int nc = 1; nc <= 4; nc *= 2) {
      if (NB % nc != 0) break;
      const size_t lds_q = (size_t)2 * (NB * 32 / nc) * (dh + 8) * 2 + (size_t)6 * NB * 32 * 4;
      if (lds_q > 150 * 1024) continue;
      f.path = ATT_BWD_STREAM_CHUNKQ; f.lds = lds_q; f.dq_chunks = nc; f.dq_waves = ATT_DQ_NW;
      break;
    }
  }
  return f;
}
// mst_attn_proj_bwd: does the W_proj input gradient run INSIDE the resident launch (f.proj, with f.lds_proj bytes of LDS), or as the
// GEMM launch ahead of the kernel attn_bwd_form chose? Inside for the dense resident kernel at head sizes 16 and 32 when every owner
// block has a wave of its own (dout_prologue forms a block's rows in its wave; phase B takes the block's dO fragments from the LDS
// tile), the model width is whole 64-deep slices and two workgroups per CU still fit. Both step shapes of configs[1] measured faster
// this way than with their two launches (docs/kernel_notes.md). f: attn_bwd_form's, for the same shape.
static void attn_bwd_proj_rule(AttnBwdForm& f, int dh, int64_t S, int64_t Dm) {
  const int NBo = (int)cdiv(S, 32) - f.lone;
  const size_t need = res_lds_bwd_proj(dh, S, Dm), lds = need > f.lds ? need : f.lds;
  f.proj = f.path == ATT_BWD_RES && !f.sparse && dh <= 32 && f.waves == NBo && Dm % DOP_KC == 0 && 2 * lds <= 160 * 1024;
  f.lds_proj = f.proj ? lds : 0;
}

// ------------------------------------------------------------------------------------ incremental decode
// One new query row per sample against the rows cached so far (inference: model.py:259-272, transformer.py:70-77,242-249).
// The cache holds the layer's K | Q | V projections of every position fed so far ([B, t_max, ld] with the training layout
// k_off / q_off / v_off); the new row (position n_keys - 1) is already in it. Per (sample, head):
//   mode 0, the reference's arithmetic: logits[k, q] = K[k].Q[q] / sqrt(dh) + mask[k], softmax over the QUERY axis — which
//           holds the single new query, so every P[k, 0] is exp(0) / 1 = 1 and the output is the plain sum of the cached
//           value rows (computed as such: the logit cancels exactly, a -1e9 mask included)
//   mode 1, softmax over the cached KEYS (conventional incremental attention), offered beside it.
// A wave per (sample, head): lanes stride over the keys, each accumulating its keys' value rows, then a cross-lane sum.
template <typename T, int DH>
__global__ __launch_bounds__(64) void attn_decode_kernel(int64_t H, int64_t n_keys, int64_t t_max, const T* __restrict__ cache,
                                                          int64_t ld, int64_t k_off, int64_t q_off, int64_t v_off, int mode,
                                                          float scale, T* __restrict__ out, int64_t ld_out) {
  const int64_t b = blockIdx.x / H, hd = blockIdx.x % H;
  const int lane = threadIdx.x;
  const T* base = cache + b * t_max * ld + hd * DH;
  float q[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) q[d] = to_f32(base[(n_keys - 1) * ld + q_off + d]);
  float m = -INFINITY;
  if (mode == 1) {
    for (int64_t k = lane; k < n_keys; k += 64) {
      float l = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) l = fmaf(to_f32(base[k * ld + k_off + d]), q[d], l);
      m = fmaxf(m, l * scale);
    }
    m = wave_max(m);
  }
  float acc[DH], z = 0.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
  for (int64_t k = lane; k < n_keys; k += 64) {
    float p = 1.f;
    if (mode == 1) {
      float l = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) l = fmaf(to_f32(base[k * ld + k_off + d]), q[d], l);
      p = __expf(l * scale - m);
    }
    z += p;
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = fmaf(p, to_f32(base[k * ld + v_off + d]), acc[d]);
  }
  z = wave_sum(z);
  const float inv = (mode == 1) ? 1.f / z : 1.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    const float v = wave_sum(acc[d]);
    if (lane == 0) out[b * ld_out + hd * DH + d] = from_f32<T>(v * inv);
  }
}

}  // namespace mst

using namespace mst;

extern "C" int mst_attn_keysoftmax_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv,
                                       int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                                       const uint8_t* keymask, float* lse, void* out, int64_t ld_out,
                                       int64_t q_limit, mst_stream_t stream) {
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc) return rc;
  MST_CHECK_ARG(qkv && keymask && lse && out, "mst_attn_keysoftmax_fwd: null pointer");
  rc = attn_check_fwd_ld(H, dh, ld_out);
  if (rc) return rc;
  AttnArgs a = attn_args(B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off, keymask, lse, fwd_q_limit(q_limit, S));
  a.out = out; a.ld_out = ld_out;
  return attn_launch_fwd(dtype, dh, a, attn_fwd_form((int)dh, S, H, B * H, a.q_limit, false), (hipStream_t)stream);
}

// the projection of a fused entry point as the GEMM launch it is, for the shapes its fused form does not take
static int proj_gemm(int dtype, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
                     int64_t ldc, mst_stream_t stream) {
  mst_gemm_args g = {};
  g.dtype = dtype; g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.B = W; g.ldb = ldw; g.C = C; g.ldc = ldc; g.bias = bias; g.alpha = 1.f;
  return mst_gemm_nt(&g, stream);
}
static void put_form(int64_t* form, const int64_t (&v)[8]) { for (int i = 0; i < 8; ++i) form[i] = v[i]; }
extern "C" int mst_attn_fwd_form(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, int64_t ld_qkv, int64_t k_off, int64_t q_off,
                                 int64_t v_off, int64_t ld_out, int64_t q_limit, int fused, int64_t ld_x, int64_t ld_w, int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_attn_fwd_form: null form");
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc == MST_OK) rc = fused ? attn_check_qkv_ld(H, dh, ld_x, ld_w, ld_qkv, k_off, q_off, v_off, ld_out) : attn_check_fwd_ld(H, dh, ld_out);
  if (rc == MST_OK) rc = check_act_dtype(dtype);
  if (rc) return rc;
  const AttnFwdForm f = attn_fwd_form((int)dh, S, H, B * H, fwd_q_limit(q_limit, S), fused != 0);
  put_form(form, {f.path, f.waves, (int64_t)f.lds, f.lone, f.grid_stats, f.grid_out, 0, 0});
  return MST_OK;
}
extern "C" int mst_attn_bwd_form(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, int64_t ld_qkv, int64_t k_off, int64_t q_off,
                                 int64_t v_off, int64_t ld_dout, int64_t ld_dqkv, int64_t q_limit, int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_attn_bwd_form: null form");
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc == MST_OK) rc = attn_check_bwd_ld(H, dh, ld_dout, ld_dqkv);
  if (rc == MST_OK) rc = check_act_dtype(dtype);
  if (rc) return rc;
  AttnBwdForm f = attn_bwd_form((int)dh, S, B * H, bwd_q_limit(q_limit, S));
  attn_bwd_proj_rule(f, (int)dh, S, H * dh);
  put_form(form, {f.path, f.waves, (int64_t)f.lds, f.sparse, f.lone, f.dq_chunks, f.dq_waves, f.proj});
  return MST_OK;
}

extern "C" int mst_attn_qkv_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* x, int64_t ld_x, const void* w,
                                int64_t ld_w, const float* bias, void* qkv, int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                                const uint8_t* keymask, float* lse, void* out, int64_t ld_out, int64_t q_limit, mst_stream_t stream) {
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc == MST_OK) rc = attn_check_qkv_ld(H, dh, ld_x, ld_w, ld_qkv, k_off, q_off, v_off, ld_out);
  if (rc) return rc;
  const int64_t Dm = H * dh;
  MST_CHECK_ARG(x && w && bias && qkv && keymask && lse && out, "mst_attn_qkv_fwd: null pointer");
  MST_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)w % 16 == 0) && ((uintptr_t)bias % 16 == 0) && ((uintptr_t)qkv % 16 == 0),
                "mst_attn_qkv_fwd: operands must be 16-byte aligned");
  rc = check_act_dtype(dtype);
  if (rc) return rc;
  AttnArgs a = attn_args(B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off, keymask, lse, fwd_q_limit(q_limit, S));
  a.out = out; a.ld_out = ld_out;
  const AttnFwdForm f = attn_fwd_form((int)dh, S, H, B * H, a.q_limit, true);
  if (f.path == ATT_FWD_FUSED) {
    a.x = x; a.ld_x = ld_x; a.w = w; a.ld_w = ld_w; a.bias = bias; a.Dm = Dm;
  } else {
    // shapes the fused form does not take: the projection as the GEMM it is, then the plain attention launch
    rc = proj_gemm(dtype, B * S, 3 * Dm, Dm, x, ld_x, w, ld_w, bias, qkv, ld_qkv, stream);
    if (rc) return rc;
  }
  return attn_launch_fwd(dtype, dh, a, f, (hipStream_t)stream);
}

extern "C" int mst_attn_keysoftmax_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv,
                                       int64_t ld_qkv, int64_t k_off, int64_t q_off, int64_t v_off,
                                       const uint8_t* keymask, const float* lse, const void* dout, int64_t ld_dout,
                                       void* dqkv, int64_t ld_dqkv, float* delta, int64_t q_limit, mst_stream_t stream) {
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc) return rc;
  MST_CHECK_ARG(qkv && keymask && lse && dout && dqkv && delta, "mst_attn_keysoftmax_bwd: null pointer");
  rc = attn_check_bwd_ld(H, dh, ld_dout, ld_dqkv);
  if (rc) return rc;
  AttnArgs a = attn_args(B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off, keymask, lse, bwd_q_limit(q_limit, S));
  a.dout = dout; a.ld_dout = ld_dout; a.dqkv = dqkv; a.ld_dqkv = ld_dqkv; a.delta = delta;
  return attn_launch_bwd(dtype, dh, a, attn_bwd_form((int)dh, S, B * H, a.q_limit), (hipStream_t)stream);
}

extern "C" int mst_attn_proj_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv, int64_t k_off,
                                 int64_t q_off, int64_t v_off, const uint8_t* keymask, const float* lse, const void* dproj, int64_t ld_dproj,
                                 const void* wt, int64_t ld_wt, void* dout_out, int64_t ld_dout, void* dqkv, int64_t ld_dqkv, float* delta,
                                 mst_stream_t stream) {
  int rc = attn_check(B, S, H, dh, ld_qkv, k_off, q_off, v_off);
  if (rc) return rc;
  const int64_t Dm = H * dh;
  MST_CHECK_ARG(qkv && keymask && lse && dproj && wt && dqkv && delta, "mst_attn_proj_bwd: null pointer");
  MST_CHECK_ARG(ld_dproj % 8 == 0 && ld_dproj >= Dm && ld_wt % 8 == 0 && ld_wt >= Dm && ld_dqkv % 8 == 0 &&
                (!dout_out || (ld_dout % 8 == 0 && ld_dout >= Dm)), "mst_attn_proj_bwd: bad leading dims");
  MST_CHECK_ARG(((uintptr_t)dproj % 16 == 0) && ((uintptr_t)wt % 16 == 0) && ((uintptr_t)dout_out % 16 == 0) && ((uintptr_t)qkv % 16 == 0),
                "mst_attn_proj_bwd: operands must be 16-byte aligned");
  rc = check_act_dtype(dtype);
  if (rc) return rc;
  AttnArgs a = attn_args(B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off, keymask, lse, 0);
  a.dqkv = dqkv; a.ld_dqkv = ld_dqkv; a.delta = delta;
  AttnBwdForm f = attn_bwd_form((int)dh, S, B * H, 0);
  attn_bwd_proj_rule(f, (int)dh, S, Dm);
  if (f.proj) {
    a.x = dproj; a.ld_x = ld_dproj; a.w = wt; a.ld_w = ld_wt; a.Dm = Dm; a.out = dout_out; a.ld_out = ld_dout;
  } else {
    // shapes the fused form does not take: the input gradient as the GEMM it is, then the plain backward launches
    MST_CHECK_ARG(dout_out != nullptr, "mst_attn_proj_bwd: this shape runs the GEMM launch first and needs dout_out");
    rc = proj_gemm(dtype, B * S, Dm, Dm, dproj, ld_dproj, wt, ld_wt, nullptr, dout_out, ld_dout, stream);
    if (rc) return rc;
    a.dout = dout_out; a.ld_dout = ld_dout;
  }
  return attn_launch_bwd(dtype, dh, a, f, (hipStream_t)stream);
}

extern "C" int mst_attn_decode(int dtype, int64_t B, int64_t H, int64_t dh, int64_t n_keys, int64_t t_max, const void* cache,
                               int64_t ld, int64_t k_off, int64_t q_off, int64_t v_off, int mode, void* out, int64_t ld_out,
                               mst_stream_t stream) {
  MST_CHECK_ARG(B > 0 && H > 0 && n_keys > 0 && n_keys <= t_max && cache && out, "mst_attn_decode: bad argument");
  MST_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "mst_attn_decode: head size must be 16, 32 or 64 (got %lld)", (long long)dh);
  MST_CHECK_ARG(mode == 0 || mode == 1, "mst_attn_decode: mode must be 0 (softmax over the query axis, the reference) or 1 (over the keys)");
  MST_CHECK_ARG(ld_out >= H * dh, "mst_attn_decode: ld_out < H*dh");
  const float scale = 1.f / sqrtf((float)dh);
  hipStream_t s = (hipStream_t)stream;
  return dispatch_attn(dtype, dh, [&](auto tag, auto dh_c) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((attn_decode_kernel<T, decltype(dh_c)::value>), dim3((unsigned)(B * H)), dim3(64), 0, s, H, n_keys, t_max, (const T*)cache, ld,
                       k_off, q_off, v_off, mode, scale, (T*)out, ld_out);
    MST_CHECK_LAUNCH("attn_decode_kernel");
    return MST_OK;
  });
}

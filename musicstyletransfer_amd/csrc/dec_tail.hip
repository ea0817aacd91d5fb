// dec_tail.hip — mst_dec_tail_step: the last decoder layer's row-wise block, the loss and their backward in one launch, built from
// the tile code of the launches it replaces (ffn_ln.hpp, gemm_bce.hpp, gemm_ln.hpp).
#include "ffn_ln.hpp"
#include "gemm_bce.hpp"
#include "gemm_checks.hpp"

namespace mst {

// The last decoder layer's row-wise block, the loss and their backward in ONE launch (mst_dec_tail_step): width 128, 128 pitches,
// whole 64-row tiles. A workgroup runs on its tile what were three consecutive launches of identical grids:
//   1  mst_proj_ffn_ln_fwd            ffn_ln_body, forward with the projection head; x2 = LayerNorm-3's output stays in the x tile
//   2  mst_gemm_sigmoid_bce           logits = x2 W_out^T from that tile, bce_tile_finish; the logit gradient stays in the x tile
//   3  ... _dgrad_ln                  dh = LayerNorm-3 backward(dlogits W_out) (gemm_epilogue_ln mode 2); dh stays in the x tile
//   4  mst_ffn_ln_bwd                 ffn_ln_body, backward, its input tile in LDS
// Every tensor the separate launches store is stored here too (the weight-gradient launch and the layers below read them), and what a
// later phase reads back from global memory (h2 and its statistics, a, h1) was written by the SAME workgroup: a barrier orders it.
// Same tile per workgroup (xcd_chunk), same chunk rotation, same K order, same epilogues: bit-identical results. Two launch floors,
// two cold prologues and two chip-wide drains go. No data crosses between workgroups.
// The two middle GEMMs (K = 128: two 64-deep stages) take their A operand from the x tile with mma_stage's arithmetic, both weight
// stages loaded to registers while the previous phase's epilogue runs.
template <typename T>
__device__ __forceinline__ void tile128_load_w(const mst_gemm_args& g, u32x4 (&rw)[2][2]) {
  const T* __restrict__ W = reinterpret_cast<const T*>(g.B);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + i * 512, row = c / 8, ch = c % 8;
      rw[s][i] = *reinterpret_cast<const u32x4*>(W + (int64_t)row * g.ldb + s * 64 + ch * 8);
    }
}
// acc = A[64, 128] (x tile `sA`, row stride 136) x W[128, 128]^T (`rw`); the caller's barrier has freed the first 32 KB of smem and
// completed the tile; on return every wave has passed the last barrier
template <typename T>
__device__ __forceinline__ void tile128_gemm(unsigned char* smem, const T* sA, const u32x4 (&rw)[2][2], f32x4 (&acc)[2][2]) {
  constexpr int BN = 128, LDA = BN + 8, CHUNKS = 8, WTM = 32, WTN = 32, TM = 2, TN = 2, WGN = 4;
  typedef typename Act<T>::vec8 vec8;
  u32x4* sB = reinterpret_cast<u32x4*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, frow = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + i * 512, row = c / CHUNKS, ch = c % CHUNKS;
      sB[s * BN * CHUNKS + row * CHUNKS + (ch ^ (row & 7))] = rw[s][i];
    }
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u32x4* cB = sB + s * BN * CHUNKS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      vec8 xf[TM], wf[TN];
      const int kc = ks * 4 + fq;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        xf[i] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sA + (wm * WTM + i * 16 + frow) * LDA + s * 64 + kc * 8));
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 16 + frow;
        wf[j] = __builtin_bit_cast(vec8, cB[row * CHUNKS + (kc ^ (row & 7))]);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[j][i] = Act<T>::mfma16(wf[j], xf[i], acc[j][i]);
    }
  }
  __syncthreads();
}

constexpr size_t DEC_TAIL_F = 512;  // hidden width the launch is built for (host check)
constexpr size_t DEC_TAIL_BODY_LDS = (size_t)2 * 128 * 64 * 2 + (size_t)2 * 64 * (128 + 8) * 2 + DEC_TAIL_F * 4 + (size_t)6 * 128 * 4;
constexpr size_t DEC_TAIL_LDS = DEC_TAIL_BODY_LDS + ((size_t)128 + 3 * 128 + DEC_TAIL_F + 3 * 128) * 4;
static_assert(DEC_TAIL_LDS <= (size_t)48 * 1024 + (size_t)2 * (64 + 128) * 64 * 2 + (size_t)3 * 128 * 4, "no more LDS than the loss launch takes");

template <typename T, bool CNT>
__global__ __launch_bounds__(512) void dec_tail_kernel(mst_gemm_args proj, mst_ln_args ln1, mst_gemm_args ff1, mst_gemm_args ff2, mst_ln_args ln3,
                                                       mst_gemm_args out, mst_bce_args bce, mst_gemm_args odg, mst_ln_args ln3b,
                                                       mst_gemm_args f2d, mst_gemm_args f1d, mst_ln_args ln1b) {
  constexpr int BM = 64, BN = 128, WGM = 2, WGN = 4, LDA = BN + 8, F = (int)DEC_TAIL_F;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ __attribute__((aligned(16))) float red[bce_red_words(CNT)];
  T* sX = reinterpret_cast<T*>(smem + (size_t)2 * BN * 64 * 2 + (size_t)BM * LDA * 2);  // ffn_ln_body's x tile
  // behind the forward block's own LDS: the parameters of the three later phases — cold lines after every optimizer step, requested now
  float* sBiasO = reinterpret_cast<float*>(smem + DEC_TAIL_BODY_LDS);  // [BN] the output layer's bias
  float* sPar3 = sBiasO + BN;                                           // [3 BN] bias | gamma | 0 of LayerNorm-3 backward
  float* sPar4 = sPar3 + 3 * BN;                                        // [F][3 BN] the backward block's (ffn_ln_body's `par`)
  const int tid = threadIdx.x;
  for (int i = tid; i < BN; i += 512) {
    sBiasO[i] = out.bias ? out.bias[i] : 0.f;
    sPar3[i] = odg.bias ? odg.bias[i] : 0.f;
    sPar3[BN + i] = ln3b.gamma[i];
    sPar3[2 * BN + i] = 0.f;
    sPar4[F + i] = f1d.bias ? f1d.bias[i] : 0.f;
    sPar4[F + BN + i] = ln1b.gamma[i];
    sPar4[F + 2 * BN + i] = 0.f;
  }
  for (int i = tid; i < F; i += 512) sPar4[i] = f2d.bias ? f2d.bias[i] : 0.f;
  const int64_t m0 = xcd_chunk(blockIdx.x, gridDim.x) * BM;  // the tile's first LOGICAL row (the loss phases' index: b T + t)
  const mst_ln_bwd_in no_lead = {};
  u32x4 rw[2][2];
  f32x4 acc[2][2];
  // ---- 1: projection + LayerNorm-1, feed-forward, LayerNorm-3; x2 also lands in the x tile
  ffn_ln_body<T, BN, WGM, WGN, 1, false, true, true, false, true, false>(smem, ff1, ff2, ln3, no_lead, proj, ln1, nullptr,
                                                                         [&] { tile128_load_w<T>(out, rw); });
  __syncthreads();  // the x tile is complete, the staging tile dead
  // ---- 2: output layer + sigmoid + BCE; the logit gradient also lands in the x tile
  tile128_gemm<T>(smem, sX, rw, acc);
  tile128_load_w<T>(odg, rw);  // (the dgrad's weights: requested in front of the loss arithmetic)
  {
    float bias8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias8[e] = sBiasO[(tid % (BN / 8)) * 8 + e];
    bce_tile_finish<T, BN, 2, CNT>(out, bce, smem, red, reinterpret_cast<u32x4*>(sX), acc, m0, 0, bias8);
  }
  __syncthreads();  // the logit-gradient tile is complete, the staging tile dead
  // ---- 3: the output layer's input gradient + LayerNorm-3 backward; dh also lands in the x tile
  tile128_gemm<T>(smem, sX, rw, acc);
  gemm_epilogue_ln<T, BM, BN, WGM, WGN, 2>(odg, ln3b, smem, acc, m0, nullptr, 0, sX, LDA, sPar3);
  __syncthreads();  // dh is complete, the column-sum scratch dead
  // ---- 4: both feed-forward dgrads + LayerNorm-1 backward on the tile in LDS
  mst_gemm_args no_gemm = {};
  const mst_ln_args no_ln = {};
  ffn_ln_body<T, BN, WGM, WGN, 2, false, true, false, true, false, true>(smem, f2d, f1d, ln1b, no_lead, no_gemm, no_ln, sPar4, [] {});
}

template <typename T, bool CNT>
static int launch_dec_tail(const mst_gemm_args& proj, const mst_ln_args& ln1, const mst_gemm_args& ff1, const mst_gemm_args& ff2,
                           const mst_ln_args& ln3, const mst_gemm_args& out, const mst_bce_args& bce, const mst_gemm_args& odg,
                           const mst_ln_args& ln3b, const mst_gemm_args& f2d, const mst_gemm_args& f1d, const mst_ln_args& ln1b, hipStream_t s) {
  static size_t granted = 64 * 1024;
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&dec_tail_kernel<T, CNT>), DEC_TAIL_LDS, &granted, "dec_tail_kernel")) return rc;
  hipLaunchKernelGGL((dec_tail_kernel<T, CNT>), dim3((unsigned)(out.M / 64)), dim3(512), DEC_TAIL_LDS, s, proj, ln1, ff1, ff2, ln3, out, bce, odg,
                     ln3b, f2d, f1d, ln1b);
  MST_CHECK_LAUNCH("dec_tail_kernel");
  return MST_OK;
}

}  // namespace mst

using namespace mst;

extern "C" int mst_dec_tail_step(const mst_gemm_args* proj, const mst_ln_args* ln1, const mst_gemm_args* ff1, const mst_gemm_args* ff2,
                                 const mst_ln_args* ln3, const mst_gemm_args* out, const mst_bce_args* bce, const mst_gemm_args* out_dgrad,
                                 const mst_ln_args* ln3_bwd, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                                 const mst_ln_args* ln1_bwd, mst_stream_t stream) {
  const char* who = "mst_dec_tail_step";
  MST_CHECK_ARG(proj && ln1 && ff1 && ff2 && ln3 && out && bce && out_dgrad && ln3_bwd && ff2_dgrad && ff1_dgrad && ln1_bwd, "%s: null args", who);
  const mst_gemm_args &o = *out, &g = *out_dgrad, &d2 = *ff2_dgrad;
  const int64_t T = bce->T;
  // the ONE shape the launch is built for; anything else is the caller's three launches (no fallback here)
  MST_CHECK_ARG(ff2->N == 128 && ff1->K == 128 && proj->N == 128 && g.N == 128 && ff1_dgrad->N == 128,
                "%s: the model width must be 128 (got %lld)", who, (long long)ff2->N);
  MST_CHECK_ARG(ff1->N == 512 && d2.N == 512, "%s: the hidden width must be 512 (got %lld)", who, (long long)ff1->N);
  MST_CHECK_ARG(o.N == 128 && o.K == 128 && g.K == 128, "%s: the output layer must have 128 pitches (got %lld)", who, (long long)o.N);
  MST_CHECK_ARG(T > 0 && T % 64 == 0, "%s: T must be a multiple of 64 (got %lld)", who, (long long)T);
  MST_CHECK_ARG(o.M > 0 && o.M % 64 == 0 && o.M % T == 0 && ff1->M == o.M && ff2->M == o.M && proj->M == o.M && g.M == o.M && d2.M == o.M &&
                ff1_dgrad->M == o.M, "%s: every part works on the same whole 64-row tiles (M %lld)", who, (long long)o.M);
  auto groups = [&](int64_t rpg, int64_t stride, int64_t off) { return rpg == T && stride == T + 1 && off == 1; };
  MST_CHECK_ARG(groups(ff1->a_rows_per_group, ff1->a_group_stride, ff1->a_group_offset) &&
                groups(o.a_rows_per_group, o.a_group_stride, o.a_group_offset) &&
                groups(g.c_rows_per_group, g.c_group_stride, g.c_group_offset) &&
                groups(d2.a_rows_per_group, d2.a_group_stride, d2.a_group_offset) && g.a_rows_per_group <= 0,
                "%s: row groups must be (T, T + 1, 1) on all three parts", who);
  MST_CHECK_ARG(ln3_bwd->mode == 2 && ln3_bwd->mask_mode == 2, "%s: the LayerNorm-3 backward takes mask mode 2 (got %d)", who, (int)ln3_bwd->mask_mode);
  MST_CHECK_ARG(o.A == ln3->out && o.lda == ln3->ld_out, "%s: the output layer's A operand must be LayerNorm-3's output", who);
  MST_CHECK_ARG(o.C && g.A == o.C && g.lda == o.ldc, "%s: the output dgrad's A operand must be the logit gradient", who);
  MST_CHECK_ARG(d2.A == g.C && d2.lda == g.ldc, "%s: the A operand of the FF2 dgrad must be the output dgrad's dX_out", who);
  MST_CHECK_ARG(proj->dtype == o.dtype && g.dtype == o.dtype && d2.dtype == o.dtype && ff1->dtype == o.dtype && !g.a_u8,
                "%s: every part must share one activation dtype", who);
  int rc = check_ffn_ln(who, ff1, ff2, ln3, 1, nullptr, proj, ln1);
  if (rc == MST_OK) rc = check_gemm_bce(o, *bce);
  if (rc == MST_OK) rc = check_gemm_ln(g, *ln3_bwd);
  if (rc == MST_OK) rc = check_ffn_ln(who, ff2_dgrad, ff1_dgrad, ln1_bwd, 2);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(o.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T_;
    if (bce->counts) return launch_dec_tail<T_, true>(*proj, *ln1, *ff1, *ff2, *ln3, o, *bce, g, *ln3_bwd, d2, *ff1_dgrad, *ln1_bwd, s);
    return launch_dec_tail<T_, false>(*proj, *ln1, *ff1, *ff2, *ln3, o, *bce, g, *ln3_bwd, d2, *ff1_dgrad, *ln1_bwd, s);
  });
}

// gemm_bce.hip — the output layer and its loss in one launch (gemm_bce.hpp: the tile code, where the design is described):
// mst_gemm_sigmoid_bce, and mst_gemm_sigmoid_bce_dgrad_ln, which adds the first launch of the backward pass.
#include "gemm_bce.hpp"
#include "gemm_ln.hpp"
#include "gemm_checks.hpp"

namespace mst {

template <typename T, int BN, bool CNT>
__global__ __launch_bounds__(512) void gemm_bce_kernel(mst_gemm_args a, mst_bce_args q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ __attribute__((aligned(16))) float red[bce_red_words(CNT)];
  gemm_bce_tile<T, BN, false, CNT>(a, q, smem, red, nullptr);
}

// mst_gemm_sigmoid_bce_dgrad_ln: the loss launch above followed IN THE SAME WORKGROUP by the first launch of the backward pass — the
// output layer's input gradient d(dec_out) = dlogits W_out (K = the 128 pitches of the tile the workgroup has just produced) with the
// last decoder layer's LayerNorm-3 backward in its epilogue (mst_gemm_nt_ln mode 2). The logit gradient still goes to HBM (the
// weight-gradient launch reads it) but is not read back here, and a launch of the dependent chain disappears.
// LDS: [0, 48 K) the first GEMM's stages, then its fp32 staging tile (33.8 K), later the LayerNorm epilogue's; [48 K, 64 K) the kept
// logit-gradient tile (two 64 x 64 stages); [64 K, 96 K) the second GEMM's weight stages; then bias | gamma | beta.
template <typename T, bool CNT>
__global__ __launch_bounds__(512) void gemm_bce_dgrad_ln_kernel(mst_gemm_args a, mst_bce_args q, mst_gemm_args g2, mst_ln_args l) {
  constexpr int BM = 64, BN = 128, WGM = 2, WGN = 4;
  constexpr size_t OFF2 = 48 * 1024, END2 = OFF2 + (size_t)2 * (BM + BN) * 64 * 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ __attribute__((aligned(16))) float red[bce_red_words(CNT)];
  float* sPar = reinterpret_cast<float*>(smem + END2);
  for (int i = threadIdx.x; i < BN; i += 512) {  // (cold lines: requested now, read by the LayerNorm epilogue)
    sPar[i] = g2.bias ? g2.bias[i] : 0.f;
    sPar[BN + i] = l.gamma[i];
    sPar[2 * BN + i] = 0.f;
  }
  gemm_bce_tile<T, BN, true, CNT>(a, q, smem, red, reinterpret_cast<u32x4*>(smem + OFF2));
  __syncthreads();  // the kept tile is complete, the staging tile dead
  f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
  int64_t m0, n0;
  gemm_mainloop<T, BM, BN, WGM, WGN, 64, true, false, true>(g2, smem + OFF2, acc, m0, n0);
  gemm_epilogue_ln<T, BM, BN, WGM, WGN, 2>(g2, l, smem, acc, m0, nullptr, 0, nullptr, 0, sPar);
}

template <typename T, bool CNT>
static int launch_gemm_bce_dgrad_ln(const mst_gemm_args& a, const mst_bce_args& q, const mst_gemm_args& g2, const mst_ln_args& l, hipStream_t s) {
  const size_t lds = (size_t)48 * 1024 + (size_t)2 * (64 + 128) * 64 * 2 + (size_t)3 * 128 * 4;
  static size_t granted = 64 * 1024;
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&gemm_bce_dgrad_ln_kernel<T, CNT>), lds, &granted, "gemm_bce_dgrad_ln_kernel")) return rc;
  hipLaunchKernelGGL((gemm_bce_dgrad_ln_kernel<T, CNT>), dim3((unsigned)cdiv(a.M, 64)), dim3(512), lds, s, a, q, g2, l);
  MST_CHECK_LAUNCH("gemm_bce_dgrad_ln_kernel");
  return MST_OK;
}

template <typename T, int BN, bool CNT>
static int launch_gemm_bce(const mst_gemm_args& a, const mst_bce_args& q, hipStream_t s) {
  const size_t lds_loop = (size_t)2 * (64 + BN) * 64 * 2, lds_epi = (size_t)64 * (BN + 4) * 4;
  const size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  static size_t granted = 64 * 1024;
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&gemm_bce_kernel<T, BN, CNT>), lds, &granted, "gemm_bce_kernel")) return rc;
  hipLaunchKernelGGL((gemm_bce_kernel<T, BN, CNT>), dim3((unsigned)(cdiv(a.M, 64) * (a.N / BN))), dim3(512), lds, s, a, q);
  MST_CHECK_LAUNCH("gemm_bce_kernel");
  return MST_OK;
}

int check_gemm_bce(const mst_gemm_args& a, const mst_bce_args& q) {
  MST_CHECK_ARG(a.M > 0 && a.K > 0 && a.K % 8 == 0 && a.lda % 8 == 0 && a.ldb % 8 == 0 && a.A && a.B,
                "mst_gemm_sigmoid_bce: bad GEMM operands");
  MST_CHECK_ARG(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0), "mst_gemm_sigmoid_bce: operands must be 16-byte aligned");
  MST_CHECK_ARG(a.N == 128 || (a.N > 0 && a.N % 256 == 0), "mst_gemm_sigmoid_bce: the row of pitches must be 128 or a multiple of 256 wide (got %lld): use "
                "mst_gemm_nt + mst_sigmoid_bce for other widths", (long long)a.N);
  MST_CHECK_ARG(a.N <= 256 || !q.downweight, "mst_gemm_sigmoid_bce: the label down-weighting counts a sample's positives in every workgroup — rows wider than "
                "one tile (256) take mst_gemm_nt + mst_sigmoid_bce");
  MST_CHECK_ARG(q.T > 0 && q.T % 64 == 0 && a.M % q.T == 0, "mst_gemm_sigmoid_bce: T must be a multiple of 64 and divide M (a tile holds one sample's rows)");
  MST_CHECK_ARG(!a.c_f32 && !a.resid && !a.gate && !a.rowadd && !a.grpadd && a.act == MST_ACT_NONE && a.dropout_p == 0.f && !a.self_resid &&
                a.c_rows_per_group <= 0 && !a.a_u8, "mst_gemm_sigmoid_bce: only bias, alpha and an A row remap are supported");
  MST_CHECK_ARG(q.labels && q.loss && (uintptr_t)q.labels % 8 == 0, "mst_gemm_sigmoid_bce: labels / loss missing or labels not 8-byte aligned");
  MST_CHECK_ARG(!a.C || (a.ldc % 8 == 0 && a.ldc >= a.N && (uintptr_t)a.C % 16 == 0), "mst_gemm_sigmoid_bce: bad dlogits layout");
  MST_CHECK_ARG(!q.probs || (q.ldp % 8 == 0 && q.ldp >= a.N && (uintptr_t)q.probs % 16 == 0), "mst_gemm_sigmoid_bce: bad probs layout");
  MST_CHECK_ARG(!q.logits || (q.ldl % 8 == 0 && q.ldl >= a.N && (uintptr_t)q.logits % 16 == 0), "mst_gemm_sigmoid_bce: bad logits layout");
  MST_CHECK_ARG((uintptr_t)q.counts % 16 == 0, "mst_gemm_sigmoid_bce: counts must be 16-byte aligned");
  return MST_OK;
}

// one launch of mst_gemm_sigmoid_bce_dgrad_ln: 128 pitches, width 128, whole 64-row tiles, and the second GEMM's A operand IS the first
// one's logit gradient
static bool bce_dgrad_ln_one_launch(const mst_gemm_args& a, const mst_gemm_args& g2, const mst_ln_args& l) {
  return a.N == 128 && g2.N == 128 && g2.K == 128 && g2.M == a.M && a.M % 64 == 0 && l.mode == 2 && a.C && g2.A == a.C &&
         g2.lda == a.ldc && g2.dtype == a.dtype && g2.a_rows_per_group <= 0 && !g2.a_u8;
}

}  // namespace mst

using namespace mst;

extern "C" int mst_gemm_sigmoid_bce_form(const mst_gemm_args* args, const mst_bce_args* bce, const mst_gemm_args* dgrad,
                                         const mst_ln_args* ln, int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_gemm_sigmoid_bce_form: null form");
  const bool pair = dgrad != nullptr || ln != nullptr;
  if (pair) MST_CHECK_ARG(args != nullptr && bce != nullptr && dgrad != nullptr && ln != nullptr, "mst_gemm_sigmoid_bce_dgrad_ln: null args");
  else MST_CHECK_ARG(args != nullptr && bce != nullptr, "mst_gemm_sigmoid_bce: null args");
  int rc = check_gemm_bce(*args, *bce);
  if (rc == MST_OK && pair) rc = check_gemm_ln(*dgrad, *ln);
  if (rc) return rc;
  return dispatch_act(args->dtype, [&](auto) -> int {
    const int64_t BN = args->N % 256 == 0 ? 256 : 128;
    form[0] = BN;
    form[1] = args->N / BN;
    form[2] = !pair ? 0 : bce_dgrad_ln_one_launch(*args, *dgrad, *ln) ? 1 : 2;
    return MST_OK;
  });
}

extern "C" int mst_gemm_sigmoid_bce(const mst_gemm_args* args, const mst_bce_args* bce, mst_stream_t stream) {
  MST_CHECK_ARG(args != nullptr && bce != nullptr, "mst_gemm_sigmoid_bce: null args");
  const mst_gemm_args& a = *args;
  const mst_bce_args& q = *bce;
  int rc = check_gemm_bce(a, q);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    if (q.counts) return a.N % 256 == 0 ? launch_gemm_bce<T, 256, true>(a, q, s) : launch_gemm_bce<T, 128, true>(a, q, s);
    return a.N % 256 == 0 ? launch_gemm_bce<T, 256, false>(a, q, s) : launch_gemm_bce<T, 128, false>(a, q, s);
  });
}

extern "C" int mst_gemm_sigmoid_bce_dgrad_ln(const mst_gemm_args* args, const mst_bce_args* bce, const mst_gemm_args* dgrad,
                                             const mst_ln_args* ln, mst_stream_t stream) {
  MST_CHECK_ARG(args != nullptr && bce != nullptr && dgrad != nullptr && ln != nullptr, "mst_gemm_sigmoid_bce_dgrad_ln: null args");
  const mst_gemm_args &a = *args, &g2 = *dgrad;
  const mst_bce_args& q = *bce;
  const mst_ln_args& l = *ln;
  int rc = check_gemm_bce(a, q);
  if (rc == MST_OK) rc = check_gemm_ln(g2, l);
  if (rc) return rc;
  if (!bce_dgrad_ln_one_launch(a, g2, l)) {
    rc = mst_gemm_sigmoid_bce(args, bce, stream);
    return rc != MST_OK ? rc : mst_gemm_nt_ln(dgrad, ln, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    return q.counts ? launch_gemm_bce_dgrad_ln<T, true>(a, q, g2, l, s) : launch_gemm_bce_dgrad_ln<T, false>(a, q, g2, l, s);
  });
}

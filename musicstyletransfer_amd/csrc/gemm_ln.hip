// gemm_ln.hip — mst_gemm_nt_ln: a GEMM (gemm_nt.hip's main loop) with LayerNorm, forward or backward, as its epilogue
// (gemm_ln.hpp: gemm_epilogue_ln). The tile spans the whole output row, so the row width is the model's: 128 or 256.
#include "gemm_ln.hpp"
#include "gemm_checks.hpp"

namespace mst {

template <typename T, int BM, int BN, int WGM, int WGN, int MODE>
__global__ __launch_bounds__(WGM * WGN * 64) void gemm_nt_ln_kernel(mst_gemm_args a, mst_ln_args l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
  int64_t m0, n0;
  // bias | gamma | beta wait in LDS behind the K-loop tiles / the staging tile (launch_gemm_ln sizes it): cold lines, requested now
  constexpr size_t LOOP_B = (size_t)2 * (BM + BN) * 64 * 2, EPI_B = (size_t)BM * (BN + 4) * 4;
  float* sPar = reinterpret_cast<float*>(smem + (LOOP_B > EPI_B ? LOOP_B : EPI_B));
  for (int i = threadIdx.x; i < BN; i += WGM * WGN * 64) {
    sPar[i] = a.bias ? a.bias[i] : 0.f;
    sPar[BN + i] = l.gamma[i];
    sPar[2 * BN + i] = (MODE == 1) ? l.beta[i] : 0.f;
  }
  gemm_mainloop<T, BM, BN, WGM, WGN, 64>(a, smem, acc, m0, n0);
  gemm_epilogue_ln<T, BM, BN, WGM, WGN, MODE>(a, l, smem, acc, m0, nullptr, 0, nullptr, 0, sPar);
}

template <typename T, int BM, int BN, int WGM, int WGN>
static int launch_gemm_ln(const mst_gemm_args& a, const mst_ln_args& l, hipStream_t s) {
  const size_t lds_loop = (size_t)2 * (BM + BN) * 64 * 2, lds_epi = (size_t)BM * (BN + 4) * 4;
  const size_t lds = (lds_loop > lds_epi ? lds_loop : lds_epi) + (size_t)3 * BN * 4;  // + bias | gamma | beta
  dim3 grid((unsigned)cdiv(a.M, BM)), block(WGM * WGN * 64);
  const int mi = l.mode == 2 ? 1 : 0;
  const void* fn = mi ? reinterpret_cast<const void*>(&gemm_nt_ln_kernel<T, BM, BN, WGM, WGN, 2>)
                      : reinterpret_cast<const void*>(&gemm_nt_ln_kernel<T, BM, BN, WGM, WGN, 1>);
  static size_t granted[2] = {64 * 1024, 64 * 1024};
  if (const int rc = lds_opt_in(fn, lds, &granted[mi], "gemm_nt_ln_kernel")) return rc;
  if (mi) hipLaunchKernelGGL((gemm_nt_ln_kernel<T, BM, BN, WGM, WGN, 2>), grid, block, lds, s, a, l);
  else hipLaunchKernelGGL((gemm_nt_ln_kernel<T, BM, BN, WGM, WGN, 1>), grid, block, lds, s, a, l);
  MST_CHECK_LAUNCH("gemm_nt_ln_kernel");
  return MST_OK;
}

int check_gemm_ln(const mst_gemm_args& a, const mst_ln_args& l) {
  int rc = check_gemm_common(a);
  if (rc) return rc;
  MST_CHECK_ARG(a.N == 256 || a.N == 128, "mst_gemm_nt_ln: the row width N must be 128 or 256 (got %lld): use mst_gemm_nt + "
                "mst_layernorm_* for other widths", (long long)a.N);
  MST_CHECK_ARG(l.mode == 1 || l.mode == 2, "mst_gemm_nt_ln: mode must be 1 (forward) or 2 (backward)");
  MST_CHECK_ARG(!a.c_f32 && !a.gate && !a.rowadd && !a.grpadd && a.act == MST_ACT_NONE,
                "mst_gemm_nt_ln: fp32 output, gate, rowadd, grpadd and activations are not supported in the fused form");
  MST_CHECK_ARG(a.ldc % 8 == 0 && a.ldc >= a.N, "mst_gemm_nt_ln: ldc must be a multiple of 8 and >= N");
  MST_CHECK_ARG(!a.resid || (a.ldr % 8 == 0 && a.ldr >= a.N && (uintptr_t)a.resid % 16 == 0), "mst_gemm_nt_ln: bad residual layout");
  MST_CHECK_ARG(l.gamma && l.mean && l.rstd, "mst_gemm_nt_ln: gamma / mean / rstd are required");
  if (l.mode == 1) {
    MST_CHECK_ARG(l.beta && l.out && l.ld_out % 8 == 0 && l.ld_out >= a.N && (uintptr_t)l.out % 16 == 0, "mst_gemm_nt_ln: forward needs beta and out");
  } else {
    MST_CHECK_ARG(l.x && l.ld_x % 8 == 0 && (uintptr_t)l.x % 16 == 0 && (l.partials || (l.dgamma && l.dbeta)),
                  "mst_gemm_nt_ln: backward needs x and dgamma + dbeta (or partials)");
    MST_CHECK_ARG((uintptr_t)l.partials % 16 == 0, "mst_gemm_nt_ln: partials must be 16-byte aligned");
    MST_CHECK_ARG(l.mask_mode >= 0 && l.mask_mode <= 2, "mst_gemm_nt_ln: mask_mode must be 0, 1 or 2");
    MST_CHECK_ARG(l.mask_mode != 1 || (l.out && l.ld_out % 8 == 0 && l.ld_out >= a.N && (uintptr_t)l.out % 16 == 0),
                  "mst_gemm_nt_ln: mask_mode 1 needs out");
    MST_CHECK_ARG(!a.self_resid, "mst_gemm_nt_ln: self_resid belongs to the forward form");
  }
  return MST_OK;
}

}  // namespace mst

using namespace mst;

extern "C" int64_t mst_gemm_nt_ln_parts(int64_t M) { return M > 0 ? cdiv(M, 64) : 0; }  // launch_gemm_ln's 64-row tiles

extern "C" int mst_gemm_nt_ln(const mst_gemm_args* args, const mst_ln_args* ln, mst_stream_t stream) {
  MST_CHECK_ARG(args != nullptr && ln != nullptr, "mst_gemm_nt_ln: null args");
  const mst_gemm_args& a = *args;
  const mst_ln_args& l = *ln;
  int rc = check_gemm_ln(a, l);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    // 8 waves on a 64-row x full-width tile (32-row tiles, two or three workgroups per CU, measured 8-25 % slower)
    if (a.N == 256) return launch_gemm_ln<T, 64, 256, 2, 4>(a, l, s);
    return launch_gemm_ln<T, 64, 128, 2, 4>(a, l, s);
  });
}

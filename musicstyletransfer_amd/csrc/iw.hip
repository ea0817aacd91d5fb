// iw.hip — the importance-weighted bound on log p(x) from K posterior draws (mst_iw_fold, mst_iw_finish; include/mst_hip.h states
// the arithmetic). Both launches are bookkeeping-sized: B waves of fp64 work per draw, one workgroup at the end. What matters is that
// a validation set is folded and summed on the device, with no host round trip per draw, and that the same inputs give the same bits.
#include <math.h>
#include "common.hpp"

namespace mst {

constexpr int IW_WAVES = 4, IW_THREADS = IW_WAVES * WAVE;  // samples per workgroup of the fold: one wave each
constexpr int IW_FIN_THREADS = 256;

// the fixed wave reduction of the header: xor butterflies 32, 16, 8, 4, 2, 1; every lane ends with the same bits
__device__ __forceinline__ double iw_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

__global__ __launch_bounds__(IW_THREADS) void iw_fold_kernel(int64_t B, int64_t Z, const float* __restrict__ eps, int64_t ld_eps,
                                                              const float* __restrict__ sigma, int64_t ld_sigma,
                                                              const float* __restrict__ z, int64_t ld_z, const float* __restrict__ recon,
                                                              double recon_scale, double* __restrict__ state) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t b = (int64_t)blockIdx.x * IW_WAVES + (threadIdx.x >> 6);  // (wave-uniform)
  if (b >= B) return;
  const float *e = eps + b * ld_eps, *sg = sigma + b * ld_sigma, *zz = z + b * ld_z;
  double part = 0.0;
  for (int64_t d = lane; d < Z; d += WAVE) {  // lane-strided, ascending
    const double ed = (double)e[d], zd = (double)zz[d], sd = (double)sg[d];
    part += 0.5 * ed * ed - 0.5 * zd * zd + log(fabs(sd));
  }
  const double lat = iw_wave_sum(part);
  if (lane != 0) return;
  // the online update: this lane owns the six cells of the sample
  double* st = state + b * 6;
  const double lw = -recon_scale * (double)recon[b] + lat;
  if (!isfinite(lw)) {  // a bad draw enters n_bad only
    st[5] += 1.0;
    return;
  }
  const double n = st[4];
  double m, s, s2;
  if (n == 0.0) {
    m = lw, s = 1.0, s2 = 1.0;
  } else {
    m = st[0], s = st[1], s2 = st[2];
    if (lw > m) {
      s = s * exp(m - lw) + 1.0;
      s2 = s2 * exp(2.0 * (m - lw)) + 1.0;
      m = lw;
    } else {
      const double r = exp(lw - m);
      s += r;
      s2 += r * r;
    }
  }
  st[0] = m, st[1] = s, st[2] = s2;
  st[3] += lw;
  st[4] = n + 1.0;
}

__global__ __launch_bounds__(IW_FIN_THREADS) void iw_finish_kernel(int64_t B, const double* __restrict__ state, double* __restrict__ out,
                                                                    double* __restrict__ acc) {
  const double dnan = __builtin_nan("");
  for (int64_t b = threadIdx.x; b < B; b += IW_FIN_THREADS) {
    const double* st = state + b * 6;
    const double m = st[0], s = st[1], s2 = st[2], sum_lw = st[3], n = st[4], n_bad = st[5];
    const bool valid = n > 0.0 && !(n_bad > 0.0);
    double* o = out + b * 4;
    o[0] = valid ? m + log(s) - log(n) : dnan;
    o[1] = valid ? sum_lw / n : dnan;
    o[2] = valid ? s * s / s2 : dnan;
    o[3] = n;
  }
  __syncthreads();  // (the rows above are this workgroup's own writes)
  if (threadIdx.x != 0) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, cnt = 0.0, bad = 0.0;
  for (int64_t b = 0; b < B; ++b) {  // ascending sample order, one thread
    const double* st = state + b * 6;
    const double* o = out + b * 4;
    if (st[4] > 0.0 && !(st[5] > 0.0)) {
      a0 += o[0], a1 += o[1], a2 += o[2], a3 += o[3], cnt += 1.0;
    } else {
      bad += 1.0;
    }
  }
  acc[0] += a0, acc[1] += a1, acc[2] += a2, acc[3] += a3, acc[4] += cnt, acc[5] += bad;
}

}  // namespace mst

using namespace mst;

extern "C" int mst_iw_fold(int64_t B, int64_t Z, const float* eps, int64_t ld_eps, const float* sigma, int64_t ld_sigma, const float* z,
                           int64_t ld_z, const float* recon, double recon_scale, double* state, mst_stream_t stream) {
  MST_CHECK_ARG(eps && sigma && z && recon && state, "mst_iw_fold: null pointer");
  MST_CHECK_ARG(B > 0 && Z > 0 && B < (1ll << 31), "mst_iw_fold: B and Z must be positive (B below 2^31)");
  MST_CHECK_ARG(ld_eps >= Z && ld_sigma >= Z && ld_z >= Z, "mst_iw_fold: ld_eps / ld_sigma / ld_z < Z");
  MST_CHECK_ARG((uintptr_t)state % 16 == 0, "mst_iw_fold: state must be 16-byte aligned");
  MST_CHECK_ARG(isfinite(recon_scale) && recon_scale > 0.0, "mst_iw_fold: recon_scale must be finite and > 0 (got %g)", recon_scale);
  hipLaunchKernelGGL(iw_fold_kernel, dim3((unsigned)cdiv(B, IW_WAVES)), dim3(IW_THREADS), 0, (hipStream_t)stream, B, Z, eps, ld_eps, sigma,
                     ld_sigma, z, ld_z, recon, recon_scale, state);
  MST_CHECK_LAUNCH("iw_fold_kernel");
  return MST_OK;
}

extern "C" int mst_iw_finish(int64_t B, const double* state, double* out, double* acc, mst_stream_t stream) {
  MST_CHECK_ARG(state && out && acc, "mst_iw_finish: null pointer");
  MST_CHECK_ARG(B > 0, "mst_iw_finish: B must be positive");
  MST_CHECK_ARG((uintptr_t)state % 16 == 0, "mst_iw_finish: state must be 16-byte aligned");
  MST_CHECK_ARG((uintptr_t)out % 8 == 0 && (uintptr_t)acc % 8 == 0, "mst_iw_finish: out and acc must be 8-byte aligned");
  hipLaunchKernelGGL(iw_finish_kernel, dim3(1), dim3(IW_FIN_THREADS), 0, (hipStream_t)stream, B, state, out, acc);
  MST_CHECK_LAUNCH("iw_finish_kernel");
  return MST_OK;
}

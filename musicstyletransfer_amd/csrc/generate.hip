// generate.hip — decoder row 0 from a latent RECIPE (mst_latent_rows): what mst_latent_fwd does for z = mu + eps * sigma of an encoded
// batch and the batch's own class, for any z a user of the latent space asks for. Per output row n (one workgroup, fp32 math):
//   base  = interp(zsrc[a[n]], zsrc[b[n]], w[n])                 a[n] < 0: base = 0 (a draw from the prior)
//   scale = ssrc ? lerp(ssrc[a[n]], ssrc[b[n]], w[n]) : 1        (a[n] < 0: 1)
//   z     = base + tau * eps(seed, site, (row0 + n) * Z + k) * scale                  (tau = 0: no draw is made)
//   row   = alpha_d * (z . Wh^T + bh + (1 - cw[n]) * cls_d[ca[n]] + cw[n] * cls_d[cb[n]]) + pos_d[0]   -> act dtype, one rounding
// interp is linear or spherical. The spherical form returns its end points exactly (w <= 0, w >= 1 are copies) and is the linear one
// where the angle between the two sources has no usable sine: either is zero, or |cos| >= 1 - 2^-16 (parallel / antiparallel within
// what an fp32 dot product of the two can tell).
// eps is the step's Gaussian (step_begin.hpp: Box-Muller over dropout_hash, element g of the stream is the cosine (g even) or sine
// (g odd) branch of pair g >> 1), indexed by the GLOBAL row number row0 + n: N rows in one call or in chunks are the same vectors.
// The product with Wh is latent_fwd.hpp's wave_dots_pre / wave_dots — per output the same lane products and the same cross-lane sum
// as mst_latent_fwd's row 0, whatever the number of waves — so the identity recipe (a = b = n, w = cw = tau = 0 on an encode's mu)
// gives that launch's row. Indices are clamped to their tables (a row index >= M reads row M - 1): a recipe is validated where it is
// built, on the host (generate.py); the clamp only keeps a bad one inside the buffers.
#include <math.h>
#include "common.hpp"
#include "latent_fwd.hpp"

namespace mst {

constexpr int ROWS_THREADS = 256;
constexpr float SLERP_COS_MAX = 1.0f - 1.0f / 65536.0f;  // 1 - 2^-16

struct LatentRowsArgs {
  int64_t N, M; int Z, Dd;
  const float *zsrc, *ssrc; const int32_t *a, *b; const float* w; int mode;
  float tau; uint64_t seed; const uint64_t* seed_ptr; uint32_t site; int64_t row0;
  const float *Wh, *bh; const int32_t *ca, *cb; const float* cw; const float* cls_d; int64_t ld_cls; int n_classes;
  const float* pos_d; float alpha_d;
  float* z_out; void* dec_in; int64_t dec_stride;
};

__device__ __forceinline__ float gauss_at(uint64_t s, uint32_t site, uint64_t g) {
  const uint64_t p = g >> 1;
  const uint32_t ha = dropout_hash(s, site, 2 * p);
  const uint32_t hb = dropout_hash(s, site, 2 * p + 1);
  const float u1 = ((float)(ha >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  const float u2 = (float)(hb >> 8) * (1.0f / 16777216.0f);           // [0, 1)
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (g & 1) ? r * sn : r * cs;
}

template <typename T>
__global__ __launch_bounds__(ROWS_THREADS) void latent_rows_kernel(LatentRowsArgs q) {
  extern __shared__ float zs[];  // [Z]
  __shared__ float red[3][ROWS_THREADS / 64];
  constexpr int NW = ROWS_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = blockIdx.x;
  const int Z = q.Z, Dd = q.Dd;
  const int32_t ai = q.a ? q.a[n] : -1;
  const bool prior = ai < 0 || !q.zsrc || q.M <= 0;
  const int64_t ia = prior ? 0 : (ai < q.M ? ai : q.M - 1);
  int64_t ib = ia;
  float wt = 0.f;
  if (!prior) {
    const int32_t bi = q.b[n];
    ib = bi < 0 ? 0 : (bi < q.M ? bi : q.M - 1);
    wt = q.w[n];
  }
  const float* za = q.zsrc + ia * Z;
  const float* zb = q.zsrc + ib * Z;
  // the two factors of the interpolation (linear: 1 - w, w)
  float fa = 1.f - wt, fb = wt;
  if (!prior && q.mode == 1) {
    if (wt <= 0.f) { fa = 1.f; fb = 0.f; }
    else if (wt >= 1.f) { fa = 0.f; fb = 1.f; }
    else {
      float dot = 0.f, na = 0.f, nb = 0.f;
      for (int k = tid; k < Z; k += ROWS_THREADS) {
        const float x = za[k], y = zb[k];
        dot = fmaf(x, y, dot); na = fmaf(x, x, na); nb = fmaf(y, y, nb);
      }
      dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
      if (lane == 0) { red[0][wave] = dot; red[1][wave] = na; red[2][wave] = nb; }
      __syncthreads();
      dot = na = nb = 0.f;
      for (int v = 0; v < NW; ++v) { dot += red[0][v]; na += red[1][v]; nb += red[2][v]; }  // (every thread, in wave order)
      const float den = sqrtf(na) * sqrtf(nb);
      const float c = den > 0.f ? dot / den : 2.f;
      if (den > 0.f && isfinite(c) && fabsf(c) < SLERP_COS_MAX) {
        const float om = acosf(c), inv = 1.f / sinf(om);
        fa = sinf((1.f - wt) * om) * inv;
        fb = sinf(wt * om) * inv;
      }
    }
  }
  const uint64_t s = q.seed ^ (q.seed_ptr ? q.seed_ptr[0] : 0ull);
  for (int k = tid; k < Z; k += ROWS_THREADS) {
    float base = 0.f, scale = 1.f;
    if (!prior) {
      base = fa * za[k] + fb * zb[k];
      if (q.ssrc) scale = (1.f - wt) * q.ssrc[ia * Z + k] + wt * q.ssrc[ib * Z + k];
    }
    float zz = base;
    if (q.tau > 0.f) zz = base + q.tau * gauss_at(s, q.site, (uint64_t)(q.row0 + n) * (uint64_t)Z + (uint64_t)k) * scale;
    q.z_out[n * Z + k] = zz;
    zs[k] = zz;
  }
  __syncthreads();
  auto clampc = [&](int32_t c) { return c < 0 ? 0 : (c < q.n_classes ? c : q.n_classes - 1); };
  const float* cla = q.cls_d + (int64_t)clampc(q.ca[n]) * q.ld_cls;
  const float* clb = q.cls_d + (int64_t)clampc(q.cb[n]) * q.ld_cls;
  const float cwt = q.cw[n];
  T* __restrict__ out = reinterpret_cast<T*>(q.dec_in) + n * q.dec_stride;
  auto emit = [&](int j, float acc) {
    const float cls = (1.f - cwt) * cla[j] + cwt * clb[j];
    out[j] = from_f32<T>(q.alpha_d * (acc + q.bh[j] + cls) + q.pos_d[j]);
  };
  if (Z <= 64 * PRE_C) wave_dots_pre<OPW, PRE_C>(zs, Z, q.Wh, Dd, wave, NW, lane, emit);
  else wave_dots<OPW>(zs, Z, q.Wh, Dd, wave, NW, lane, emit);
}

}  // namespace mst

using namespace mst;

extern "C" int mst_latent_rows(int dtype, int64_t N, int64_t M, int64_t Z, int64_t Dd, const float* zsrc, const float* ssrc, const int32_t* a,
                               const int32_t* b, const float* w, int mode, float tau, uint64_t seed, const uint64_t* seed_ptr, uint32_t site,
                               int64_t row0, const float* Wh, const float* bh, const int32_t* ca, const int32_t* cb, const float* cw,
                               const float* cls_d, int64_t ld_cls, int64_t n_classes, const float* pos_d, float alpha_d, float* z_out,
                               void* dec_in, int64_t dec_stride, mst_stream_t stream) {
  MST_CHECK_ARG(N > 0 && N < (1ll << 31) && M >= 0 && Z > 0 && Dd > 0 && row0 >= 0, "mst_latent_rows: sizes must be positive (row0 >= 0)");
  MST_CHECK_ARG((size_t)Z * sizeof(float) <= 60000, "mst_latent_rows: latent size too large for one workgroup");
  MST_CHECK_ARG(mode == 0 || mode == 1, "mst_latent_rows: mode must be 0 (linear) or 1 (spherical)");
  MST_CHECK_ARG(tau >= 0.f && tau <= 3.0e38f, "mst_latent_rows: tau < 0 (or not finite)");
  MST_CHECK_ARG(M == 0 || (zsrc && a && b && w), "mst_latent_rows: null source vectors or source index / weight arrays (M > 0)");
  MST_CHECK_ARG(M > 0 || !ssrc, "mst_latent_rows: a scale source without source vectors");
  MST_CHECK_ARG(ca && cb && cw, "mst_latent_rows: class index / weight arrays missing");
  MST_CHECK_ARG(Wh && bh && cls_d && pos_d && z_out && dec_in, "mst_latent_rows: null pointer");
  MST_CHECK_ARG(n_classes > 0 && n_classes < (1ll << 31) && ld_cls >= Dd && dec_stride >= Dd,
                "mst_latent_rows: class table of no rows, or a row stride below the decoder width");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    LatentRowsArgs q = {N, M, (int)Z, (int)Dd, zsrc, ssrc, a, b, w, mode, tau, seed, seed_ptr, site, row0, Wh, bh, ca, cb, cw, cls_d, ld_cls,
                        (int)n_classes, pos_d, alpha_d, z_out, dec_in, dec_stride};
    hipLaunchKernelGGL((latent_rows_kernel<T>), dim3((unsigned)N), dim3(ROWS_THREADS), sizeof(float) * (size_t)Z, (hipStream_t)stream, q);
    MST_CHECK_LAUNCH("latent_rows_kernel");
    return MST_OK;
  });
}

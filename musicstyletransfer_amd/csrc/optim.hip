// optim.hip — multi-tensor Adam over one flat fp32 bucket + 16-bit shadow maintenance.
//
// Replaces gluon.Trainer.step(batch_size) → mxnet.optimizer.Adam → adam_update, called once per
// parameter tensor in the reference (58 launches; trainer.py:94-101,177), by ONE launch over the
// flat parameter / gradient / moment buffers (the same flat gradient buffer RCCL all-reduces):
//   g   = clip(grad * rescale + wd * w, ±clip)            (clip < 0: no clipping)
//   m   = b1*m + (1-b1)*g ;  v = b2*v + (1-b2)*g*g
//   w  -= lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
// HBM-bound: 16 B/param read (w,g,m,v) + 12 B/param written (w,m,v) + 2 B/param 16-bit shadow; in the averaging form
// (mst_adam_args.ema) 4 + 4 B/param more for the exponential moving average of the weights, which the same thread keeps.
// The step counter lives on the device and is advanced by a 1-thread kernel in the same stream,
// so a captured graph replays with the right bias correction.
#include <math.h>
#include "common.hpp"
#include "loss_combine.hpp"
#include "shadows.hpp"

namespace mst {

// state[0] = step count t (int32), state[1] = bits of lr_t (float)
__global__ void adam_tick_kernel(int32_t* state, double lr, double beta1, double beta2) {
  const int t = state[0] + 1;
  state[0] = t;
  const double c1 = 1.0 - pow(beta1, (double)t);
  const double c2 = 1.0 - pow(beta2, (double)t);
  reinterpret_cast<float*>(state)[1] = (float)(lr * sqrt(c2) / c1);
}

// transposed shadows kept current by the optimizer itself (mst_adam_args.emb): up to two matrices, flat offsets relative to the
// launch's own `w`
struct AdamEmb {
  int n;
  int64_t lo[2], hi[2], dst[2];
  int32_t rows[2], cols[2];
  void* wt16;
};
template <typename T>
__device__ __forceinline__ void adam_emb_store(const AdamEmb& e, int64_t i, float wnew) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (j < e.n && i >= e.lo[j] && i < e.hi[j]) {
      const uint32_t k = (uint32_t)(i - e.lo[j]);
      const uint32_t r = k / (uint32_t)e.cols[j], c = k - r * (uint32_t)e.cols[j];
      const int64_t ld_t = ((int64_t)e.rows[j] + 7) / 8 * 8;
      reinterpret_cast<T*>(e.wt16)[e.dst[j] + (int64_t)c * ld_t + r] = from_f32<T>(wnew);
    }
}

// workgroups of mst_grad_sumsq = rows of its `parts` (mst_grad_sumsq_parts): one per compute unit of an MI355X
constexpr int kGnormParts = 256;

// global-norm clipping (mst_adam_args.parts): the per-workgroup sums of squares of mst_grad_sumsq, the bound, the statistics block
struct AdamGnorm {
  const float* parts;
  float max_norm;
  float* gstat;
};

// wave_sum (common.hpp) on doubles: every level adds the values of two lanes, a commutative sum, so both partners — and in the end
// all 64 lanes — hold the same bits
template <int CTRL> __device__ __forceinline__ double dpp_mov_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_mov_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_f64<0x141>(v);  // row_half_mirror
  v += dpp_mov_f64<0x140>(v);  // row_mirror
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)b, 0x401F);  // swizzle(SWAP, 16)
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(b >> 32), 0x401F);
  v += __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// S = the sum of parts[0 .. kGnormParts) in double, by every wave alike: lane l takes parts[4l .. 4l + 3] (one 16-byte load, `gp`)
// as (p0 + p1) + (p2 + p3), then wave_sum_f64's six pairwise levels across the lanes. Every wave of every workgroup of every range
// of a step runs these instructions on the same words, so all of them hold the same norm and the same factor.
// norm = sqrtf((float)S); c = max_norm / (norm + 1e-8f), 1 unless below 1 (fp32, correctly rounded division and square root:
// engine.clip_scale states the same in np.float32).
static_assert(kGnormParts == 4 * 64, "one f32x4 of parts per lane of a wave");
__device__ __forceinline__ float gnorm_of_parts(f32x4 gp) {
  const double s = ((double)gp[0] + (double)gp[1]) + ((double)gp[2] + (double)gp[3]);
  return sqrtf((float)wave_sum_f64(s));
}
__device__ __forceinline__ float gnorm_clip_scale(float norm, float max_norm) {
  const float c = max_norm / (norm + 1e-8f);
  return c < 1.f ? c : 1.f;
}

// the average of mst_adam_args.ema: the shadow bucket and the configured decay (ema == nullptr in every other form)
struct AdamEma {
  float* ema;
  float decay;
};

// d_t of the average at Adam's step count t (engine.ema_decay_at states the same in np.float32): the warm-up (1 + t) / (10 + t), one
// correctly rounded fp32 division, capped at the configured decay
__device__ __forceinline__ float ema_decay_at(int32_t t, float decay) {
  const float tf = (float)t;
  return fminf(decay, (1.f + tf) / (10.f + tf));
}
// e <- fl(fl(d * e) + fl(omd * w)), omd = fl(1 - d): two rounded products and one rounded sum, never contracted into an FMA
// (engine.ema_update states the same in np.float32, and the tests ask for its bits)
__device__ __forceinline__ float ema_mix(float d, float omd, float e, float w) {
#pragma clang fp contract(off)
  const float a = d * e;
  const float b = omd * w;
  return a + b;
}

// One element of the update for the averaging form, its operations and their order stated: exactly what contraction makes of the
// expressions in adam_flat_kernel's other instantiations (read off their ISA, main loop and tail alike; tests/test_ema_gpu.py holds the
// two to the same bits). Those keep their expressions, so that their instructions stay what they were; the averaging form cannot: with
// the average's products next to them its tail came out with both products of g rounded.
//   g = fma(grad, rescale, fl(wd * w)), clipped;  m = fma(b1, m, fl((1 - b1) * g));  v = fma(b2, v, fl(fl((1 - b2) * g) * g))
//   w = w - fl(lr_t * m) / (sqrtf(v) + eps)
__device__ __forceinline__ void adam_elem(float& w, float grad, float& m, float& v, float rescale, float wd, float clip, float beta1,
                                          float beta2, float lr_t, float eps) {
#pragma clang fp contract(off)
  float g = fmaf(grad, rescale, wd * w);
  if (clip >= 0.f) g = fminf(fmaxf(g, -clip), clip);
  m = fmaf(beta1, m, (1.f - beta1) * g);
  v = fmaf(beta2, v, ((1.f - beta2) * g) * g);
  w = w - (lr_t * m) / (sqrtf(v) + eps);
}

// SCHED (mst_adam_args.sched): the bookkeeping takes the KL weight and the free bits from the device schedule block
// GNORM (mst_adam_args.parts): the gradient is clipped by its global L2 norm, and a step whose norm is not finite is skipped
// EMA (mst_adam_args.ema): every thread folds the weight it has just written into the exponential moving average em.ema. t is read
// from state[0] behind the guards: only the bookkeeping thread of this launch ever writes that word, and only on a step the guards
// skip — where every thread has returned before this read — so on a step that counts nobody writes it while it is read
template <typename T, bool SCHED, bool GNORM, bool EMA = false>
__global__ __launch_bounds__(256) void adam_flat_kernel(int64_t n, float* __restrict__ w, const float* __restrict__ grad,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        T* __restrict__ w16, const int32_t* __restrict__ state,
                                                        float beta1, float beta2, float eps, float wd, float rescale,
                                                        float clip, mst_step_metrics mt, int32_t* state_rw, AdamEmb emb,
                                                        const float* __restrict__ sched, AdamGnorm gn, AdamEma em) {
  __shared__ float red[2][4];
  f32x4 gp;
  if constexpr (GNORM) gp = reinterpret_cast<const f32x4*>(gn.parts)[threadIdx.x & 63];  // (asked for ahead of the guards' loads)
  bool incomplete;
  if (step_is_bad(mt, incomplete)) {
    // the step's position-0 tail did not finish (mst_step_metrics): no update, no metric sums, the step count taken back —
    // by the launch that carries the step's bookkeeping (a second range of the same step only skips)
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.recon) {
      step_mark_bad(mt, incomplete);
      state_rw[0] -= 1;
    }
    return;
  }
  if (step_loss_nonfinite(mt)) {  // (uniform over the launch: every workgroup reads the same losses)
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.recon) {
      __hip_atomic_fetch_add(mt.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      state_rw[0] -= 1;
    }
    return;
  }
  if constexpr (GNORM) {
    // (uniform over the launch and over the launches of a step: gnorm_of_parts) — rescale holds r * c from here on, rounded once
    const float norm = gnorm_of_parts(gp);
    if (!(norm <= 3.0e38f)) {  // (inf, or NaN: a non-finite gradient somewhere in the bucket) — the launch with gstat keeps the books
      if (blockIdx.x == 0 && threadIdx.x == 0 && gn.gstat) {
        if (mt.status) __hip_atomic_fetch_add(mt.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        state_rw[0] -= 1;
      }
      return;
    }
    const float c = gnorm_clip_scale(norm, gn.max_norm);
    rescale = rescale * c;
    if (blockIdx.x == 0 && threadIdx.x == 0 && gn.gstat) {
      float* gs = gn.gstat;  // {norm, c, sum of norms, largest norm, steps, clipped steps}
      gs[0] = norm;
      gs[1] = c;
      gs[2] += norm;
      gs[3] = fmaxf(gs[3], norm);
      gs[4] += 1.f;
      gs[5] += c < 1.f ? 1.f : 0.f;
    }
  }
  if (blockIdx.x == 0 && mt.recon) {  // (uniform branch)
    if constexpr (SCHED) loss_combine_sched_wg(mt.B, mt.recon, mt.kl, sched, mt.total, mt.metric, red);
    else loss_combine_wg(mt.B, mt.recon, mt.kl, mt.kl_weight, mt.total, mt.metric, red);
  }
  const float lr_t = reinterpret_cast<const float*>(state)[1];
  float ema_d = 0.f, ema_omd = 0.f;
  if constexpr (EMA) {
    ema_d = ema_decay_at(state[0], em.decay);
    ema_omd = 1.f - ema_d;
  }
  const int64_t nvec = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    f32x4 wv = reinterpret_cast<const f32x4*>(w)[i];
    f32x4 gv = reinterpret_cast<const f32x4*>(grad)[i];
    f32x4 mv = reinterpret_cast<const f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(v)[i];
    f32x4 ev;
    if constexpr (EMA) ev = reinterpret_cast<const f32x4*>(em.ema)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (EMA) {
        float ww = wv[e], mm = mv[e], v2 = vv[e];
        adam_elem(ww, gv[e], mm, v2, rescale, wd, clip, beta1, beta2, lr_t, eps);
        wv[e] = ww; mv[e] = mm; vv[e] = v2;
      } else {
        float g = gv[e] * rescale + wd * wv[e];
        if (clip >= 0.f) g = fminf(fmaxf(g, -clip), clip);
        mv[e] = beta1 * mv[e] + (1.f - beta1) * g;
        vv[e] = beta2 * vv[e] + (1.f - beta2) * g * g;
        wv[e] = wv[e] - lr_t * mv[e] / (sqrtf(vv[e]) + eps);
      }
      if constexpr (EMA) ev[e] = ema_mix(ema_d, ema_omd, ev[e], wv[e]);
    }
    if constexpr (EMA) reinterpret_cast<f32x4*>(em.ema)[i] = ev;
    reinterpret_cast<f32x4*>(w)[i] = wv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (w16) {
      u32x2 o;
      o[0] = (uint32_t)f32_to_bits<T>(wv[0]) | ((uint32_t)f32_to_bits<T>(wv[1]) << 16);
      o[1] = (uint32_t)f32_to_bits<T>(wv[2]) | ((uint32_t)f32_to_bits<T>(wv[3]) << 16);
      reinterpret_cast<u32x2*>(w16)[i] = o;
    }
    if (emb.n > 0 && ((4 * i + 3 >= emb.lo[0] && 4 * i < emb.hi[0]) || (emb.n > 1 && 4 * i + 3 >= emb.lo[1] && 4 * i < emb.hi[1]))) {
#pragma unroll
      for (int e = 0; e < 4; ++e) adam_emb_store<T>(emb, 4 * i + e, wv[e]);
    }
  }
  // tail (n not a multiple of 4)
  if (blockIdx.x == 0) {
    for (int64_t i = nvec * 4 + threadIdx.x; i < n; i += 256) {
      float ww, mm, vv;
      if constexpr (EMA) {
        ww = w[i]; mm = m[i]; vv = v[i];
        adam_elem(ww, grad[i], mm, vv, rescale, wd, clip, beta1, beta2, lr_t, eps);
      } else {
        float g = grad[i] * rescale + wd * w[i];
        if (clip >= 0.f) g = fminf(fmaxf(g, -clip), clip);
        mm = beta1 * m[i] + (1.f - beta1) * g;
        vv = beta2 * v[i] + (1.f - beta2) * g * g;
        ww = w[i] - lr_t * mm / (sqrtf(vv) + eps);
      }
      m[i] = mm; v[i] = vv; w[i] = ww;
      if constexpr (EMA) em.ema[i] = ema_mix(ema_d, ema_omd, em.ema[i], ww);
      if (w16) w16[i] = from_f32<T>(ww);
      adam_emb_store<T>(emb, i, ww);
    }
  }
}

// transposed 16-bit shadows: for matrix i, src fp32 [rows, cols] at w + desc[4i], dst [cols, ld_t] at
// wt16 + desc[4i+1] with ld_t = roundup8(rows); pad columns rows..ld_t are zeroed.
template <typename T>
__global__ __launch_bounds__(256) void transpose_shadows_kernel(const float* __restrict__ w, T* __restrict__ wt16,
                                                                const int64_t* __restrict__ desc,
                                                                const int64_t* __restrict__ tile_prefix, int n_mat) {
  __shared__ float tile[32][33];
  shadow_tile_wg<T>(w, wt16, desc, tile_prefix, n_mat, (int64_t)blockIdx.x, tile);
}

template <typename T>
__global__ __launch_bounds__(256) void cast_kernel(int64_t n, const float* __restrict__ src, T* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = from_f32<T>(src[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void add_kernel(int64_t n, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = from_f32<T>(to_f32(a[i]) + to_f32(b[i]));
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(int64_t n, float p, uint64_t seed, uint32_t site, uint8_t* keep) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    keep[i] = dropout_keep(seed, site, (uint64_t)i, p) ? 1 : 0;
}

}  // namespace mst

using namespace mst;

static unsigned grid_for(int64_t n, int per_thread) {
  int64_t g = cdiv(n, 256 * (int64_t)per_thread);
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (unsigned)g;
}

// One Adam launch as the host has decided it: the kernel's by-value blocks and the three switches that choose its instantiation.
struct AdamPlan {
  mst_step_metrics mt;
  AdamEmb emb;
  AdamGnorm gn;
  AdamEma em;
  bool sched, gnorm, ema, tick;
};

// Every check of mst_adam_flat, in the header's order, before any HIP call: mst_adam_flat launches what this leaves in `p`,
// mst_adam_flat_form reports it.
static int adam_plan(const mst_adam_args* args, AdamPlan& p) {
  MST_CHECK_ARG(args != nullptr, "mst_adam_flat: null args");
  const mst_adam_args& a = *args;
  p = AdamPlan{};
  MST_CHECK_ARG(a.ema != nullptr || a.decay == 0.f, "mst_adam_flat: decay without ema (the averaging form takes both)");
  if (a.ema) {
    MST_CHECK_ARG((uintptr_t)a.ema % 16 == 0, "mst_adam_flat: ema must be 16-byte aligned");
    MST_CHECK_ARG(a.decay > 0.f && a.decay < 1.f, "mst_adam_flat: decay must lie in (0, 1)");
    p.em = {a.ema, a.decay};
  }
  MST_CHECK_ARG(a.parts != nullptr || (a.n_parts == 0 && a.max_norm == 0.f && a.gstat == nullptr),
                "mst_adam_flat: n_parts, max_norm or gstat without parts (mst_grad_sumsq writes them)");
  if (a.parts) {
    MST_CHECK_ARG((uintptr_t)a.parts % 16 == 0, "mst_adam_flat: parts must be 16-byte aligned");
    MST_CHECK_ARG(a.n_parts == kGnormParts, "mst_adam_flat: n_parts must be mst_grad_sumsq_parts() = %d", kGnormParts);
    MST_CHECK_ARG(a.max_norm > 0.f && a.max_norm <= 3.0e38f, "mst_adam_flat: max_norm must be positive and finite");
    p.gn = {a.parts, a.max_norm, a.gstat};
  }
  MST_CHECK_ARG(a.n_emb >= 0 && a.n_emb <= 2 && (a.n_emb == 0 || (a.emb && a.wt16)) && a.base >= 0,
                "mst_adam_flat: up to two matrices, with their table and wt16");
  for (int j = 0; j < (int)a.n_emb; ++j) {
    const int64_t so = a.emb[4 * j], dst = a.emb[4 * j + 1], rows = a.emb[4 * j + 2], cols = a.emb[4 * j + 3];
    MST_CHECK_ARG(rows > 0 && cols > 0 && rows * cols < (1ll << 31) && dst >= 0, "mst_adam_flat: bad matrix %d", j);
    // (a matrix outside this launch's range [base, base + n) simply never matches)
    AdamEmb& e = p.emb;
    e.lo[e.n] = so - a.base; e.hi[e.n] = so - a.base + rows * cols; e.dst[e.n] = dst; e.rows[e.n] = (int32_t)rows; e.cols[e.n] = (int32_t)cols;
    ++e.n;
  }
  p.emb.wt16 = a.wt16;
  MST_CHECK_ARG(!a.advance_step || (!a.sched && !a.emb && !a.parts && !a.ema),
                "mst_adam_flat: advance_step goes with none of sched, emb, parts and ema (their step count is mst_step_begin's)");
  MST_CHECK_ARG(a.n > 0 && a.w && a.grad && a.m && a.v && a.step_state, "mst_adam_flat: bad argument");
  if (a.metrics) {
    MST_CHECK_ARG(a.metrics->recon == nullptr || (a.metrics->B > 0 && a.metrics->kl), "mst_adam_flat: metrics need B, recon and kl");
    MST_CHECK_ARG(a.metrics->status || (!a.metrics->expect_ptr0 && !a.metrics->expect_ptr1), "mst_adam_flat: expectations need the status words");
    p.mt = *a.metrics;
  }
  MST_CHECK_ARG(((uintptr_t)a.w % 16 == 0) && ((uintptr_t)a.grad % 16 == 0) && ((uintptr_t)a.m % 16 == 0) && ((uintptr_t)a.v % 16 == 0),
                "mst_adam_flat: buffers must be 16-byte aligned");
  p.sched = a.sched != nullptr; p.gnorm = a.parts != nullptr; p.ema = a.ema != nullptr; p.tick = a.advance_step != 0;
  return dispatch_act(a.dtype, [](auto) -> int { return MST_OK; });
}

// the eight instantiations of one activation type, indexed [EMA][GNORM][SCHED]
template <typename T> using AdamKernel = decltype(&adam_flat_kernel<T, false, false, false>);
template <typename T>
static constexpr AdamKernel<T> kAdamKernels[2][2][2] = {
    {{adam_flat_kernel<T, false, false, false>, adam_flat_kernel<T, true, false, false>},
     {adam_flat_kernel<T, false, true, false>, adam_flat_kernel<T, true, true, false>}},
    {{adam_flat_kernel<T, false, false, true>, adam_flat_kernel<T, true, false, true>},
     {adam_flat_kernel<T, false, true, true>, adam_flat_kernel<T, true, true, true>}}};

extern "C" int mst_adam_flat_form(const mst_adam_args* args, int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_adam_flat_form: null form");
  AdamPlan p;
  if (const int rc = adam_plan(args, p)) return rc;
  form[0] = p.sched; form[1] = p.gnorm; form[2] = p.ema; form[3] = p.emb.n; form[4] = p.tick;
  return MST_OK;
}

extern "C" int mst_adam_flat(const mst_adam_args* args, mst_stream_t stream) {
  AdamPlan p;
  if (const int rc = adam_plan(args, p)) return rc;
  const mst_adam_args& a = *args;
  hipStream_t s = (hipStream_t)stream;
  if (p.tick) {  // a launch behind mst_step_begin, or over a second range of the same step, passes 0
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, a.step_state, a.lr, a.beta1, a.beta2);
    MST_CHECK_LAUNCH("adam_tick_kernel");
  }
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL(kAdamKernels<T>[p.ema][p.gnorm][p.sched], dim3(grid_for(a.n, 4)), dim3(256), 0, s, a.n, a.w, a.grad, a.m, a.v,
                       (T*)a.w16, a.step_state, (float)a.beta1, (float)a.beta2, a.eps, a.wd, a.rescale, a.clip, p.mt, a.step_state, p.emb,
                       a.sched, p.gn, p.em);
    MST_CHECK_LAUNCH("adam_flat_kernel");
    return MST_OK;
  });
}

// w[i] <-> ema[i] over the flat bucket, w16[i] from the new w[i] (the cast the Adam launch writes): 16-byte loads and stores over a
// grid-stride loop, the up-to-three tail elements on the last workgroup (as grad_sumsq_kernel takes them)
template <typename T>
__global__ __launch_bounds__(256) void ema_swap_kernel(int64_t n, float* __restrict__ w, float* __restrict__ ema, T* __restrict__ w16) {
  const int64_t nvec = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[i];
    const f32x4 ev = reinterpret_cast<const f32x4*>(ema)[i];
    reinterpret_cast<f32x4*>(w)[i] = ev;
    reinterpret_cast<f32x4*>(ema)[i] = wv;
    if (w16) {
      u32x2 o;
      o[0] = (uint32_t)f32_to_bits<T>(ev[0]) | ((uint32_t)f32_to_bits<T>(ev[1]) << 16);
      o[1] = (uint32_t)f32_to_bits<T>(ev[2]) | ((uint32_t)f32_to_bits<T>(ev[3]) << 16);
      reinterpret_cast<u32x2*>(w16)[i] = o;
    }
  }
  if (blockIdx.x == gridDim.x - 1) {
    const int64_t k = nvec * 4 + threadIdx.x;
    if (k < n) {
      const float ww = w[k], ee = ema[k];
      w[k] = ee;
      ema[k] = ww;
      if (w16) w16[k] = from_f32<T>(ee);
    }
  }
}

extern "C" int mst_ema_swap(int dtype, int64_t n, float* w, float* ema, void* w16, mst_stream_t stream) {
  MST_CHECK_ARG(n > 0 && w && ema && w != ema, "mst_ema_swap: bad argument (n > 0, w and ema given and distinct)");
  MST_CHECK_ARG(((uintptr_t)w % 16 == 0) && ((uintptr_t)ema % 16 == 0) && ((uintptr_t)w16 % 8 == 0),
                "mst_ema_swap: w and ema must be 16-byte aligned, w16 8-byte aligned");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((ema_swap_kernel<T>), dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, w, ema, (T*)w16);
    MST_CHECK_LAUNCH("ema_swap_kernel");
    return MST_OK;
  });
}

// sums of squares of the rescaled flat gradient for mst_adam_flat's clipping group: workgroup j leaves parts[j]. Per thread an fp32 chain over
// its grid-stride elements, then wave_sum (DPP), then the four waves through LDS in wave order: no atomics, a fixed order
__global__ __launch_bounds__(256) void grad_sumsq_kernel(int64_t n, const float* __restrict__ grad, int64_t cut, float rescale_lo,
                                                         float rescale_hi, float* __restrict__ parts) {
  __shared__ float red[4];
  const int64_t nvec = n / 4, stride = (int64_t)kGnormParts * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  f32x4 cur = {0.f, 0.f, 0.f, 0.f};
  if (i < nvec) cur = reinterpret_cast<const f32x4*>(grad)[i];  // the first load is on its way before anything else
  float acc = 0.f;
  while (i < nvec) {
    const int64_t nx = i + stride;
    f32x4 nxt = {0.f, 0.f, 0.f, 0.f};
    if (nx < nvec) nxt = reinterpret_cast<const f32x4*>(grad)[nx];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = cur[e] * (4 * i + e < cut ? rescale_lo : rescale_hi);
      acc += x * x;
    }
    cur = nxt;
    i = nx;
  }
  // tail (n not a multiple of 4): up to three elements, on the last workgroup
  if (blockIdx.x == kGnormParts - 1) {
    const int64_t k = nvec * 4 + threadIdx.x;
    if (k < n) {
      const float x = grad[k] * (k < cut ? rescale_lo : rescale_hi);
      acc += x * x;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int64_t mst_grad_sumsq_parts(void) { return kGnormParts; }

extern "C" int mst_grad_sumsq(int64_t n, const float* grad, int64_t cut, float rescale_lo, float rescale_hi, float* parts,
                              mst_stream_t stream) {
  MST_CHECK_ARG(n > 0 && grad && parts && cut >= 0 && cut <= n, "mst_grad_sumsq: bad argument (n > 0, 0 <= cut <= n, grad and parts given)");
  MST_CHECK_ARG((uintptr_t)grad % 16 == 0, "mst_grad_sumsq: grad must be 16-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(kGnormParts), dim3(256), 0, (hipStream_t)stream, n, grad, cut, rescale_lo, rescale_hi, parts);
  MST_CHECK_LAUNCH("grad_sumsq_kernel");
  return MST_OK;
}

extern "C" int mst_transpose_shadows(int dtype, const float* w, void* wt16, const int64_t* desc,
                                     const int64_t* tile_prefix, int64_t n_mat, int64_t total_tiles,
                                     mst_stream_t stream) {
  MST_CHECK_ARG(w && wt16 && desc && tile_prefix && n_mat > 0 && total_tiles > 0, "mst_transpose_shadows: bad argument");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((transpose_shadows_kernel<T>), dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, w, (T*)wt16,
                       desc, tile_prefix, (int)n_mat);
    MST_CHECK_LAUNCH("transpose_shadows_kernel");
    return MST_OK;
  });
}

// per-tensor gradient norms for the reference's periodic gradient log (trainer.py:257-270): out[i] = sum of squares of
// x[offsets[i] .. offsets[i+1]) — one workgroup per tensor of the flat bucket, one launch for all of them
__global__ __launch_bounds__(256) void segment_sumsq_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets,
                                                            float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t lo = offsets[2 * blockIdx.x], hi = offsets[2 * blockIdx.x + 1];
  float acc = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) acc += x[i] * x[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

extern "C" int mst_segment_sumsq(const float* x, const int64_t* ranges, int64_t n_segments, float* out, mst_stream_t stream) {
  MST_CHECK_ARG(x && ranges && out && n_segments > 0 && n_segments <= 65535, "mst_segment_sumsq: bad argument");
  hipLaunchKernelGGL(segment_sumsq_kernel, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, x, ranges, out);
  MST_CHECK_LAUNCH("segment_sumsq_kernel");
  return MST_OK;
}

extern "C" int mst_cast_f32_to_act(int dtype, int64_t n, const float* src, void* dst, mst_stream_t stream) {
  MST_CHECK_ARG(n > 0 && src && dst, "mst_cast_f32_to_act: bad argument");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((cast_kernel<T>), dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, src, (T*)dst);
    MST_CHECK_LAUNCH("cast_kernel");
    return MST_OK;
  });
}

extern "C" int mst_add_act(int dtype, int64_t n, const void* a, const void* b, void* y, mst_stream_t stream) {
  MST_CHECK_ARG(n > 0 && a && b && y, "mst_add_act: bad argument");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((add_kernel<T>), dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, (const T*)a, (const T*)b, (T*)y);
    MST_CHECK_LAUNCH("add_kernel");
    return MST_OK;
  });
}

extern "C" int mst_dropout_mask(int64_t n, float p, uint64_t seed, uint32_t site, uint8_t* keep, mst_stream_t stream) {
  MST_CHECK_ARG(n > 0 && keep && p >= 0.f && p <= 1.f, "mst_dropout_mask: bad argument");
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, p, seed, site, keep);
  MST_CHECK_LAUNCH("dropout_mask_kernel");
  return MST_OK;
}

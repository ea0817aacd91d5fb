// row_tail_fwd.hpp — the forward position-0 tail kernel (overview: row_tail.hip; barriers, join, riders: row_tail.hpp)
#pragma once
#include "row_tail.hpp"

namespace mst {

// LayerNorm of one row held as 4 elements per lane (D = 256) or 2 (D = 128): layernorm_fwd_kernel's arithmetic
template <typename T, int D>
__device__ __forceinline__ void ln_row(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                       int lane, float (&y)[D / 64], float& mean, float& rstd) {
  constexpr int E = D / 64;
  float v[E];
  float s = 0.f;
  row_raw<E> r[1];
  row_load_l2_nowait<T, E>(r[0], x + lane * E);
  l2_wait(r);
  row_unpack<T, E>(r[0], v);
#pragma unroll
  for (int e = 0; e < E; ++e) s += v[e];
  mean = wave_sum(s) * (1.f / (float)D);
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) { const float d = v[e] - mean; ss += d * d; }
  rstd = 1.f / sqrtf(wave_sum(ss) * (1.f / (float)D) + eps);
#pragma unroll
  for (int e = 0; e < E; ++e) y[e] = (v[e] - mean) * rstd * gamma[lane * E + e] + beta[lane * E + e];
}

// RIDE: 0, or the rider tile's rows (128 / 256) — one rider form per kernel: both in one made the register allocator spill
template <typename T, int D, int RIDE = 0>
__global__ __launch_bounds__(1024) void row_tail_fwd_kernel(mst_row_tail_args q, mst_gemm_args ride, int ride_tiles, uint32_t* ride_queue,
                                                            TailShadow ride_sh) {
  constexpr int G = D / 16, F = 4 * D, LDX = D + 8, E = D / 64;
  constexpr int KQ1 = D / 32 / 4, KQ2 = F / 32 / 4;  // k-steps per K quarter of the two 16-column stages
  __shared__ __attribute__((aligned(16))) T sX1[64 * LDX];  // LayerNorm-1 output of every row (FFN1's operand, FFN2's residual)
  __shared__ __attribute__((aligned(16))) float sP[4 * 64 * 16];
  // every bias / gamma / beta of the chain, requested at once at the start: they are cold lines after an optimizer step, and
  // each would be one more dependent round trip inside its stage ([bp | g1 | be1 | b2 | g2 | be2 | b1])
  __shared__ __attribute__((aligned(16))) float sPar[6 * D + F];
  typedef typename Act<T>::vec8 vec8;
  typedef row_raw<E> raw_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = wave & 3, wq = wave >> 2;
  const int g = tail_join(q.sync, G);
  if (g < 0) {
    if constexpr (RIDE != 0) {
      extern __shared__ __attribute__((aligned(16))) unsigned char ride_smem[];
      if (g == -1) tail_ride_bm<T, RIDE>(ride, ride_tiles, ride_queue, ride_smem, ride_sh);
    }
    return;
  }
  for (int i = tid; i < D; i += TAIL_WAVES * 64) {
    sPar[i] = q.bp[i]; sPar[D + i] = q.g1[i]; sPar[2 * D + i] = q.be1[i];
    sPar[3 * D + i] = q.b2[i]; sPar[4 * D + i] = q.g2[i]; sPar[5 * D + i] = q.be2[i];
  }
  for (int i = tid; i < F; i += TAIL_WAVES * 64) sPar[6 * D + i] = q.b1[i];
  const float* const s_bp = sPar, * const s_g1 = sPar + D, * const s_be1 = sPar + 2 * D, * const s_b2 = sPar + 3 * D,
             * const s_g2 = sPar + 4 * D, * const s_be2 = sPar + 5 * D, * const s_b1 = sPar + 6 * D;
  const int li = lane & 15, lq = lane >> 4;
  const int B = (int)q.B;
  const int m = mi * 16 + li;  // the row this lane's accumulator column belongs to
  const bool m_ok = m < B;
  const int mc = m_ok ? m : 0;  // (row of the unconditional loads)
  const int64_t pm = (int64_t)m * q.phys_stride;  // physical row in the [B * S, N] tensors: the dropout counter's row
  const float p = q.dropout_p;
  const bool drop = p > 0.f;
  const uint64_t dseed = q.dropout_seed ^ ((drop && q.dropout_seed_ptr) ? q.dropout_seed_ptr[0] : 0ull);
  const uint32_t thr = dropout_thr(p);
  const float inv_keep = dropout_inv_keep(p);
  const T* att = reinterpret_cast<const T*>(q.att);
  const T* xin = reinterpret_cast<const T*>(q.resid);
  T* h1 = reinterpret_cast<T*>(q.h1); T* x1 = reinterpret_cast<T*>(q.x1); T* a = reinterpret_cast<T*>(q.a);
  T* h2 = reinterpret_cast<T*>(q.h2); T* x2 = reinterpret_cast<T*>(q.x2);

  auto finish4 = [&](const f32x4& acc, const float* bias, int n, uint32_t site, int64_t N, bool relu, const T* res /* row ptr or null */,
                     T* dst /* row ptr */) {
    // one lane's four consecutive output columns n..n+3 of row m: bias, ReLU, dropout, residual, rounding — gemm_epilogue's order
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + n);
    uint32_t keep = 0xFu;
    if (drop) keep = dropout_keep4k(dropout_key(dseed, site), (uint64_t)(pm * N + n) >> 2, thr);
    float r4[4] = {0.f, 0.f, 0.f, 0.f};
    if (res) row_unpack<T, 4>(*reinterpret_cast<const u32x2*>(res + n), r4);
    uint16_t hb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = acc[e] + b4[e];
      if (relu) t = fmaxf(t, 0.f);
      if (drop) t = ((keep >> e) & 1u) ? t * inv_keep : 0.f;
      hb[e] = f32_to_bits<T>(t + r4[e]);
    }
    store8_l2(dst + n, pack_bits(hb[0], hb[1], hb[2], hb[3]));
  };

  TAIL_STAMP(0);
  // ---------------- stage 1: h1[:, 16 g .. 16 g + 15] = x_in + dropout(att W_proj^T + b)     (K quarter wq per wave)
  {
    const int n0 = g * 16;
    const T* Wp = reinterpret_cast<const T*>(q.Wp) + (int64_t)(n0 + li) * q.ldwp + 8 * lq + 32 * KQ1 * wq;
    const T* Ar = att + (int64_t)m * q.rs_att + 8 * lq + 32 * KQ1 * wq;
    vec8 wf[KQ1], xf[KQ1];
#pragma unroll
    for (int ks = 0; ks < KQ1; ++ks) { wf[ks] = frag16<T>(Wp + 32 * ks, true); xf[ks] = frag16<T>(Ar + 32 * ks, m_ok); }
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KQ1; ++ks) part = Act<T>::mfma16(wf[ks], xf[ks], part);
    const f32x4 acc = quarter_sum(sP, part, wq, m, lq);
    if (wq == 0 && m_ok) finish4(acc, s_bp, n0 + 4 * lq, q.site0, D, false, xin + (int64_t)m * q.rs_res, h1 + (int64_t)m * q.rs_d);
  }
  // (memory-level parallelism is the whole game here: every stage is a few dependent L2 / fabric round trips, so the
  // next stage's weight fragments are requested BEFORE the barrier they do not depend on, and rows are loaded in batches)
  const int n1 = g * 64 + 16 * wq;  // this wave's 16-column block of the FFN1 slice
  const T* W1p = reinterpret_cast<const T*>(q.W1) + (int64_t)(n1 + li) * q.ldw1 + 8 * lq;
  vec8 w1f[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) w1f[ks] = frag16<T>(W1p + 32 * ks, true);
  TAIL_STAMP(1);
  grid_sync(q.sync, G, q.status, MST_TAIL_SPIN_FWD);
  TAIL_STAMP(2);

  // ---------------- stage 2: x1 = LN1(h1) for every row (each workgroup, into LDS; the rows' owner also to HBM), then
  //                  a[:, 64 g .. 64 g + 63] = dropout(relu(x1 W1^T + b1))
  {
    constexpr int RPW = 4;  // rows per wave: rows wave, wave + 16, ...
    float v[RPW][E];
    // all rows requested at once, unconditionally (a row past the batch re-reads the last one and is zeroed below)
    raw_t raw[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i, rc = r < B ? r : B - 1;
      row_load_l2_nowait<T, E>(raw[i], h1 + (int64_t)rc * q.rs_d + lane * E);
    }
    l2_wait(raw);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const bool ok = wave + TAIL_WAVES * i < B;
      if constexpr (E == 4) {  // (spelled out: row_unpack with the select behind it was tried and changed code generation)
        const u32x2 t = raw[i];
        v[i][0] = ok ? bits_to_f32<T>((uint16_t)(t[0] & 0xffff)) : 0.f; v[i][1] = ok ? bits_to_f32<T>((uint16_t)(t[0] >> 16)) : 0.f;
        v[i][2] = ok ? bits_to_f32<T>((uint16_t)(t[1] & 0xffff)) : 0.f; v[i][3] = ok ? bits_to_f32<T>((uint16_t)(t[1] >> 16)) : 0.f;
      } else {
        const uint32_t t = raw[i];
        v[i][0] = ok ? bits_to_f32<T>((uint16_t)(t & 0xffff)) : 0.f; v[i][1] = ok ? bits_to_f32<T>((uint16_t)(t >> 16)) : 0.f;
      }
    }
    float gm[E], bt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { gm[e] = s_g1[lane * E + e]; bt[e] = s_be1[lane * E + e]; }
#ifdef MST_TAIL_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TAIL_STAMP(8);
#endif
    float mean[RPW], rstd[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      mean[i] = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) mean[i] += v[i][e];
    }
    wave_sum_batch<RPW>(mean);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      mean[i] *= (1.f / (float)D);
      rstd[i] = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) { const float d = v[i][e] - mean[i]; rstd[i] += d * d; }
    }
    wave_sum_batch<RPW>(rstd);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i;
      rstd[i] = 1.f / sqrtf(rstd[i] * (1.f / (float)D) + q.eps);
      uint16_t yb[E];
#pragma unroll
      for (int e = 0; e < E; ++e) yb[e] = (r < B) ? f32_to_bits<T>((v[i][e] - mean[i]) * rstd[i] * gm[e] + bt[e]) : (uint16_t)0;  // rows past the batch: zeros
      raw_t o;
      if constexpr (E == 4) o = pack_bits(yb[0], yb[1], yb[2], yb[3]);
      else o = pack_bits(yb[0], yb[1]);
      row_store<T, E>(sX1 + r * LDX + lane * E, o, false);
      if (r < B && r % G == g) row_store<T, E>(x1 + (int64_t)r * q.rs_d + lane * E, o, false);
      if (r < B && r % G == g && lane == 0) { q.mean1[(int64_t)r * q.stat_stride] = mean[i]; q.rstd1[(int64_t)r * q.stat_stride] = rstd[i]; }
    }
  }
  TAIL_STAMP(9);
  __syncthreads();
  TAIL_STAMP(10);
  const int n2 = g * 16;
  const T* W2p = reinterpret_cast<const T*>(q.W2) + (int64_t)(n2 + li) * q.ldw2 + 8 * lq + 32 * KQ2 * wq;
  vec8 w2f[KQ2];  // this wave's quarter of the FFN2 weights: requested before the barrier
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      const vec8 xf = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sX1 + m * LDX + 32 * ks + 8 * lq));
      acc = Act<T>::mfma16(w1f[ks], xf, acc);
    }
    TAIL_STAMP(11);
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) w2f[ks] = frag16<T>(W2p + 32 * ks, true);
    if (m_ok) finish4(acc, s_b1, n1 + 4 * lq, q.site0 + 1, F, true, nullptr, a + (int64_t)m * q.rs_a);
  }
  TAIL_STAMP(3);
  grid_sync(q.sync, 2 * G, q.status, MST_TAIL_SPIN_FWD);
  TAIL_STAMP(4);

  // ---------------- stage 3: h2[:, 16 g ..] = x1 + dropout(a W2^T + b2)        (K = 4 D: the whole hidden row, a quarter per wave)
  {
    const T* Ar = a + (int64_t)mc * q.rs_a + 8 * lq + 32 * KQ2 * wq;
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
    u32x4 xr[KQ2];  // the hidden row's fragments: every load in flight at once
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) load16_l2_nowait(xr[ks], Ar + ks * 32);
    l2_wait(xr);
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) part = Act<T>::mfma16(w2f[ks], __builtin_bit_cast(vec8, m_ok ? xr[ks] : u32x4{0u, 0u, 0u, 0u}), part);
    const f32x4 acc = quarter_sum(sP, part, wq, m, lq);
    if (wq == 0 && m_ok) finish4(acc, s_b2, n2 + 4 * lq, q.site0 + 2, D, false, sX1 + m * LDX, h2 + (int64_t)m * q.rs_d);
  }
  TAIL_STAMP(5);
  grid_sync(q.sync, 3 * G, q.status, MST_TAIL_SPIN_FWD);
  TAIL_STAMP(6);
  uint32_t ride_seen = 0u;  // (riders) the tile queue's counter as of now: tail_drain
  if constexpr (RIDE != 0) { if (tid == 0) load4_sc1_nowait(ride_seen, ride_queue); }

  // ---------------- stage 4: x2 = LN2(h2), rows dealt to the workgroups
  for (int r = g + G * wave; r < B; r += TAIL_WAVES * G) {
    float y[E], mean, rstd;
    ln_row<T, D>(h2 + (int64_t)r * q.rs_d, s_g2, s_be2, q.eps, lane, y, mean, rstd);
    uint16_t yb[E];  // (spelled out: row_pack / row_store were tried here and changed code generation)
#pragma unroll
    for (int e = 0; e < E; ++e) yb[e] = f32_to_bits<T>(y[e]);
    if constexpr (E == 4) *reinterpret_cast<u32x2*>(x2 + (int64_t)r * q.rs_d + lane * 4) =
        u32x2{(uint32_t)yb[0] | ((uint32_t)yb[1] << 16), (uint32_t)yb[2] | ((uint32_t)yb[3] << 16)};
    else *reinterpret_cast<uint32_t*>(x2 + (int64_t)r * q.rs_d + lane * 2) = (uint32_t)yb[0] | ((uint32_t)yb[1] << 16);
    if (lane == 0) { q.mean2[(int64_t)r * q.stat_stride] = mean; q.rstd2[(int64_t)r * q.stat_stride] = rstd; }
  }
  TAIL_STAMP(7);
  if constexpr (RIDE != 0) {  // the chain is done: whatever the riders left in the queue (normally nothing)
    extern __shared__ __attribute__((aligned(16))) unsigned char ride_smem[];
    __syncthreads();
    tail_drain<T, RIDE>(ride, ride_tiles, ride_queue, ride_seen, ride_smem, ride_sh);
  }
}

}  // namespace mst

// row_tail_bwd.hpp — the backward position-0 tail kernel (overview: row_tail.hip; barriers, join, riders: row_tail.hpp)
#pragma once
#include "row_tail.hpp"

namespace mst {

// The same rows on the way back (mst_row_tail_bwd): LayerNorm-2 backward -> FFN2 dgrad (ReLU gate) -> FFN1 dgrad (+ the
// residual branch) -> LayerNorm-1 backward -> W_proj dgrad, five launches of the step (two LayerNorm backward launches on B
// rows and three GEMMs with M = B) as one, with the forward kernel's decomposition: D / 16 workgroups, each owning 64 hidden
// columns of the FFN2 dgrad and 16 output columns of the FFN1 and W_proj dgrads; both LayerNorm backward passes are
// recomputed by every workgroup on all rows (their results are the next GEMM's operand, kept in LDS), so only two results
// cross a grid barrier: d(pre-activation) and the FFN1 dgrad's output. The workgroup's FFN2-dgrad weights wait in LDS.
template <typename T, int D, int RIDE = 0>
__global__ __launch_bounds__(1024) void row_tail_bwd_kernel(mst_row_tail_bwd_args q, mst_gemm_args ride, int ride_tiles, uint32_t* ride_queue) {
  constexpr int G = D / 16, F = 4 * D, LDX = D + 8, E = D / 64, RPW = 4;
  constexpr int KQ1 = D / 32 / 4, KQ2 = F / 32 / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char tail_smem[];
  T* sA = reinterpret_cast<T*>(tail_smem);                     // [64][LDX] masked LayerNorm-backward rows: the GEMM operand
  T* sW = sA + 64 * LDX;                                        // [64][LDX] W2t rows 64 g .. 64 g + 63
  float* sRed = reinterpret_cast<float*>(sW + 64 * LDX);        // [16 waves][2][D]
  float* sP = sRed + TAIL_WAVES * 2 * D;                        // [4][64][16]
  float* sGam = sP + 4 * 64 * 16;                               // [g2 | g1]: cold parameter lines, requested at the start
  typedef typename Act<T>::vec8 vec8;
  typedef row_raw<E> raw_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = wave & 3, wq = wave >> 2;
  const int g = tail_join(q.sync, G);
  if (g < 0) {
    if constexpr (RIDE != 0) {
      if (g == -1) tail_ride_bm<T, RIDE>(ride, ride_tiles, ride_queue, tail_smem, TailShadow{});
    }
    return;
  }
  const int li = lane & 15, lq = lane >> 4;
  const int B = (int)q.B;
  const int m = mi * 16 + li;
  const bool m_ok = m < B;
  const int mc = m_ok ? m : 0;
  const float p = q.dropout_p;
  const bool drop = p > 0.f;
  const uint64_t dseed = q.dropout_seed ^ ((drop && q.dropout_seed_ptr) ? q.dropout_seed_ptr[0] : 0ull);
  const uint32_t thr = dropout_thr(p);
  const float inv_keep = dropout_inv_keep(p), inv_d = 1.f / (float)D;
  const T* dy = reinterpret_cast<const T*>(q.dy);
  const T* h2 = reinterpret_cast<const T*>(q.h2); const T* h1 = reinterpret_cast<const T*>(q.h1);
  const T* a = reinterpret_cast<const T*>(q.a);
  T* dh = reinterpret_cast<T*>(q.dh); T* dhm = reinterpret_cast<T*>(q.dhm); T* dx1 = reinterpret_cast<T*>(q.dx1);
  T* dh1m = reinterpret_cast<T*>(q.dh1m); T* dpre = reinterpret_cast<T*>(q.dpre); T* dh1 = reinterpret_cast<T*>(q.dh1);
  T* datt = reinterpret_cast<T*>(q.datt);
  const int n1 = g * 64 + 16 * wq, n2 = g * 16;

  // LayerNorm backward of every row (rows wave, wave + 16, ... of this wave; columns E * lane ..): layernorm_bwd_kernel's
  // arithmetic. raw_dy / raw_x: the rows' dy and pre-norm x; the masked result goes to sA, the rows this workgroup owns
  // (r % G == g) to dx_out / dxm_out; dgamma / dbeta are added by workgroup 0.
  auto ln_bwd_rows = [&](raw_t (&raw_dy)[RPW], raw_t (&raw_x)[RPW], const float* mean_in, const float* rstd_in, const float* gamma,
                         uint32_t site, T* dx_out, int64_t rs_dx, bool dx_through, T* dxm_out, int64_t rs_dxm, float* dgamma, float* dbeta) {
    float gm[E], dg[E], db[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { gm[e] = gamma[lane * E + e]; dg[e] = 0.f; db[e] = 0.f; }
    float xh[RPW][E], gv[RPW][E], s1[RPW], s2[RPW], rs[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i, rc = r < B ? r : B - 1;
      const bool ok = r < B;
      const float mean = mean_in[(int64_t)rc * q.stat_stride];
      rs[i] = rstd_in[(int64_t)rc * q.stat_stride];
      float xv[E], dv[E];
      row_unpack<T, E>(raw_x[i], xv); row_unpack<T, E>(raw_dy[i], dv);
      s1[i] = 0.f; s2[i] = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float x_hat = ok ? (xv[e] - mean) * rs[i] : 0.f, d = ok ? dv[e] : 0.f, gg = d * gm[e];
        xh[i][e] = x_hat; gv[i][e] = gg;
        s1[i] += gg; s2[i] += gg * x_hat;
        dg[e] += d * x_hat; db[e] += d;
      }
    }
    wave_sum_batch<RPW>(s1);
    wave_sum_batch<RPW>(s2);
    const uint32_t key = dropout_key(dseed, site);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i;
      const bool ok = r < B;
      const float m1 = s1[i] * inv_d, m2 = s2[i] * inv_d;
      uint32_t keep = 0xFu;
      if (drop) keep = dropout_keep4k(key, (uint64_t)((int64_t)r * q.phys_stride * D + lane * E) >> 2, thr) >> ((lane * E) & 3);
      float o[E], om[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        o[e] = rs[i] * (gv[i][e] - m1 - xh[i][e] * m2);
        om[e] = drop ? (((keep >> e) & 1u) ? o[e] * inv_keep : 0.f) : o[e];
        if (!ok) { o[e] = 0.f; om[e] = 0.f; }
      }
      const raw_t ob = row_pack<T, E>(o), mb = row_pack<T, E>(om);
      *reinterpret_cast<raw_t*>(sA + r * LDX + lane * E) = mb;
      if (ok && r % G == g) {
        row_store<T, E>(dx_out + (int64_t)r * rs_dx + lane * E, ob, dx_through);
        row_store<T, E>(dxm_out + (int64_t)r * rs_dxm + lane * E, mb, false);
      }
    }
    if (g == 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) { sRed[(wave * 2 + 0) * D + lane * E + e] = dg[e]; sRed[(wave * 2 + 1) * D + lane * E + e] = db[e]; }
    }
    __syncthreads();  // (also: sA is complete)
    if (g == 0) {
      for (int c = tid; c < 2 * D; c += TAIL_WAVES * 64) {
        const int which = c / D, col = c % D;
        float t = 0.f;
        for (int w = 0; w < TAIL_WAVES; ++w) t += sRed[(w * 2 + which) * D + col];
        atomicAdd((which ? dbeta : dgamma) + col, t);
      }
    }
  };

  TAIL_STAMP(0);
  // ---------------- this workgroup's FFN2-dgrad weights -> LDS; stage 1's rows requested
  {
    const T* W2t = reinterpret_cast<const T*>(q.W2t);
    constexpr int CPR = D / 8, WCH = 64 * CPR / (TAIL_WAVES * 64);
    u32x4 wv[WCH];
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int c = tid + i * TAIL_WAVES * 64, row = c / CPR, ch = c % CPR;
      wv[i] = *reinterpret_cast<const u32x4*>(W2t + (int64_t)(g * 64 + row) * q.ldw2t + ch * 8);
    }
    raw_t rdy[RPW], rx[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i, rc = r < B ? r : B - 1;
      rdy[i] = *reinterpret_cast<const raw_t*>(dy + (int64_t)rc * q.rs_dy + lane * E);
      rx[i] = *reinterpret_cast<const raw_t*>(h2 + (int64_t)rc * q.rs_d + lane * E);
    }
    float gpre[2] = {0.f, 0.f};
    if (tid < D) { gpre[0] = q.g2[tid]; gpre[1] = q.g1[tid]; }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int c = tid + i * TAIL_WAVES * 64, row = c / CPR, ch = c % CPR;
      *reinterpret_cast<u32x4*>(sW + row * LDX + ch * 8) = wv[i];
    }
    if (tid < D) { sGam[tid] = gpre[0]; sGam[D + tid] = gpre[1]; }
    __syncthreads();  // (the gammas; every load of this stage is already in flight)
    // ---------------- stage 1: LayerNorm-2 backward of every row
    ln_bwd_rows(rdy, rx, q.mean2, q.rstd2, sGam, q.site0 + 2, dh, q.rs_c, true, dhm, q.rs_c, q.dg2, q.db2);
  }
  TAIL_STAMP(1);
  // ---------------- stage 2: d(pre)[:, 64 g ..] = ((dhm W2t^T) / (1 - p)) gated by a > 0     (16-column block wq per wave)
  const T* W1t = reinterpret_cast<const T*>(q.W1t) + (int64_t)(n2 + li) * q.ldw1t + 8 * lq + 32 * KQ2 * wq;
  vec8 w1f[KQ2];  // this wave's quarter of the FFN1-dgrad weights of stage 3: requested before the barrier
  {
    const u32x2 gate8 = m_ok ? *reinterpret_cast<const u32x2*>(a + (int64_t)m * q.rs_a + n1 + 4 * lq) : u32x2{0u, 0u};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      const vec8 xf = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sA + m * LDX + 32 * ks + 8 * lq));
      const vec8 wf = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sW + (16 * wq + li) * LDX + 32 * ks + 8 * lq));
      acc = Act<T>::mfma16(wf, xf, acc);
    }
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) w1f[ks] = frag16<T>(W1t + 32 * ks, true);
    if (m_ok) {
      // (spelled out: row_unpack of the gate was tried and changed code generation)
      const uint16_t gb[4] = {(uint16_t)(gate8[0] & 0xffff), (uint16_t)(gate8[0] >> 16), (uint16_t)(gate8[1] & 0xffff), (uint16_t)(gate8[1] >> 16)};
      uint16_t hb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) hb[e] = f32_to_bits<T>((bits_to_f32<T>(gb[e]) > 0.f) ? acc[e] * inv_keep : 0.f);
      store8_l2(dpre + (int64_t)m * q.rs_dpre + n1 + 4 * lq, pack_bits(hb[0], hb[1], hb[2], hb[3]));
    }
  }
  TAIL_STAMP(2);
  grid_sync(q.sync, G, q.status, MST_TAIL_SPIN_BWD);
  TAIL_STAMP(3);

  // ---------------- stage 3: dx1[:, 16 g ..] = d(pre) W1t^T + dh        (K = 4 D, a quarter per wave)
  const T* Wpt = reinterpret_cast<const T*>(q.Wpt) + (int64_t)(n2 + li) * q.ldwpt + 8 * lq + 32 * KQ1 * wq;
  vec8 wpf[KQ1];
  {
    const T* Ar = dpre + (int64_t)mc * q.rs_dpre + 8 * lq + 32 * KQ2 * wq;
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
    u32x4 xr[KQ2];
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) load16_l2_nowait(xr[ks], Ar + ks * 32);
    u32x2 rvv[1];
    load8_l2_nowait(rvv[0], dh + (int64_t)mc * q.rs_c + n2 + 4 * lq);
    l2_wait(xr);
    l2_wait(rvv);
    const u32x2 rv = rvv[0];
#pragma unroll
    for (int ks = 0; ks < KQ1; ++ks) wpf[ks] = frag16<T>(Wpt + 32 * ks, true);  // stage 5's weights
#pragma unroll
    for (int ks = 0; ks < KQ2; ++ks) part = Act<T>::mfma16(w1f[ks], __builtin_bit_cast(vec8, m_ok ? xr[ks] : u32x4{0u, 0u, 0u, 0u}), part);
    const f32x4 acc = quarter_sum(sP, part, wq, m, lq);
    if (wq == 0 && m_ok) {
      float r4[4];
      row_unpack<T, 4>(rv, r4);
      uint16_t hb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) hb[e] = f32_to_bits<T>(acc[e] + r4[e]);
      store8_l2(dx1 + (int64_t)m * q.rs_c + n2 + 4 * lq, pack_bits(hb[0], hb[1], hb[2], hb[3]));
    }
  }
  TAIL_STAMP(4);
  grid_sync(q.sync, 2 * G, q.status, MST_TAIL_SPIN_BWD);
  TAIL_STAMP(5);
  uint32_t ride_seen = 0u;  // (riders) the tile queue's counter as of now: tail_drain
  if constexpr (RIDE != 0) { if (tid == 0) load4_sc1_nowait(ride_seen, ride_queue); }

  // ---------------- stage 4: LayerNorm-1 backward of every row (operand of stage 5 in LDS)
  {
    raw_t rdy[RPW], rx[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + TAIL_WAVES * i, rc = r < B ? r : B - 1;
      row_load_l2_nowait<T, E>(rdy[i], dx1 + (int64_t)rc * q.rs_c + lane * E);
      rx[i] = *reinterpret_cast<const raw_t*>(h1 + (int64_t)rc * q.rs_d + lane * E);
    }
    l2_wait(rdy);
    ln_bwd_rows(rdy, rx, q.mean1, q.rstd1, sGam + D, q.site0, dh1, q.rs_dh1, false, dh1m, q.rs_c, q.dg1, q.db1);
  }
  TAIL_STAMP(6);
  // ---------------- stage 5: datt[:, 16 g ..] = dh1m Wpt^T        (K quarter per wave)
  {
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KQ1; ++ks) {
      const vec8 xf = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sA + m * LDX + 32 * (KQ1 * wq + ks) + 8 * lq));
      part = Act<T>::mfma16(wpf[ks], xf, part);
    }
    const f32x4 acc = quarter_sum(sP, part, wq, m, lq);
    if (wq == 0 && m_ok) {
      uint16_t hb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) hb[e] = f32_to_bits<T>(acc[e]);
      *reinterpret_cast<u32x2*>(datt + (int64_t)m * q.rs_datt + n2 + 4 * lq) = pack_bits(hb[0], hb[1], hb[2], hb[3]);
    }
  }
  TAIL_STAMP(7);
  if constexpr (RIDE != 0) {  // the chain is done: whatever the riders left in the queue (normally nothing)
    __syncthreads();
    tail_drain<T, RIDE>(ride, ride_tiles, ride_queue, ride_seen, tail_smem, TailShadow{});
  }
}

}  // namespace mst

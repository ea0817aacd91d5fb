// gemm_ln.hpp — LayerNorm as the epilogue of a GEMM tile that spans the whole output row: the device code shared by mst_gemm_nt_ln
// (gemm_ln.hip), the feed-forward block (ffn_ln.hpp), the loss launch's dgrad (gemm_bce.hip) and dec_tail_kernel (dec_tail.hip).
#pragma once
#include <math.h>
#include "common.hpp"
#include "gemm_tile.hpp"

namespace mst {

// diagnostic build only (-DMST_FFN_STAMPS): one workgroup leaves s_memtime stamps per stage (tools/bench_ffn_stamps.py)
// (internal linkage: every unit built with the flag owns a copy; mst_debug_ffn_stamps reads ffn_ln.hip's)
#ifdef MST_FFN_STAMPS
static __device__ uint64_t g_ffn_stamps[8 + 48 * 4];  // [0..3] kernel phases, [5..7] LayerNorm epilogue, [8 + 4k..] stage k, [190, 191] realtime
#define FFN_STAMP(slot) do { if (blockIdx.x == 64 && threadIdx.x == 0 && (slot) < 8 + 48 * 4) g_ffn_stamps[slot] = __builtin_amdgcn_s_memtime(); } while (0)
#define FFN_RT(slot) do { if (blockIdx.x == 64 && threadIdx.x == 0) g_ffn_stamps[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FFN_STAMP(slot) do { } while (0)
#define FFN_RT(slot) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm fused into the epilogue of a GEMM whose tile spans the whole output row (BN == N).
//   mode 1 (forward):  h = epi(acc) is written to C as usual (the backward pass needs the pre-norm tensor) and
//                      y = LayerNorm(h) goes to ln.out, mean / rstd to ln.mean / ln.rstd — what mst_layernorm_fwd would
//                      compute from C (two-pass statistics on the 16-bit-rounded row, gluon.nn.LayerNorm eps).
//   mode 2 (backward): dy = epi(acc) is NOT stored; dx = LayerNorm-backward(dy; x, mean, rstd, gamma) goes to C, the
//                      dropout-masked copy (mask_mode 1) to ln.out, dgamma / dbeta are accumulated — mst_layernorm_bwd
//                      on the GEMM's result, without the round trip through HBM and without its launch.
// Supported epilogue features: bias, alpha, dropout / self_resid, residual, C row remap (the others are rejected on the
// host). One thread finishes 8 columns of a row; the N/8 threads of a row are consecutive lanes, so row sums are
// xor-shuffles inside a 32- or 16-lane group.
template <int LANES>
__device__ __forceinline__ float row_sum(float v) { return group_sum<LANES>(v); }

template <typename T, int BM, int BN, int WGM, int WGN, int MODE>
__device__ __forceinline__ void gemm_epilogue_ln(const mst_gemm_args& a, const mst_ln_args& l, unsigned char* smem,
                                                 f32x4 (&acc)[(BN / WGN) / 16][(BM / WGM) / 16], int64_t m0,
                                                 const T* lds_resid = nullptr, int lds_resid_ld = 0,
                                                 T* lds_out = nullptr, int lds_out_ld = 0, const float* lds_par = nullptr,
                                                 const uint64_t* dseed_pre = nullptr /* the step's dropout seed, already loaded */) {
  // lds_resid: the workgroup's BM residual rows already sit in LDS (row stride lds_resid_ld elements, outside the staging
  // tile): they are read from there instead of from a.resid
  // lds_par: [bias | gamma | beta] (3 x BN floats) already in LDS (outside the staging tile): in a kernel that is one
  // workgroup per CU these cold parameter lines (the optimizer rewrote them) are an exposed round trip at the epilogue's start
  // lds_out: the result rows ALSO go to this LDS tile (outside the staging tile; rows past M as zeros): the LayerNorm output
  // (mode 1) or the input gradient — its masked copy when there is one — (mode 2), for a GEMM that follows in the same launch
  constexpr int NT = WGM * WGN * 64;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int LDS_F = BN + 4, CPR = BN / 8, RSTEP = NT / CPR, ITERS = BM / RSTEP;
  static_assert(CPR == 32 || CPR == 16, "a row must be a 32- or 16-lane group");
  static_assert(BM % RSTEP == 0, "rows per thread must be whole");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int frow = lane & 15, fq = lane >> 4;
  float* sF = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      *reinterpret_cast<f32x4*>(sF + (wm * WTM + i * 16 + frow) * LDS_F + wn * WTN + j * 16 + fq * 4) = acc[j][i];
  __syncthreads();
  FFN_STAMP(5);

  const int ch = tid % CPR, nc = ch * 8, row0 = tid / CPR;
  const float inv_n = 1.f / (float)BN;
  const float inv_keep = dropout_inv_keep(a.dropout_p);
  const bool has_drop = a.dropout_p > 0.f;
  const uint64_t dseed = dseed_pre ? *dseed_pre : a.dropout_seed ^ ((has_drop && a.dropout_seed_ptr) ? a.dropout_seed_ptr[0] : 0ull);
  const uint32_t dkey = dropout_key(dseed, a.dropout_site), dthr = dropout_thr(a.dropout_p);
  const T* resid = reinterpret_cast<const T*>(a.resid);
  float bias8[8], gam8[8], bet8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (lds_par) {
      bias8[e] = lds_par[nc + e];
      gam8[e] = lds_par[BN + nc + e];
      bet8[e] = (MODE == 1) ? lds_par[2 * BN + nc + e] : 0.f;
    } else {
      bias8[e] = a.bias ? a.bias[nc + e] : 0.f;
      gam8[e] = l.gamma[nc + e];
      bet8[e] = (MODE == 1) ? l.beta[nc + e] : 0.f;
    }
  }
  float dg8[8], db8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { dg8[e] = 0.f; db8[e] = 0.f; }

  // every global load of the thread's rows (residual; backward: x, mean, rstd) is issued before the first row is finished:
  // in the step these lines are cold, and a row-by-row loop exposed one memory round trip per row at 8 waves per CU
  u32x4 rv[ITERS], xv[ITERS];
  float mean_r[ITERS], rstd_r[ITERS];
  // the row remap once per tile where a tile cannot straddle a group (the step's remapped launch: rows 1..T of T + 1, T a multiple
  // of the tile height): per row it is two 64-bit divisions, ~200 instructions each, in front of every row's loads
  const bool tile_remap = a.c_rows_per_group <= 0 || a.c_rows_per_group % BM == 0;
  const int64_t pm0 = remap_row(m0, a.c_rows_per_group, a.c_group_stride, a.c_group_offset);
  auto phys_row = [&](int64_t m) { return tile_remap ? pm0 + (m - m0) : remap_row(m, a.c_rows_per_group, a.c_group_stride, a.c_group_offset); };
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int64_t m = m0 + row0 + it * RSTEP;
    rv[it] = u32x4{0u, 0u, 0u, 0u}; xv[it] = rv[it]; mean_r[it] = 0.f; rstd_r[it] = 0.f;
    if (m < a.M) {
      const int64_t pm = phys_row(m);
      if (lds_resid) rv[it] = *reinterpret_cast<const u32x4*>(lds_resid + (row0 + it * RSTEP) * lds_resid_ld + nc);
      else if (resid) rv[it] = *reinterpret_cast<const u32x4*>(resid + m * a.ldr + nc);
      if (MODE == 2) {
        xv[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(l.x) + pm * l.ld_x + nc);
        mean_r[it] = l.mean[pm];
        rstd_r[it] = l.rstd[pm];
      }
    }
  }
  FFN_STAMP(6);
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int row = row0 + it * RSTEP;
    const int64_t m = m0 + row;
    if (m < a.M) {  // uniform for the lanes of a row
      const int64_t pm = phys_row(m);
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(sF + row * LDS_F + nc);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(sF + row * LDS_F + nc + 4);
      float t[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      // ---- the GEMM's own epilogue (same order as gemm_epilogue): bias, alpha, dropout / self_resid, residual
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = (t[e] + bias8[e]) * a.alpha;
      if (MODE == 1 && (has_drop || a.self_resid)) {
        float u0[4] = {t[0], t[1], t[2], t[3]}, u1[4] = {t[4], t[5], t[6], t[7]};
        if (has_drop) {
          const uint64_t w = (uint64_t)(pm * a.N + nc) >> 2;
          dropout_apply4(dkey, w, dthr, inv_keep, u0);
          dropout_apply4(dkey, w + 1, dthr, inv_keep, u1);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[e] = a.self_resid ? t[e] + u0[e] : u0[e];
          t[4 + e] = a.self_resid ? t[4 + e] + u1[e] : u1[e];
        }
      }
      if (resid || lds_resid) {
        Pack8 p8; p8.u = rv[it];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] += bits_to_f32<T>(p8.h[e]);
      }
      // the value the unfused pipeline would have stored and re-read: round to the activation type first
      Pack8 hb;
#pragma unroll
      for (int e = 0; e < 8; ++e) { hb.h[e] = f32_to_bits<T>(t[e]); t[e] = bits_to_f32<T>(hb.h[e]); }
      if (MODE == 1) {
        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(a.C) + pm * a.ldc + nc) = hb.u;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += t[e];
        const float mean = row_sum<CPR>(s) * inv_n;
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { t[e] -= mean; ss += t[e] * t[e]; }
        const float rstd = 1.f / sqrtf(row_sum<CPR>(ss) * inv_n + l.eps);
        Pack8 yb;
#pragma unroll
        for (int e = 0; e < 8; ++e) yb.h[e] = f32_to_bits<T>(t[e] * rstd * gam8[e] + bet8[e]);
        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(l.out) + pm * l.ld_out + nc) = yb.u;
        if (lds_out) *reinterpret_cast<u32x4*>(lds_out + row * lds_out_ld + nc) = yb.u;
        if (ch == 0) { l.mean[pm] = mean; l.rstd[pm] = rstd; }
      } else {
        const int64_t rid = pm;  // x, the statistics and the forward's dropout counter live at the PHYSICAL row of C
        const float mean = mean_r[it], rstd = rstd_r[it];
        Pack8 xb; xb.u = xv[it];
        float xh[8], g[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[e] = (bits_to_f32<T>(xb.h[e]) - mean) * rstd;
          g[e] = t[e] * gam8[e];
          s1 += g[e];
          s2 += g[e] * xh[e];
          dg8[e] += t[e] * xh[e];
          db8[e] += t[e];
        }
        s1 = row_sum<CPR>(s1) * inv_n;
        s2 = row_sum<CPR>(s2) * inv_n;
        uint32_t keep8 = 0xFFu;
        if (l.mask_mode != 0 && has_drop) {
          const uint64_t w = (uint64_t)(rid * BN + nc) >> 2;  // the forward's counter: forward row id, N == BN columns
          keep8 = dropout_keep4k(dkey, w, dthr) | (dropout_keep4k(dkey, w + 1, dthr) << 4);
        }
        Pack8 ob, mb;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float o = rstd * (g[e] - s1 - xh[e] * s2);
          float om = 0.f;
          if (l.mask_mode != 0) {
            const float k = has_drop ? (((keep8 >> e) & 1u) ? inv_keep : 0.f) : 1.f;
            if (l.mask_mode == 1) om = o * k; else o = o * (1.f + k);
          }
          ob.h[e] = f32_to_bits<T>(o);
          mb.h[e] = f32_to_bits<T>(om);
        }
        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(a.C) + pm * a.ldc + nc) = ob.u;
        if (l.mask_mode == 1) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(l.out) + m * l.ld_out + nc) = mb.u;
        if (lds_out) *reinterpret_cast<u32x4*>(lds_out + row * lds_out_ld + nc) = l.mask_mode == 1 ? mb.u : ob.u;
      }
    } else if (lds_out) {
      *reinterpret_cast<u32x4*>(lds_out + row * lds_out_ld + nc) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  FFN_STAMP(7);
  if (MODE == 2) {
    // dgamma / dbeta: sum the RSTEP row groups through LDS (the staged tile is dead), one atomic per column per workgroup
    __syncthreads();
    float* red = sF;  // [2][RSTEP][BN]
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[row0 * BN + nc + e] = dg8[e];
      red[(RSTEP + row0) * BN + nc + e] = db8[e];
    }
    __syncthreads();
    for (int c = tid; c < 2 * BN; c += NT) {
      const int which = c / BN, col = c % BN;
      float s = 0.f;
      for (int r = 0; r < RSTEP; ++r) s += red[(which * RSTEP + r) * BN + col];
      if (l.partials) l.partials[(int64_t)blockIdx.x * 2 * BN + c] = s;  // [dgamma | dbeta], summed by partial_sums_kernel
      else atomicAdd((which ? l.dbeta : l.dgamma) + col, s);
    }
  }
}

}  // namespace mst

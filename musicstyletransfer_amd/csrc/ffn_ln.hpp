// ffn_ln.hpp — ffn_ln_body: the feed-forward block of a Transformer layer on one 64-row tile, as a device function. ffn_ln_kernel
// (ffn_ln.hip) is this body alone; dec_tail_kernel (dec_tail.hip) runs it as the first and the last phase of a workgroup.
#pragma once
#include <type_traits>
#include "gemm_ln.hpp"

namespace mst {

// The whole feed-forward block of a Transformer layer in ONE launch (mst_ffn_ln_fwd):
//     a  = dropout(relu(x W1^T + b1))                 (transformer.py:38-40 / 152-153)
//     h2 = epi(a W2^T + b2) with the layer's residual form, y = LayerNorm(h2)      (transformer.py:157-158 / 199-200)
// = mst_gemm_nt(ff1) followed by mst_gemm_nt_ln(ff2, mode 1), bit for bit: the same MFMA sequence per output element (K
// in the same order), the same epilogues. A workgroup owns 64 rows for both GEMMs. The hidden activation is produced
// in chunks of BN (= the model width) columns: one chunk is a 64 x BN tile of the first GEMM (K = BN), finished in
// registers (bias, ReLU, dropout, rounding), parked in LDS as 16-bit — from where it is the A operand of the second GEMM's
// K-slice for that chunk, and is copied out to `a` for the backward pass with full-line stores. So the hidden tensor
// (33 MB at configs[1]) is written once and never read back, the 64 x BN accumulators of the second GEMM stay in
// registers across the F / BN chunks, and three launches (FFN1, FFN2, LayerNorm) become one. Weights stream through a
// double-buffered LDS stage exactly as in gemm_mainloop (both GEMMs of a chunk are stages of ONE pipelined stream);
// every workgroup reads both matrices once (1 MB at configs[1]: ~8 us at the ~127 GB/s a CU pulls from L2).
// MODE 2 is the block's backward pass with the same skeleton (mst_ffn_ln_bwd): the first GEMM is the FFN2 dgrad
// (d(pre-activation) = (dff W2) * alpha, then the ReLU gate a > 0), the second the FFN1 dgrad with the LayerNorm backward in
// its epilogue (mst_gemm_nt_ln mode 2). The gate is applied in a row-layout pass over the parked chunk (coalesced 16-byte
// reads of `a`), which is also the pass that stores the chunk for the weight-gradient launch.
// LEAD (backward only): the block's input tile is not loaded but COMPUTED — the layer's leading LayerNorm backward on the
// workgroup's 64 rows (mst_ffn_ln_bwd_lead), one launch and one 8 + 8 MB round trip less.
// FULL: M is a multiple of 64 (no row guards). The guards, like every other conditional load in the stage loop, are not
// free: hipcc cannot count outstanding loads across a branch and falls back to s_waitcnt vmcnt(0), which drains the
// weight ring — the launch is bound by a single workgroup's serial latency (35 us for ONE workgroup, 42 for 256), so
// every such drain is a full L2 round trip on the critical path. Hence also: bias of the first GEMM read from LDS
// (it was a global load + vmcnt(0) inside the chunk epilogue), prefetches issued unconditionally (clamped).
// EXTRA: one more GEMM on the workgroup's rows in FRONT, in the same launch (gx; its weights are extra stages of the same stream).
// Forward (mst_proj_ffn_ln_fwd): the attention output projection (width x width) + residual + LayerNorm — the input
// tile is the attention output, the block's input x1 = LayerNorm(h1) is computed by mst_gemm_nt_ln's forward epilogue
// (gx, lnx) into the x tile (and stored, with h1 and the statistics, for the backward pass).
// Backward, with LEAD (mst_kqv_ffn_ln_bwd): the K | Q | V input gradient of the layer ABOVE (width x 3 width, + residual) — the
// gradient tile LEAD starts from is not loaded but computed, with mst_gemm_nt's arithmetic (K ascending, one rounding behind the
// residual add), into the x tile; LEAD then takes its dy pieces from there. Twelve more stages of the same stream at width 256; the
// 64 x 3 width A operand passes through the two activation tiles in three slices (x tile, hidden tile, x tile), the third slice
// and the residual waiting in registers from the prologue on — no load inside the head's stage loop but the weight ring's.
// (The mirror image of the forward head — the projection's dgrad behind the backward block — and a form with every wave loading
// its own weight fragments straight into MFMA operand registers were built, measured slower / not worth a third shadow layout,
// and removed: docs/kernel_notes.md.)
// The block is a device function (ffn_ln_body) so that a launch can run it as one of several phases of a workgroup (dec_tail_kernel):
//   X_IN_LDS   the input tile already sits in the x tile (the previous phase's epilogue left it there): it is not loaded
//   KEEP_OUT   the last epilogue's result rows ALSO stay in the x tile (gemm_epilogue_ln's lds_out), for the phase that follows
//   PAR_READY  the first GEMM's bias and bias | gamma | beta of the last epilogue already wait at `par` ([F][3 BN] floats)
//   before_epilogue()  called in front of the last epilogue (the next phase's first loads, whose latency then runs under it)
// The argument structs come by value: the row-group form rewrites their M, and the compiler sees private copies, as in a kernel.
template <typename T, int BN, int WGM, int WGN, int MODE, bool LEAD, bool FULL, bool EXTRA, bool X_IN_LDS = false, bool KEEP_OUT = false,
          bool PAR_READY = false, typename Hook>
__device__ __forceinline__ void ffn_ln_body(unsigned char* smem, mst_gemm_args g1, mst_gemm_args g2, const mst_ln_args ln,
                                            const mst_ln_bwd_in lead, mst_gemm_args gx, const mst_ln_args lnx, float* par,
                                            Hook&& before_epilogue) {
  constexpr bool HEAD = EXTRA, FHEAD = EXTRA && MODE == 1, BHEAD = EXTRA && MODE == 2;  // (HEAD: what both heads share — the stream)
  static_assert(!(X_IN_LDS && (LEAD || EXTRA)), "a tile left in LDS is the block's own input");
  static_assert(!BHEAD || LEAD, "the backward form's head computes the gradient tile of the leading LayerNorm backward");
  constexpr int BM = 64, BK = 64, CHUNKS = BK / 8;
  constexpr int NT = WGM * WGN * 64;
  constexpr int WTM = BM / WGM, WTN = BN / WGN, TM = WTM / 16, TN = WTN / 16;
  constexpr int B_CH = BN * CHUNKS / NT;  // 16-byte pieces of a weight stage per thread
  constexpr int LDA = BN + 8;                  // row stride (elements) of the two activation tiles: conflict-free b128 reads
  constexpr int KST = BN / BK;                 // K stages of one GEMM of a chunk (K = BN for both)
  constexpr int XST = BHEAD ? 3 * KST : KST;   // K stages of the head GEMM (forward: K = BN; backward: K = 3 BN)
  static_assert(BN * CHUNKS % NT == 0 && (BM * BN / 8) % NT == 0, "tile/threads mismatch");
  typedef typename Act<T>::vec8 vec8;
  // [weight stages 2 x BN x 64][hidden chunk 64 x LDA][x tile 64 x LDA]; the LayerNorm epilogue's fp32 staging tile reuses
  // the first two regions (both dead by then)
  u32x4* sB = reinterpret_cast<u32x4*>(smem);
  T* sH = reinterpret_cast<T*>(smem + (size_t)2 * BN * BK * 2);
  T* sX = sH + BM * LDA;
  float* sBias1 = PAR_READY ? par : reinterpret_cast<float*>(sX + BM * LDA);  // [F] the first GEMM's bias (zeros without one)
  float* sPar = sBias1 + g1.N;   // [2][3 BN]: bias | gamma | beta of the final epilogue, then of the head's (EXTRA forward)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, frow = lane & 15, fq = lane >> 4;
  // (row tiles in XCD-contiguous eighths, like the GEMMs' tiles and the attention workgroups: common.hpp xcd_chunk)
  int64_t m0 = xcd_chunk(blockIdx.x, gridDim.x) * BM;
  // Row groups (g1's A remap, the only remap the block takes): the block's M rows are rows [offset, offset + rows_per_group) of
  // every group of `stride` physical rows — the last decoder layer skips each sample's position-0 row, whose output is dropped
  // before the loss (model.py:253): 64 x 256 rows are 256 tiles, one resident round, where 64 x 257 were 257. Groups are whole
  // tiles (host check), so the tile moves as a block and every row address below is m0 + row as before; the dropout counters and
  // the LayerNorm statistics stay indexed by the PHYSICAL row.
  if (g1.a_rows_per_group > 0) {
    const uint32_t grp = (uint32_t)m0 / (uint32_t)g1.a_rows_per_group;
    m0 += (int64_t)grp * (g1.a_group_stride - g1.a_rows_per_group) + g1.a_group_offset;
    // (the epilogues' row guards compare physical rows against M: every row of a whole tile exists)
    g1.M = g2.M = gx.M = (g1.M / g1.a_rows_per_group) * g1.a_group_stride;
  }
  const int64_t F = g1.N;
  FFN_STAMP(0); FFN_RT(190);
  const int64_t Mg = FULL ? (int64_t)1 << 62 : g1.M;  // row guards compare against this (FULL: always true, folded away)
  if constexpr (!PAR_READY)
  for (int i = tid * 4; i < (int)F; i += NT * 4)
    *reinterpret_cast<f32x4*>(sBias1 + i) = g1.bias ? *reinterpret_cast<const f32x4*>(g1.bias + i) : f32x4{0.f, 0.f, 0.f, 0.f};
  // (the step's dropout seed words too: a scalar load at an epilogue's start is one more exposed round trip)
  const uint64_t seed2 = g2.dropout_seed ^ ((g2.dropout_p > 0.f && g2.dropout_seed_ptr) ? g2.dropout_seed_ptr[0] : 0ull);
  const uint64_t seedx = FHEAD ? gx.dropout_seed ^ ((gx.dropout_p > 0.f && gx.dropout_seed_ptr) ? gx.dropout_seed_ptr[0] : 0ull) : 0ull;
  if constexpr (!PAR_READY)
  for (int i = tid; i < BN; i += NT) {
    sPar[i] = g2.bias ? g2.bias[i] : 0.f;
    sPar[BN + i] = ln.gamma[i];
    sPar[2 * BN + i] = (MODE == 1) ? ln.beta[i] : 0.f;
    if constexpr (FHEAD) {
      sPar[3 * BN + i] = gx.bias ? gx.bias[i] : 0.f;
      sPar[4 * BN + i] = lnx.gamma[i];
      sPar[5 * BN + i] = lnx.beta[i];
    }
  }
  const int n_chunks = (int)(F / BN);
  // Chunk order rotated per workgroup: every workgroup streams BOTH weight matrices in full, and 256 of them walking the
  // same lines in lockstep hit the same L2 channels at the same time. Workgroup i of an XCD starts at hidden chunk
  // i mod n_chunks; the second GEMM's sum over the chunks then runs in rotated order (fp32, a different rounding order
  // than the three-launch form; `a` itself is unchanged). The K order inside a GEMM is not rotated, so `a` stays
  // bit-identical to the three-launch form.
  const int rot = (int)((blockIdx.x / 8) % (unsigned)n_chunks);
  auto phys = [&](int c) { const int pc = c + rot; return pc >= n_chunks ? pc - n_chunks : pc; };
  const T* __restrict__ W1 = reinterpret_cast<const T*>(g1.B);
  const T* __restrict__ W2 = reinterpret_cast<const T*>(g2.B);
  const T* __restrict__ WX = reinterpret_cast<const T*>(gx.B);  // EXTRA: chunk -1 (head) / chunk n_chunks (tail) of the stream

  // ---- weight stream: stage s of chunk c is GEMM 1 (s < KST: W1 rows c*BN.., columns s*64..) or GEMM 2 (W2 rows 0..BN-1,
  // columns c*BN + (s-KST)*64..). Per-thread element offsets are constants; the uniform base moves.
  uint32_t off1[B_CH], off2[B_CH], offx[B_CH];
  int b_lds[B_CH];
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    const int c = tid + i * NT;
    const int row = c / CHUNKS, ch = c % CHUNKS;
    off1[i] = (uint32_t)row * (uint32_t)g1.ldb + (uint32_t)ch * 8u;
    off2[i] = (uint32_t)row * (uint32_t)g2.ldb + (uint32_t)ch * 8u;
    offx[i] = EXTRA ? (uint32_t)row * (uint32_t)gx.ldb + (uint32_t)ch * 8u : 0u;
    b_lds[i] = row * CHUNKS + (ch ^ (row & 7));
  }
  // The stream runs AHEAD stages in front of the MFMAs, in a register ring: with one 8-wave workgroup per CU (BN = 256:
  // 133 KB of LDS) nothing else hides a weight load's ~1.5 us, and a single stage of lookahead (gemm_mainloop's scheme,
  // which relies on 2-5 co-resident workgroups) made every stage as long as that latency: 52 us for the launch.
  constexpr int SPC = 2 * KST;                 // stages per chunk (a multiple of the ring: slots are compile-time)
  constexpr int RING = BN >= 256 ? 4 : 2, AHEAD = RING - 1;
  static_assert(SPC % RING == 0, "ring slots must repeat per chunk");
  u32x4 ring[RING][B_CH];
  auto load_stage = [&](int c, int s, u32x4 (&rb)[B_CH]) {  // (c, s) uniform
    if (HEAD && c < 0) {  // the extra GEMM's K stage s
      const T* base = WX + s * BK;
#pragma unroll
      for (int i = 0; i < B_CH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(base + offx[i]);
    } else if (s < KST) {
      const T* base = W1 + (int64_t)phys(c) * BN * g1.ldb + s * BK;
#pragma unroll
      for (int i = 0; i < B_CH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(base + off1[i]);
    } else {
      const T* base = W2 + (int64_t)phys(c) * BN + (s - KST) * BK;
#pragma unroll
      for (int i = 0; i < B_CH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(base + off2[i]);
    }
  };
  auto load_piece = [&](int c, int s, u32x4 (&rb)[B_CH], auto ic) {  // one 16-byte piece of load_stage
    constexpr int i = decltype(ic)::value;
    const T* base;
    uint32_t off;
    if (HEAD && c < 0) { base = WX + s * BK; off = offx[i]; }
    else if (s < KST) { base = W1 + (int64_t)phys(c) * BN * g1.ldb + s * BK; off = off1[i]; }
    else { base = W2 + (int64_t)phys(c) * BN + (s - KST) * BK; off = off2[i]; }
    rb[i] = *reinterpret_cast<const u32x4*>(base + off);
  };
  auto store_stage = [&](int buf, const u32x4 (&rb)[B_CH]) {
#pragma unroll
    for (int i = 0; i < B_CH; ++i) sB[buf * BN * CHUNKS + b_lds[i]] = rb[i];
  };
  // the first AHEAD stages are requested before the input tile is built: their latency runs under it
  {
    auto pro = [&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr (HEAD) {
        static_assert(!HEAD || AHEAD <= XST, "the head GEMM's stages cover the prologue");
        if (j < AHEAD) load_stage(-1, j, ring[j % RING]);
      } else {
        if (j < AHEAD && (j < SPC || n_chunks > 1)) load_stage(j / SPC, j % SPC, ring[j % RING]);
      }
    };
    pro(std::integral_constant<int, 0>()); pro(std::integral_constant<int, 1>()); pro(std::integral_constant<int, 2>());
    pro(std::integral_constant<int, 3>()); pro(std::integral_constant<int, 4>()); pro(std::integral_constant<int, 5>());
    pro(std::integral_constant<int, 6>());
    static_assert(AHEAD <= 7, "the prologue list covers seven stages");
  }
  // ---- LEAD: the input tile = LayerNorm backward of the incoming gradient (the arithmetic of gemm_epilogue_ln's mode 2 on dy).
  // A thread owns the 16-byte pieces (row lrow0 + it * L_RSTEP, columns lnc..lnc+7) of the tile. Two parts: the loads (everything
  // the rows need from global memory), then the rows themselves — back to back, or (BHEAD) with the head GEMM in between, whose
  // stages then run over the latency of x, mean and rstd.
  constexpr int L_CPR = BN / 8, L_RSTEP = NT / L_CPR, L_ITERS = BM / L_RSTEP;
  const int lnc = (tid % L_CPR) * 8, lrow0 = tid / L_CPR;
  uint32_t ldkey = 0u, ldthr = 0u;
  float linv_keep = 1.f, gam8[8], dg8[8], db8[8];
  u32x4 dyv[L_ITERS], xv[L_ITERS];
  float mean_r[L_ITERS], rstd_r[L_ITERS];
  // BHEAD: the third K-slice of the head's A operand and the head's residual tile, in registers until their LDS tile is free
  u32x4 ha2[L_ITERS], hres[L_ITERS];
  auto lead_loads = [&] {
    constexpr int RSTEP = L_RSTEP, ITERS = L_ITERS;
    const int nc = lnc, row0 = lrow0;
    const bool has_drop = lead.dropout_p > 0.f && lead.mask_mode == 1;
    const uint64_t dseed = lead.dropout_seed ^ ((has_drop && lead.dropout_seed_ptr) ? lead.dropout_seed_ptr[0] : 0ull);
    ldkey = dropout_key(dseed, lead.dropout_site); ldthr = dropout_thr(lead.dropout_p);
    linv_keep = dropout_inv_keep(lead.dropout_p);
#pragma unroll
    for (int e = 0; e < 8; ++e) { gam8[e] = lead.gamma[nc + e]; dg8[e] = 0.f; db8[e] = 0.f; }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int64_t m = m0 + row0 + it * RSTEP;
      dyv[it] = u32x4{0u, 0u, 0u, 0u}; xv[it] = dyv[it]; mean_r[it] = 0.f; rstd_r[it] = 0.f;
      if (m < Mg) {
        if constexpr (!BHEAD) dyv[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(lead.dy) + m * lead.ld_dy + nc);
        xv[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(lead.x) + m * lead.ld_x + nc);
        mean_r[it] = lead.mean[m];
        rstd_r[it] = lead.rstd[m];
      }
    }
  };
  auto lead_rows = [&] {
    constexpr int CPR = L_CPR, RSTEP = L_RSTEP, ITERS = L_ITERS;
    const int nc = lnc, row0 = lrow0;
    const float inv_n = 1.f / (float)BN;
    const bool has_drop = lead.dropout_p > 0.f && lead.mask_mode == 1;
    const uint32_t dkey = ldkey, dthr = ldthr;
    const float inv_keep = linv_keep;
    if constexpr (BHEAD) {
      // the head left the rounded gradient tile in the x tile (published by its barrier); gx.C, when given, receives it
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int row = row0 + it * RSTEP;
        const int64_t m = m0 + row;
        if (m < Mg) {
          dyv[it] = *reinterpret_cast<const u32x4*>(sX + row * LDA + nc);
          if (gx.C) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(gx.C) + m * gx.ldc + nc) = dyv[it];
        }
      }
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = row0 + it * RSTEP;
      const int64_t m = m0 + row;
      Pack8 db, xb;
      db.u = dyv[it]; xb.u = xv[it];
      float xh[8], g[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = bits_to_f32<T>(db.h[e]);
        xh[e] = (bits_to_f32<T>(xb.h[e]) - mean_r[it]) * rstd_r[it];
        g[e] = d * gam8[e];
        s1 += g[e];
        s2 += g[e] * xh[e];
        dg8[e] += d * xh[e];
        db8[e] += d;
      }
      s1 = row_sum<CPR>(s1) * inv_n;
      s2 = row_sum<CPR>(s2) * inv_n;
      uint32_t keep8 = 0xFFu;
      if (has_drop) {
        const uint64_t w = (uint64_t)(m * BN + nc) >> 2;
        keep8 = dropout_keep4k(dkey, w, dthr) | (dropout_keep4k(dkey, w + 1, dthr) << 4);
      }
      Pack8 ob, mb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float o = rstd_r[it] * (g[e] - s1 - xh[e] * s2);
        const float k = has_drop ? (((keep8 >> e) & 1u) ? inv_keep : 0.f) : 1.f;
        ob.h[e] = f32_to_bits<T>(o);
        mb.h[e] = f32_to_bits<T>(o * k);
      }
      if (m < Mg) {
        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(lead.dx) + m * lead.ld_dx + nc) = ob.u;
        if (lead.mask_mode == 1) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(lead.dx_masked) + m * lead.ld_dxm + nc) = mb.u;
      }
      *reinterpret_cast<u32x4*>(sX + row * LDA + nc) = (m < Mg) ? (lead.mask_mode == 1 ? mb.u : ob.u) : u32x4{0u, 0u, 0u, 0u};
    }
    // dgamma / dbeta: the RSTEP row groups summed through LDS (the weight-stage region is not in use yet)
    float* red = reinterpret_cast<float*>(smem);  // [2][RSTEP][BN]
    static_assert((size_t)2 * RSTEP * BN * 4 <= (size_t)2 * BN * BK * 2, "reduction scratch must fit the weight stages");
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[row0 * BN + nc + e] = dg8[e];
      red[(RSTEP + row0) * BN + nc + e] = db8[e];
    }
    __syncthreads();
    for (int c = tid; c < 2 * BN; c += NT) {
      const int which = c / BN, col = c % BN;
      float sm = 0.f;
      for (int r = 0; r < RSTEP; ++r) sm += red[(which * RSTEP + r) * BN + col];
      if (lead.partials) lead.partials[(int64_t)blockIdx.x * 2 * BN + c] = sm;
      else atomicAdd((which ? lead.dbeta : lead.dgamma) + col, sm);
    }
    __syncthreads();  // the scratch becomes the first weight stage
  };
  if constexpr (BHEAD) {
    // ---- the head's A operand (64 x 3 BN) and residual tile, all requested here: slices 0 and 1 go to the x tile and the hidden
    // tile (dead until the first chunk), slice 2 and the residual wait in registers (extra_gemm stores them once their tile is free)
    constexpr int RSTEP = L_RSTEP, ITERS = L_ITERS;
    const T* HA = reinterpret_cast<const T*>(gx.A);
    const T* HR = reinterpret_cast<const T*>(gx.resid);
    u32x4 ha0[ITERS], ha1[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int64_t m = m0 + lrow0 + it * RSTEP;
      ha0[it] = u32x4{0u, 0u, 0u, 0u}; ha1[it] = ha0[it]; ha2[it] = ha0[it]; hres[it] = ha0[it];
      if (m < Mg) {
        const T* ap = HA + m * gx.lda + lnc;
        ha0[it] = *reinterpret_cast<const u32x4*>(ap);
        ha1[it] = *reinterpret_cast<const u32x4*>(ap + BN);
        ha2[it] = *reinterpret_cast<const u32x4*>(ap + 2 * BN);
        hres[it] = *reinterpret_cast<const u32x4*>(HR + m * gx.ldr + lnc);  // (the head always has a residual: host check)
      }
    }
    lead_loads();
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = lrow0 + it * RSTEP;
      *reinterpret_cast<u32x4*>(sX + row * LDA + lnc) = ha0[it];
      *reinterpret_cast<u32x4*>(sH + row * LDA + lnc) = ha1[it];
    }
  } else if constexpr (LEAD) {
    lead_loads();
    lead_rows();
  } else if constexpr (!X_IN_LDS)
  // ---- the x tile (rows past M read as zero)
  {
    // (HEAD: the attention output tile, the extra GEMM's A operand; the block's own input is computed from it below)
    const T* X = reinterpret_cast<const T*>(HEAD ? gx.A : g1.A);
    const int64_t ldx = HEAD ? gx.lda : g1.lda;
    constexpr int CPR = BN / 8;
#pragma unroll
    for (int i = 0; i < BM * CPR / NT; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m0 + row < Mg) v = *reinterpret_cast<const u32x4*>(X + (m0 + row) * ldx + ch * 8);
      *reinterpret_cast<u32x4*>(sX + row * LDA + ch * 8) = v;
    }
  }
  // one 64-deep K stage: acc += A[64, 64] (`sA`: the stage's first column in an LDS tile of row stride LDA) x stage `buf`
  // hook(k), k < 2 * TN: called behind the k-th row of MFMAs of the stage — the staged form hangs the weight staging
  // there (IL below), piece by piece, instead of issuing it in front of / behind the whole stage
  auto mma_stage = [&](f32x4 (&acc)[TN][TM], const T* sA, int buf, const u32x4 (&rb)[B_CH], auto&& hook) {
    const u32x4* cB = sB + buf * BN * CHUNKS;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      vec8 xf[TM], wf[TN];
      const int kc = ks * 4 + fq;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        xf[i] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(sA + (wm * WTM + i * 16 + frow) * LDA + kc * 8));
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 16 + frow;
        wf[j] = __builtin_bit_cast(vec8, cB[row * CHUNKS + (kc ^ (row & 7))]);
      }
      auto row = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j < TN) {
#pragma unroll
          for (int i = 0; i < TM; ++i) acc[j][i] = Act<T>::mfma16(wf[j], xf[i], acc[j][i]);
          if (ks == 0) hook(std::integral_constant<int, j>()); else hook(std::integral_constant<int, TN + j>());
        }
      };
      static_assert(TN <= 4, "row list");
      row(std::integral_constant<int, 0>()); row(std::integral_constant<int, 1>());
      row(std::integral_constant<int, 2>()); row(std::integral_constant<int, 3>());
    }
  };
  auto no_hook = [](auto) {};

  f32x4 acc1[TN][TM], acc2[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc2[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float p1 = g1.dropout_p;
  const bool drop1 = MODE == 1 && p1 > 0.f;  // (the backward form takes neither dropout nor an activation: host check)
  const uint64_t seed1 = g1.dropout_seed ^ ((drop1 && g1.dropout_seed_ptr) ? g1.dropout_seed_ptr[0] : 0ull);
  const uint32_t dkey1 = dropout_key(seed1, g1.dropout_site), dthr1 = dropout_thr(p1);
  const float inv_keep1 = dropout_inv_keep(p1);
  const bool idx32 = (uint64_t)g1.M * (uint64_t)F < (1ull << 32);  // every element index of the hidden tensor fits 32 bits (uniform)
  const bool relu1 = MODE == 1 && g1.act == MST_ACT_RELU;
  const bool step_form1 = MODE == 1 && relu1 && drop1 && idx32 && g1.alpha == 1.f;  // (x * 1.0f == x bit for bit)
  // dropout counters of this thread's rows, premultiplied (dropout_apply4_pre): ((m0 + row) F / 2) * DROPOUT_MUL mod 2^32 (F % 4 == 0: host check)
  uint32_t rowmul[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rowmul[i] = (uint32_t)(m0 + wm * WTM + i * 16 + frow) * (uint32_t)(F >> 1) * DROPOUT_MUL;
  T* Aout = reinterpret_cast<T*>(g1.C);

  // the XST stages of the extra GEMM (stream position `cx` = -1: in front of the chunks) into acc1. K-slice s / KST of its A operand
  // sits in the x tile (even slices) or the hidden tile (odd ones); BHEAD: behind the barrier that ends a slice's last stage, the
  // tile it frees takes what waited in registers for it — slice 2 the x tile, the residual the hidden tile
  auto extra_gemm = [&](int cx) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc1[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    store_stage(0, ring[0]);
    __syncthreads();
    auto xstage = [&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if constexpr (s < XST) {
        constexpr int t = s + AHEAD;
        if constexpr (t < XST) load_stage(cx, t, ring[t % RING]);
        else if constexpr (HEAD) load_stage(0, t - XST, ring[t % RING]);  // the first chunk's stages follow (XST % RING == 0)
        mma_stage(acc1, (((s / KST) & 1) ? sH : sX) + (s % KST) * BK, s & 1, ring[s % RING], no_hook);
        if constexpr (s + 1 < XST) store_stage((s + 1) & 1, ring[(s + 1) % RING]);
        __syncthreads();
        if constexpr (BHEAD && (s == KST - 1 || s == 2 * KST - 1)) {
#pragma unroll
          for (int it = 0; it < L_ITERS; ++it)
            *reinterpret_cast<u32x4*>((s == KST - 1 ? sX : sH) + (lrow0 + it * L_RSTEP) * LDA + lnc) = s == KST - 1 ? ha2[it] : hres[it];
        }
      }
    };
    // (an even stage count: the first chunk starts in LDS buffer 0, as without a head)
    static_assert(!EXTRA || (XST <= 12 && XST % RING == 0 && XST % 2 == 0), "the extra GEMM stage list / ring slots");
    xstage(std::integral_constant<int, 0>()); xstage(std::integral_constant<int, 1>());
    xstage(std::integral_constant<int, 2>()); xstage(std::integral_constant<int, 3>());
    xstage(std::integral_constant<int, 4>()); xstage(std::integral_constant<int, 5>());
    xstage(std::integral_constant<int, 6>()); xstage(std::integral_constant<int, 7>());
    xstage(std::integral_constant<int, 8>()); xstage(std::integral_constant<int, 9>());
    xstage(std::integral_constant<int, 10>()); xstage(std::integral_constant<int, 11>());
  };
  if constexpr (BHEAD) {
    // dy = round16(acc + resid): gemm_epilogue's residual add and its one rounding, in accumulator layout (the residual tile sits
    // in the hidden tile, the result goes to the x tile, both free behind the last stage's barrier); then the LayerNorm backward
    extra_gemm(-1);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + frow, n = wn * WTN + j * 16 + fq * 4;
        const u32x2 rb = *reinterpret_cast<const u32x2*>(sH + row * LDA + n);
        uint16_t hb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          hb[e] = f32_to_bits<T>(acc1[j][i][e] + bits_to_f32<T>((uint16_t)(rb[e >> 1] >> ((e & 1) * 16))));
        *reinterpret_cast<u32x2*>(sX + row * LDA + n) =
            u32x2{(uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16)};
      }
    __syncthreads();
    lead_rows();
  }
  if constexpr (FHEAD) {
    // h1 = epi(att Wp^T) (+ x), x1 = LayerNorm(h1): mst_gemm_nt_ln's forward epilogue; x1 also lands in the x tile
    extra_gemm(-1);
    gemm_epilogue_ln<T, BM, BN, WGM, WGN, 1>(gx, lnx, smem, acc1, m0, nullptr, 0, sX, LDA, sPar + 3 * BN, &seedx);
    __syncthreads();  // the staging tile (over the weight stages) is dead, the x tile complete
  }
  store_stage(0, ring[0]);
  __syncthreads();  // (also publishes the x tile)
  FFN_STAMP(1);
  for (int c = 0; c < n_chunks; ++c) {
    const int pc = phys(c);  // the hidden chunk this iteration computes
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc1[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // backward: this chunk's gate rows (the forward's hidden activation), requested now, used after the first GEMM
    constexpr int OUT_CH = BM * (BN / 8) / NT;
    u32x4 gv[OUT_CH];
    if constexpr (MODE == 2) {
      const T* G = reinterpret_cast<const T*>(g1.gate);
#pragma unroll
      for (int i = 0; i < OUT_CH; ++i) {
        const int cc = tid + i * NT, row = cc / (BN / 8), ch = cc % (BN / 8);
        gv[i] = u32x4{0u, 0u, 0u, 0u};
        if (m0 + row < Mg) gv[i] = *reinterpret_cast<const u32x4*>(G + (m0 + row) * g1.ldg + (int64_t)pc * BN + ch * 8);
      }
    }
    auto stage = [&](auto sc) {
      constexpr int s = decltype(sc)::value;      // stage within the chunk: ring slot s % RING, LDS buffer s % 2
      if constexpr (s < SPC) {
        constexpr bool IL = BN >= 256 && B_CH <= 2 * TN;  // (width 128, two workgroups per CU: measured 1 us slower)
        // request stage s + AHEAD of the stream (it may belong to the next chunk)
        constexpr int t = s + AHEAD;
        // (unconditional: past the last chunk the clamped load fetches a stage nobody stores)
        const int tc = t < SPC ? c : (c + 1 < n_chunks ? c + 1 : c);
        const bool more = s + 1 < SPC || c + 1 < n_chunks;  // a next stage exists: its weights go to the other LDS buffer
        // interleaved form: piece k of { load of stage s + AHEAD, LDS store of stage s + 1 } behind the k-th row of MFMAs
        auto piece = [&](auto kc) {
          constexpr int k = decltype(kc)::value;
          if constexpr (IL && k < B_CH) {
            __builtin_amdgcn_sched_barrier(0);
            load_piece(tc, t % SPC, ring[t % RING], kc);
            if (more) sB[((s + 1) & 1) * BN * CHUNKS + b_lds[k]] = ring[(s + 1) % RING][k];
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        if constexpr (!IL) load_stage(tc, t % SPC, ring[t % RING]);
        FFN_STAMP(8 + (c * SPC + s) * 4);
        if constexpr (s < KST) mma_stage(acc1, sX + s * BK, s & 1, ring[s % RING], piece);
        else mma_stage(acc2, sH + (s - KST) * BK, s & 1, ring[s % RING], piece);
        FFN_STAMP(8 + (c * SPC + s) * 4 + 1);
        if constexpr (s == KST - 1) {
          // ---- chunk epilogue of GEMM 1, in registers: bias, ReLU, dropout, rounding (the order of gemm_epilogue) -> sH.
          // (The previous chunk's GEMM-2 stages, which read sH, ended with a barrier.)
          // Two bodies behind ONE uniform branch: the training step's form (ReLU, alpha 1, dropout, 32-bit counters) without a
          // select or a multiplication per optional feature, and the general one. (Run-time feature flags inside the element loop
          // are if-converted into a v_cndmask each: this epilogue is VALU-issue-bound — 592 vector instructions per chunk and wave
          // before, ~300 in the first body.)
          auto chunk_epilogue = [&](auto step_form) {
            constexpr bool STEP = decltype(step_form)::value;
            const uint32_t cmul = ((uint32_t)pc * (BN / 2) + (uint32_t)((wn * WTN + fq * 4) / 2)) * DROPOUT_MUL;  // this chunk, this lane's columns
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const int n = wn * WTN + j * 16 + fq * 4;   // column within the chunk
              const int64_t col = (int64_t)pc * BN + n;    // hidden unit
              const f32x4 b4 = *reinterpret_cast<const f32x4*>(sBias1 + col);
#pragma unroll
              for (int i = 0; i < TM; ++i) {
                const int row = wm * WTM + i * 16 + frow;
                float tv[4];
                if constexpr (STEP) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) tv[e] = fmaxf(acc1[j][i][e] + b4[e], 0.f);
                  // element index (m0 + row) F + col; the word pair of its group of four = dropout_word32(index / 2), + 1
                  dropout_apply4_pre(dkey1, rowmul[i] + cmul + (uint32_t)(j * 8) * DROPOUT_MUL, dthr1, inv_keep1, tv);
                } else {
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    tv[e] = (acc1[j][i][e] + b4[e]) * g1.alpha;
                    if (relu1) tv[e] = fmaxf(tv[e], 0.f);
                  }
                  if (drop1) dropout_apply4(dkey1, (uint64_t)((m0 + row) * F + col) >> 2, dthr1, inv_keep1, tv);
                }
                uint16_t hb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) hb[e] = f32_to_bits<T>(tv[e]);
                *reinterpret_cast<u32x2*>(sH + row * LDA + n) =
                    u32x2{(uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16)};
              }
            }
          };
          if (step_form1) chunk_epilogue(std::true_type()); else chunk_epilogue(std::false_type());
        }
        // the next stage of the stream (requested AHEAD iterations ago) -> the other LDS buffer
        if (!IL && more) store_stage((s + 1) & 1, ring[(s + 1) % RING]);
        FFN_STAMP(8 + (c * SPC + s) * 4 + 2);
        __syncthreads();
        FFN_STAMP(8 + (c * SPC + s) * 4 + 3);
        if constexpr (s == KST - 1) {
          // the finished chunk goes out to `a` (the backward pass needs it) as whole 16-byte pieces of rows, while the
          // second GEMM's stages run
          constexpr int CPR = BN / 8;
#pragma unroll
          for (int i = 0; i < BM * CPR / NT; ++i) {
            const int cc = tid + i * NT, row = cc / CPR, ch = cc % CPR;
            u32x4 v = *reinterpret_cast<const u32x4*>(sH + row * LDA + ch * 8);
            if constexpr (MODE == 2) {  // ReLU backward: pass where the forward activation was positive (gemm_epilogue's gate)
              Pack8 pv, pg;
              pv.u = v; pg.u = gv[i];
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if (!(bits_to_f32<T>(pg.h[e]) > 0.f)) pv.h[e] = 0;
              v = pv.u;
              *reinterpret_cast<u32x4*>(sH + row * LDA + ch * 8) = v;
            }
            if (m0 + row < Mg) *reinterpret_cast<u32x4*>(Aout + (m0 + row) * g1.ldc + (int64_t)pc * BN + ch * 8) = v;
          }
          if constexpr (MODE == 2) __syncthreads();  // the gated chunk is what the second GEMM reads
        }
      }
    };
    static_assert(SPC <= 8, "the stage list below covers eight stages per chunk");
    stage(std::integral_constant<int, 0>()); stage(std::integral_constant<int, 1>());
    stage(std::integral_constant<int, 2>()); stage(std::integral_constant<int, 3>());
    stage(std::integral_constant<int, 4>()); stage(std::integral_constant<int, 5>());
    stage(std::integral_constant<int, 6>()); stage(std::integral_constant<int, 7>());
  }
  // ---- the second GEMM's epilogue + LayerNorm: exactly mst_gemm_nt_ln's (staging tile over the dead weight / hidden regions)
  // (a residual that IS the block's input — the encoder's x1 + dropout(ff) — is taken from the x tile in LDS)
  const bool resid_is_x = g2.resid == g1.A && g2.ldr == g1.lda;
  FFN_STAMP(2);
  before_epilogue();
  // (KEEP_OUT with the residual in the x tile: a thread reads its own residual pieces before it writes the same pieces back)
  gemm_epilogue_ln<T, BM, BN, WGM, WGN, MODE>(g2, ln, smem, acc2, m0, resid_is_x ? sX : nullptr, LDA, KEEP_OUT ? sX : nullptr, KEEP_OUT ? LDA : 0,
                                              sPar, &seed2);
  FFN_STAMP(3); FFN_RT(191);
}

}  // namespace mst

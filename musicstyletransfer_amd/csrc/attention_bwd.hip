// attention_bwd.hip — the backward launches of key-row attention (attention.hip states the operation and chooses the form): streaming,
// attn_bwd_kv_kernel then attn_bwd_q_kernel or the chunked attn_bwd_q_chunk_kernel; resident, attn_bwd_res_kernel with both as phases of
// one launch (attention.hpp: "resident kernels"), dense, sparse and with the W_proj input gradient formed in the launch (dout_prologue).
// The kernels of one direction stay in one unit (attention_fwd.hip says why).
#include "attention_forms.hpp"

namespace mst {

// ------------------------------------------------------------------------------------ bwd_kv
template <typename T, int DH, bool SPARSE = false>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(AttnArgs a) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  __shared__ __attribute__((aligned(16))) T sQ[ATT_STAGE * LdsLd<DH>::V];
  __shared__ __attribute__((aligned(16))) T sdO[ATT_STAGE * LdsLd<DH>::V];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tile; int64_t bh;
  attn_wg_coords(a.B, a.H, tile, bh);
  const int64_t b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;  // (B * H <= 65535: a 32-bit division, not the ~200-instruction 64-bit one, at the head of the kernel)
  const int64_t S = a.S;
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  const T* Kg = base + a.k_off;
  const T* Qg = base + a.q_off;
  const T* Vg = base + a.v_off;
  const T* dOg = reinterpret_cast<const T*>(a.dout) + b * S * a.ld_dout + hd * DH;
  const int64_t k_wave0 = (int64_t)tile * ATT_WG_ROWS + wave * 32;
  const int64_t k_lane = k_wave0 + (lane & 31);
  StageRegs<T, DH> rq, rdo;
  stage_load<T, DH>(rq, Qg, a.ld_qkv, 0, S, tid);
  stage_load<T, DH>(rdo, dOg, a.ld_dout, 0, S, tid);

  typename Act<T>::vec8 kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = glb_row_frag<T>(Kg, a.ld_qkv, k_lane, S, s, lane);
    vf[s] = glb_row_frag<T>(Vg, a.ld_qkv, k_lane, S, s, lane);
  }
  float sk2, ck2, madd, rmax, logl;
  bool exact;
  {
    const bool in = k_lane < S;
    const bool vk = in && a.keymask[b * S + k_lane];
    rmax = in ? a.lse[bh * S + k_lane] : 0.f;
    logl = in ? a.lse[a.B * a.H * S + bh * S + k_lane] : INFINITY;
    madd = vk ? 0.f : MASK_VALUE;
    key_consts(in, vk, rmax, in ? logl : 0.f, a.scale, sk2, ck2);
    exact = __any(in && !vk);  // wave-uniform: one of this wave's 32 keys is padded
  }
  const float ck2s = ck2 + __log2f(a.scale);  // pass 1: the exponential is P * scale

  f32x16 acc[DB];
  float neg_delta = 0.f;
  T* const drow = (k_lane < S) ? reinterpret_cast<T*>(a.dqkv) + (b * S + k_lane) * a.ld_dqkv + hd * DH : nullptr;
  // Sparse mode (0 < q_limit <= 32: dO is zero from row q_limit on — the top encoder layer, as in attn_bwd_res_kernel): dV and delta
  // need the first query tile alone (pass 0 is one stage, one tile), every other tile of dK is the LIGHT form (dP = 0). The dense
  // kernel spent the same 139 us on this layer as on the one below it.
  constexpr bool sparse = SPARSE;  // host: 0 < q_limit <= 32 (a separate instantiation: as run-time branches the dense kernel paid 18 us for them)
  // pass 0: dV and delta; pass 1: dK
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = zero16<DH>();
    const int64_t Sp = (sparse && pass == 0 && S > ATT_STAGE) ? ATT_STAGE : S;  // query rows this pass sweeps
    for (int64_t q0 = 0; q0 < Sp; q0 += ATT_STAGE) {
      __syncthreads();
      stage_store<T, DH>(sQ, rq, tid);
      stage_store<T, DH>(sdO, rdo, tid);
      {  // next stage (wrapping to the first one for the second pass)
        const int64_t qn = (q0 + ATT_STAGE < Sp) ? q0 + ATT_STAGE : 0;
        if (qn != 0 || pass == 0) {
          stage_load<T, DH>(rq, Qg, a.ld_qkv, qn, S, tid);
          stage_load<T, DH>(rdo, dOg, a.ld_dout, qn, S, tid);
        }
      }
      __syncthreads();
#pragma unroll
      for (int blk = 0; blk < ATT_STAGE / 32; ++blk) {
        if (q0 + blk * 32 >= S) break;
        // (query rows >= S need no guard: their staged Q and dO rows are zero)
        if (pass == 0) {
          if (sparse && (q0 > 0 || blk > 0)) break;  // (their dO rows are zero: nothing for dV)
          if (exact) bwd_kv_tile<T, DH, 0, true>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
          else bwd_kv_tile<T, DH, 0, false>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
        } else if (sparse && (q0 > 0 || blk > 0)) {
          if (exact) bwd_kv_tile<T, DH, 1, true, true>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
          else bwd_kv_tile<T, DH, 1, false, true>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
        } else {
          if (exact) bwd_kv_tile<T, DH, 1, true>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
          else bwd_kv_tile<T, DH, 1, false>(sQ, sdO, blk, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
        }
      }
    }
    if (pass == 0) {
      const float delta = delta_from_dv<T, DH>(acc, vf, lane);
      if (lane < 32 && k_lane < S) a.delta[bh * S + k_lane] = delta;
      neg_delta = -delta;
    }
    owner_store<T, DH>(drow ? drow + (pass == 0 ? a.v_off : a.k_off) : nullptr, acc, lane);
  }
}

// ------------------------------------------------------------------------------------ bwd_q
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(AttnArgs a) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  __shared__ __attribute__((aligned(16))) T sK[ATT_STAGE * LdsLd<DH>::V];
  __shared__ __attribute__((aligned(16))) T sV[ATT_STAGE * LdsLd<DH>::V];
  __shared__ __attribute__((aligned(16))) float sSk[ATT_STAGE], sCk[ATT_STAGE], sNd[ATT_STAGE], sMadd[ATT_STAGE], sMax[ATT_STAGE], sLogl[ATT_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tile; int64_t bh;
  attn_wg_coords(a.B, a.H, tile, bh);
  const int64_t b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;  // (B * H <= 65535: a 32-bit division, not the ~200-instruction 64-bit one, at the head of the kernel)
  const int64_t S = a.S;
  const int64_t plane = a.B * a.H * S;
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  const T* Kg = base + a.k_off;
  const T* Qg = base + a.q_off;
  const T* Vg = base + a.v_off;
  const T* dOg = reinterpret_cast<const T*>(a.dout) + b * S * a.ld_dout + hd * DH;
  const int64_t q_wave0 = (int64_t)tile * ATT_WG_ROWS + wave * 32;
  const int64_t q_lane = q_wave0 + (lane & 31);
  const float log2_scale = __log2f(a.scale);
  StageRegs<T, DH> rk, rv;
  KeyRegs kr;
  stage_load<T, DH>(rk, Kg, a.ld_qkv, 0, S, tid);
  stage_load<T, DH>(rv, Vg, a.ld_qkv, 0, S, tid);
  key_load(kr, a.keymask, a.lse, a.delta, plane, b, bh, S, tid, tid < ATT_STAGE);

  typename Act<T>::vec8 qf[KS], dof[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = glb_row_frag<T>(Qg, a.ld_qkv, q_lane, S, s, lane);
    dof[s] = glb_row_frag<T>(dOg, a.ld_dout, q_lane, S, s, lane);
  }
  f32x16 acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) acc[d] = zero16<DH>();

  for (int64_t k0 = 0; k0 < S; k0 += ATT_STAGE) {
    __syncthreads();
    stage_store<T, DH>(sK, rk, tid);
    stage_store<T, DH>(sV, rv, tid);
    int padded = 0;
    if (tid < ATT_STAGE) {
      float sk2, ck2;
      key_consts(kr.in, kr.valid, kr.rmax, kr.logl, a.scale, sk2, ck2);
      sSk[tid] = sk2; sCk[tid] = ck2 + log2_scale;  // the exponential is P * scale (bwd_q_tile)
      sMadd[tid] = kr.valid ? 0.f : MASK_VALUE; sMax[tid] = kr.rmax; sLogl[tid] = kr.in ? kr.logl : INFINITY;
      sNd[tid] = -kr.delta;
      padded = kr.in && !kr.valid;
    }
    if (k0 + ATT_STAGE < S) {
      stage_load<T, DH>(rk, Kg, a.ld_qkv, k0 + ATT_STAGE, S, tid);
      stage_load<T, DH>(rv, Vg, a.ld_qkv, k0 + ATT_STAGE, S, tid);
      key_load(kr, a.keymask, a.lse, a.delta, plane, b, bh, S, k0 + ATT_STAGE + tid, tid < ATT_STAGE);
    }
    const bool exact = __syncthreads_or(padded);
#pragma unroll
    for (int blk = 0; blk < ATT_STAGE / 32; ++blk) {
      if (k0 + blk * 32 >= S) break;
      if (exact) bwd_q_tile<T, DH, true>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, sNd, blk, a.scale, qf, dof, acc, lane);
      else bwd_q_tile<T, DH, false>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, sNd, blk, a.scale, qf, dof, acc, lane);
    }
  }
  T* dst = reinterpret_cast<T*>(a.dqkv) + b * S * a.ld_dqkv + hd * DH + a.q_off;
  owner_store<T, DH>(q_lane < S ? dst + q_lane * a.ld_dqkv : nullptr, acc, lane);
}

// ---- dQ with the keys staged in CHUNKS (sequences too long for the resident backward kernel: configs[4]'s encoder, S 1024).
// The streaming attn_bwd_q_kernel re-stages 64 keys at a time for four waves and spends 860 cycles per tile visit — twice the
// resident kernels — on per-stage bookkeeping; here one workgroup owns a (batch, head), stages K | V in chunks of CR keys for all
// of its waves at once, fills the per-key constants once, and every wave carries the dQ accumulators of its (up to OBM) query
// blocks across the chunks. Same tile arithmetic (bwd_q_tile). 8 waves: 256 registers each hold four blocks' accumulators and fragments.
template <typename T, int DH, int OBM>
__global__ __launch_bounds__(512) void attn_bwd_q_chunk_kernel(AttnArgs a, int n_chunks) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32, LD = LdsLd<DH>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char att_smem[];
  const int64_t S = a.S;
  const int NB = (int)((S + 31) / 32), SP = NB * 32, CR = SP / n_chunks;
  T* sK = reinterpret_cast<T*>(att_smem);
  T* sV = sK + CR * LD;
  float* sSk = reinterpret_cast<float*>(sV + CR * LD);
  float* sCk = sSk + SP; float* sMadd = sCk + SP; float* sMax = sMadd + SP; float* sLogl = sMax + SP; float* sNd = sLogl + SP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, NW = nthr >> 6;
  const int64_t bh = res_wg_bh(a.B, a.H), b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;
  const int64_t plane = a.B * a.H * S;
  const float log2_scale = __log2f(a.scale);
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  const T* dOg = reinterpret_cast<const T*>(a.dout) + b * S * a.ld_dout + hd * DH;
  const bool sparse = a.q_limit > 0 && a.q_limit <= 32;    // dO is zero from row q_limit on (the top encoder layer)
  const int64_t do_rows = sparse ? a.q_limit : S;
  // the owned blocks' Q / dO fragments: requested first, they are not needed before the first chunk is staged
  typename Act<T>::vec8 qf[OBM][KS], dof[OBM][KS];
  f32x16 acc[OBM][DB];
  bool act[OBM];
#pragma unroll
  for (int i = 0; i < OBM; ++i) {
    const int ob = wave + i * NW;
    act[i] = ob < NB;
    const int64_t q_lane = act[i] ? (int64_t)ob * 32 + (lane & 31) : S;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[i][s] = glb_row_frag<T>(base + a.q_off, a.ld_qkv, q_lane, S, s, lane);
      dof[i][s] = glb_row_frag<T>(dOg, a.ld_dout, q_lane, do_rows, s, lane);
    }
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[i][d] = zero16<DH>();
  }
  // per-key constants of the whole sequence (attn_bwd_q_kernel computes them per stage)
  int padded = 0;
  for (int k = tid; k < SP; k += nthr) {
    const bool in = k < S;
    const bool vk = in && a.keymask[b * S + k];
    const float rmax = in ? a.lse[bh * S + k] : 0.f, logl = in ? a.lse[plane + bh * S + k] : 0.f;
    float sk2, ck2;
    key_consts(in, vk, rmax, logl, a.scale, sk2, ck2);
    sSk[k] = sk2; sCk[k] = ck2 + log2_scale;  // the exponential is P * scale (bwd_q_tile)
    sMadd[k] = vk ? 0.f : MASK_VALUE; sMax[k] = rmax; sLogl[k] = in ? logl : INFINITY;
    sNd[k] = in ? -a.delta[bh * S + k] : 0.f;
    padded |= (in && !vk);
  }
  const bool exact = __syncthreads_or(padded);
  const uint64_t pad_tiles = exact ? padded_tile_mask(sSk, sCk, NB, lane) : 0ull;
  const int tiles_c = CR / 32;
  for (int c = 0; c < n_chunks; ++c) {
    if (c > 0) __syncthreads();  // every wave is done with the previous chunk
    const int64_t k0 = (int64_t)c * CR;
    if (k0 >= S) break;  // (uniform)
    stage_pair<T, DH>(sK, base + a.k_off + k0 * a.ld_qkv, a.ld_qkv, S - k0, sV, base + a.v_off + k0 * a.ld_qkv, a.ld_qkv, S - k0, CR, tid, nthr);
    __syncthreads();
    const int nt = (NB - c * tiles_c) < tiles_c ? (NB - c * tiles_c) : tiles_c;
#pragma unroll
    for (int i = 0; i < OBM; ++i) {
      if (!act[i]) continue;
      const bool light = sparse && (wave + i * NW) > 0;  // this block's dO rows are zero
      if (light) {
        if (exact) {
          const uint64_t padc = (pad_tiles >> (c * tiles_c)) & tile_bits(nt);
          MST_FOR_TILES(kt, ~padc & tile_bits(nt)) bwd_q_tile<T, DH, false, true>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
          MST_FOR_TILES(kt, padc) bwd_q_tile<T, DH, true, true>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
        } else for (int kt = 0; kt < nt; ++kt) bwd_q_tile<T, DH, false, true>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
      } else if (exact) {
        const uint64_t padc = (pad_tiles >> (c * tiles_c)) & tile_bits(nt);
        MST_FOR_TILES(kt, ~padc & tile_bits(nt)) bwd_q_tile<T, DH, false>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
        MST_FOR_TILES(kt, padc) bwd_q_tile<T, DH, true>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
      } else {
        for (int kt = 0; kt < nt; ++kt) bwd_q_tile<T, DH, false>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, sNd + k0, kt, a.scale, qf[i], dof[i], acc[i], lane);
      }
    }
  }
  T* dst = reinterpret_cast<T*>(a.dqkv) + b * S * a.ld_dqkv + hd * DH + a.q_off;
#pragma unroll
  for (int i = 0; i < OBM; ++i) {
    const int64_t q_lane = (int64_t)(wave + i * NW) * 32 + (lane & 31);
    owner_store<T, DH>((act[i] && q_lane < S) ? dst + q_lane * a.ld_dqkv : nullptr, acc[i], lane);
  }
}

// ---- the W_proj INPUT GRADIENT of ONE (batch, head) inside the attention backward launch (head sizes 16 and 32). The dO tile the
// workgroup stages, dproj[b] (S x D) . Wt[hd dh .. hd dh + dh, :]^T, is one column tile of the GEMM that used to write `datt` (6.4 and
// 8.9 us as launches of their own at configs[1], and 12.6 MB written and read straight back): no sum crosses heads. Every wave forms
// the rows of ITS 32-row block — the rows nobody else needs before the tile is complete —, so the contraction loop has no workgroup
// barrier: a wave stages its own 32 x 64 slice of dproj through LDS with whole-line loads (8 lanes x 16 bytes per row) one slice
// ahead in registers, and only the head's weight panel [dh][D] (staged once, up front) is shared. The product is gemm_mainloop's:
// mfma16 with the weights as the A operand, 32-deep steps in ascending K, one rounding to the activation type — the bits of the
// GEMM launch. The slices borrow the LDS of the Q / dO tiles and the per-key arrays (free until phase A); the launch is given
// max(the kernel's own LDS, res_lds_bwd_proj) bytes, two workgroups per CU still fit (attn_bwd_proj_rule).
// The lone row (lone_row_shape): the last wave also forms the 16-row sub-tile that holds row S - 1.
// On return the dO tile (zeros in rows >= S) is in bufB and Q in bufA, as stage_pair leaves them; the caller's barrier completes them.
__device__ __forceinline__ void wave_lds_fence() {  // LDS traffic of ONE wave is in order: only the compiler has to be held
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <typename T, int DH>
__device__ __forceinline__ void dout_prologue(const AttnArgs& a, unsigned char* smem, T* bufA, T* bufB, const T* __restrict__ Qg, int64_t b,
                                              int64_t hd, int NB, bool lone) {
  constexpr int LD = LdsLd<DH>::V, TN = DH / 16, TMX = DH <= 16 ? 3 : 2, CPR = DH / 8;
  typedef typename Act<T>::vec8 vec8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, NW = nthr >> 6;
  const int64_t S = a.S;
  const int SP = NB * 32, D = (int)a.Dm, LDW = D + 8, nch = D / DOP_KC;
  T* const sX = reinterpret_cast<T*>(smem);  // [SP][72]: wave w owns rows 32 w .. 32 w + 31 (the last one the lone row's block too)
  T* const sW = sX + SP * DOP_LDS;           // [DH][D + 8]
  const T* xg = reinterpret_cast<const T*>(a.x) + b * S * a.ld_x;
  const T* wg = reinterpret_cast<const T*>(a.w) + hd * DH * a.ld_w;
  // this wave's slice pieces of 16 bytes: piece q = (row q / 8 of the block, chunk q % 8), four per lane. Rows beyond the sequence read
  // the last row (their results are zeroed below); every load is unconditional, as in qkv_prologue
  const int rb0 = wave * 32;
  const T* xsrc[4]; T* xdst[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = lane + 64 * i, r = rb0 + (q >> 3), ch = q & 7;
    xsrc[i] = xg + (int64_t)(r < S ? r : S - 1) * a.ld_x + ch * 8;
    xdst[i] = sX + r * DOP_LDS + ch * 8;
  }
  const bool extra = TMX == 3 && lone && wave == NW - 1;  // (wave-uniform) rows 32 NW .. 32 NW + 7: row S - 1 and seven copies of it
  const int re = 32 * NW + (lane >> 3);
  const T* const xsrc_e = xg + (int64_t)(re < S ? re : S - 1) * a.ld_x + (lane & 7) * 8;
  T* const xdst_e = sX + re * DOP_LDS + (lane & 7) * 8;
  u32x4 xr[4], xe = {0u, 0u, 0u, 0u};
  auto load_slice = [&](int kc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) xr[i] = *reinterpret_cast<const u32x4*>(xsrc[i] + kc * DOP_KC);
    if (extra) xe = *reinterpret_cast<const u32x4*>(xsrc_e + kc * DOP_KC);
  };
  auto store_slice = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(xdst[i]) = xr[i];
    if (extra) *reinterpret_cast<u32x4*>(xdst_e) = xe;
  };
  load_slice(0);
  // Q: requested now, stored after the contraction (two pieces per thread cover the SP x DH tile: NW >= NB - 1)
  u32x4 qr[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + i * nthr, row = c / CPR, ch = c % CPR;
    const bool ok = c < SP * CPR && row < S;
    const u32x4 v = *reinterpret_cast<const u32x4*>(Qg + (int64_t)(ok ? row : 0) * a.ld_qkv + (ok ? ch : 0) * 8);
    qr[i] = ok ? v : u32x4{0u, 0u, 0u, 0u};
  }
  {  // the head's weight panel
    const int wpr = D / 8;
    for (int p = tid; p < DH * wpr; p += nthr) {
      const int r = p / wpr, ch = p - r * wpr;
      *reinterpret_cast<u32x4*>(sW + r * LDW + ch * 8) = *reinterpret_cast<const u32x4*>(wg + (int64_t)r * a.ld_w + ch * 8);
    }
  }
  store_slice();
  __syncthreads();
  f32x4 acc[TN][TMX];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TMX; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fq = lane >> 4;
  const T* const fx = sX + (rb0 + frow) * DOP_LDS + 8 * fq;
  const T* const fxe = sX + (32 * NW + frow) * DOP_LDS + 8 * fq;
  const T* const fw = sW + frow * LDW + 8 * fq;
  for (int kc = 0; kc < nch; ++kc) {
    if (kc + 1 < nch) load_slice(kc + 1);
#pragma unroll
    for (int ks = 0; ks < DOP_KC / 32; ++ks) {
      vec8 xf[2], wf[TN];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(fx + i * 16 * DOP_LDS + 32 * ks));
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[j] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(fw + j * 16 * LDW + kc * DOP_KC + 32 * ks));
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = Act<T>::mfma16(wf[j], xf[i], acc[j][i]);
      if constexpr (TMX == 3) {
        if (extra) {
          const vec8 xf2 = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(fxe + 32 * ks));
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[j][2] = Act<T>::mfma16(wf[j], xf2, acc[j][2]);
        }
      }
    }
    wave_lds_fence();  // this wave has read its slice
    if (kc + 1 < nch) store_slice();
    wave_lds_fence();
  }
  __syncthreads();  // every wave is done with the slices and the panel: the tiles may be written over them
  // one rounding (gemm_epilogue's, alpha 1, no bias): lane (frow, fq) holds columns 16 j + 4 fq .. + 3 of row frow of each sub-tile
#pragma unroll
  for (int i = 0; i < TMX; ++i) {
    if (i == 2 && !(lone && wave == NW - 1)) break;
    const int row = i == 2 ? 32 * NW + frow : rb0 + 16 * i + frow;
    const bool in = row < S;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      u32x2 o = {0u, 0u};
      if (in) {
        o[0] = (uint32_t)f32_to_bits<T>(acc[j][i][0]) | ((uint32_t)f32_to_bits<T>(acc[j][i][1]) << 16);
        o[1] = (uint32_t)f32_to_bits<T>(acc[j][i][2]) | ((uint32_t)f32_to_bits<T>(acc[j][i][3]) << 16);
      }
      *reinterpret_cast<u32x2*>(bufB + row * LD + 16 * j + 4 * fq) = o;
      if (i == 2) *reinterpret_cast<u32x2*>(bufB + (row + 16) * LD + 16 * j + 4 * fq) = u32x2{0u, 0u};  // (the block's other sixteen rows)
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + i * nthr, row = c / CPR, ch = c % CPR;
    if (c < SP * CPR) *reinterpret_cast<u32x4*>(bufA + row * LD + ch * 8) = qr[i];
  }
}

// PROJ: dO is formed in the launch (dout_prologue) instead of read: a.x / a.ld_x = dproj, a.w / a.ld_w = the transposed W_proj shadow,
// a.Dm = D, a.out / a.ld_out = where to store the dO tile as well (may be null); a.dout is not looked at. Dense, head sizes 16 and 32,
// one wave per owner block (attn_bwd_proj_rule). A separate instantiation: the other kernels keep their registers and instructions.
template <typename T, int DH, bool SPARSE, bool PROJ = false>
__global__ __launch_bounds__(RES_MAX_WAVES<DH> * 64) __attribute__((amdgpu_waves_per_eu(DH == 16 ? ATT16_WAVES : (DH == 64 ? 2 : 4)))) void attn_bwd_res_kernel(AttnArgs a) {
  static_assert(!PROJ || (!SPARSE && DH <= 32), "the projection prologue: dense, head sizes 16 and 32");
  constexpr int KS = DH / 16, DB = (DH + 31) / 32, LD = LdsLd<DH>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char att_smem[];
  const int64_t S = a.S;
  const int NB = (int)((S + 31) / 32), SP = NB * 32;
  T* bufA = reinterpret_cast<T*>(att_smem);  // phase A: Q   phase B: K
  T* bufB = bufA + SP * LD;                  // phase A: dO  phase B: V
  float* sSk = reinterpret_cast<float*>(bufB + SP * LD);
  float* sCk = sSk + SP; float* sMadd = sCk + SP; float* sMax = sMadd + SP; float* sLogl = sMax + SP; float* sNd = sLogl + SP;
  float* sRed = sNd + SP;  // [LONE_RED]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, NW = nthr >> 6;
  const int64_t bh = res_wg_bh(a.B, a.H), b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;  // (32-bit division: B * H <= 65535)
  const int64_t plane = a.B * a.H * S;
  const bool lone = !SPARSE && lone_row_shape(S, DH);  // the last row is handled apart (see lone_row_shape)
  const int NBo = lone ? NB - 1 : NB;                    // owner blocks swept with MFMA tiles
  const float log2_scale = __log2f(a.scale);
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  const T* Kg = base + a.k_off;
  const T* Qg = base + a.q_off;
  const T* Vg = base + a.v_off;
  const T* dOg = reinterpret_cast<const T*>(a.dout) + b * S * a.ld_dout + hd * DH;
  T* dbase = reinterpret_cast<T*>(a.dqkv) + b * S * a.ld_dqkv + hd * DH;
  // Sparse mode (0 < q_limit <= 32: dO is zero from row q_limit on — the top encoder layer, whose output is read at
  // position 0 only): dP vanishes outside query block 0, so dV and delta need that block alone and every other
  // tile of dK / dQ is the LIGHT form. Same arithmetic as the dense path on the zero rows, about 45 % of its work.
  constexpr bool sparse = SPARSE;  // host: 0 < q_limit <= 32 (a separate instantiation keeps the dense kernel's registers)
  const int64_t do_rows = sparse ? a.q_limit : S;  // rows of dO that are read; the staged tile is zero beyond them
  // the first owned key block's K / V fragments are requested before the staging loads: one exposed round trip, not two
  typename Act<T>::vec8 kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = glb_row_frag<T>(Kg, a.ld_qkv, wave * 32 + (lane & 31), S, s, lane);
    vf[s] = glb_row_frag<T>(Vg, a.ld_qkv, wave * 32 + (lane & 31), S, s, lane);
  }
  ATT_STAMP(0);
  if constexpr (PROJ) dout_prologue<T, DH>(a, att_smem, bufA, bufB, Qg, b, hd, NB, lone);
  else stage_pair<T, DH>(bufA, Qg, a.ld_qkv, S, bufB, dOg, a.ld_dout, do_rows, SP, tid, nthr);
  __syncthreads();
  if constexpr (PROJ) {
    if (a.out) {  // the dO tile as the GEMM launch stored it (the engine passes null: nothing else reads it)
      T* const og = reinterpret_cast<T*>(a.out) + b * S * a.ld_out + hd * DH;
      for (int c = tid; c < (int)S * (DH / 8); c += nthr) {
        const int row = c / (DH / 8), ch = c % (DH / 8);
        *reinterpret_cast<u32x4*>(og + (int64_t)row * a.ld_out + ch * 8) = *reinterpret_cast<const u32x4*>(bufB + row * LD + ch * 8);
      }
    }
  }
  ATT_STAMP(1);
  const int nq0 = sparse ? 1 : NBo;  // (whole) query tiles that contribute to pass 0

  // ---- phase A: dV, delta, dK for the owned keys (attn_bwd_kv_kernel's two passes over the query tiles)
  int padded = 0;
  for (int ob = wave; ob < NBo; ob += NW) {
    const int64_t k_lane = ob * 32 + (lane & 31);
    if (ob != wave) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        kf[s] = glb_row_frag<T>(Kg, a.ld_qkv, k_lane, S, s, lane);
        vf[s] = glb_row_frag<T>(Vg, a.ld_qkv, k_lane, S, s, lane);
      }
    }
    const bool in = k_lane < S;
    const bool vk = in && a.keymask[b * S + k_lane];
    const float rmax = in ? a.lse[bh * S + k_lane] : 0.f;
    const float logl = in ? a.lse[plane + bh * S + k_lane] : INFINITY;
    const float madd = vk ? 0.f : MASK_VALUE;
    float sk2, ck2;
    key_consts(in, vk, rmax, in ? logl : 0.f, a.scale, sk2, ck2);
    const float ck2s = ck2 + log2_scale;  // pass 1 and phase B: the exponential is P * scale
    const bool exact_w = __any(in && !vk);  // wave-uniform: one of this block's 32 keys is padded
    padded |= (in && !vk);
    f32x16 acc[DB];
    float neg_delta = 0.f;
    T* const drow = in ? dbase + k_lane * a.ld_dqkv : nullptr;
    // four straight-line tile loops (pass x exact) instead of branches inside one: the merged form shuffled the
    // probability tile through 15 v_mov per tile to reconcile the two passes' register assignments
    // ---- pass 0: dV, then delta = V . dV
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = zero16<DH>();
    if (exact_w) for (int qt = 0; qt < nq0; ++qt) bwd_kv_tile<T, DH, 0, true>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
    else for (int qt = 0; qt < nq0; ++qt) bwd_kv_tile<T, DH, 0, false>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
    if constexpr (DH <= 16 && !SPARSE) {
      if (lone) {  // the ninth query tile holds the lone query only
        if (exact_w) bwd_kv_tile<T, DH, 0, true, false, true>(bufA, bufB, NB - 1, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
        else bwd_kv_tile<T, DH, 0, false, false, true>(bufA, bufB, NB - 1, a.scale, kf, vf, sk2, ck2, madd, rmax, logl, neg_delta, acc, lane);
      }
    }
    {
      const float delta = delta_from_dv<T, DH>(acc, vf, lane);
      if (lane < 32 && in) a.delta[bh * S + k_lane] = delta;
      neg_delta = -delta;
    }
    owner_store<T, DH>(drow ? drow + a.v_off : nullptr, acc, lane);
    ATT_STAMP(2);
    // ---- pass 1: dK
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = zero16<DH>();
    if (exact_w) for (int qt = 0; qt < nq0; ++qt) bwd_kv_tile<T, DH, 1, true>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
    else for (int qt = 0; qt < nq0; ++qt) bwd_kv_tile<T, DH, 1, false>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
    if (sparse) {
      if (exact_w) for (int qt = nq0; qt < NB; ++qt) bwd_kv_tile<T, DH, 1, true, true>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
      else for (int qt = nq0; qt < NB; ++qt) bwd_kv_tile<T, DH, 1, false, true>(bufA, bufB, qt, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
    }
    if constexpr (DH <= 16 && !SPARSE) {
      if (lone) {
        if (exact_w) bwd_kv_tile<T, DH, 1, true, false, true>(bufA, bufB, NB - 1, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
        else bwd_kv_tile<T, DH, 1, false, false, true>(bufA, bufB, NB - 1, a.scale, kf, vf, sk2, ck2s, madd, rmax, logl, neg_delta, acc, lane);
      }
    }
    owner_store<T, DH>(drow ? drow + a.k_off : nullptr, acc, lane);
    if (lane < 32) {
      sSk[k_lane] = sk2; sCk[k_lane] = ck2s; sMadd[k_lane] = madd; sMax[k_lane] = rmax; sLogl[k_lane] = logl;
      sNd[k_lane] = in ? neg_delta : 0.f;
    }
  }
  if constexpr (DH <= 16 && !SPARSE) {
    if (lone) {  // the lone key: queries on the lanes; dV, delta = V . dV, then dK (two sweeps, as the MFMA form)
      const int64_t e = S - 1;
      float ke[DH], ve[DH], acc[DH];
#pragma unroll
      for (int f = 0; f < DH; ++f) { ke[f] = to_f32(Kg[e * a.ld_qkv + f]); ve[f] = to_f32(Vg[e * a.ld_qkv + f]); }
      const bool vk = a.keymask[b * S + e];
      const float rmax = a.lse[bh * S + e], logl = a.lse[plane + bh * S + e], madd = vk ? 0.f : MASK_VALUE;
      float sk2, ck2;
      key_consts(true, vk, rmax, logl, a.scale, sk2, ck2);
      const float ck2s = ck2 + log2_scale;
      padded |= !vk;
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = 0.f;
      for (int q = tid; q < S; q += nthr) {
        const float x = lds_row_dot<T, DH>(bufA + q * LD, ke);
        const float pr = vk ? fast_exp2(fmaf(x, sk2, ck2)) : exact_prob(x, a.scale, madd, rmax, logl);
        lds_row_axpy<T, DH>(pr, bufB + q * LD, acc);
      }
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = wave_sum(acc[f]);
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < DH; ++f) sRed[wave * DH + f] = acc[f];
      }
      __syncthreads();
      if (tid < DH) {
        float dv = 0.f;
        for (int w = 0; w < NW; ++w) dv += sRed[w * DH + tid];
        sRed[LONE_RED / 2 + tid] = dv;
        dbase[e * a.ld_dqkv + a.v_off + tid] = (T)dv;
      }
      __syncthreads();
      float delta = 0.f;
#pragma unroll
      for (int f = 0; f < DH; ++f) delta = fmaf(ve[f], sRed[LONE_RED / 2 + f], delta);
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = 0.f;
      for (int q = tid; q < S; q += nthr) {
        const float x = lds_row_dot<T, DH>(bufA + q * LD, ke);
        const float ps = vk ? fast_exp2(fmaf(x, sk2, ck2s)) : exact_prob(x, a.scale, madd, rmax, logl) * a.scale;
        const float dl = ps * (lds_row_dot<T, DH>(bufB + q * LD, ve) - delta);
        lds_row_axpy<T, DH>(dl, bufA + q * LD, acc);
      }
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = wave_sum(acc[f]);
      __syncthreads();  // (the dV partials have been read)
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < DH; ++f) sRed[wave * DH + f] = acc[f];
      }
      __syncthreads();
      if (tid < DH) {
        float dk = 0.f;
        for (int w = 0; w < NW; ++w) dk += sRed[w * DH + tid];
        dbase[e * a.ld_dqkv + a.k_off + tid] = (T)dk;
      }
      if (tid == 0) {
        a.delta[bh * S + e] = delta;
        sSk[e] = sk2; sCk[e] = ck2s; sMadd[e] = madd; sMax[e] = rmax; sLogl[e] = logl; sNd[e] = -delta;
        for (int k = (int)S; k < SP; ++k) {
          float s0, c0;
          key_consts(false, false, 0.f, 0.f, a.scale, s0, c0);
          sSk[k] = s0; sCk[k] = c0 + log2_scale; sMadd[k] = MASK_VALUE; sMax[k] = 0.f; sLogl[k] = INFINITY; sNd[k] = 0.f;
        }
      }
    }
  }
  ATT_STAMP(3);
  // phase B's first Q / dO fragments: requested before the barrier and the K / V staging
  typename Act<T>::vec8 qf[KS], dof[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = glb_row_frag<T>(Qg, a.ld_qkv, wave * 32 + (lane & 31), S, s, lane);
    if constexpr (PROJ) dof[s] = lds_row_frag<T, DH>(bufB, wave * 32, s, lane);  // (dO is in no other place; same elements, zero beyond S)
    else dof[s] = glb_row_frag<T>(dOg, a.ld_dout, wave * 32 + (lane & 31), do_rows, s, lane);
  }
  if constexpr (PROJ && DH <= 16) {  // the lone query's dO row, kept for its dQ sweep behind phase B (a corner of sRed no reduction uses)
    if (lone && tid < DH) sRed[LONE_RED / 2 + DH + tid] = to_f32(bufB[(S - 1) * LD + tid]);
  }
  __syncthreads();  // every wave is done with the staged Q and dO
  stage_pair<T, DH>(bufA, Kg, a.ld_qkv, S, bufB, Vg, a.ld_qkv, S, SP, tid, nthr);
  const bool exact = __syncthreads_or(padded);
  const uint64_t pad_tiles = exact ? padded_tile_mask(sSk, sCk, NB, lane) : 0ull;  // (the barrier above: every key's constants are in LDS)
  ATT_STAMP(4);

  // ---- phase B: dQ for the owned queries (attn_bwd_q_kernel's tiles)
  for (int ob = wave; ob < NBo; ob += NW) {
    const int64_t q_lane = ob * 32 + (lane & 31);
    if (ob != wave) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        qf[s] = glb_row_frag<T>(Qg, a.ld_qkv, q_lane, S, s, lane);
        if constexpr (!PROJ) dof[s] = glb_row_frag<T>(dOg, a.ld_dout, q_lane, do_rows, s, lane);  // (PROJ: one block per wave, never here)
      }
    }
    f32x16 acc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = zero16<DH>();
    if (sparse && ob > 0) {  // this block's dO rows are zero
      if (exact) {
        MST_FOR_TILES(kt, ~pad_tiles & tile_bits(NB)) bwd_q_tile<T, DH, false, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
        MST_FOR_TILES(kt, pad_tiles & tile_bits(NB)) bwd_q_tile<T, DH, true, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
      } else for (int kt = 0; kt < NB; ++kt) bwd_q_tile<T, DH, false, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
    } else if (exact) {
      MST_FOR_TILES(kt, ~pad_tiles & tile_bits(NBo)) bwd_q_tile<T, DH, false>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
      MST_FOR_TILES(kt, pad_tiles & tile_bits(NBo)) bwd_q_tile<T, DH, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
    } else {
      for (int kt = 0; kt < NBo; ++kt) bwd_q_tile<T, DH, false>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, kt, a.scale, qf, dof, acc, lane);
    }
    if constexpr (DH <= 16 && !SPARSE) {
      if (lone) {  // the ninth key tile holds the lone key only
        if (exact) bwd_q_tile<T, DH, true, false, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, NB - 1, a.scale, qf, dof, acc, lane);
        else bwd_q_tile<T, DH, false, false, true>(bufA, bufB, sSk, sCk, sMadd, sMax, sLogl, sNd, NB - 1, a.scale, qf, dof, acc, lane);
      }
    }
    owner_store<T, DH>(q_lane < S ? dbase + a.q_off + q_lane * a.ld_dqkv : nullptr, acc, lane);
  }
  ATT_STAMP(5);
  if constexpr (DH <= 16 && !SPARSE) {
    if (lone) {  // dQ of the lone query: keys on the lanes
      const int64_t e = S - 1;
      float qe[DH], doe[DH], acc[DH];
#pragma unroll
      for (int f = 0; f < DH; ++f) {
        qe[f] = to_f32(Qg[e * a.ld_qkv + f]); acc[f] = 0.f;
        if constexpr (PROJ) doe[f] = sRed[LONE_RED / 2 + DH + f];
        else doe[f] = to_f32(dOg[e * a.ld_dout + f]);
      }
      for (int k = tid; k < S; k += nthr) {
        const float x = lds_row_dot<T, DH>(bufA + k * LD, qe);
        const float ps = exact ? exact_prob(x, a.scale, sMadd[k], sMax[k], sLogl[k]) * a.scale : fast_exp2(fmaf(x, sSk[k], sCk[k]));
        const float dl = ps * (lds_row_dot<T, DH>(bufB + k * LD, doe) + sNd[k]);
        lds_row_axpy<T, DH>(dl, bufA + k * LD, acc);
      }
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = wave_sum(acc[f]);
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < DH; ++f) sRed[wave * DH + f] = acc[f];
      }
      __syncthreads();
      if (tid < DH) {
        float dq = 0.f;
        for (int w = 0; w < NW; ++w) dq += sRed[w * DH + tid];
        dbase[e * a.ld_dqkv + a.q_off + tid] = (T)dq;
      }
    }
  }
}

// ---- launch code: the form is attention.hip's (attn_bwd_form, attn_bwd_proj_rule)
template <typename T, int DH, bool SPARSE, bool PROJ>
static int launch_bwd_res(const AttnArgs& a, int waves, size_t lds, hipStream_t s, const char* what) {
  static size_t granted = 64 * 1024;
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&attn_bwd_res_kernel<T, DH, SPARSE, PROJ>), lds, &granted, what)) return rc;
  hipLaunchKernelGGL((attn_bwd_res_kernel<T, DH, SPARSE, PROJ>), dim3((unsigned)(a.B * a.H)), dim3(waves * 64), lds, s, a);
  MST_CHECK_LAUNCH(what);
  return MST_OK;
}
template <typename T, int DH>
static int launch_bwd(const AttnArgs& a, const AttnBwdForm& f, hipStream_t s) {
  if (f.proj) {  // (mst_attn_proj_bwd alone sets it)
    if constexpr (DH <= 32) return launch_bwd_res<T, DH, false, true>(a, f.waves, f.lds_proj, s, "attn_bwd_res_kernel (fused projection)");
    set_error("attention backward: the fused projection has no kernel at head size %d", DH);
    return MST_ERR_INVALID;
  }
  if (f.path == ATT_BWD_RES)
    return f.sparse ? launch_bwd_res<T, DH, true, false>(a, f.waves, f.lds, s, "attn_bwd_res_kernel")
                    : launch_bwd_res<T, DH, false, false>(a, f.waves, f.lds, s, "attn_bwd_res_kernel");
  const dim3 grid((unsigned)cdiv(a.S, ATT_WG_ROWS), (unsigned)(a.B * a.H));
  if (f.sparse) hipLaunchKernelGGL((attn_bwd_kv_kernel<T, DH, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_bwd_kv_kernel<T, DH, false>), grid, dim3(256), 0, s, a);
  MST_CHECK_LAUNCH("attn_bwd_kv_kernel");
  if (f.path == ATT_BWD_STREAM_CHUNKQ) {
    if constexpr (DH == 32) {
      static size_t granted = 64 * 1024;
      if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&attn_bwd_q_chunk_kernel<T, DH, ATT_DQ_OBM>), f.lds, &granted, "attn_bwd_q_chunk_kernel")) return rc;
      hipLaunchKernelGGL((attn_bwd_q_chunk_kernel<T, DH, ATT_DQ_OBM>), dim3((unsigned)(a.B * a.H)), dim3(f.dq_waves * 64), f.lds, s, a, f.dq_chunks);
      MST_CHECK_LAUNCH("attn_bwd_q_chunk_kernel");
      return MST_OK;
    }
    set_error("attention backward: chunked dQ has no kernel at head size %d", DH);
    return MST_ERR_INVALID;
  }
  hipLaunchKernelGGL((attn_bwd_q_kernel<T, DH>), grid, dim3(256), 0, s, a);
  MST_CHECK_LAUNCH("attn_bwd_q_kernel");
  return MST_OK;
}

int attn_launch_bwd(int dtype, int64_t dh, const AttnArgs& a, const AttnBwdForm& f, hipStream_t s) {
  return dispatch_attn(dtype, dh, [&](auto tag, auto dh_c) -> int { return launch_bwd<decltype(tag), decltype(dh_c)::value>(a, f, s); });
}

}  // namespace mst

#ifdef MST_ATT_STAMPS
extern "C" int mst_debug_att_stamps(uint64_t* host_out) {  // diagnostic builds only: 1024 x 8 realtime stamps
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mst::g_att_stamps), sizeof(uint64_t) * 8192) == hipSuccess ? 0 : -1;
}
#endif

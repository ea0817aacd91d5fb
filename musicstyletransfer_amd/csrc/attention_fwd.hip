// attention_fwd.hip — the forward launches of key-row attention (attention.hip states the operation and chooses the form): streaming,
// attn_fwd_stats_kernel + attn_fwd_out_kernel for any sequence length; resident, attn_fwd_res_kernel with both as phases of one launch
// (attention.hpp: "resident kernels") in its plain, restaged, chunked and fused-projection (qkv_prologue) forms.
// The kernels of one direction stay in one unit: they share the instantiations of attention.hpp's tile functions, and the compiler
// forms a kernel's code differently (more scratch backward) when the other users of those are not beside it.
#include "attention_forms.hpp"

namespace mst {

// ------------------------------------------------------------------------------------ fwd_stats
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_fwd_stats_kernel(AttnArgs a) {
  constexpr int KS = DH / 16;
  __shared__ __attribute__((aligned(16))) T sQ[ATT_STAGE * LdsLd<DH>::V];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tile; int64_t bh;
  attn_wg_coords(a.B, a.H, tile, bh);
  const int64_t b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;  // (B * H <= 65535: a 32-bit division, not the ~200-instruction 64-bit one, at the head of the kernel)
  const int64_t S = a.S;
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  const T* Kg = base + a.k_off;
  const T* Qg = base + a.q_off;
  const int64_t k_lane = (int64_t)tile * ATT_WG_ROWS + wave * 32 + (lane & 31);
  StageRegs<T, DH> rq;
  stage_load<T, DH>(rq, Qg, a.ld_qkv, 0, S, tid);

  typename Act<T>::vec8 kf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) kf[s] = glb_row_frag<T>(Kg, a.ld_qkv, k_lane, S, s, lane);
  const bool key_ok = k_lane < S && a.keymask[b * S + k_lane];
  const float madd = key_ok ? 0.f : MASK_VALUE;
  const bool exact_w = __any(!key_ok);  // a padded (or out-of-range) key on this wave: reference operation order

  float m = NEG_BIG, l = 0.f;
  for (int64_t q0 = 0; q0 < S; q0 += ATT_STAGE) {
    __syncthreads();
    stage_store<T, DH>(sQ, rq, tid);
    if (q0 + ATT_STAGE < S) stage_load<T, DH>(rq, Qg, a.ld_qkv, q0 + ATT_STAGE, S, tid);
    __syncthreads();
    const int64_t left = S - q0;
    stats_sweep<T, DH>(sQ, (int)((left < ATT_STAGE ? left : ATT_STAGE) + 31) / 32, q0, S, a.scale, madd, exact_w, kf, m, l, lane);
  }
  // the two lane halves hold disjoint query subsets of the same key
  const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64);
  const float M = fmaxf(m, m2);
  const float L = l * __expf(m - M) + l2 * __expf(m2 - M);
  // Stored as TWO planes (row max, log of the row sum): for a padded key row the max is -1e9 and a
  // single fp32 logsumexp would round log(S) away, turning the uniform 1/S row into ones.
  if (lane < 32 && k_lane < S) {
    a.lse[bh * S + k_lane] = M;
    a.lse[a.B * a.H * S + bh * S + k_lane] = __logf(L);
  }
}

// ------------------------------------------------------------------------------------ fwd_out
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_fwd_out_kernel(AttnArgs a) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  __shared__ __attribute__((aligned(16))) T sK[ATT_STAGE * LdsLd<DH>::V];
  __shared__ __attribute__((aligned(16))) T sV[ATT_STAGE * LdsLd<DH>::V];
  __shared__ __attribute__((aligned(16))) float sSk[ATT_STAGE], sCk[ATT_STAGE], sMadd[ATT_STAGE], sMax[ATT_STAGE], sLogl[ATT_STAGE];
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
  const int64_t q_wave0 = (int64_t)tile * ATT_WG_ROWS + wave * 32;
  const int64_t q_lane = q_wave0 + (lane & 31);
  StageRegs<T, DH> rk, rv;
  KeyRegs kr;
  stage_load<T, DH>(rk, Kg, a.ld_qkv, 0, S, tid);
  stage_load<T, DH>(rv, Vg, a.ld_qkv, 0, S, tid);
  key_load(kr, a.keymask, a.lse, nullptr, plane, b, bh, S, tid, tid < ATT_STAGE);

  typename Act<T>::vec8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = glb_row_frag<T>(Qg, a.ld_qkv, q_lane, S, s, lane);

  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o[d] = zero16<DH>();
  const bool wave_active = q_wave0 < a.q_limit;  // inactive waves still stage tiles and meet the barriers

  for (int64_t k0 = 0; k0 < S; k0 += ATT_STAGE) {
    __syncthreads();
    stage_store<T, DH>(sK, rk, tid);
    stage_store<T, DH>(sV, rv, tid);
    int padded = 0;
    if (tid < ATT_STAGE) {
      key_consts(kr.in, kr.valid, kr.rmax, kr.logl, a.scale, sSk[tid], sCk[tid]);
      sMadd[tid] = kr.valid ? 0.f : MASK_VALUE; sMax[tid] = kr.rmax; sLogl[tid] = kr.in ? kr.logl : INFINITY;
      padded = kr.in && !kr.valid;
    }
    if (k0 + ATT_STAGE < S) {
      stage_load<T, DH>(rk, Kg, a.ld_qkv, k0 + ATT_STAGE, S, tid);
      stage_load<T, DH>(rv, Vg, a.ld_qkv, k0 + ATT_STAGE, S, tid);
      key_load(kr, a.keymask, a.lse, nullptr, plane, b, bh, S, k0 + ATT_STAGE + tid, tid < ATT_STAGE);
    }
    const bool exact = __syncthreads_or(padded);  // wave-uniform: does this stage hold a padded key?
    if (!wave_active) continue;
#pragma unroll
    for (int blk = 0; blk < ATT_STAGE / 32; ++blk) {
      if (k0 + blk * 32 >= S) break;
      if (exact) fwd_out_tile<T, DH, true>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, blk, a.scale, qf, o, lane);
      else fwd_out_tile<T, DH, false>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, blk, a.scale, qf, o, lane);
    }
  }
  T* og = reinterpret_cast<T*>(a.out) + b * S * a.ld_out + hd * DH;
  owner_store<T, DH>((q_lane < S && q_lane < a.q_limit) ? og + q_lane * a.ld_out : nullptr, o, lane);
}

// ---- the K | Q | V projection of ONE (batch, head) inside the attention launch (head size 32). The Dense layers' GEMM
// (transformer.py:88-93: three Dense(D -> D) on the same input, run as one [3 D, D] product) has exactly this workgroup's
// operands as one of its tiles: rows = the sample's S positions, columns = the head's 32 columns of K, of Q and of V. As a
// launch of its own it cost 17.6 us and wrote 25 MB that the attention launch read straight back; here every wave forms the
// three 32 x 32 tiles of its 32 rows (x fragments straight from global, the head's 96 weight rows staged through LDS in
// 32-deep slices shared by the waves), adds the bias, rounds once to the activation type and leaves the SAME bits in the
// staged LDS tiles and in `qkv` (the backward pass recomputes the probabilities from what is stored).
// Accumulators are [feature, row-on-lane] (weights = A operand, x = B operand): owner_store's layout.
constexpr int QKV_LDS = QKV_KC + 8;                // row stride (elements) of the staged slices: 144-byte rows, conflict-free fragments
constexpr int QKV_WROWS = 3 * 32;                  // the head's weight rows: 32 of K, of Q and of V
// The slices are staged in the LDS the attention phases use afterwards for the Q / K / V tiles themselves (free until the
// projection's epilogue writes them): x slice [SP][72] over the Q and K tiles, weight slice [96][72] over the V tile. Both are
// fetched with whole-line loads (8 lanes x 16 bytes per row) through registers one slice ahead. A first form read every wave's x
// fragments straight from global — 32 rows x 32 bytes per instruction, i.e. 32 cache lines touched per load — and its 8-slice
// loop took 10.9 us per workgroup for 0.6 us of MFMAs per wave, bound by the CU's address / tag pipeline.
template <typename T>
__device__ __forceinline__ void qkv_prologue(const AttnArgs& a, T* sQ, T* sK, T* sV, int64_t b, int64_t hd, int NB) {
  constexpr int DH = 32, LD = LdsLd<DH>::V;
  static_assert(2 * LD >= QKV_LDS && QKV_WROWS * QKV_LDS <= 256 * LD, "the staged slices must fit the tiles they borrow");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
  const int64_t S = a.S;
  const int SP = NB * 32;
  T* const sX = sQ;   // [SP][72]: spans the Q and K tiles (contiguous)
  T* const sW = sV;   // [96][72]
  const T* xg = reinterpret_cast<const T*>(a.x) + b * S * a.ld_x;
  const T* wg = reinterpret_cast<const T*>(a.w);
  const int nch = (int)(a.Dm / QKV_KC);
  const int64_t sec_off[3] = {a.k_off, a.q_off, a.v_off};
  const bool active = wave < NB;
  const int64_t row = (int64_t)wave * 32 + (lane & 31);
  // accumulators start at the bias: feature (8 g + 4 h + e) of the section on the register axis (owner_store's layout)
  const int h4 = 4 * (lane >> 5);
  f32x16 acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + sec_off[c] + hd * DH + 8 * g + h4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][4 * g + e] = bv[e];
    }
  // staging pieces of 16 bytes: x piece p = (row p / 8, chunk p % 8) for p < SP * 8, four per thread at most (512 threads, SP <= 256);
  // weight piece p < 768 likewise, two per thread. Rows beyond the sequence read the last row (their products are dropped below);
  // every load is unconditional (a conditional load costs a vmcnt(0) drain at the join): surplus pieces re-read piece 0.
  constexpr int XP = 4, WP = 2;
  const T* xsrc[XP]; T* xdst[XP]; bool xok[XP];
  const T* wsrc[WP]; T* wdst[WP]; bool wok[WP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int p = tid + i * nthr;
    xok[i] = p < SP * 8;
    const int r = xok[i] ? p >> 3 : 0, ch = xok[i] ? p & 7 : 0;
    xsrc[i] = xg + (int64_t)(r < S ? r : S - 1) * a.ld_x + ch * 8;
    xdst[i] = sX + r * QKV_LDS + ch * 8;
  }
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int p = tid + i * nthr;
    wok[i] = p < QKV_WROWS * 8;
    const int r = wok[i] ? p >> 3 : 0, ch = wok[i] ? p & 7 : 0;
    wsrc[i] = wg + (sec_off[r >> 5] + hd * DH + (r & 31)) * a.ld_w + ch * 8;
    wdst[i] = sW + r * QKV_LDS + ch * 8;
  }
  u32x4 xr[XP], wr[WP];
  auto load_slice = [&](int kc) {
    const int k = (kc < nch ? kc : nch - 1) * QKV_KC;
#pragma unroll
    for (int i = 0; i < XP; ++i) xr[i] = *reinterpret_cast<const u32x4*>(xsrc[i] + k);
#pragma unroll
    for (int i = 0; i < WP; ++i) wr[i] = *reinterpret_cast<const u32x4*>(wsrc[i] + k);
  };
  auto store_slice = [&]() {
#pragma unroll
    for (int i = 0; i < XP; ++i)
      if (xok[i]) *reinterpret_cast<u32x4*>(xdst[i]) = xr[i];
#pragma unroll
    for (int i = 0; i < WP; ++i)
      if (wok[i]) *reinterpret_cast<u32x4*>(wdst[i]) = wr[i];
  };
  LOOP_STAMP(0);
  load_slice(0);
  store_slice();
  __syncthreads();
  LOOP_STAMP(1);
  const T* const fx = sX + (wave * 32 + (lane & 31)) * QKV_LDS + 8 * (lane >> 5);
  const T* const fw = sW + (lane & 31) * QKV_LDS + 8 * (lane >> 5);
  // (Measured and not kept: the next slice's loads interleaved between the MFMAs — the loop is bound by LDS fragment traffic,
  // 16 KB per wave and slice of which 12 are the weight fragments every wave re-reads, next to 44 KB per slice through the CU's
  // 64-byte-per-clock load path: 9.3 -> 9.5 us either way for 3.4 us of MFMAs per SIMD.)
  for (int kc = 0; kc < nch; ++kc) {
    load_slice(kc + 1);  // (past the end: the last slice again)
    LOOP_STAMP(2 + 5 * kc);
#pragma unroll
    for (int s4 = 0; s4 < QKV_KC / 16; ++s4) {
      const typename Act<T>::vec8 xv = __builtin_bit_cast(typename Act<T>::vec8, *reinterpret_cast<const u32x4*>(fx + 16 * s4));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(fw + c * 32 * QKV_LDS + 16 * s4);
        acc[c] = Act<T>::mfma32(__builtin_bit_cast(typename Act<T>::vec8, v), xv, acc[c]);
      }
    }
    LOOP_STAMP(3 + 5 * kc);
    __syncthreads();  // every wave has read this slice
    LOOP_STAMP(4 + 5 * kc);
    store_slice();
    LOOP_STAMP(5 + 5 * kc);
    __syncthreads();
    LOOP_STAMP(6 + 5 * kc);
  }
  ATT_STAMP(1);
  if (!active) return;
  // epilogue: one rounding, the same bits to the LDS tiles and to HBM. Nothing between the stores: a first form loaded each bias
  // vector right before its use, and since stores count in vmcnt every one of those loads waited for the previous store's
  // acknowledgement (12 dependent round trips, 6.9 us per workgroup; 3.4 with the bias in the accumulators from the start).
  const bool in = row < S;
  T* const tiles[3] = {sK, sQ, sV};
  T* qrow = reinterpret_cast<T*>(const_cast<void*>(a.qkv)) + (b * S + row) * a.ld_qkv + hd * DH;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 o = {0u, 0u};
      if (in) {
        o[0] = (uint32_t)f32_to_bits<T>(acc[c][4 * g]) | ((uint32_t)f32_to_bits<T>(acc[c][4 * g + 1]) << 16);
        o[1] = (uint32_t)f32_to_bits<T>(acc[c][4 * g + 2]) | ((uint32_t)f32_to_bits<T>(acc[c][4 * g + 3]) << 16);
        *reinterpret_cast<u32x2*>(qrow + sec_off[c] + 8 * g + h4) = o;
      }
      *reinterpret_cast<u32x2*>(tiles[c] + row * LD + 8 * g + h4) = o;  // (rows beyond the sequence: zeros, as stage_all leaves them)
    }
  }
}

// CHUNKED (a.restage = C >= 2, sequences whose K and V do not fit LDS even without Q — configs[4]'s encoder, S 1024 at head size 32):
// the output phase stages K and V in C chunks of SP / C keys over the Q tile and every wave carries the accumulators of its (at most
// two) owned query blocks across the chunks. A separate instantiation: the two accumulator sets are registers the other forms do not pay.
template <typename T, int DH, bool QKV = false, bool CHUNKED = false>
__global__ __launch_bounds__((FWD_MAX_WAVES<DH, QKV || CHUNKED> * 64)) __attribute__((amdgpu_waves_per_eu((DH == 16 ? ATT16_WAVES : (FWD_MAX_WAVES<DH, QKV || CHUNKED> == 8 ? 2 : 4))))) void attn_fwd_res_kernel(AttnArgs a) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32, LD = LdsLd<DH>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char att_smem[];
  const int64_t S = a.S;
  const int NB = (int)((S + 31) / 32), SP = NB * 32;
  const bool restage = !QKV && a.restage;  // two tiles: [Q, then K][V]; CHUNKED: one tile: [Q, then a chunk of K | the same chunk of V]
  const int CR = CHUNKED ? SP / a.restage : SP;  // keys staged at a time in the output phase
  T* sQ = reinterpret_cast<T*>(att_smem);
  T* sK = restage ? sQ : sQ + SP * LD;
  T* sV = sK + CR * LD;
  float* sSk = reinterpret_cast<float*>(CHUNKED ? sQ + SP * LD : sV + SP * LD);
  float* sCk = sSk + SP; float* sMadd = sCk + SP; float* sMax = sMadd + SP; float* sLogl = sMax + SP;
  float* sRed = sLogl + SP;  // [LONE_RED]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, NW = nthr >> 6;
  const int64_t bh = res_wg_bh(a.B, a.H), b = (int64_t)((uint32_t)bh / (uint32_t)a.H), hd = bh - b * a.H;  // (32-bit division: B * H <= 65535)
  const int64_t plane = a.B * a.H * S;
  const bool lone = lone_row_shape(S, DH) && a.q_limit >= S;  // the last row is handled apart (attention.hpp, "the LONE ROW")
  const int NBo = lone ? NB - 1 : NB;                            // owner blocks swept with MFMA tiles
  const T* base = reinterpret_cast<const T*>(a.qkv) + b * S * a.ld_qkv + hd * DH;
  ATT_STAMP(0);
  if constexpr (QKV) {
    static_assert(DH == 32, "the fused projection is built for head size 32");
    qkv_prologue<T>(a, sQ, sK, sV, b, hd, NB);
  } else {
    stage_all<T, DH>(sQ, base + a.q_off, a.ld_qkv, S, SP, tid, nthr);
    if (!restage) {
      stage_all<T, DH>(sK, base + a.k_off, a.ld_qkv, S, SP, tid, nthr);
      stage_all<T, DH>(sV, base + a.v_off, a.ld_qkv, S, SP, tid, nthr);
    }
  }
  __syncthreads();  // (a workgroup barrier waits for LDS traffic only: the projection's qkv stores drain under the statistics phase)
  ATT_STAMP(2);

  // ---- phase A: softmax statistics of every key row (the arithmetic of attn_fwd_stats_kernel)
  int padded = 0;
  for (int ob = wave; ob < NBo; ob += NW) {
    const int64_t k_lane = ob * 32 + (lane & 31);
    typename Act<T>::vec8 kf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) kf[s] = restage ? glb_row_frag<T>(base + a.k_off, a.ld_qkv, k_lane, S, s, lane) : lds_row_frag<T, DH>(sK, ob * 32, s, lane);
    const bool in = k_lane < S;
    const bool vk = in && a.keymask[b * S + k_lane];
    const float madd = vk ? 0.f : MASK_VALUE;
    float m = NEG_BIG, l = 0.f;
    stats_sweep<T, DH>(sQ, NB, 0, S, a.scale, madd, __any(!vk), kf, m, l, lane, lone);
    const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64);
    const float M = fmaxf(m, m2);
    const float logl = __logf(l * __expf(m - M) + l2 * __expf(m2 - M));
    if (lane < 32) {
      if (in) {
        a.lse[bh * S + k_lane] = M;
        a.lse[plane + bh * S + k_lane] = logl;
      }
      key_consts(in, vk, in ? M : 0.f, in ? logl : 0.f, a.scale, sSk[k_lane], sCk[k_lane]);
      sMadd[k_lane] = madd; sMax[k_lane] = in ? M : 0.f; sLogl[k_lane] = in ? logl : INFINITY;
    }
    padded |= (in && !vk);
  }
  if constexpr (DH <= 16) {
    if (lone) {  // statistics of the lone key: queries on the lanes, the reference's operation order (stats_tile_exact)
      const int64_t e = S - 1;
      const bool vk = a.keymask[b * S + e];
      const float madd = vk ? 0.f : MASK_VALUE;
      float ke[DH];
      if (restage) {
#pragma unroll
        for (int f = 0; f < DH; ++f) ke[f] = to_f32(base[a.k_off + e * a.ld_qkv + f]);
      } else {
        lds_row_load<T, DH>(sK + e * LD, ke);
      }
      float m = NEG_BIG, l = 0.f;
      for (int q = tid; q < S; q += nthr) {
        const float t = fmaf(lds_row_dot<T, DH>(sQ + q * LD, ke), a.scale, madd);
        const float m_new = fmaxf(m, t);
        l = l * __expf(m - m_new) + __expf(t - m_new);
        m = m_new;
      }
      const float mw = wave_max(m);
      const float lw = wave_sum(l * __expf(m - mw));  // (a lane without a query: l = 0)
      if (lane == 0) { sRed[wave] = mw; sRed[16 + wave] = lw; }
      __syncthreads();
      if (tid == 0) {
        float M = NEG_BIG, L = 0.f;
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sRed[w]);
        for (int w = 0; w < NW; ++w) L += sRed[16 + w] * __expf(sRed[w] - M);
        const float logl = __logf(L);
        a.lse[bh * S + e] = M;
        a.lse[plane + bh * S + e] = logl;
        key_consts(true, vk, M, logl, a.scale, sSk[e], sCk[e]);
        sMadd[e] = madd; sMax[e] = M; sLogl[e] = logl;
        for (int k = (int)S; k < SP; ++k) { key_consts(false, false, 0.f, 0.f, a.scale, sSk[k], sCk[k]); sMadd[k] = MASK_VALUE; sMax[k] = 0.f; sLogl[k] = INFINITY; }
      }
      padded |= !vk;
    }
  }
  const bool exact = __syncthreads_or(padded);  // does this sequence hold a padded key?
  const uint64_t pad_tiles = exact ? padded_tile_mask(sSk, sCk, NB, lane) : 0ull;  // ... and which of its key tiles do
  ATT_STAMP(3);
  if constexpr (CHUNKED) {
    // ---- phase B in C chunks of CR keys; this wave's owned query blocks are ob0 = wave and ob1 = wave + NW (host: NB <= 2 NW, no lone row)
    constexpr int OBM = 2;
    typename Act<T>::vec8 qf[OBM][KS];
    f32x16 o[OBM][DB];
    bool act[OBM];
#pragma unroll
    for (int i = 0; i < OBM; ++i) {
      const int ob = wave + i * NW;
      act[i] = ob < NBo && (int64_t)ob * 32 < a.q_limit;
#pragma unroll
      for (int s = 0; s < KS; ++s) qf[i][s] = glb_row_frag<T>(base + a.q_off, a.ld_qkv, act[i] ? (int64_t)ob * 32 + (lane & 31) : S, S, s, lane);
#pragma unroll
      for (int d = 0; d < DB; ++d) o[i][d] = zero16<DH>();
    }
    const int tiles_c = CR / 32;
    for (int c = 0; c < a.restage; ++c) {
      if (c > 0) __syncthreads();  // every wave is done with the previous chunk (c = 0: with the staged Q, the barrier above)
      const int64_t k0 = (int64_t)c * CR;
      stage_pair<T, DH>(sK, base + a.k_off + k0 * a.ld_qkv, a.ld_qkv, S - k0, sV, base + a.v_off + k0 * a.ld_qkv, a.ld_qkv, S - k0, CR, tid, nthr);
      __syncthreads();
      const int nt = (NBo - c * tiles_c) < tiles_c ? (NBo - c * tiles_c) : tiles_c;  // (the last chunk may hold fewer tiles)
#pragma unroll
      for (int i = 0; i < OBM; ++i) {
        if (!act[i]) continue;
        if (exact) {
          // (two loops, not a branch per tile: with both forms in one loop body the register allocator spilled 44 registers)
          const uint64_t padc = (pad_tiles >> (c * tiles_c)) & tile_bits(nt);
          MST_FOR_TILES(kt, ~padc & tile_bits(nt)) fwd_out_tile<T, DH, false>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, kt, a.scale, qf[i], o[i], lane);
          MST_FOR_TILES(kt, padc) fwd_out_tile<T, DH, true>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, kt, a.scale, qf[i], o[i], lane);
        } else {
          for (int kt = 0; kt < nt; ++kt) fwd_out_tile<T, DH, false>(sK, sV, sSk + k0, sCk + k0, sMadd + k0, sMax + k0, sLogl + k0, kt, a.scale, qf[i], o[i], lane);
        }
      }
    }
    T* og = reinterpret_cast<T*>(a.out) + b * S * a.ld_out + hd * DH;
#pragma unroll
    for (int i = 0; i < OBM; ++i) {
      const int64_t q_lane = (int64_t)(wave + i * NW) * 32 + (lane & 31);
      owner_store<T, DH>((act[i] && q_lane < S && q_lane < a.q_limit) ? og + q_lane * a.ld_out : nullptr, o[i], lane);
    }
    return;
  }
  if (restage) {  // (every wave is done with the staged Q)
    stage_pair<T, DH>(sK, base + a.k_off, a.ld_qkv, S, sV, base + a.v_off, a.ld_qkv, S, SP, tid, nthr);
    __syncthreads();
  }

  // ---- phase B: O = P^T V for the owned queries (attn_fwd_out_kernel's tiles)
  for (int ob = wave; ob < NBo; ob += NW) {
    if ((int64_t)ob * 32 >= a.q_limit) break;
    typename Act<T>::vec8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = restage ? glb_row_frag<T>(base + a.q_off, a.ld_qkv, (int64_t)ob * 32 + (lane & 31), S, s, lane) : lds_row_frag<T, DH>(sQ, ob * 32, s, lane);
    f32x16 o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = zero16<DH>();
    if (exact) {
      MST_FOR_TILES(kt, ~pad_tiles & tile_bits(NBo)) fwd_out_tile<T, DH, false>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, kt, a.scale, qf, o, lane);
      MST_FOR_TILES(kt, pad_tiles & tile_bits(NBo)) fwd_out_tile<T, DH, true>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, kt, a.scale, qf, o, lane);
    } else {
      for (int kt = 0; kt < NBo; ++kt) fwd_out_tile<T, DH, false>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, kt, a.scale, qf, o, lane);
    }
    if constexpr (DH <= 16) {
      if (lone) {  // the ninth key tile holds the lone key only
        if (exact) fwd_out_tile<T, DH, true, true>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, NB - 1, a.scale, qf, o, lane);
        else fwd_out_tile<T, DH, false, true>(sK, sV, sSk, sCk, sMadd, sMax, sLogl, NB - 1, a.scale, qf, o, lane);
      }
    }
    T* og = reinterpret_cast<T*>(a.out) + b * S * a.ld_out + hd * DH;
    const int64_t q_lane = ob * 32 + (lane & 31);
    owner_store<T, DH>((q_lane < S && q_lane < a.q_limit) ? og + q_lane * a.ld_out : nullptr, o, lane);
  }
  ATT_STAMP(4);
  if constexpr (DH <= 16) {
    if (lone) {  // O[e] = sum_k P[k,e] V[k]: keys on the lanes (P stays fp32 here; the MFMA form rounds it to the activation type)
      const int64_t e = S - 1;
      float qe[DH], acc[DH];
      if (restage) {
#pragma unroll
        for (int f = 0; f < DH; ++f) qe[f] = to_f32(base[a.q_off + e * a.ld_qkv + f]);
      } else {
        lds_row_load<T, DH>(sQ + e * LD, qe);
      }
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = 0.f;
      for (int k = tid; k < S; k += nthr) {
        const float x = lds_row_dot<T, DH>(sK + k * LD, qe);
        const float p = exact ? exact_prob(x, a.scale, sMadd[k], sMax[k], sLogl[k]) : fast_exp2(fmaf(x, sSk[k], sCk[k]));
        lds_row_axpy<T, DH>(p, sV + k * LD, acc);
      }
#pragma unroll
      for (int f = 0; f < DH; ++f) acc[f] = wave_sum(acc[f]);
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < DH; ++f) sRed[wave * DH + f] = acc[f];
      }
      __syncthreads();
      if (tid < DH) {
        float o_e = 0.f;
        for (int w = 0; w < NW; ++w) o_e += sRed[w * DH + tid];
        T* og = reinterpret_cast<T*>(a.out) + b * S * a.ld_out + hd * DH;
        og[e * a.ld_out + tid] = (T)o_e;
      }
    }
  }
}

// ---- launch code: the form is attention.hip's (attn_fwd_form)
template <typename T, int DH, bool QKV, bool CHUNKED>
static int launch_fwd_res(const AttnArgs& a, const AttnFwdForm& f, hipStream_t s, const char* what) {
  static size_t granted = 64 * 1024;
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&attn_fwd_res_kernel<T, DH, QKV, CHUNKED>), f.lds, &granted, what)) return rc;
  hipLaunchKernelGGL((attn_fwd_res_kernel<T, DH, QKV, CHUNKED>), dim3((unsigned)(a.B * a.H)), dim3(f.waves * 64), f.lds, s, a);
  MST_CHECK_LAUNCH(what);
  return MST_OK;
}
template <typename T, int DH>
static int launch_fwd(const AttnArgs& a_in, const AttnFwdForm& f, hipStream_t s) {
  AttnArgs a = a_in;
  a.restage = f.restage;
  switch (f.path) {
    case ATT_FWD_FUSED:
      if constexpr (DH == 32) return launch_fwd_res<T, DH, true, false>(a, f, s, "attn_fwd_res_kernel (fused projection)");
      break;
    case ATT_FWD_CHUNKED:
      if constexpr (DH >= 32) return launch_fwd_res<T, DH, false, true>(a, f, s, "attn_fwd_res_kernel (chunked)");
      break;
    case ATT_FWD_RES3:
    case ATT_FWD_RES2:
      return launch_fwd_res<T, DH, false, false>(a, f, s, "attn_fwd_res_kernel");
    case ATT_FWD_STREAM: {
      const dim3 grid((unsigned)f.grid_stats, (unsigned)(a.B * a.H));
      hipLaunchKernelGGL((attn_fwd_stats_kernel<T, DH>), grid, dim3(256), 0, s, a);
      MST_CHECK_LAUNCH("attn_fwd_stats_kernel");
      const dim3 grid_o((unsigned)f.grid_out, (unsigned)(a.B * a.H));
      hipLaunchKernelGGL((attn_fwd_out_kernel<T, DH>), grid_o, dim3(256), 0, s, a);
      MST_CHECK_LAUNCH("attn_fwd_out_kernel");
      return MST_OK;
    }
  }
  set_error("attention forward: form %d has no kernel at head size %d", f.path, DH);
  return MST_ERR_INVALID;
}

int attn_launch_fwd(int dtype, int64_t dh, const AttnArgs& a, const AttnFwdForm& f, hipStream_t s) {
  return dispatch_attn(dtype, dh, [&](auto tag, auto dh_c) -> int { return launch_fwd<decltype(tag), decltype(dh_c)::value>(a, f, s); });
}

}  // namespace mst

#ifdef MST_ATT_STAMPS
extern "C" int mst_debug_att_loop(uint64_t* host_out) {  // diagnostic builds only
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mst::g_att_loop), sizeof(uint64_t) * 256) == hipSuccess ? 0 : -1;
}
extern "C" int mst_debug_att_stamps(uint64_t* host_out) {  // diagnostic builds only: 1024 x 8 realtime stamps
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mst::g_att_stamps), sizeof(uint64_t) * 8192) == hipSuccess ? 0 : -1;
}
#endif

// attention.hpp — device code the units of key-row attention share (attention.hip states the operation and chooses every launch form):
//   the tile arithmetic of the key-row softmax, used by every kernel of attention_fwd.hip and attention_bwd.hip: key_consts ..
//   delta_from_dv, AttnArgs, the stats_* tiles and sweep, fwd_out_tile, bwd_q_tile, bwd_kv_tile;
//   then what the resident and chunked kernels share: whole-sequence staging, the lone row, their launch bounds, the phase stamps.
#pragma once
#include <math.h>
#include <type_traits>
#include "common.hpp"

namespace mst {

// rows staged in LDS per step by the streaming kernels (128 and 256 change nothing forward and cost 20 % backward, in
// registers: docs/kernel_notes.md)
constexpr int ATT_STAGE = 64;
// LDS row stride of the staged tiles: +8 elements (16 bytes). With rows of exactly DH*2 = 32/64/128 bytes the
// 16-byte row-fragment reads of 16 different rows fall on 4 bank groups (4-way conflict, measured 57 % of LDS cycles
// in attn_bwd_kv); 80-byte rows put them on 16 distinct ones and leave the transposed reads at most 2-way.
template <int DH> struct LdsLd { static constexpr int V = DH + 8; };
constexpr int ATT_WG_ROWS = 128;  // owner rows per workgroup (4 waves x 32)
constexpr float MASK_VALUE = -1e9f;
constexpr float NEG_BIG = -3.0e38f;
constexpr float LOG2E = 1.4426950408889634f;

// Softmax probabilities are evaluated as  P[k,q] = exp2(x * sk2[k] + ck2[k])  with per-key constants
//   unmasked key: sk2 = scale*log2(e),  ck2 = -(rowmax + log(rowsum)) * log2(e)
//   padded key  : sk2 = 0,              ck2 = -log(rowsum) * log2(e)
//   key >= S    : sk2 = 0,              ck2 = -inf                       (P = 0, no per-element guard)
// i.e. one FMA and one v_exp_f32 per element. For a padded key this is exact only while |x*scale| < 32, where
// fl(x*scale - 1e9) == -1e9 == rowmax and the logit cancels (transformer.py:111-125). Beyond that the reference's
// fp32 sum lands on another multiple of 64 and the row stops being uniform, so whenever a tile holds a padded key
// the kernels take the EXACT path instead (exact_prob: the reference's operation order in fp32); the fast form is
// used for tiles without padding (all of them in a full-length batch).
__device__ __forceinline__ void key_consts(bool in_range, bool valid_key, float rmax, float logl, float scale, float& sk2,
                                           float& ck2) {
  if (!in_range) { sk2 = 0.f; ck2 = -INFINITY; }
  else if (!valid_key) { sk2 = 0.f; ck2 = -logl * LOG2E; }
  else { sk2 = scale * LOG2E; ck2 = -(rmax + logl) * LOG2E; }
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// (the tiles of a bit set, lowest first: scalar loop control)
#define MST_FOR_TILES(kt, bits) for (uint64_t mst_m_ = (bits); mst_m_; mst_m_ &= mst_m_ - 1) if (const int kt = __builtin_ctzll(mst_m_); true)
__device__ __forceinline__ uint64_t tile_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
// Which 32-key tiles of a sequence hold a PADDED key (bit t: keys 32 t .. 32 t + 31), from the per-key constants in LDS: a padded
// key has sk2 = 0 with a finite ck2 (a key beyond the sequence: ck2 = -inf, and its P = 0 needs no exact arithmetic). The
// query-owner phases take the exact form for those tiles only; a padded batch used to pay it for every tile of every sequence
// that holds a padded key at all (attention forward + backward at S 256, lengths uniform in [S/2, S]: +29 % over a full batch).
// Scalar (wave-uniform) result; sequences of up to 64 tiles (the resident kernels' LDS bounds them far below that).
__device__ __forceinline__ uint64_t padded_tile_mask(const float* sSk, const float* sCk, int n_tiles, int lane) {
  uint32_t lo = 0u, hi = 0u;
  for (int t = 0; t < n_tiles; ++t) {
    const int k = t * 32 + (lane & 31);
    const bool p = sSk[k] == 0.f && sCk[k] > -INFINITY;
    if (__any(p)) { if (t < 32) lo |= 1u << t; else hi |= 1u << (t - 32); }
  }
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
}
// the reference's arithmetic, step by step: t = fl(x*scale + madd); p = exp((t - rowmax) - log(rowsum))
__device__ __forceinline__ float exact_prob(float x, float scale, float madd, float rmax, float logl) {
  return fast_exp2(((fmaf(x, scale, madd) - rmax) - logl) * LOG2E);
}

__device__ __forceinline__ i16x4 att_tr_read(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(uintptr_t)p);
}

// Staging of rows [row0, row0+ATT_STAGE) x DH of a [S, ld] matrix is split in two so that it can be software-pipelined:
// stage_load issues the global loads into registers (zero for rows >= S), stage_store writes them to the LDS tile
// [ATT_STAGE][DH+8]. Every streaming kernel loads stage i+1 right after storing stage i, i.e. BEFORE it computes on
// stage i, so the L2 / Infinity-Cache latency of the next tile runs under the current tile's MFMA + exp work
// (measured before: 55-67 % of the wave cycles of these kernels were waits on exactly that latency, five exposed
// round trips per workgroup).
template <typename T, int DH> struct StageRegs {
  static constexpr int CPR = DH / 8;
  static constexpr int N = (ATT_STAGE * CPR + 255) / 256;
  u32x4 v[N];
};
template <typename T, int DH>
__device__ __forceinline__ void stage_load(StageRegs<T, DH>& r, const T* __restrict__ g, int64_t ld, int64_t row0, int64_t S, int tid) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int i = 0; i < StageRegs<T, DH>::N; ++i) {
    const int c = tid + i * 256, row = c / CPR, ch = c % CPR;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (c < ATT_STAGE * CPR && row0 + row < S) v = *reinterpret_cast<const u32x4*>(g + (row0 + row) * ld + ch * 8);
    r.v[i] = v;
  }
}
template <typename T, int DH>
__device__ __forceinline__ void stage_store(T* lds, const StageRegs<T, DH>& r, int tid) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int i = 0; i < StageRegs<T, DH>::N; ++i) {
    const int c = tid + i * 256, row = c / CPR, ch = c % CPR;
    if (c < ATT_STAGE * CPR) *reinterpret_cast<u32x4*>(lds + row * LdsLd<DH>::V + ch * 8) = r.v[i];
  }
}

// per-key scalars of one stage (thread t < ATT_STAGE holds key k0 + t)
struct KeyRegs { float rmax, logl, delta; bool in, valid; };
__device__ __forceinline__ void key_load(KeyRegs& kr, const uint8_t* __restrict__ keymask, const float* __restrict__ lse,
                                         const float* __restrict__ delta, int64_t plane, int64_t b, int64_t bh, int64_t S,
                                         int64_t k, bool active) {
  kr.in = active && k < S;
  kr.valid = kr.in && keymask[b * S + k];
  kr.rmax = kr.in ? lse[bh * S + k] : 0.f;
  kr.logl = kr.in ? lse[plane + bh * S + k] : 0.f;
  kr.delta = (kr.in && delta) ? delta[bh * S + k] : 0.f;
}

// Workgroup -> (row tile, batch*head). Linear workgroup ids are dealt round-robin to the 8 XCDs; when the batch is a
// multiple of 8 the ids are remapped so that every tile of every head of one batch element runs on the same XCD:
// the K / V rows that the tiles of a head share, and the other half of each 128-byte line (the neighbouring head),
// are then re-read from that XCD's L2 instead of crossing the fabric again.
__device__ __forceinline__ void attn_wg_coords(int64_t B, int64_t H, int& tile, int64_t& bh) {
  const uint32_t gx = gridDim.x;  // (32-bit quotients: grid.x * grid.y < 2^31 workgroups)
  if (B % 8 == 0) {
    const uint32_t lin = blockIdx.x + gx * blockIdx.y, xcd = lin % 8u, j = lin / 8u, G = (uint32_t)H * gx;
    const uint32_t jq = j / G, r = j - jq * G, rq = r / gx;
    bh = (int64_t)(xcd + 8u * jq) * H + rq;
    tile = (int)(r - rq * gx);
  } else {
    tile = blockIdx.x;
    bh = blockIdx.y;
  }
}

// row fragment (A or B operand, k-contiguous) of rows [r0, r0+32) from an LDS tile with DH columns
template <typename T, int DH>
__device__ __forceinline__ typename Act<T>::vec8 lds_row_frag(const T* tile, int r0, int s, int lane) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(tile + (r0 + (lane & 31)) * LdsLd<DH>::V + 16 * s + 8 * (lane >> 5));
  return __builtin_bit_cast(typename Act<T>::vec8, v);
}

// row fragment straight from global (owner rows, loaded once per wave); zero beyond S
template <typename T>
__device__ __forceinline__ typename Act<T>::vec8 glb_row_frag(const T* __restrict__ g, int64_t ld, int64_t row, int64_t S, int s,
                                                              int lane) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < S) v = *reinterpret_cast<const u32x4*>(g + row * ld + 16 * s + 8 * (lane >> 5));
  return __builtin_bit_cast(typename Act<T>::vec8, v);
}

// B operand of an X^T·B product where X is a 32x32 accumulator tile used as the A operand:
// element j of lane-half h must be row 16*s2 + 8*(j>>2) + 4*h + (j&3) of the staged tile, column d0 + (lane&31).
template <typename T, int DH>
__device__ __forceinline__ typename Act<T>::vec8 lds_tr_frag(const T* tile, int r0, int s2, int d0, int lane) {
  const int h = lane >> 5, i = lane & 15, q = i >> 2, p = i & 3;
  const int c0 = (DH >= 32) ? d0 + 16 * ((lane >> 4) & 1) : 0;
  const int rlo = r0 + 16 * s2 + 4 * h + q;
  const i16x4 lo = att_tr_read(tile + rlo * LdsLd<DH>::V + c0 + 4 * p);
  const i16x4 hi = att_tr_read(tile + (rlo + 8) * LdsLd<DH>::V + c0 + 4 * p);
  const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename Act<T>::vec8, v);
}

template <typename T>
__device__ __forceinline__ typename Act<T>::vec8 acc_to_frag(const f32x16& x, int s2) {
  typename Act<T>::vec8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = (T)x[8 * s2 + j];
  return a;
}

__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

template <int DH>
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// Output tiles are accumulated "owner row on the lane": the accumulator of a 32-wide block of d holds rows d (registers)
// x owner rows (lane & 31) — the X-as-B-operand form of the accumulator-as-operand products below — so a lane holds
// elements d = 32 blk + 8 g + 4 (lane >> 5) + e (g, e = 0..3) of ITS row in registers 4 g + e: four 8-byte row pieces
// per block instead of sixteen 2-byte stores scattered over 16 rows.
template <typename T, int DH>
__device__ __forceinline__ void owner_store(T* __restrict__ row /* this lane's output row; nullptr: nothing to store */,
                                            const f32x16 (&acc)[(DH + 31) / 32], int lane) {
  if (!row) return;
  const int h4 = 4 * (lane >> 5);
#pragma unroll
  for (int d = 0; d < (DH + 31) / 32; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (32 * d + 8 * g < DH) {
        u32x2 o;
        o[0] = (uint32_t)f32_to_bits<T>(acc[d][4 * g]) | ((uint32_t)f32_to_bits<T>(acc[d][4 * g + 1]) << 16);
        o[1] = (uint32_t)f32_to_bits<T>(acc[d][4 * g + 2]) | ((uint32_t)f32_to_bits<T>(acc[d][4 * g + 3]) << 16);
        *reinterpret_cast<u32x2*>(row + 32 * d + 8 * g + h4) = o;
      }
}

// delta[k] = sum_q P[k,q] dP[k,q] with dP[k,q] = dO[q].V[k]  =  V[k] . (sum_q P[k,q] dO[q])  =  V[k] . dV[k]
// (the key-row analogue of flash attention's rowsum(dO o O)): one dot product per key from the finished dV accumulator
// instead of two MFMAs and sixteen FMAs per 32 x 32 tile of the dV sweep. acc is in owner_store's layout (key on the
// lane); vf is the key's V row as an MFMA fragment (lane half h' holds d = 16 u + 8 h' + j), so each lane half gets the
// four elements per 16 it lacks from its partner lane.
template <typename T, int DH>
__device__ __forceinline__ float delta_from_dv(const f32x16 (&acc)[(DH + 31) / 32], const typename Act<T>::vec8 (&vf)[DH / 16], int lane) {
  const bool hi_half = (lane >> 5) != 0;
  float dsum = 0.f;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) {
    const u32x4 w = __builtin_bit_cast(u32x4, vf[u]);
    const uint32_t s0 = hi_half ? w[0] : w[2], s1 = hi_half ? w[1] : w[3];
    const uint32_t r0 = (uint32_t)__shfl_xor((int)s0, 32, 64), r1 = (uint32_t)__shfl_xor((int)s1, 32, 64);
    const uint32_t e4[4] = {hi_half ? r0 : w[0], hi_half ? r1 : w[1], hi_half ? w[2] : r0, hi_half ? w[3] : r1};
    const int blk = u / 2, g = 2 * (u % 2);  // registers 4 g .. 4 g + 7 of block blk: d = 16 u + {4 h + e, 8 + 4 h + e}
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint16_t bits = (uint16_t)((e4[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
      dsum = fmaf(acc[blk][4 * g + e], bits_to_f32<T>(bits), dsum);
    }
  }
  return dsum + __shfl_xor(dsum, 32, 64);
}

struct AttnArgs {
  int64_t B, S, H;
  const void* qkv; int64_t ld_qkv, k_off, q_off, v_off;
  const uint8_t* keymask;
  float* lse;
  void* out; int64_t ld_out;
  const void* dout; int64_t ld_dout;
  void* dqkv; int64_t ld_dqkv;
  float* delta;
  float scale;
  int64_t q_limit;  // forward: only queries [0, q_limit) are produced (the top encoder layer needs query 0 alone)
  // fused K | Q | V projection (attn_fwd_res_kernel<.., QKV = true>): qkv = x W^T + bias is COMPUTED here (and written to
  // `qkv` for the backward pass) instead of read. x: [B*S, ld_x] layer input; w: [3 Dm, ld_w] 16-bit weights whose row c is
  // output column c of the qkv layout; bias: fp32 [3 Dm]
  const void* x; int64_t ld_x; const void* w; int64_t ld_w; const float* bias; int64_t Dm;
  // resident forward with TWO staged tiles instead of three (sequences whose Q | K | V do not fit together: Q for the statistics phase,
  // then K and V over it for the output phase; the owners' own fragments come from global memory)
  int restage;
};

// Online softmax statistics of one 32-query x 32-key tile, key on the lane.
// stats_tile_exact keeps the reference's operation order, t = fl(x*scale + madd) then exp(t - max): needed when the
// wave holds a padded key (madd = -1e9 swallows the logit, see key_consts). stats_tile_fast is for waves without one
// (madd = 0 for every lane): it tracks the maximum of the raw products and works in the exp2 domain,
//   m2 = max(x) * c,  l += exp2(x * c - m2),  c = scale * log2(e)
// i.e. max, fma, v_exp, add per element instead of fma, select, max, sub, mul, v_exp, select, add.
// GUARD: the tile may hold query rows beyond the sequence (the last tile of a ragged sequence); a whole tile needs neither the
// sixteen 64-bit row comparisons nor the selects around the exponentials (207 -> 110 issue slots; same values).
template <typename T, int DH, bool GUARD>
__device__ __forceinline__ void stats_tile_exact(const T* sQ, int r0, int64_t q_base, int64_t S, float scale, float madd,
                                                 const typename Act<T>::vec8 (&kf)[DH / 16], float& m, float& l, int lane) {
  f32x16 x = zero16<DH>();
#pragma unroll
  for (int s = 0; s < DH / 16; ++s) x = Act<T>::mfma32(lds_row_frag<T, DH>(sQ, r0, s, lane), kf[s], x);
  float t[16], tmax = NEG_BIG;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool valid = !GUARD || q_base + acc_row(r, lane) < S;
    t[r] = valid ? fmaf(x[r], scale, madd) : NEG_BIG;
    tmax = fmaxf(tmax, t[r]);
  }
  const float m_new = fmaxf(m, tmax);
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) sum += (!GUARD || t[r] > NEG_BIG) ? __expf(t[r] - m_new) : 0.f;
  l = l * __expf(m - m_new) + sum;
  m = m_new;
}
template <typename T, int DH, bool GUARD>
__device__ __forceinline__ void stats_tile_fast(const T* sQ, int r0, int64_t q_base, int64_t S, float c,
                                                const typename Act<T>::vec8 (&kf)[DH / 16], float& m2, float& l, int lane) {
  f32x16 x = zero16<DH>();
#pragma unroll
  for (int s = 0; s < DH / 16; ++s) x = Act<T>::mfma32(lds_row_frag<T, DH>(sQ, r0, s, lane), kf[s], x);
  if (GUARD) {
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = (q_base + acc_row(r, lane) < S) ? x[r] : -INFINITY;
  }
  float tmax = x[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, x[r]);
  const float m_new = fmaxf(m2, tmax * c);
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) sum += fast_exp2(fmaf(x[r], c, -m_new));
  l = l * fast_exp2(m2 - m_new) + sum;
  m2 = m_new;
}
// THIN tile: only the tile's first partner row exists (the lone row of a 32 n + 1 sequence, lone_row_shape): accumulator
// element 0 of the lower lane half; one exponential instead of sixteen.
template <typename T, int DH>
__device__ __forceinline__ void stats_tile_thin(const T* sQ, int r0, float c, const typename Act<T>::vec8 (&kf)[DH / 16], float& m2, float& l,
                                                int lane) {
  f32x16 x = zero16<DH>();
#pragma unroll
  for (int s = 0; s < DH / 16; ++s) x = Act<T>::mfma32(lds_row_frag<T, DH>(sQ, r0, s, lane), kf[s], x);
  const float x0 = (lane < 32) ? x[0] : -INFINITY;
  const float m_new = fmaxf(m2, x0 * c);
  l = l * fast_exp2(m2 - m_new) + fast_exp2(fmaf(x0, c, -m_new));
  m2 = m_new;
}
// Full statistics of the 32 keys on this wave's lanes over the query tiles [0, n_tiles) staged at sQ (tile t at rows
// 32 t, global query index q0 + 32 t): updates the running (max, sum) pair, natural-log domain on entry and exit.
constexpr float LN2 = 0.6931471805599453f;
template <typename T, int DH>
__device__ __forceinline__ void stats_sweep(const T* sQ, int n_tiles, int64_t q0, int64_t S, float scale, float madd, bool exact_w,
                                            const typename Act<T>::vec8 (&kf)[DH / 16], float& m, float& l, int lane, bool thin_tail = false) {
  if (exact_w) {
    for (int t = 0; t < n_tiles; ++t) {
      if (q0 + t * 32 + 32 <= S) stats_tile_exact<T, DH, false>(sQ, t * 32, q0 + t * 32, S, scale, madd, kf, m, l, lane);
      else stats_tile_exact<T, DH, true>(sQ, t * 32, q0 + t * 32, S, scale, madd, kf, m, l, lane);
    }
    return;
  }
  const float c = scale * LOG2E;
  float m2 = (m > NEG_BIG) ? m * LOG2E : NEG_BIG;
  for (int t = 0; t < n_tiles; ++t) {
    if (q0 + t * 32 + 32 <= S) stats_tile_fast<T, DH, false>(sQ, t * 32, q0 + t * 32, S, c, kf, m2, l, lane);
    else if (thin_tail) stats_tile_thin<T, DH>(sQ, t * 32, c, kf, m2, l, lane);
    else stats_tile_fast<T, DH, true>(sQ, t * 32, q0 + t * 32, S, c, kf, m2, l, lane);
  }
  m = (m2 > NEG_BIG) ? m2 * LN2 : NEG_BIG;
}

// One 32-key x 32-query tile of the query-owner kernels. Straight-line on purpose: EXACT is a template parameter (the
// callers branch once per tile), so the compiler is free to issue the per-key constant reads ahead of the exps.
// (THIN: only the tile's first key exists — accumulator element 0; the other fifteen probabilities are zero)
template <typename T, int DH, bool EXACT, bool THIN = false>
__device__ __forceinline__ void fwd_out_tile(const T* sK, const T* sV, const float* sSk, const float* sCk, const float* sMadd,
                                             const float* sMax, const float* sLogl, int blk, float scale,
                                             const typename Act<T>::vec8 (&qf)[DH / 16], f32x16 (&o)[(DH + 31) / 32], int lane) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  typename Act<T>::vec8 kfr[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) kfr[s] = lds_row_frag<T, DH>(sK, blk * 32, s, lane);
  typename Act<T>::vec8 vfr[2][DB];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int d = 0; d < DB; ++d) vfr[s2][d] = lds_tr_frag<T, DH>(sV, blk * 32, s2, d * 32, lane);
  f32x16 x = zero16<DH>();
#pragma unroll
  for (int s = 0; s < KS; ++s) x = Act<T>::mfma32(kfr[s], qf[s], x);
  if constexpr (THIN) {
    const int kr = blk * 32 + 4 * (lane >> 5);  // (upper lane half: a key beyond the sequence, its constants give p = 0)
    const float p0 = EXACT ? exact_prob(x[0], scale, sMadd[kr], sMax[kr], sLogl[kr]) : fast_exp2(fmaf(x[0], sSk[kr], sCk[kr]));
    x = zero16<DH>();
    x[0] = p0;
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, 0);  // (keys 8.. of the tile: all zero, no second product)
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = Act<T>::mfma32(vfr[0][d], pf, o[d]);
    return;
  }
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {  // accumulator rows 4g..4g+3 are 4 consecutive keys: one 16-byte read per constant
    const int kr = blk * 32 + 8 * g4 + 4 * (lane >> 5);
    const f32x4 c0 = *reinterpret_cast<const f32x4*>((EXACT ? sMadd : sSk) + kr);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>((EXACT ? sMax : sCk) + kr);
    f32x4 c2 = c1;
    if (EXACT) c2 = *reinterpret_cast<const f32x4*>(sLogl + kr);  // +inf for keys >= S: p = 0
#pragma unroll
    for (int e = 0; e < 4; ++e)
      x[4 * g4 + e] = EXACT ? exact_prob(x[4 * g4 + e], scale, c0[e], c1[e], c2[e]) : fast_exp2(fmaf(x[4 * g4 + e], c0[e], c1[e]));
  }
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, s2);
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = Act<T>::mfma32(vfr[s2][d], pf, o[d]);  // O^T += V^T P: rows d, query on the lane
  }
}

// dQ tile. With sCk holding ck2 + log2(scale) (so the exponential IS P * scale) and the dP accumulator started at
// -delta[k] (sNd, one value per accumulator row), dL = P (dP - delta) scale is one multiply per element:
//   x = exp2(S sk2 + ck2') * (dO.V - delta);  acc^T += K^T-fragment x   (rows d, query on the lane)
// LIGHT: the owned queries' dO rows are zero (dP = 0): no V fragments, no dP MFMAs.
template <typename T, int DH, bool EXACT, bool LIGHT = false, bool THIN = false>
__device__ __forceinline__ void bwd_q_tile(const T* sK, const T* sV, const float* sSk, const float* sCk, const float* sMadd,
                                           const float* sMax, const float* sLogl, const float* sNd, int blk, float scale,
                                           const typename Act<T>::vec8 (&qf)[DH / 16], const typename Act<T>::vec8 (&dof)[DH / 16],
                                           f32x16 (&acc)[(DH + 31) / 32], int lane) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  typename Act<T>::vec8 kfr[KS], vfr[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kfr[s] = lds_row_frag<T, DH>(sK, blk * 32, s, lane);
    if (!LIGHT) vfr[s] = lds_row_frag<T, DH>(sV, blk * 32, s, lane);
  }
  typename Act<T>::vec8 ktr[2][DB];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int d = 0; d < DB; ++d) ktr[s2][d] = lds_tr_frag<T, DH>(sK, blk * 32, s2, d * 32, lane);
  f32x16 x = zero16<DH>(), dp;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {  // accumulator rows 4g..4g+3 are 4 consecutive keys: one 16-byte read
    const f32x4 nd = *reinterpret_cast<const f32x4*>(sNd + blk * 32 + 8 * g4 + 4 * (lane >> 5));
#pragma unroll
    for (int e = 0; e < 4; ++e) dp[4 * g4 + e] = nd[e];
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    x = Act<T>::mfma32(kfr[s], qf[s], x);
    if (!LIGHT) dp = Act<T>::mfma32(vfr[s], dof[s], dp);
  }
  if constexpr (THIN) {  // only the tile's first key exists (accumulator element 0)
    const int kr = blk * 32 + 4 * (lane >> 5);
    const float pr = EXACT ? exact_prob(x[0], scale, sMadd[kr], sMax[kr], sLogl[kr]) * scale : fast_exp2(fmaf(x[0], sSk[kr], sCk[kr]));
    const float d0 = pr * dp[0];
    x = zero16<DH>();
    x[0] = d0;
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, 0);
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = Act<T>::mfma32(ktr[0][d], pf, acc[d]);
    return;
  }
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int kr = blk * 32 + 8 * g4 + 4 * (lane >> 5);
    const f32x4 c0 = *reinterpret_cast<const f32x4*>((EXACT ? sMadd : sSk) + kr);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>((EXACT ? sMax : sCk) + kr);
    f32x4 c2 = c1;
    if (EXACT) c2 = *reinterpret_cast<const f32x4*>(sLogl + kr);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pr = EXACT ? exact_prob(x[4 * g4 + e], scale, c0[e], c1[e], c2[e]) * scale : fast_exp2(fmaf(x[4 * g4 + e], c0[e], c1[e]));
      x[4 * g4 + e] = pr * dp[4 * g4 + e];  // (LIGHT: dp is still -delta)
    }
  }
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, s2);
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = Act<T>::mfma32(ktr[s2][d], pf, acc[d]);
  }
}

// One 32-query x 32-key tile of the key-owner backward, key on the lane throughout.
//   PASS 0: dV^T += dO^T-fragment P                     (delta follows from the finished dV: delta_from_dv)
//   PASS 1: dK^T += Q^T-fragment (P scale (dP - delta)): ck2s = ck2 + log2(scale) makes the exponential P * scale, and the
//           dP accumulator starts at -delta (the key's own value in every register), so dL is one multiply per element.
// sQ / sdO are the staged query-side operands (rows >= S are zero, so query rows beyond the sequence contribute nothing
// and need no guard).
// LIGHT (PASS 1 only): the tile's dO rows are all zero, so dP = 0 and dL = -P * delta * s — no dO fragments, no dP MFMAs;
// bit-identical to the full tile on zero dO rows (its accumulator stays at -delta).
template <typename T, int DH, int PASS, bool EXACT, bool LIGHT = false, bool THIN = false>
__device__ __forceinline__ void bwd_kv_tile(const T* sQ, const T* sdO, int qt, float scale, const typename Act<T>::vec8 (&kf)[DH / 16],
                                            const typename Act<T>::vec8 (&vf)[DH / 16], float sk2, float ck2x /* PASS 1: ck2s */, float madd,
                                            float rmax, float logl, float neg_delta, f32x16 (&acc)[(DH + 31) / 32], int lane) {
  constexpr int KS = DH / 16, DB = (DH + 31) / 32;
  static_assert(!LIGHT || PASS == 1, "a light tile contributes nothing to pass 0");
  constexpr bool NEED_DP = PASS == 1 && !LIGHT;
  typename Act<T>::vec8 qfr[KS], dofr[KS], trf[2][DB];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qfr[s] = lds_row_frag<T, DH>(sQ, qt * 32, s, lane);
    if (NEED_DP) dofr[s] = lds_row_frag<T, DH>(sdO, qt * 32, s, lane);
  }
  const T* tr_src = (PASS == 0) ? sdO : sQ;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int d = 0; d < DB; ++d) trf[s2][d] = lds_tr_frag<T, DH>(tr_src, qt * 32, s2, d * 32, lane);
  f32x16 x = zero16<DH>(), dp;
#pragma unroll
  for (int r = 0; r < 16; ++r) dp[r] = neg_delta;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    x = Act<T>::mfma32(qfr[s], kf[s], x);
    if (NEED_DP) dp = Act<T>::mfma32(dofr[s], vf[s], dp);
  }
  if constexpr (THIN) {  // only the tile's first query exists (accumulator element 0; the upper lane half's row is a zero row of sQ / sdO)
    float p0 = EXACT ? exact_prob(x[0], scale, madd, rmax, logl) : fast_exp2(fmaf(x[0], sk2, ck2x));
    if (PASS == 1) p0 = (EXACT ? p0 * scale : p0) * dp[0];
    x = zero16<DH>();
    x[0] = p0;
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, 0);
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = Act<T>::mfma32(trf[0][d], pf, acc[d]);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (PASS == 0) x[r] = EXACT ? exact_prob(x[r], scale, madd, rmax, logl) : fast_exp2(fmaf(x[r], sk2, ck2x));
    else x[r] = (EXACT ? exact_prob(x[r], scale, madd, rmax, logl) * scale : fast_exp2(fmaf(x[r], sk2, ck2x))) * dp[r];
  }
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const typename Act<T>::vec8 pf = acc_to_frag<T>(x, s2);
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = Act<T>::mfma32(trf[s2][d], pf, acc[d]);
  }
}

// ------------------------------------------------------------------------------------ resident kernels
// One workgroup per (batch, head) with the whole sequence resident in LDS: the two kernels of each direction become
// two PHASES of one launch (every launch in the captured step costs ~4.7 us before its first wave does useful work,
// and the streaming kernels re-stage the other operand once per 128 owner rows). Rows are owned in blocks of
// 32 by the waves of the workgroup round-robin (block ob -> wave ob % NW), first as keys (phase A: lane = key, the
// softmax axis in-lane), then as queries (phase B: lane = query, contraction over keys from the accumulators). The
// tile arithmetic is the streaming kernels' own (same functions, same operation order), so results are identical.
// Used when the staged operands fit in LDS (choose_resident, attention.hip); longer sequences take the streaming kernels.
template <typename T, int DH>
__device__ __forceinline__ void stage_all(T* lds, const T* __restrict__ g, int64_t ld, int64_t S, int SP, int tid, int nthr) {
  constexpr int CPR = DH / 8;
#pragma unroll 4
  for (int c = tid; c < SP * CPR; c += nthr) {
    const int row = c / CPR, ch = c % CPR;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < S) v = *reinterpret_cast<const u32x4*>(g + (int64_t)row * ld + ch * 8);
    *reinterpret_cast<u32x4*>(lds + row * LdsLd<DH>::V + ch * 8) = v;
  }
}

// Two tensors at once: every global load of both is issued before the first LDS store (stage_all twice is two exposed
// round trips: the second tensor's loads wait behind the first one's stores)
template <typename T, int DH>
__device__ __forceinline__ void stage_pair(T* ldsA, const T* __restrict__ gA, int64_t ldA, int64_t rowsA, T* ldsB,
                                           const T* __restrict__ gB, int64_t ldB, int64_t rowsB, int SP, int tid, int nthr) {
  constexpr int CPR = DH / 8, BATCH = 4;
  for (int c0 = tid; c0 < SP * CPR; c0 += nthr * BATCH) {
    u32x4 va[BATCH], vb[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const int c = c0 + i * nthr, row = c / CPR, ch = c % CPR;
      va[i] = u32x4{0u, 0u, 0u, 0u}; vb[i] = va[i];
      if (c < SP * CPR && row < rowsA) va[i] = *reinterpret_cast<const u32x4*>(gA + (int64_t)row * ldA + ch * 8);
      if (c < SP * CPR && row < rowsB) vb[i] = *reinterpret_cast<const u32x4*>(gB + (int64_t)row * ldB + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const int c = c0 + i * nthr, row = c / CPR, ch = c % CPR;
      if (c < SP * CPR) {
        *reinterpret_cast<u32x4*>(ldsA + row * LdsLd<DH>::V + ch * 8) = va[i];
        *reinterpret_cast<u32x4*>(ldsB + row * LdsLd<DH>::V + ch * 8) = vb[i];
      }
    }
  }
}

// ---- the LONE ROW of a sequence of 32 n + 1 rows (the decoder of configs[1]: 257 = the state row + 256 positions).
// As a ninth 32-row owner block it costs a whole wave's sweep over all nine partner tiles for one useful lane — 81 tile
// visits per sweep instead of 64, and nine waves per workgroup leave room for one workgroup per CU instead of two. As a
// PARTNER the row is no problem (the ninth partner tile is an ordinary partial tile). As an OWNER it is handled here with
// the roles turned over: the partner rows go on the lanes, each lane forms its row's dot products with the lone row
// in-lane (rows are read straight from the staged LDS tiles), and what the MFMA form gets by summing down the register
// axis becomes one cross-lane sum per output element at the end of the sweep — ~300 VALU operations per wave instead of
// ~1200, and the owner blocks left are whole: eight waves, two workgroups per CU, one resident round.
template <typename T, int DH>
__device__ __forceinline__ void lds_row_load(const T* row, float (&v)[DH]) {
#pragma unroll
  for (int c = 0; c < DH / 8; ++c) {
    Pack8 p; p.u = *reinterpret_cast<const u32x4*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * c + e] = bits_to_f32<T>(p.h[e]);
  }
}
template <typename T, int DH>
__device__ __forceinline__ float lds_row_dot(const T* row, const float (&w)[DH]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < DH / 8; ++c) {
    Pack8 p; p.u = *reinterpret_cast<const u32x4*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(bits_to_f32<T>(p.h[e]), w[8 * c + e], s);
  }
  return s;
}
template <typename T, int DH>
__device__ __forceinline__ void lds_row_axpy(float alpha, const T* row, float (&acc)[DH]) {
#pragma unroll
  for (int c = 0; c < DH / 8; ++c) {
    Pack8 p; p.u = *reinterpret_cast<const u32x4*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[8 * c + e] = fmaf(alpha, bits_to_f32<T>(p.h[e]), acc[8 * c + e]);
  }
}
constexpr int LONE_RED = 16 * 32;  // floats of cross-wave reduction scratch behind the per-key arrays
__host__ __device__ inline bool lone_row_shape(int64_t S, int dh) { return dh <= 16 && S > 32 && (S & 31) == 1; }  // (head size 32: the three fp32 rows spill the dense kernel)

// waves per SIMD the head-size-16 resident kernels are compiled for (5 = 96 VGPRs, two 9-wave workgroups per CU, measured no faster forward and spills backward: the kernels are VALU-bound, not occupancy-bound)
constexpr int ATT16_WAVES = 4;
// Waves per workgroup the resident kernels are compiled for. Head size 64 carries twice the fragments and accumulators per
// wave: under 1024-thread bounds (128 registers per lane) its kernels spilled 46-162 registers; eight waves (256 registers,
// two per SIMD) hold everything, and three 64-wide tiles of a sequence leave room for one workgroup per CU anyway.
template <int DH> constexpr int RES_MAX_WAVES = DH == 64 ? 8 : 16;
// (the plain forward kernel fits 118 registers at head size 64 and keeps sixteen waves — a 257- or 512-row sequence wants more
// than eight owners —; its chunked and fused-projection forms are the ones that spilled)
template <int DH, bool HEAVY> constexpr int FWD_MAX_WAVES = HEAVY ? RES_MAX_WAVES<DH> : 16;

// (batch*head) of a 1-D grid; batch elements are dealt to the XCDs so that the heads of one element share an L2
__device__ __forceinline__ int64_t res_wg_bh(int64_t B, int64_t H) {
  // (batch, head) pairs in XCD-contiguous eighths: the samples whose K | Q | V rows the projection GEMM's tiles left in
  // this XCD's L2 (common.hpp xcd_chunk; the heads of a sample stay together)
  return xcd_chunk(blockIdx.x, B * H);
}

// diagnostic build only (-DMST_ATT_STAMPS on ONE of attention_fwd.hip / attention_bwd.hip): realtime stamps (100 MHz) of the
// resident kernel's phases, per workgroup (internal linkage: the unit built with the flag owns the arrays and exports their readers)
#ifdef MST_ATT_STAMPS
static __device__ uint64_t g_att_stamps[1024 * 8];
#define ATT_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_att_stamps[8 * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
static __device__ uint64_t g_att_loop[4 * 64];  // workgroups 0, 100, 300, 500: s_memtime stamps inside the projection loop
#define LOOP_STAMP(k) do { if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == 100 || blockIdx.x == 300 || blockIdx.x == 500) && (k) < 64) \
    g_att_loop[(blockIdx.x == 0 ? 0 : blockIdx.x == 100 ? 1 : blockIdx.x == 300 ? 2 : 3) * 64 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ATT_STAMP(k) do { } while (0)
#define LOOP_STAMP(k) do { } while (0)
#endif

}  // namespace mst

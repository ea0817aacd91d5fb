// attention_causal.hip — causal self-attention with a softmax over the KEY axis, forward and backward (the decoder's opt-in
// causal mode, VAEConfig.d_causal; the reference's own key-row softmax lives in attention.hip and its units attention_fwd.hip /
// attention_bwd.hip and is not touched here).
//
// Per (batch b, head h), with keymask[b,k] the decoder's mask k < seq_len[b] + 1:
//   logit[q,k] = Q[q]·K[k] / sqrt(dh)              for k <= q and keymask[b,k]; excluded (P = 0) otherwise
//   P[q,:]     = softmax over k of the non-excluded logits
//   O[q]       = sum_k P[q,k] V[k]
// A query without an admissible key (key 0 masked, or every key up to it): O[q] = 0, lse = -inf in both planes (m stays -inf, l stays
// 0, logf(0)), delta = 0, and no pair of its row is admitted by the backward, so it reaches no gradient and its dQ row is 0.
// This is the model DecodePlan(attention="key") samples from (attention.hip attn_decode_kernel, mode 1).
//
// Three kernels on v_mfma_f32_32x32x16, one wave per workgroup and per 32-row block, the blocks of a (batch, head) walked in a
// fixed order so every sum is reproducible bit for bit (no atomics):
//   fwd    (query block on the lanes): online softmax over key blocks 0 .. qb; O and the row statistics
//   bwd_dq (query block on the lanes): pass 1 delta[q] = sum_k P dP, pass 2 dQ = s * sum_k dS K,  dS = P (dP - delta)
//   bwd_dkv (key block on the lanes) : over query blocks kb .. NB-1: dV = sum_q P dO,  dK = s * sum_q dS Q
// Key blocks above the diagonal are neither loaded nor computed. The logit tiles are computed with the owner rows on the
// lanes (column of the 32x32 accumulator) and the summed-over rows in the registers, so the probability tile is the B
// operand of the next product as it stands (converted to 16 bits); its A operand (V, K, dO or Q transposed) is staged in
// LDS as [dim][row] and read as two 8-byte pieces in the k order that the accumulator's register order implies.
#include <math.h>
#include "common.hpp"

namespace mst {
namespace causal {

constexpr int BLK = 32;       // rows per block (the 32x32 MFMA tile)
constexpr int LDT = BLK + 8;  // LDS row stride (elements) of a transposed [dim][row] tile: 80-byte rows, 8-byte aligned pieces
constexpr float L2E = 1.4426950408889634f;

struct Args {
  int64_t B, S, H;
  const void* qkv;
  int64_t ld_qkv, k_off, q_off, v_off;
  const uint8_t* keymask;
  float* lse;  // [2, B, H, S]: plane 0 = row max, plane 1 = log row sum
  void* out;
  int64_t ld_out;
  const void* dout;
  int64_t ld_dout;
  void* dqkv;
  int64_t ld_dqkv;
  float* delta;  // [B, H, S]
  float scale;
};

template <typename T> using V8 = typename Act<T>::vec8;

// the 32x32 accumulator's row of register i in lane half hh (its column is lane & 31)
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// 8 consecutive elements of row `row` from column `col` (zero for rows beyond the sequence)
template <typename T>
__device__ __forceinline__ V8<T> load_row8(const T* base, int64_t ld, int row, int S, int col) {
  u32x4 u = {0u, 0u, 0u, 0u};
  if (row < S) u = *reinterpret_cast<const u32x4*>(base + (int64_t)row * ld + col);
  return __builtin_bit_cast(V8<T>, u);
}

// rows [r0, r0 + 32) x DH of a row-major matrix into Xt[d][r] (zero beyond the sequence)
template <typename T, int DH>
__device__ __forceinline__ void stage_t(uint16_t* Xt, const T* base, int64_t ld, int r0, int S, int lane) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int c = lane; c < BLK * CPR; c += WAVE) {
    const int r = c / CPR, d0 = (c % CPR) * 8;
    Pack8 p;
    p.u = u32x4{0u, 0u, 0u, 0u};
    if (r0 + r < S) p.u = *reinterpret_cast<const u32x4*>(base + (int64_t)(r0 + r) * ld + d0);
#pragma unroll
    for (int e = 0; e < 8; ++e) Xt[(d0 + e) * LDT + r] = p.h[e];
  }
}

// A operand (rows d, k-step s) of a product whose B operand is an accumulator tile (k-step s = its registers 8s .. 8s+7):
// element j of lane half hh is k = 16 s + 8 (j >> 2) + 4 hh + (j & 3). Rows d >= DH are zero (head size 16).
template <typename T, int DH>
__device__ __forceinline__ V8<T> frag_t(const uint16_t* Xt, int d, int s, int hh) {
  u32x4 u = {0u, 0u, 0u, 0u};
  if (d < DH) {
    const u32x2 lo = *reinterpret_cast<const u32x2*>(Xt + d * LDT + 16 * s + 4 * hh);
    const u32x2 hi = *reinterpret_cast<const u32x2*>(Xt + d * LDT + 16 * s + 8 + 4 * hh);
    u = u32x4{lo[0], lo[1], hi[0], hi[1]};
  }
  return __builtin_bit_cast(V8<T>, u);
}

// registers 8s .. 8s+7 of an accumulator tile as a 16-bit B operand
template <typename T>
__device__ __forceinline__ V8<T> pack_acc(const f32x16& x, int s) {
  V8<T> v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (T)x[8 * s + j];
  return v;
}

// a transposed [dim][row] accumulator tile (rows dt*32 + acc_row, column = the lane's row `row`) scaled by `mul` into
// row `row` of a row-major output: four contiguous dims per 8-byte store
template <typename T, int DH>
__device__ __forceinline__ void store_t(T* dst, const f32x16& acc, int dt, int hh, float mul) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int d = dt * 32 + 8 * g + 4 * hh;
    if (d < DH) {
      union { u32x2 u; uint16_t h[4]; } p;
#pragma unroll
      for (int e = 0; e < 4; ++e) p.h[e] = f32_to_bits<T>(acc[4 * g + e] * mul);
      *reinterpret_cast<u32x2*>(dst + d) = p.u;
    }
  }
}

// bit j: key k0 + j is inside the sequence and not padding
__device__ __forceinline__ uint32_t key_bits(const uint8_t* km, int k0, int S, int lane) {
  const int k = k0 + lane;
  return (uint32_t)__ballot(lane < BLK && k < S && km[k] != 0);
}

template <typename T, int DH>
__global__ __launch_bounds__(64) void attn_causal_fwd_kernel(Args a) {
  constexpr int KS = DH / 16, DT = (DH + 31) / 32;
  __shared__ uint16_t Vt[DH * LDT];
  const int S = (int)a.S, NB = (S + BLK - 1) / BLK;
  const int qb = NB - 1 - (int)blockIdx.x;  // longest rows first
  const int64_t bh = blockIdx.y, b = bh / a.H, hd = bh % a.H;
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const T* base = (const T*)a.qkv + b * a.S * a.ld_qkv + hd * DH;
  const T *Kb = base + a.k_off, *Qb = base + a.q_off, *Vb = base + a.v_off;
  const uint8_t* km = a.keymask + b * a.S;
  const int q = qb * BLK + r;
  V8<T> qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = load_row8<T>(Qb, a.ld_qkv, q, S, 16 * s + 8 * hh);
  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
  float m = -INFINITY, l = 0.f;
  for (int kb = 0; kb <= qb; ++kb) {
    const int k0 = kb * BLK;
    __syncthreads();
    stage_t<T, DH>(Vt, Vb, a.ld_qkv, k0, S, lane);
    const uint32_t kbits = key_bits(km, k0, S, lane);
    f32x16 x = {};
#pragma unroll
    for (int s = 0; s < KS; ++s) x = Act<T>::mfma32(load_row8<T>(Kb, a.ld_qkv, k0 + r, S, 16 * s + 8 * hh), qf[s], x);
    __syncthreads();
    float tmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = acc_row(i, hh);
      x[i] = ((kbits >> j) & 1u) && k0 + j <= q ? x[i] * a.scale : -INFINITY;
      tmax = fmaxf(tmax, x[i]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax), mu = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f((m - mu) * L2E);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] = __builtin_amdgcn_exp2f((x[i] - mu) * L2E);
      ps += x[i];
    }
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const V8<T> pf = pack_acc<T>(x, s);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = Act<T>::mfma32(frag_t<T, DH>(Vt, dt * 32 + r, s, hh), pf, o[dt]);
    }
  }
  if (q < S) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* dst = (T*)a.out + (b * a.S + q) * a.ld_out + hd * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) store_t<T, DH>(dst, o[dt], dt, hh, inv);
    if (hh == 0) {
      a.lse[bh * a.S + q] = m;
      a.lse[(a.B * a.H + bh) * a.S + q] = logf(l);
    }
  }
}

// query-owner backward: delta and dQ
template <typename T, int DH>
__global__ __launch_bounds__(64) void attn_causal_bwd_dq_kernel(Args a) {
  constexpr int KS = DH / 16, DT = (DH + 31) / 32;
  __shared__ uint16_t Kt[DH * LDT];
  const int S = (int)a.S, NB = (S + BLK - 1) / BLK;
  const int qb = NB - 1 - (int)blockIdx.x;
  const int64_t bh = blockIdx.y, b = bh / a.H, hd = bh % a.H;
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const T* base = (const T*)a.qkv + b * a.S * a.ld_qkv + hd * DH;
  const T *Kb = base + a.k_off, *Qb = base + a.q_off, *Vb = base + a.v_off;
  const T* Gb = (const T*)a.dout + b * a.S * a.ld_dout + hd * DH;
  const uint8_t* km = a.keymask + b * a.S;
  const int q = qb * BLK + r;
  V8<T> qf[KS], gf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = load_row8<T>(Qb, a.ld_qkv, q, S, 16 * s + 8 * hh);
    gf[s] = load_row8<T>(Gb, a.ld_dout, q, S, 16 * s + 8 * hh);
  }
  const float c = q < S ? a.lse[bh * a.S + q] + a.lse[(a.B * a.H + bh) * a.S + q] : 0.f;
  // P^T and dP^T of key block kb: logits with the keys in the registers, this lane's query in the column
  auto tiles = [&](int kb, f32x16& p, f32x16& dp) {
    const int k0 = kb * BLK;
    const uint32_t kbits = key_bits(km, k0, S, lane);
    p = f32x16{};
    dp = f32x16{};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      p = Act<T>::mfma32(load_row8<T>(Kb, a.ld_qkv, k0 + r, S, 16 * s + 8 * hh), qf[s], p);
      dp = Act<T>::mfma32(load_row8<T>(Vb, a.ld_qkv, k0 + r, S, 16 * s + 8 * hh), gf[s], dp);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = acc_row(i, hh);
      p[i] = ((kbits >> j) & 1u) && k0 + j <= q && q < S ? __builtin_amdgcn_exp2f((p[i] * a.scale - c) * L2E) : 0.f;
    }
  };
  float dsum = 0.f;
  for (int kb = 0; kb <= qb; ++kb) {
    f32x16 p, dp;
    tiles(kb, p, dp);
#pragma unroll
    for (int i = 0; i < 16; ++i) dsum = fmaf(p[i], dp[i], dsum);
  }
  const float delta = dsum + __shfl_xor(dsum, 32, 64);
  if (q < S && hh == 0) a.delta[bh * a.S + q] = delta;
  f32x16 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x16{};
  for (int kb = 0; kb <= qb; ++kb) {
    __syncthreads();
    stage_t<T, DH>(Kt, Kb, a.ld_qkv, kb * BLK, S, lane);
    f32x16 p, dp;
    tiles(kb, p, dp);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] *= dp[i] - delta;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const V8<T> df = pack_acc<T>(p, s);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dq[dt] = Act<T>::mfma32(frag_t<T, DH>(Kt, dt * 32 + r, s, hh), df, dq[dt]);
    }
  }
  if (q < S) {
    T* dst = (T*)a.dqkv + (b * a.S + q) * a.ld_dqkv + a.q_off + hd * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) store_t<T, DH>(dst, dq[dt], dt, hh, a.scale);
  }
}

// key-owner backward: dK and dV (reads the delta bwd_dq wrote)
template <typename T, int DH>
__global__ __launch_bounds__(64) void attn_causal_bwd_dkv_kernel(Args a) {
  constexpr int KS = DH / 16, DT = (DH + 31) / 32;
  __shared__ uint16_t Qt[DH * LDT], Gt[DH * LDT];
  __shared__ float sc[BLK], sd[BLK];
  const int S = (int)a.S, NB = (S + BLK - 1) / BLK;
  const int kb = (int)blockIdx.x;  // (block 0 has the most query blocks: longest first)
  const int64_t bh = blockIdx.y, b = bh / a.H, hd = bh % a.H;
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const T* base = (const T*)a.qkv + b * a.S * a.ld_qkv + hd * DH;
  const T *Kb = base + a.k_off, *Qb = base + a.q_off, *Vb = base + a.v_off;
  const T* Gb = (const T*)a.dout + b * a.S * a.ld_dout + hd * DH;
  const int key = kb * BLK + r;
  const bool kvalid = key < S && a.keymask[b * a.S + key] != 0;
  V8<T> kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = load_row8<T>(Kb, a.ld_qkv, key, S, 16 * s + 8 * hh);
    vf[s] = load_row8<T>(Vb, a.ld_qkv, key, S, 16 * s + 8 * hh);
  }
  const float* lse1 = a.lse + a.B * a.H * a.S;
  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x16{};
  for (int qb = kb; qb < NB; ++qb) {
    const int q0 = qb * BLK;
    __syncthreads();
    stage_t<T, DH>(Qt, Qb, a.ld_qkv, q0, S, lane);
    stage_t<T, DH>(Gt, Gb, a.ld_dout, q0, S, lane);
    if (lane < BLK) {
      const int qq = q0 + lane;
      sc[lane] = qq < S ? a.lse[bh * a.S + qq] + lse1[bh * a.S + qq] : 0.f;
      sd[lane] = qq < S ? a.delta[bh * a.S + qq] : 0.f;
    }
    // logits with the queries in the registers, this lane's key in the column
    f32x16 p = {}, dp = {};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      p = Act<T>::mfma32(load_row8<T>(Qb, a.ld_qkv, q0 + r, S, 16 * s + 8 * hh), kf[s], p);
      dp = Act<T>::mfma32(load_row8<T>(Gb, a.ld_dout, q0 + r, S, 16 * s + 8 * hh), vf[s], dp);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = acc_row(i, hh), qq = q0 + j;
      const float pv = kvalid && key <= qq && qq < S ? __builtin_amdgcn_exp2f((p[i] * a.scale - sc[j]) * L2E) : 0.f;
      p[i] = pv;
      dp[i] = pv * (dp[i] - sd[j]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const V8<T> pf = pack_acc<T>(p, s), df = pack_acc<T>(dp, s);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[dt] = Act<T>::mfma32(frag_t<T, DH>(Gt, dt * 32 + r, s, hh), pf, dv[dt]);
        dk[dt] = Act<T>::mfma32(frag_t<T, DH>(Qt, dt * 32 + r, s, hh), df, dk[dt]);
      }
    }
  }
  if (key < S) {
    T* row = (T*)a.dqkv + (b * a.S + key) * a.ld_dqkv + hd * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      store_t<T, DH>(row + a.k_off, dk[dt], dt, hh, a.scale);
      store_t<T, DH>(row + a.v_off, dv[dt], dt, hh, 1.f);
    }
  }
}

static int check(const char* fn, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv, int64_t k_off,
                 int64_t q_off, int64_t v_off) {
  MST_CHECK_ARG(B > 0 && S > 0 && H > 0 && S < (1 << 24), "%s: B, S, H must be positive (S below 2^24)", fn);
  MST_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "%s: head size must be 16, 32 or 64 (got %lld)", fn, (long long)dh);
  MST_CHECK_ARG(ld_qkv % 8 == 0 && k_off % 8 == 0 && q_off % 8 == 0 && v_off % 8 == 0 && k_off >= 0 && q_off >= 0 && v_off >= 0,
                "%s: ld and offsets must be non-negative multiples of 8", fn);
  MST_CHECK_ARG(k_off + H * dh <= ld_qkv && q_off + H * dh <= ld_qkv && v_off + H * dh <= ld_qkv, "%s: a section runs past ld_qkv", fn);
  MST_CHECK_ARG(B * H <= 65535, "%s: B*H too large for grid.y", fn);
  MST_CHECK_ARG(qkv && (uintptr_t)qkv % 16 == 0, "%s: qkv must be a 16-byte aligned pointer", fn);
  return MST_OK;
}

}  // namespace causal
}  // namespace mst

using namespace mst;
using namespace mst::causal;

extern "C" int mst_attn_causal_fwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv,
                                   int64_t k_off, int64_t q_off, int64_t v_off, const uint8_t* keymask, float* lse, void* out,
                                   int64_t ld_out, mst_stream_t stream) {
  int rc = check("mst_attn_causal_fwd", B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off);
  if (rc) return rc;
  MST_CHECK_ARG(keymask && lse && out, "mst_attn_causal_fwd: null pointer");
  MST_CHECK_ARG(ld_out % 8 == 0 && ld_out >= H * dh && (uintptr_t)out % 16 == 0,
                "mst_attn_causal_fwd: out must be 16-byte aligned with ld_out a multiple of 8 and >= H*dh");
  Args a = {};
  a.B = B; a.S = S; a.H = H; a.qkv = qkv; a.ld_qkv = ld_qkv; a.k_off = k_off; a.q_off = q_off; a.v_off = v_off;
  a.keymask = keymask; a.lse = lse; a.out = out; a.ld_out = ld_out;
  a.scale = 1.f / sqrtf((float)dh);
  const dim3 grid((unsigned)cdiv(S, BLK), (unsigned)(B * H));
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    if (dh == 16) hipLaunchKernelGGL((attn_causal_fwd_kernel<T, 16>), grid, dim3(64), 0, s, a);
    else if (dh == 32) hipLaunchKernelGGL((attn_causal_fwd_kernel<T, 32>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((attn_causal_fwd_kernel<T, 64>), grid, dim3(64), 0, s, a);
    MST_CHECK_LAUNCH("attn_causal_fwd_kernel");
    return MST_OK;
  });
}

extern "C" int mst_attn_causal_bwd(int dtype, int64_t B, int64_t S, int64_t H, int64_t dh, const void* qkv, int64_t ld_qkv,
                                   int64_t k_off, int64_t q_off, int64_t v_off, const uint8_t* keymask, const float* lse,
                                   const void* dout, int64_t ld_dout, void* dqkv, int64_t ld_dqkv, float* delta,
                                   mst_stream_t stream) {
  int rc = check("mst_attn_causal_bwd", B, S, H, dh, qkv, ld_qkv, k_off, q_off, v_off);
  if (rc) return rc;
  MST_CHECK_ARG(keymask && lse && dout && dqkv && delta, "mst_attn_causal_bwd: null pointer");
  MST_CHECK_ARG(ld_dout % 8 == 0 && ld_dout >= H * dh && (uintptr_t)dout % 16 == 0,
                "mst_attn_causal_bwd: dout must be 16-byte aligned with ld_dout a multiple of 8 and >= H*dh");
  MST_CHECK_ARG(ld_dqkv % 8 == 0 && (uintptr_t)dqkv % 16 == 0 && k_off + H * dh <= ld_dqkv &&
                    q_off + H * dh <= ld_dqkv && v_off + H * dh <= ld_dqkv,
                "mst_attn_causal_bwd: dqkv must be 16-byte aligned with ld_dqkv a multiple of 8 that covers every section");
  Args a = {};
  a.B = B; a.S = S; a.H = H; a.qkv = qkv; a.ld_qkv = ld_qkv; a.k_off = k_off; a.q_off = q_off; a.v_off = v_off;
  a.keymask = keymask; a.lse = const_cast<float*>(lse); a.dout = dout; a.ld_dout = ld_dout; a.dqkv = dqkv; a.ld_dqkv = ld_dqkv;
  a.delta = delta;
  a.scale = 1.f / sqrtf((float)dh);
  const dim3 grid((unsigned)cdiv(S, BLK), (unsigned)(B * H));
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    if (dh == 16) hipLaunchKernelGGL((attn_causal_bwd_dq_kernel<T, 16>), grid, dim3(64), 0, s, a);
    else if (dh == 32) hipLaunchKernelGGL((attn_causal_bwd_dq_kernel<T, 32>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((attn_causal_bwd_dq_kernel<T, 64>), grid, dim3(64), 0, s, a);
    MST_CHECK_LAUNCH("attn_causal_bwd_dq_kernel");
    if (dh == 16) hipLaunchKernelGGL((attn_causal_bwd_dkv_kernel<T, 16>), grid, dim3(64), 0, s, a);
    else if (dh == 32) hipLaunchKernelGGL((attn_causal_bwd_dkv_kernel<T, 32>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((attn_causal_bwd_dkv_kernel<T, 64>), grid, dim3(64), 0, s, a);
    MST_CHECK_LAUNCH("attn_causal_bwd_dkv_kernel");
    return MST_OK;
  });
}

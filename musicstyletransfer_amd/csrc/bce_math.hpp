// bce_math.hpp — one element of sigmoid + BinaryCrossEntropy (loss.py:27-80) and its logit gradient, shared by
// sigmoid_bce_kernel (losses.hip) and the output-layer GEMM's epilogue (gemm_bce.hpp: bce_tile_finish), so the two produce
// the same bits.
//
// bce_exact is the reference's operation order in fp32:
//     p = 1 / (1 + e^-x);  bce = -(s log(1e-12 + p) + (1 - s) log(1e-12 + (1 - p)))                     loss.py:40-48
//     d bce / dx = -(s / (1e-12 + p) - (1 - s) / (1e-12 + (1 - p))) p (1 - p)
// — six transcendental instructions per element; at configs[2] (33.5 M elements) that arithmetic, not HBM, was the loss
// launch (92 us). bce_fast needs three (exp, rcp, log): with q = 1 / (1 + e^-|x|) the LARGER of (p, 1 - p) — so q >= 1/2,
// 1e-12 + q == q in fp32 and log q is as accurate as the reference's —, the smaller is e^-|x| q, its log is log q - |x|,
// and the gradient collapses to p - s (the 1e-12 terms cancel to below one ulp). It agrees with bce_exact to fp32 rounding
// while the 1e-12 epsilons are invisible (smaller probability >= 1e-7: x >= -16) AND while the reference's own
// fl(1 - p) still resolves the smaller probability (x <= 9: beyond that p is within a few ulp of 1 and the reference's
// log(1 - p) is off by 1e-4 and more — which parity keeps); outside [-16, 9] callers take bce_exact. The choice is per
// ELEMENT (bce_fast_domain), so the fused and the unfused launch agree bit for bit whatever their element-to-lane maps;
// callers evaluate bce_exact only in waves that hold an out-of-domain element (a wave-uniform vote), then select.
#pragma once
#include "common.hpp"

namespace mst {

constexpr float BCE_FAST_LO = -16.f, BCE_FAST_HI = 9.f;

__device__ __forceinline__ bool bce_fast_domain(float x) { return x >= BCE_FAST_LO && x <= BCE_FAST_HI; }

// y in {0, 1}; s = (1 - ls) y + ls / 2 (loss.py:34-36); dw: the (w bce) bce form where y == 0 (loss.py:52-54)
template <bool DW>
__device__ __forceinline__ void bce_exact(float x, float y, float ls, float w, float& p, float& bce, float& dbce) {
  p = __frcp_rn(1.f + __expf(-x));  // v_rcp_f32 (1 ulp) instead of the ~10-instruction IEEE divide
  const float omp = 1.f - p;
  const float s = (1.f - ls) * y + 0.5f * ls;
  const float lp = __logf(1e-12f + p), lq = __logf(1e-12f + omp);
  bce = -(s * lp + (1.f - s) * lq);
  // d bce / d logit = d bce/dp * p(1-p)
  dbce = -(s * __frcp_rn(1e-12f + p) - (1.f - s) * __frcp_rn(1e-12f + omp)) * p * omp;
  if (DW && y == 0.f) {
    dbce = 2.f * w * bce * dbce;
    bce = w * bce * bce;
  }
}

template <bool DW>
__device__ __forceinline__ void bce_fast(float x, float y, float s1 /* s for y = 1 */, float s0 /* s for y = 0 */, float w, float& p,
                                         float& bce, float& dbce) {
  // raw v_exp_f32 / v_rcp_f32 / v_log_f32 (1 ulp): every argument is a normal number inside the fast domain, and hipcc expands
  // __expf / __logf / __frcp_rn into denormal-safe scaling and a ~10-instruction IEEE division
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_exp2f(-1.4426950408889634f * ax);  // e^-|x| in (1e-7, 1]
  const float q = __builtin_amdgcn_rcpf(1.f + t);                     // the larger probability, in [1/2, 1)
  const float lbig = 0.6931471805599453f * __builtin_amdgcn_logf(q), lsmall = lbig - ax;
  const bool pos = x >= 0.f;
  p = pos ? q : t * q;
  const float lp = pos ? lbig : lsmall, lq = pos ? lsmall : lbig;
  const float s = (y != 0.f) ? s1 : s0;
  bce = -(s * lp + (1.f - s) * lq);
  dbce = p - s;
  if (DW && y == 0.f) {
    dbce = 2.f * w * bce * dbce;
    bce = w * bce * bce;
  }
}

// ---- piano-roll counts (mst_hip.h: mst_bce_args.counts, mst_sigmoid_bce_counts). A cell is "predicted" where the 16-bit logit the
// loss is computed from is > 0 (false for +-0 and NaN); labels are {0,1} bytes; the four counts are tp, pred, pos, cells.
// roll_predicted: byte e = 1 where cell e (of the first n of VEC consecutive ones) is predicted — the layout the label bytes have
template <int VEC>
__device__ __forceinline__ uint64_t roll_predicted(const float (&x)[VEC], int n) {
  uint64_t pm = 0;
#pragma unroll
  for (int e = 0; e < VEC; ++e) pm |= (e < n && x[e] > 0.f) ? 1ull << (8 * e) : 0ull;
  return pm;
}
// the counts of up to 8 cells in four fields of BITS bits, tp | pred << BITS | pos << 2 BITS | cells << 3 BITS (lab: no byte set
// beyond cell n)
template <int BITS>
__device__ __forceinline__ uint64_t roll_pack(uint64_t pm, uint64_t lab, int n) {
  const uint64_t pos = lab & 0x0101010101010101ull;
  return (uint64_t)__popcll(pm & pos) | (uint64_t)__popcll(pm) << BITS | (uint64_t)__popcll(pos) << (2 * BITS) | (uint64_t)n << (3 * BITS);
}
// one thread adds the workgroup's four counts to its slot, linear workgroup id % MST_ROLL_SLOTS: ordinary 64-bit vector atomics,
// integer sums, so the totals over the slots do not depend on the arrival order
__device__ __forceinline__ void roll_add_slot(uint64_t* counts, uint64_t tp, uint64_t pred, uint64_t pos, uint64_t cells) {
  const unsigned wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  unsigned long long* slot = reinterpret_cast<unsigned long long*>(counts) + (size_t)(wg % MST_ROLL_SLOTS) * 4;
  atomicAdd(slot + 0, (unsigned long long)tp);
  atomicAdd(slot + 1, (unsigned long long)pred);
  atomicAdd(slot + 2, (unsigned long long)pos);
  atomicAdd(slot + 3, (unsigned long long)cells);
}
// The threads' packed counts (roll_pack<16>) of a workgroup with at most 2^15 cells: every field's sum over the workgroup stays below
// 2^16, so fp32 sums (wave_sum's DPP butterflies) are exact integers. roll_wave16: all lanes; lane 0 stores the wave's four sums at
// part[4 wave ..]. roll_total16: ONE thread, behind a barrier, adds the NW waves' sums to the slot.
__device__ __forceinline__ void roll_wave16(uint64_t roll, float* part) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum((float)(uint32_t)((roll >> (16 * k)) & 0xFFFFull));
  if ((threadIdx.x & 63) == 0) *reinterpret_cast<f32x4*>(part + (threadIdx.x >> 6) * 4) = f32x4{v[0], v[1], v[2], v[3]};
}
template <int NW>
__device__ __forceinline__ void roll_total16(const float* part, uint64_t* counts) {
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NW; ++i) t += *reinterpret_cast<const f32x4*>(part + i * 4);
  roll_add_slot(counts, (uint64_t)t[0], (uint64_t)t[1], (uint64_t)t[2], (uint64_t)t[3]);
}

}  // namespace mst

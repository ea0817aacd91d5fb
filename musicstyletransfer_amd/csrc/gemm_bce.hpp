// gemm_bce.hpp — the output layer's 64 x BN logit tile finished as sigmoid + BCE: the device code shared by the loss launches
// (gemm_bce.hip) and dec_tail_kernel (dec_tail.hip).
#pragma once
#include <type_traits>
#include "common.hpp"
#include "gemm_tile.hpp"
#include "bce_math.hpp"

namespace mst {

// Output layer + per-pitch BCE in ONE launch (mst_gemm_sigmoid_bce): the decoder's Dense[D -> P] (model.py:253-256) with
// sigmoid + BinaryCrossEntropy (loss.py:27-80) in its epilogue. A tile is 64 frames x BN pitches (128 or 256: the LDS-staged
// (time x pitch) tile) — the whole row of pitches at configs[1], one of P / 256 column tiles of it at configs[2]'s 2048 (the
// loss is a plain sum over frames and pitches, so column tiles only share the sample's atomic) — and the logits never reach
// HBM: the epilogue turns the fp32 accumulators into the
// logit gradient (the backward pass's operand), optionally the probabilities (reconstruction output), and the sample's
// loss sum — the arithmetic of sigmoid_bce_kernel on the logit rounded to the activation type, which is what the two-launch
// form reads back. A tile holds rows of ONE sample (the host requires T % 64 == 0): one atomic per workgroup.
// keepA (KEEP): the logit-gradient tile ALSO goes to LDS as the A operand of a GEMM that follows in the same launch, in
// gemm_mainloop's stage layout (BK = 64: columns [64 s, 64 s + 64) in stage buffer s, 16-byte chunks XOR-swizzled by the row)
// bce_tile_finish: the tile's epilogue, from the fp32 accumulators of the 64 x BN logit tile at (m0, n0). KEEP 1: the stage layout
// above; KEEP 2: the kept tile is row-major with a row stride of BN + 8 elements (ffn_ln_body's x tile: dec_tail_kernel).
// `red`, the static LDS a kernel hands to bce_tile_finish (16-byte aligned): a word per wave for the loss and the positive count, then
// (CNT) four per wave for the piano-roll counts
constexpr int BCE_RED_LOSS = 512 / 64;
constexpr int bce_red_words(bool cnt) { return cnt ? 5 * BCE_RED_LOSS : BCE_RED_LOSS; }
// CNT: the launch keeps the piano-roll counts (q.counts is set). A compile-time switch: as a run-time test of the pointer the counting
// code cost dec_tail_kernel six more spilled SGPRs and 2.1 us with counts == NULL (docs/kernel_notes.md); without CNT the code is the
// kernel's of before.
template <typename T, int BN, int KEEP, bool CNT>
__device__ __forceinline__ void bce_tile_finish(const mst_gemm_args& a, const mst_bce_args& q, unsigned char* smem, float* red, u32x4* keepA,
                                                f32x4 (&acc)[(BN / 4) / 16][(64 / 2) / 16], int64_t m0, int64_t n0, const float (&bias8)[8]) {
  constexpr int BM = 64, WGM = 2, WGN = 4, NT = 512;
  constexpr int WTM = BM / WGM, WTN = BN / WGN, TM = WTM / 16, TN = WTN / 16;
  constexpr int LDS_F = BN + 4, CPR = BN / 8, RSTEP = NT / CPR, ITERS = BM / RSTEP;
  const int64_t P = a.N;                       // pitches per frame (a multiple of BN: this tile holds columns [n0, n0 + BN))
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, frow = lane & 15, fq = lane >> 4;
  float* sF = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      *reinterpret_cast<f32x4*>(sF + (wm * WTM + i * 16 + frow) * LDS_F + wn * WTN + j * 16 + fq * 4) = acc[j][i];
  const int64_t b = m0 / q.T;                  // the tile's sample
  const int64_t per_sample = q.T * P;
  float w = 0.f;
  if (q.downweight) {                          // loss.py:58-81: w_b = n_pos / (n_neg + 1e-12) over the SAMPLE's labels
    const uint8_t* lab = q.labels + b * per_sample;
    int cnt = 0;
    for (int64_t i = (int64_t)tid * 8; i < per_sample; i += (int64_t)NT * 8)
      cnt += __popcll(*reinterpret_cast<const uint64_t*>(lab + i) & 0x0101010101010101ull);
    float c = wave_sum((float)cnt);
    if (lane == 0) red[wave] = c;
    __syncthreads();
    float np = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) np += red[i];
    w = np / (((float)q.T * (float)P - np) + 1e-12f);
  }
  __syncthreads();                              // staged tile visible (and `red` free again)
  const int ch = tid % CPR, nc = ch * 8, row0 = tid / CPR;
  const int64_t gc = n0 + nc;                   // this thread's 8 pitches in the frame
  const float inv_n = 1.f / ((float)q.T * (float)P), ls = q.label_smoothing;
  float lsum = 0.f;
  // the piano-roll counts of this thread's live cells (mst_bce_args.counts), 16 bits each: tp | pred << 16 | pos << 32 | cells << 48
  // (a tile has 64 BN <= 2^14 cells, so the workgroup's sums stay inside their fields)
  uint64_t roll = 0;
  const float s1 = (1.f - ls) + 0.5f * ls, s0 = 0.5f * ls;
  auto sweep = [&](auto dwc) {
    constexpr bool DW = decltype(dwc)::value;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = row0 + it * RSTEP;
      const int64_t m = m0 + row;
      const bool live = m < a.M;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(sF + row * LDS_F + nc);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(sF + row * LDS_F + nc + 4);
      const float t8[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      const uint64_t lab8 = live ? *reinterpret_cast<const uint64_t*>(q.labels + m * P + gc) : 0ull;
      Pack8 pb, gb, xb;
      float x8[8];
      bool in_dom = true;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xb.h[e] = f32_to_bits<T>((t8[e] + bias8[e]) * a.alpha);  // the logit as the unfused pipeline stores it
        x8[e] = bits_to_f32<T>(xb.h[e]);
        in_dom = in_dom && bce_fast_domain(x8[e]);
      }
      const bool fast = __all(in_dom || !live);  // wave-uniform (bce_math.hpp: three transcendental instructions per element, not six)
      if (CNT && live) roll += roll_pack<16>(roll_predicted<8>(x8, 8), lab8, 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float y = (float)((lab8 >> (8 * e)) & 0xFFull);
        float p, bce, dbce;
        bce_fast<DW>(x8[e], y, s1, s0, w, p, bce, dbce);
        if (!fast) {  // a saturated logit somewhere in this wave: ITS element takes the reference's operation order (an element's
                      // result depends on its own logit only, so the fused and the two-launch forms agree bit for bit)
          float p2, b2, d2;
          bce_exact<DW>(x8[e], y, ls, w, p2, b2, d2);
          if (!bce_fast_domain(x8[e])) { p = p2; bce = b2; dbce = d2; }
        }
        lsum += live ? bce : 0.f;
        pb.h[e] = f32_to_bits<T>(p);
        gb.h[e] = f32_to_bits<T>(dbce * inv_n * q.gscale);
      }
      if (!live) continue;
      if (a.C) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(a.C) + m * a.ldc + gc) = gb.u;
      if constexpr (KEEP == 1) keepA[(ch >> 3) * (BM * 8) + row * 8 + ((ch & 7) ^ (row & 7))] = gb.u;  // (KEEP: P == BN)
      if constexpr (KEEP == 2) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(keepA) + row * (BN + 8) + nc) = gb.u;
      if (q.probs) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(q.probs) + m * q.ldp + gc) = pb.u;
      if (q.logits) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(q.logits) + m * q.ldl + gc) = xb.u;
    }
  };
  if (q.downweight) sweep(std::true_type()); else sweep(std::false_type());
  lsum = wave_sum(lsum);
  if (lane == 0) red[wave] = lsum;
  if constexpr (CNT) roll_wave16(roll, red + BCE_RED_LOSS);
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) tot += red[i];
    atomicAdd(q.loss + b, tot * inv_n);
    if constexpr (CNT) roll_total16<NT / 64>(red + BCE_RED_LOSS, q.counts);
  }
}

template <typename T, int BN, bool KEEP, bool CNT>
__device__ __forceinline__ void gemm_bce_tile(const mst_gemm_args& a, const mst_bce_args& q, unsigned char* smem, float* red, u32x4* keepA) {
  constexpr int BM = 64, WGM = 2, WGN = 4;
  f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
  int64_t m0, n0;
  float bias8[8];
  gemm_bias_preload<BM, BN>(a, bias8);
  gemm_mainloop<T, BM, BN, WGM, WGN, 64>(a, smem, acc, m0, n0);
  bce_tile_finish<T, BN, KEEP ? 1 : 0, CNT>(a, q, smem, red, keepA, acc, m0, n0, bias8);
}

}  // namespace mst

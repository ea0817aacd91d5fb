// class_job.hpp — the decoder class table's gradient, dcls[class_b, j] += t[b, j] (model.py:229-232), from the rows the latent
// block's backward launch leaves in its scratch buffer (tvec). Nothing downstream but the optimizer reads it, so like the latent
// block's outer products (outer_jobs.hpp) it rides as extra workgroups on the weight-gradient reduction pass (gemm_wgrad.hip) — or
// is one launch of its own (latent.hip: class_table_grad_kernel) when there is no reduction pass, or when mst_latent_bwd_vec is
// given the table's gradient to fill itself. Either way the workgroups run class_table_block: same batch quarters, same order, same
// bits.
#pragma once
#include "common.hpp"

namespace mst {

// dcls[class_b, j] += t[b, j] without fp32 atomics, whose arrival order made the table's
// gradient — and, through Adam, whole training runs — differ in the last bits from run to run. A 256-thread block owns 64
// columns; as in batch_outer its four waves take a quarter of the batch each, 16 rows of loads in flight, and the quarters are
// added in order through LDS. Classes go four at a time in registers (the class index selects, so nothing is indexed
// dynamically); the table here has two.
constexpr int CT_ROWS = 16, CT_CLS = 4;
__device__ __forceinline__ void class_table_block(int blk, int tid, int64_t B, int Dd, const float* __restrict__ tvec,
                                                  const int32_t* __restrict__ classes, float* __restrict__ dcls, int64_t ld_cls) {
  __shared__ int s_ncls;
  __shared__ float red[CT_CLS][4][64];
  // (part is the wave's index, said so to the compiler: the batch rows and their classes are then scalar — one base register and the
  // column for all 16 loads of a chunk, 30 VGPRs; as a per-lane value every load had an address pair of its own, 128 VGPRs, which
  // is what the whole reduction pass would run at when this is a branch of it)
  const int o = tid & 63, part = __builtin_amdgcn_readfirstlane(tid >> 6), j = blk * 64 + o;
  const bool col = j < Dd;
  const int64_t per = (B + 3) / 4, b0 = part * per, b1 = b0 + per < B ? b0 + per : B;
  if (tid == 0) s_ncls = 0;
  __syncthreads();
  // the number of classes comes out of the first pass's own loads (an integer max in LDS: order-free); a table of more than
  // CT_CLS classes takes more passes over the batch
  for (int c0 = 0, n_cls = CT_CLS; c0 < n_cls; c0 += CT_CLS) {
    float acc[CT_CLS];
#pragma unroll
    for (int q = 0; q < CT_CLS; ++q) acc[q] = 0.f;
    int mx = 0;
    int64_t b = b0;
    for (; b + CT_ROWS <= b1; b += CT_ROWS) {  // whole chunks: every load of the chunk in flight at once
      float v[CT_ROWS];
      int cl[CT_ROWS];
#pragma unroll
      for (int u = 0; u < CT_ROWS; ++u) {
        cl[u] = classes[b + u];
        v[u] = col ? tvec[(b + u) * Dd + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < CT_ROWS; ++u) {
        mx = max(mx, cl[u] + 1);
#pragma unroll
        for (int q = 0; q < CT_CLS; ++q) acc[q] += cl[u] - c0 == q ? v[u] : 0.f;  // (rows in batch order; x + 0 is exact)
      }
    }
    for (; b < b1; ++b) {
      const int cl = classes[b];
      const float v = col ? tvec[b * Dd + j] : 0.f;
      mx = max(mx, cl + 1);
#pragma unroll
      for (int q = 0; q < CT_CLS; ++q) acc[q] += cl - c0 == q ? v : 0.f;
    }
    if (c0 == 0) atomicMax(&s_ncls, mx);
#pragma unroll
    for (int q = 0; q < CT_CLS; ++q) red[q][part][o] = acc[q];
    __syncthreads();
    n_cls = s_ncls;
    if (part == 0 && col)
#pragma unroll
      for (int q = 0; q < CT_CLS; ++q)
        if (c0 + q < n_cls) dcls[(int64_t)(c0 + q) * ld_cls + j] += ((red[q][0][o] + red[q][1][o]) + red[q][2][o]) + red[q][3][o];
    __syncthreads();
  }
}

// One deferred class-table job: wgs == 0 is "none". Workgroup blk < wgs owns columns [64 blk, 64 blk + 64).
struct ClassJob {
  const int32_t* classes;  // [B]
  const float* tvec;       // [B, Dd] fp32 contiguous (mst_latent_bwd_vec's scratch[0 .. B * Dd))
  float* dcls;             // [n_classes, ld_cls] fp32, accumulated into
  int64_t ld_cls, B;
  int Dd, wgs;
};

// host: validate and pack; all-null / zero arguments are "no job". Returns MST_OK or a status with mst_last_error() set
static inline int pack_class_job(const int32_t* classes, const float* tvec, float* dcls, int64_t ld_cls, int64_t B, int64_t Dd,
                                 ClassJob& c) {
  c = ClassJob{};
  if (!classes && !tvec && !dcls && B == 0 && Dd == 0) return MST_OK;
  MST_CHECK_ARG(classes && tvec && dcls, "mst_class_table_grad: null pointer");
  MST_CHECK_ARG(B > 0 && Dd > 0 && Dd < (1ll << 30), "mst_class_table_grad: B and Dd must be positive (Dd below 2^30)");
  MST_CHECK_ARG(ld_cls >= Dd, "mst_class_table_grad: ld_cls < Dd");
  c.classes = classes; c.tvec = tvec; c.dcls = dcls; c.ld_cls = ld_cls; c.B = B;
  c.Dd = (int)Dd; c.wgs = (int)cdiv(Dd, 64);
  return MST_OK;
}

}  // namespace mst

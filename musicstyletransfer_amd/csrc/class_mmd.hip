// class_mmd.hip — the class-conditional MMD penalty on z and its gradient (mst_class_mmd; include/mst_hip.h states the arithmetic).
// One wave per row i, MMD_ROWS rows per workgroup. Phase 1: a lane owns a partner row j of a 64-row chunk and walks the dimensions
// (q_ij in fp32, the exponential, then w_ij and c_ij in fp64, left in LDS). Phase 2: a lane owns a dimension and walks the chunk's j in
// ascending order (g_i[d] and — the same sum in every lane — L_i, fp64). z goes through LDS in 64 x 64 tiles padded by one column: phase 1
// reads a tile by rows (stride 65 words: no bank conflict), phase 2 by columns. The gradient part then adds coef * g_i to the row's
// d[mu | sigma]; the sixteen rows' additions then go through LDS and the workgroup multiplies them with Wl — a lane owns one column and
// four rows of d(enc_out), and requests 32 rows of Wl at a time. The workgroup that draws the last ticket adds the rows in ascending order.
// Bookkeeping-sized: at B = 64, Z = 64, De = 256 four workgroups, ~8 K exponentials and 2 M multiply-adds.
#include <math.h>
#include "common.hpp"

namespace mst {

constexpr int MMD_ROWS = 16, MMD_THREADS = MMD_ROWS * WAVE, MMD_TILE = 64, MMD_MAXG = 4;  // Z <= MMD_TILE * MMD_MAXG
constexpr int MMD_ZMAX = MMD_TILE * MMD_MAXG;
constexpr int MMD_COLS = 16, MMD_RG = WAVE / MMD_COLS, MMD_RPL = MMD_ROWS / MMD_RG;  // the product: 16 columns x 4 groups of 4 rows per wave
constexpr int MMD_JB = 32;                                                          // rows of Wl in flight per lane
// LDS: the arrays of the two phases, and over them — they are dead by then — the sixteen rows' additions for the d(enc_out) product
constexpr int MMD_OFF_ZI = MMD_TILE * (MMD_TILE + 1) * 4, MMD_OFF_C = MMD_OFF_ZI + MMD_ROWS * MMD_TILE * 4;
constexpr int MMD_OFF_T = MMD_OFF_C + MMD_ROWS * MMD_TILE * 8, MMD_PHASE_BYTES = MMD_OFF_T + MMD_ROWS * MMD_TILE * 8;
constexpr int MMD_ADD_BYTES = MMD_ROWS * (2 * MMD_ZMAX + 1) * 4;
constexpr int MMD_LDS_BYTES = MMD_PHASE_BYTES > MMD_ADD_BYTES ? MMD_PHASE_BYTES : MMD_ADD_BYTES;
static_assert(MMD_OFF_C % 8 == 0 && MMD_ROWS * MMD_TILE * 8 >= MMD_THREADS * 8, "fp64 arrays aligned; s_c holds the closing sum's rows");

template <typename T>
__global__ __launch_bounds__(MMD_THREADS) void class_mmd_kernel(int64_t B, int Z, int De, const float* __restrict__ z, int64_t ld_z,
                                                                 const float* __restrict__ eps, int64_t ld_eps,
                                                                 const int32_t* __restrict__ classes, float s2, float coef,
                                                                 const float* __restrict__ Wl, float* __restrict__ dlat,
                                                                 T* __restrict__ d_enc_out, int64_t denc_stride, double* __restrict__ rows,
                                                                 uint32_t* __restrict__ ticket, double* __restrict__ acc) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[MMD_LDS_BYTES];
  float (*s_zj)[MMD_TILE + 1] = reinterpret_cast<float (*)[MMD_TILE + 1]>(smem);            // rows jc .. jc + 63, dimensions dc .. dc + 63 (0 outside the batch / past Z)
  float (*s_zi)[MMD_TILE] = reinterpret_cast<float (*)[MMD_TILE]>(smem + MMD_OFF_ZI);       // the workgroup's own rows, the same dimensions
  double (*s_c)[MMD_TILE] = reinterpret_cast<double (*)[MMD_TILE]>(smem + MMD_OFF_C);      // c_ij of the chunk (0 for j >= B); reused by the closing sum
  double (*s_t)[MMD_TILE] = reinterpret_cast<double (*)[MMD_TILE]>(smem + MMD_OFF_T);      // w_ij k_ij of the chunk
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t i_raw = (int64_t)blockIdx.x * MMD_ROWS + w;
  const bool active = i_raw < B;                    // (a wave past the batch works on the last row and writes nothing)
  const int64_t i = active ? i_raw : B - 1;
  const int ng = (Z + MMD_TILE - 1) / MMD_TILE;
  const float* zi = z + i * ld_z;
  const int ci = classes[i];
  // n_{c_i}: the rows of row i's class (classes are compared, never an index)
  int n_ci = 0;
  for (int64_t j0 = 0; j0 < B; j0 += WAVE) {
    const int64_t j = j0 + lane;
    n_ci += __popcll(__ballot(j < B && classes[j < B ? j : 0] == ci));
  }
  const double n = (double)B, s2d = (double)s2;
  const double w_same = 1.0 / (n * (double)n_ci) - 1.0 / (n * n), w_diff = 0.0 - 1.0 / (n * n);
  const float two_s2 = 2.f * s2;  // (exact)
  float zi_r[MMD_MAXG];
  double g[MMD_MAXG];
#pragma unroll
  for (int k = 0; k < MMD_MAXG; ++k) {
    const int d = k * MMD_TILE + lane;
    zi_r[k] = d < Z ? zi[d] : 0.f;
    g[k] = 0.0;
  }
  double L = 0.0;

  auto stage = [&](int64_t jc, int dc, bool own) {
#pragma unroll
    for (int r = 0; r < MMD_TILE * MMD_TILE / MMD_THREADS; ++r) {
      const int idx = tid + r * MMD_THREADS, row = idx / MMD_TILE, col = idx % MMD_TILE;
      const int64_t j = jc + row;
      s_zj[row][col] = (j < B && dc + col < Z) ? z[j * ld_z + dc + col] : 0.f;
    }
    if (own) s_zi[w][lane] = dc + lane < Z ? zi[dc + lane] : 0.f;
  };

  for (int64_t jc = 0; jc < B; jc += MMD_TILE) {
    // ---- phase 1: lane owns j = jc + lane, q_ij by fmaf in ascending d
    float q = 0.f;
    for (int dc = 0; dc < Z; dc += MMD_TILE) {
      __syncthreads();  // the tile's previous readers are done
      stage(jc, dc, true);
      __syncthreads();
      const int dn = Z - dc < MMD_TILE ? Z - dc : MMD_TILE;
#pragma unroll 8
      for (int d = 0; d < dn; ++d) {
        const float diff = s_zi[w][d] - s_zj[lane][d];
        q = fmaf(diff, diff, q);
      }
    }
    {
      const int64_t j = jc + lane;
      const bool valid = j < B;
      const float kf = expf(-q / two_s2);  // (i == j: q = 0, exactly 1)
      const double kd = (double)kf;
      const double wij = (valid && classes[valid ? j : 0] == ci) ? w_same : w_diff;
      s_c[w][lane] = valid ? 2.0 * wij * kd / s2d : 0.0;
      s_t[w][lane] = valid ? wij * kd : 0.0;
    }
    // ---- phase 2: lane owns d = k * 64 + lane, sums over the chunk's j in ascending order
    const int jn = B - jc < MMD_TILE ? (int)(B - jc) : MMD_TILE;
#pragma unroll
    for (int k = 0; k < MMD_MAXG; ++k) {
      if (k < ng) {
        if (ng > 1) {  // (one tile of dimensions: phase 1 left it in place)
          __syncthreads();
          stage(jc, k * MMD_TILE, false);
        }
        __syncthreads();  // (also orders this wave's s_c / s_t stores in front of its loads)
        const double zid = (double)zi_r[k];
        double gk = g[k];
#pragma unroll 8
        for (int jj = 0; jj < jn; ++jj) {
          gk += s_c[w][jj] * ((double)s_zj[jj][lane] - zid);
          if (k == 0) L += s_t[w][jj];
        }
        g[k] = gk;
      }
    }
  }

  // (a write-through store at agent scope: the closing sum's loads, at the same scope, see it without a release / acquire pair)
  if (active && lane == 0)
    __hip_atomic_store(reinterpret_cast<uint64_t*>(rows + i), __builtin_bit_cast(uint64_t, L), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // ---- gradient: the additions to d[mu | sigma] of row i, and their product with Wl added to d(enc_out) of the workgroup's rows
  if (dlat != nullptr) {
    __syncthreads();  // the phases' arrays are dead: the additions of the sixteen rows go over them
    const int lda = 2 * Z + 1;
    float* s_add = reinterpret_cast<float*>(smem);  // [MMD_ROWS][lda]; a row past the batch holds zeros
    {
      float* dl = dlat + i * 2 * (int64_t)Z;
      const double cf = (double)coef;
#pragma unroll
      for (int k = 0; k < MMD_MAXG; ++k) {
        const int d = k * MMD_TILE + lane;
        if (d < Z) {
          float am = 0.f, as = 0.f;
          if (active) {
            am = (float)(cf * g[k]);
            as = (float)(cf * g[k] * (double)eps[i * ld_eps + d]);
            dl[d] += am;
            dl[Z + d] += as;
          }
          s_add[w * lda + d] = am;
          s_add[w * lda + Z + d] = as;
        }
      }
    }
    __syncthreads();
    // d(enc_out)[r, e] += sum_j add[r, j] Wl[j, e], fmaf in ascending j: a lane owns one column e and MMD_RPL rows, a wave MMD_COLS
    // columns, the workgroup 256; MMD_JB rows of Wl are requested before the first is used (the loads are the launch's latency)
    const int col = lane & (MMD_COLS - 1), r0 = (lane / MMD_COLS) * MMD_RPL, J = 2 * Z;
    for (int e0 = 0; e0 < De; e0 += MMD_ROWS * MMD_COLS) {
      const int e = e0 + w * MMD_COLS + col;
      const bool ok = e < De;
      float a[MMD_RPL];
#pragma unroll
      for (int r = 0; r < MMD_RPL; ++r) a[r] = 0.f;
      for (int j0 = 0; j0 < J; j0 += MMD_JB) {
        float wv[MMD_JB];
#pragma unroll
        for (int u = 0; u < MMD_JB; ++u) wv[u] = (ok && j0 + u < J) ? Wl[(int64_t)(j0 + u) * De + e] : 0.f;
#pragma unroll
        for (int u = 0; u < MMD_JB; ++u) {
          if (j0 + u < J) {
#pragma unroll
            for (int r = 0; r < MMD_RPL; ++r) a[r] = fmaf(s_add[(r0 + r) * lda + j0 + u], wv[u], a[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < MMD_RPL; ++r) {
        const int64_t row = (int64_t)blockIdx.x * MMD_ROWS + r0 + r;
        if (ok && row < B) {
          T* de = d_enc_out + row * denc_stride + e;
          *de = from_f32<T>(to_f32(*de) + a[r]);
        }
      }
    }
    __syncthreads();  // (the closing sum reuses s_c)
  }

  // ---- the last workgroup adds the rows: every wave's write-through store of its row has completed before the workgroup draws its
  // ticket, and the rows are read back at agent scope (no fence: a release here would write back the whole L2 of the step's activations)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const uint32_t drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = drawn == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  double* s_rows = &s_c[0][0];  // MMD_THREADS doubles
  double sum = 0.0;
  for (int64_t r0 = 0; r0 < B; r0 += MMD_THREADS) {
    if (r0 + tid < B) s_rows[tid] = __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const uint64_t*>(rows + r0 + tid), __ATOMIC_RELAXED,
                                                                                 __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    if (tid == 0) {
      const int rn = B - r0 < MMD_THREADS ? (int)(B - r0) : MMD_THREADS;
      for (int r = 0; r < rn; ++r) sum += s_rows[r];  // ascending i, one thread
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (isfinite(sum)) {
      acc[0] += sum;
      acc[1] += 1.0;
    } else {
      acc[2] += 1.0;
    }
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // left at zero for the next launch
  }
}

}  // namespace mst

using namespace mst;

extern "C" int mst_class_mmd(int dtype, int64_t B, int64_t Z, int64_t De, const float* z, int64_t ld_z, const float* eps, int64_t ld_eps,
                             const int32_t* classes, float s2, float coef, const float* Wl, float* dlat, void* d_enc_out,
                             int64_t denc_sample_stride, double* rows, uint32_t* ticket, double* acc, mst_stream_t stream) {
  MST_CHECK_ARG(z && classes && rows && ticket && acc, "mst_class_mmd: null pointer");
  MST_CHECK_ARG(B > 0 && Z > 0 && De > 0, "mst_class_mmd: B, Z and De must be positive");
  MST_CHECK_ARG(B < (1ll << 31) && Z <= MMD_ZMAX && De < (1ll << 30),
                "mst_class_mmd: B must be below 2^31, Z at most %d, De below 2^30", MMD_ZMAX);
  MST_CHECK_ARG(ld_z >= Z, "mst_class_mmd: ld_z < Z");
  MST_CHECK_ARG(isfinite(s2) && s2 > 0.f, "mst_class_mmd: s2 must be finite and > 0 (got %g)", (double)s2);
  MST_CHECK_ARG(isfinite(coef), "mst_class_mmd: coef must be finite");
  MST_CHECK_ARG((uintptr_t)rows % 8 == 0 && (uintptr_t)acc % 8 == 0 && (uintptr_t)ticket % 4 == 0,
                "mst_class_mmd: rows and acc must be 8-byte aligned, ticket 4-byte aligned");
  const bool grad = dlat != nullptr;
  MST_CHECK_ARG(grad ? (Wl && d_enc_out && eps) : (!Wl && !d_enc_out && !eps),
                "mst_class_mmd: Wl, dlat, d_enc_out and eps are all given (value and gradient) or all NULL (value only)");
  const dim3 grid((unsigned)cdiv(B, MMD_ROWS)), block(MMD_THREADS);
  if (!grad) {
    hipLaunchKernelGGL(class_mmd_kernel<__bf16>, grid, block, 0, (hipStream_t)stream, B, (int)Z, (int)De, z, ld_z, (const float*)nullptr,
                       (int64_t)0, classes, s2, coef, (const float*)nullptr, (float*)nullptr, (__bf16*)nullptr, (int64_t)0, rows, ticket, acc);
    MST_CHECK_LAUNCH("class_mmd_kernel");
    return MST_OK;
  }
  MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "mst_class_mmd: unsupported activation dtype %d (want MST_BF16 or MST_F16)", dtype);
  MST_CHECK_ARG(ld_eps >= Z && denc_sample_stride >= De, "mst_class_mmd: ld_eps < Z or denc_sample_stride < De");
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    hipLaunchKernelGGL(class_mmd_kernel<T>, grid, block, 0, (hipStream_t)stream, B, (int)Z, (int)De, z, ld_z, eps, ld_eps, classes, s2, coef,
                       Wl, dlat, (T*)d_enc_out, denc_sample_stride, rows, ticket, acc);
    MST_CHECK_LAUNCH("class_mmd_kernel");
    return MST_OK;
  });
}

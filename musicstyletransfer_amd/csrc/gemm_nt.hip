// gemm_nt.hip — C[M,N] = epilogue(A[M,K] · B[N,K]^T), 16-bit operands, fp32 accumulate on MFMA.
//
// Replaces gluon.nn.Dense(flatten=False) (y = x W^T + b, W stored [units, in_units]) at
// VarAutoEncoder/transformer.py:36-40,65-68 and model.py:214-227, and — called with the W^T
// shadow as B — the data-gradient of the same layers.
//
// Design (gfx950): both operands are K-contiguous, so every MFMA fragment is one 16-byte LDS
// read. The product is formed "swapped" (MFMA A-operand = weight rows n, B-operand = activation
// rows m) so an accumulator register quad is 4 consecutive n of one output row: the epilogue
// reads bias/residual/gate and writes C with 8-byte (16-bit C) or 16-byte (fp32 C) accesses.
// Tiles are staged global → registers → LDS (XOR-swizzled 16-byte chunks, conflict-free
// ds_read_b128), double-buffered with one barrier per 64-deep K tile; the global loads of tile
// t+1 are issued before the MFMAs of tile t and written to LDS after them.
// The tile code is gemm_tile.hpp; the fused launches built on it are units of their own (gemm_ln.hip, ffn_ln.hip,
// gemm_bce.hip, dec_tail.hip).
#include <math.h>
#include "common.hpp"
#include "gemm_tile.hpp"
#include "gemm_checks.hpp"
#include "step_begin.hpp"
#include "shadows.hpp"

namespace mst {

template <typename T, int BM, int BN, int WGM, int WGN, bool C_F32, int BK, bool ROWOPS, int PATH, bool DROP, bool AU8 = false>
__global__ __launch_bounds__(WGM * WGN * 64) void gemm_nt_kernel(mst_gemm_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
  int64_t m0, n0;
  float bias_pre[8];
  gemm_bias_preload<BM, BN>(a, bias_pre);
  gemm_mainloop<T, BM, BN, WGM, WGN, BK, ROWOPS, AU8, false, PATH == 1 || PATH == 4>(a, smem, acc, m0, n0);  // (PATH 1, 4: whole tiles, whole K stages)
  // (the launch allocates max(K-loop tiles, BM x (BN+4) fp32 staging) bytes of LDS: launch_gemm)
  gemm_epilogue<T, BM, BN, WGM, WGN, C_F32, ROWOPS, PATH, DROP>(a, smem, acc, m0, n0, bias_pre);
}

// Two GEMMs of one kernel form in ONE launch (mst_gemm_nt_pair): the first `tiles0` workgroups are the first problem's tiles,
// the rest the second's. The piano-roll ends' two embedding GEMMs (model.py:81-91 and :241-245: the same uint8 frames against the
// encoder's and the decoder's table) — small launches whose cost is mostly the launch.
// n_begin > 0 (mst_gemm_nt_pair_begin): the first n_begin workgroups of the grid are the step's bookkeeping (step_begin.hpp).
template <typename T, int BM, int BN, int WGM, int WGN, int BK, int PATH>
__global__ __launch_bounds__(WGM * WGN * 64) void gemm_nt_pair_kernel(mst_gemm_args a0, mst_gemm_args a1, int tiles0, int tiles1, StepBegin sb,
                                                                       int n_begin) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if ((int)blockIdx.x < n_begin) {
    step_begin_wg<WGM * WGN * 64>(sb, (int)blockIdx.x, n_begin);
    return;
  }
  f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
  int64_t m0, n0;
  float bias_pre[8];
  const int64_t tile = (int64_t)blockIdx.x - n_begin;  // (n_begin is a multiple of 8: a tile keeps its XCD)
  if (tile >= tiles0 + tiles1) {
    // behind the GEMM tiles: the transposed 16-bit shadows of the matrices only the backward pass reads, rebuilt from the weights the
    // previous step's optimizer left (mst_step_begin_args.sh_*) — as a launch of their own behind the optimizer they cost 6.5 us
    shadow_tile_wg<T>(sb.sh_w, reinterpret_cast<T*>(sb.sh_wt16), sb.sh_desc, sb.sh_prefix, sb.sh_n_mat, tile - tiles0 - tiles1,
                      reinterpret_cast<float(*)[33]>(smem));
    return;
  }
  // (two straight-line copies of the tile, each reading its own argument block from the kernel arguments)
  if (tile < tiles0) {
    gemm_bias_preload<BM, BN>(a0, bias_pre, tile);
    gemm_mainloop<T, BM, BN, WGM, WGN, BK, true, true, false, true>(a0, smem, acc, m0, n0, tile);  // (whole tiles, whole K stages: host check)
    gemm_epilogue<T, BM, BN, WGM, WGN, false, true, PATH, false>(a0, smem, acc, m0, n0, bias_pre);
  } else {
    const int64_t bid = tile - tiles0;
    gemm_bias_preload<BM, BN>(a1, bias_pre, bid);
    gemm_mainloop<T, BM, BN, WGM, WGN, BK, true, true, false, true>(a1, smem, acc, m0, n0, bid);
    gemm_epilogue<T, BM, BN, WGM, WGN, false, true, PATH, false>(a1, smem, acc, m0, n0, bias_pre);
  }
}

// 128 x 128 tiles at THREE or four workgroups per CU: 32-deep K stages (32 KB) and the accumulators staged one 64-row block at
// a time (34 KB) instead of 64 KB + 68 KB. For launches of 513..768 tiles (the K | Q | V projections: 768) that is one
// resident round instead of a full one and a half-empty one at two per CU. Eligibility (gemm_3cu_form) as launch_gemm's fast
// form without dropout / row ops.
static bool gemm_3cu_form(const mst_gemm_args& a) {
  constexpr int BM = 128, BN = 128, BK = 32;
  const bool rowops = a.rowadd || a.grpadd || a.a_rows_per_group > 0 || a.c_rows_per_group > 0;
  return !a.c_f32 && !a.a_u8 && !rowops && a.dropout_p == 0.f && !a.self_resid && a.M % BM == 0 && a.N % BN == 0 && a.K % BK == 0 &&
         a.ldc % 8 == 0 && (uint64_t)a.M * (uint64_t)a.N < (1ull << 32) &&
         (!a.resid || (a.ldr % 8 == 0 && (uintptr_t)a.resid % 16 == 0)) && (!a.gate || (a.ldg % 8 == 0 && (uintptr_t)a.gate % 16 == 0));
}
template <typename T>
static int launch_gemm_3cu(const mst_gemm_args& a, hipStream_t s) {
  constexpr int BM = 128, BN = 128, BK = 32;
  const size_t lds_loop = (size_t)2 * (BM + BN) * BK * 2, lds_epi = (size_t)(BM / 2) * (BN + 4) * 4;
  const size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  hipLaunchKernelGGL((gemm_nt_kernel<T, BM, BN, 2, 2, false, BK, false, 4, false>), dim3((unsigned)((a.M / BM) * (a.N / BN))), dim3(256), lds, s, a);
  MST_CHECK_LAUNCH("gemm_nt_kernel");
  return MST_OK;
}

// every tile interior and every optional operand 16-byte friendly: the launch takes the kernel that holds only the fast row loop
template <int BM, int BN>
static bool gemm_fast_form(const mst_gemm_args& a) {
  const bool rowops = a.rowadd || a.grpadd || a.a_rows_per_group > 0 || a.c_rows_per_group > 0;
  const int64_t phys_rows = a.c_rows_per_group > 0 ? (a.M / a.c_rows_per_group + 1) * a.c_group_stride + a.c_group_offset : a.M;
  return !a.c_f32 && a.M % BM == 0 && a.N % BN == 0 && a.ldc % 8 == 0 &&
         (a.c_rows_per_group <= 0 || a.c_rows_per_group % BM == 0) &&
         (uint64_t)phys_rows * (uint64_t)a.N < (1ull << 32) &&
         (!a.resid || (a.ldr % 8 == 0 && (uintptr_t)a.resid % 16 == 0)) &&
         (!a.gate || (a.ldg % 8 == 0 && (uintptr_t)a.gate % 16 == 0)) &&
         (!rowops || (a.rowadd_period % BM == 0 && (!a.rowadd || (a.ldra % 4 == 0 && (uintptr_t)a.rowadd % 16 == 0)) &&
                      (!a.grpadd || (a.ldga % 4 == 0 && (uintptr_t)a.grpadd % 16 == 0))));
}

// The epilogue variant of a launch with BM x BN tiles and BK-deep stages:
// [row-ops][fast without dropout | fast with dropout | general 16-bit | general fp32], then [8], [9]: uint8 A, fast / general
// ("row ops" in the kernel choice: row-indexed adds or a row remap of A or C)
// (an epilogue finished in accumulator layout — 8-byte accesses, no LDS round trip — measured +4 us per step and was removed)
template <int BM, int BN, int BK>
static int gemm_variant(const mst_gemm_args& a) {
  const bool rowops = a.rowadd || a.grpadd || a.a_rows_per_group > 0 || a.c_rows_per_group > 0;
  const bool fast = gemm_fast_form<BM, BN>(a) && a.K % BK == 0;  // (the fast kernels' K loop is unguarded too)
  const bool drop = a.dropout_p > 0.f || a.self_resid;
  return a.a_u8 ? (fast ? 8 : 9) : (a.c_f32 ? 3 : (fast ? (drop ? 1 : 0) : 2)) + (rowops ? 4 : 0);
}

// THE choice of kernel for a valid mst_gemm_nt problem, from the arguments alone (no HIP call): tile * 16 + variant, the
// codes of mst_gemm_nt_form (include/mst_hip.h). mst_gemm_nt launches what this returns and decides nothing itself.
static int gemm_nt_form(const mst_gemm_args& a) {
  const int64_t big_tiles = cdiv(a.M, 128) * cdiv(a.N, 128);
  // Tile shape is second-order here: 64x64, 128x64, 64x128 and 128x128 tiles measured within 5 % of each other on
  // every GEMM of the step (time = 4.7 us fixed + 1.7 us per 8.4 MB of output + 4.2 us per 2.1 GFLOP: with K <= 1024
  // a tile's main loop is 2-16 stages of one exposed L2 round trip each, at 12 TB/s of L2->LDS traffic for the
  // K = 1024 shapes). 128x128 is used where it still leaves >= 1.5 workgroups per CU.
  // Two 128x128 workgroups fit a CU (LDS), 512 on the chip: a launch of 516 (the decoder's M = 64 x 257 rows: 129 row
  // tiles x 4) runs a second resident round for four workgroups — 21 us against 13 us with 64x64 tiles.
  const int64_t last_round = big_tiles % 512;
  const bool stub_round = big_tiles > 512 && last_round > 0 && last_round < 128;
  // (a launch whose rows are whole 64-row tiles but not whole 128-row tiles — the decoder's 64 x 257 — keeps the
  // fast-epilogue kernel with 64x64 tiles)
  const bool ragged128 = a.M % 128 != 0 && a.M % 64 == 0 && a.N % 128 == 0 && !a.c_f32;
  if (big_tiles > 512 && big_tiles <= 768 && a.N >= 128 && !ragged128 && gemm_3cu_form(a)) return 3 * 16;
  if (big_tiles >= 384 && a.N >= 128 && !stub_round && !ragged128) return 2 * 16 + gemm_variant<128, 128, 64>(a);
  if (a.M <= 64 && a.K >= 512 && a.K % 256 == 0) return 1 * 16 + gemm_variant<64, 64, 256>(a);
  // (32-deep K stages for launches of 1281..2048 64 x 64 tiles — eight workgroups per CU, one resident round for the decoder's
  // 257 x 6 projection tiles — measured no faster: +2 us per step)
  return gemm_variant<64, 64, 64>(a);
}

template <typename T, int BM, int BN, int WGM, int WGN, int BK = 64>
static int launch_gemm(const mst_gemm_args& a, int variant, hipStream_t s) {
  const int64_t tiles = cdiv(a.M, BM) * cdiv(a.N, BN);
  const size_t lds_loop = (size_t)2 * (BM + BN) * BK * 2, lds_epi = (size_t)BM * (BN + 4) * 4;
  const size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  dim3 grid((unsigned)tiles), block(WGM * WGN * 64);
  // kernels: [row-ops][fast without dropout | fast with dropout | general 16-bit | general fp32] (gemm_variant)
  typedef void (*kern_t)(mst_gemm_args);
  // [8], [9]: uint8 A operand (the piano-roll embedding GEMMs: row ops, 16-bit C, no dropout), fast / general
  const kern_t fns[10] = {&gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, false, 1, false>, &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, false, 1, true>,
                         &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, false, 2, true>, &gemm_nt_kernel<T, BM, BN, WGM, WGN, true, BK, false, 2, true>,
                         &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, true, 1, false>, &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, true, 1, true>,
                         &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, true, 2, true>, &gemm_nt_kernel<T, BM, BN, WGM, WGN, true, BK, true, 2, true>,
                         &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, true, 1, false, true>, &gemm_nt_kernel<T, BM, BN, WGM, WGN, false, BK, true, 2, false, true>};
  static size_t granted[10] = {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024};
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(fns[variant]), lds, &granted[variant], "gemm_nt_kernel")) return rc;
  hipLaunchKernelGGL(fns[variant], grid, block, lds, s, a);
  MST_CHECK_LAUNCH("gemm_nt_kernel");
  return MST_OK;
}

// what every launch built on these tiles asks of a GEMM's arguments (gemm_checks.hpp)
int check_gemm_common(const mst_gemm_args& a) {
  MST_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "mst_gemm_nt: M,N,K must be positive (got %lld,%lld,%lld)",
                (long long)a.M, (long long)a.N, (long long)a.K);
  MST_CHECK_ARG(a.K % 8 == 0 && a.lda % 8 == 0 && a.ldb % 8 == 0,
                "mst_gemm_nt: K, lda, ldb must be multiples of 8 (got %lld,%lld,%lld)", (long long)a.K,
                (long long)a.lda, (long long)a.ldb);
  MST_CHECK_ARG(a.A && a.B && a.C, "mst_gemm_nt: null operand");
  MST_CHECK_ARG(a.dropout_p >= 0.f && a.dropout_p < 1.f, "mst_gemm_nt: dropout_p must be in [0,1)");
  MST_CHECK_ARG(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.C % 16 == 0),
                "mst_gemm_nt: operands must be 16-byte aligned");
  return MST_OK;
}

}  // namespace mst

using namespace mst;

static int check_gemm_nt(const mst_gemm_args* args) {
  MST_CHECK_ARG(args != nullptr, "mst_gemm_nt: null args");
  const mst_gemm_args& a = *args;
  MST_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "mst_gemm_nt: M,N,K must be positive (got %lld,%lld,%lld)",
                (long long)a.M, (long long)a.N, (long long)a.K);
  MST_CHECK_ARG(a.K % 8 == 0 && a.lda % 8 == 0 && a.ldb % 8 == 0,
                "mst_gemm_nt: K, lda, ldb must be multiples of 8 (got %lld,%lld,%lld)", (long long)a.K,
                (long long)a.lda, (long long)a.ldb);
  MST_CHECK_ARG(a.ldc % 4 == 0 && a.ldc >= a.N, "mst_gemm_nt: ldc must be a multiple of 4 and >= N");
  MST_CHECK_ARG(a.A && a.B && a.C, "mst_gemm_nt: null operand");
  MST_CHECK_ARG(!a.resid || (a.ldr % 4 == 0 && a.ldr >= a.N), "mst_gemm_nt: ldr must be a multiple of 4 and >= N");
  MST_CHECK_ARG(!a.gate || (a.ldg % 4 == 0 && a.ldg >= a.N), "mst_gemm_nt: ldg must be a multiple of 4 and >= N");
  MST_CHECK_ARG((!a.rowadd && !a.grpadd) || a.rowadd_period > 0, "mst_gemm_nt: rowadd_period must be > 0");
  MST_CHECK_ARG(!a.grpadd || a.grp_index, "mst_gemm_nt: grpadd needs grp_index");
  MST_CHECK_ARG(a.dropout_p >= 0.f && a.dropout_p < 1.f, "mst_gemm_nt: dropout_p must be in [0,1)");
  MST_CHECK_ARG(a.dropout_p == 0.f || a.N % 4 == 0, "mst_gemm_nt: dropout needs N to be a multiple of 4");
  MST_CHECK_ARG(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.C % 16 == 0),
                "mst_gemm_nt: operands must be 16-byte aligned");
  MST_CHECK_ARG(!a.a_u8 || (!a.c_f32 && a.dropout_p == 0.f && !a.self_resid),
                "mst_gemm_nt: a uint8 A operand comes with a 16-bit C and without dropout / self_resid");
  if (a.dtype != MST_BF16 && a.dtype != MST_F16) return dispatch_act(a.dtype, [](auto) { return 0; });  // (its message and status)
  return MST_OK;
}

extern "C" int mst_gemm_nt_form(const mst_gemm_args* args) {
  const int rc = check_gemm_nt(args);
  return rc != MST_OK ? rc : gemm_nt_form(*args);
}

extern "C" int mst_gemm_nt(const mst_gemm_args* args, mst_stream_t stream) {
  const int rc = check_gemm_nt(args);
  if (rc != MST_OK) return rc;
  const mst_gemm_args& a = *args;
  const int form = gemm_nt_form(a), variant = form & 15;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    switch (form >> 4) {  // (the tile forms of gemm_nt_form)
      case 3: return launch_gemm_3cu<T>(a, s);
      case 2: return launch_gemm<T, 128, 128, 2, 2>(a, variant, s);
      case 1: return launch_gemm<T, 64, 64, 2, 2, 256>(a, variant, s);
      default: return launch_gemm<T, 64, 64, 2, 2>(a, variant, s);
    }
  });
}

extern "C" int mst_gemm_nt_pair(const mst_gemm_args* args0, const mst_gemm_args* args1, mst_stream_t stream) {
  return mst_gemm_nt_pair_begin(args0, args1, nullptr, stream);
}

extern "C" int mst_gemm_nt_pair_begin(const mst_gemm_args* args0, const mst_gemm_args* args1, const mst_step_begin_args* begin,
                                      mst_stream_t stream) {
  MST_CHECK_ARG(args0 != nullptr && args1 != nullptr, "mst_gemm_nt_pair: null args");
  const mst_gemm_args &a0 = *args0, &a1 = *args1;
  // one launch for two uint8-A problems of the fast row-op form (what the embedding GEMMs are); anything else is two launches
  // of mst_gemm_nt, which also reports what is wrong with an argument
  auto plain = [](const mst_gemm_args& a) {
    return a.a_u8 && !a.c_f32 && a.M > 0 && a.N > 0 && a.K > 0 && a.K % 8 == 0 && a.lda % 8 == 0 && a.ldb % 8 == 0 && a.ldc >= a.N &&
           a.A && a.B && a.C && (uintptr_t)a.A % 16 == 0 && (uintptr_t)a.B % 16 == 0 && (uintptr_t)a.C % 16 == 0 && !a.resid && !a.gate &&
           a.act == 0 && a.dropout_p == 0.f && !a.self_resid && ((!a.rowadd && !a.grpadd) || a.rowadd_period > 0) &&
           (!a.grpadd || a.grp_index) && gemm_fast_form<64, 64>(a) && a.K % 64 == 0 && cdiv(a.M, 64) * cdiv(a.N, 64) < (1 << 20);
  };
  if (a0.dtype != a1.dtype || !plain(a0) || !plain(a1) || (begin && begin->sh_w && begin->sh_dtype != a0.dtype)) {
    int rc = begin ? mst_step_begin(begin, stream) : MST_OK;  // (runs the shadow refresh as a launch of its own)
    if (rc == MST_OK) rc = mst_gemm_nt(args0, stream);
    return rc != MST_OK ? rc : mst_gemm_nt(args1, stream);
  }
  StepBegin sb = {};
  int n_begin = 0;
  if (begin) {
    int64_t grid = 0;
    int rc = pack_step_begin(*begin, sb, &grid);
    if (rc) return rc;
    if (begin->in_keep) {
      // a decoder-input dropout job: the decoder's problem reads the masked frames the bookkeeping writes, so the bookkeeping is a
      // launch of its own in front of this one (mst_step_begin(begin), then mst_gemm_nt_pair(args0, args1)) — whatever the caller
      // asked for. A shadow refresh stays behind this launch's tiles: nothing here reads or writes what it touches.
      mst_step_begin_args own = *begin;
      own.sh_w = nullptr;
      if ((rc = mst_step_begin(&own, stream)) != MST_OK) return rc;
      StepBegin sh = {};
      sh.sh_w = sb.sh_w; sh.sh_wt16 = sb.sh_wt16; sh.sh_desc = sb.sh_desc; sh.sh_prefix = sb.sh_prefix; sh.sh_n_mat = sb.sh_n_mat; sh.sh_tiles = sb.sh_tiles;
      sb = sh;
    } else {
      n_begin = (int)((grid + 7) / 8 * 8);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a0.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    const int64_t sh_tiles = sb.sh_w ? sb.sh_tiles : 0;
    // long contractions (configs[2]: 2048 pitch columns per frame): 128 x 128 tiles — the uint8 frames cross L2 -> LDS once per
    // 128 output columns instead of once per 64 (three times instead of six for the two tables), 33 K stages amortise the tile's
    // prologue and epilogue; at configs[1]'s K = 128 the 64 x 64 form stays (1 536 short tiles fill the chip, 384 long ones do not)
    if (a0.K >= 1024 && a1.K >= 1024 && gemm_fast_form<128, 128>(a0) && gemm_fast_form<128, 128>(a1)) {
      const int t0 = (int)((a0.M / 128) * (a0.N / 128)), t1 = (int)((a1.M / 128) * (a1.N / 128));
      const size_t lds_b = (size_t)2 * (128 + 128) * 64 * 2;  // (epilogue: one 64-row block of the tile at a time, PATH 4: 34 KB)
      static size_t granted = 64 * 1024;  // (these stages are exactly the 64 KB a kernel has without asking)
      if (const int rc = lds_opt_in(reinterpret_cast<const void*>(&gemm_nt_pair_kernel<T, 128, 128, 2, 2, 64, 4>), lds_b, &granted, "gemm_nt_pair_kernel")) return rc;
      hipLaunchKernelGGL((gemm_nt_pair_kernel<T, 128, 128, 2, 2, 64, 4>), dim3((unsigned)(n_begin + t0 + t1 + sh_tiles)), dim3(256), lds_b, s, a0, a1,
                         t0, t1, sb, n_begin);
      MST_CHECK_LAUNCH("gemm_nt_pair_kernel");
      return MST_OK;
    }
    const int tiles0 = (int)((a0.M / 64) * (a0.N / 64)), tiles1 = (int)((a1.M / 64) * (a1.N / 64));
    const size_t lds = (size_t)2 * (64 + 64) * 64 * 2;  // K-loop stages; the 64 x 68 fp32 epilogue staging is smaller
    hipLaunchKernelGGL((gemm_nt_pair_kernel<T, 64, 64, 2, 2, 64, 1>), dim3((unsigned)(n_begin + tiles0 + tiles1 + sh_tiles)), dim3(256), lds, s, a0,
                       a1, tiles0, tiles1, sb, n_begin);
    MST_CHECK_LAUNCH("gemm_nt_pair_kernel");
    return MST_OK;
  });
}

// row_tail.hip — the position-0 tail of the top encoder layer in ONE launch.
//
// The model reads the encoder at position 0 only (VarAutoEncoder/model.py:97), so after the attention mix the top layer's
//     h1 = x_in + dropout(att W_proj^T + b)        x1 = LN1(h1)                         (transformer.py:154-155)
//     a  = dropout(relu(x1 W1^T + b1))             h2 = x1 + dropout(a W2^T + b2)       (transformer.py:42-46,157)
//     x2 = LN2(h2)                                                                        (transformer.py:158)
// run on B rows (one per sample): microseconds of arithmetic that used to be five launches of ~9 us each, every one a
// dependent launch boundary plus a cold fetch of its weights. Here the chain is one launch of G = D / 16 workgroups that
// each own a slice of every GEMM's OUTPUT columns (so every workgroup streams 1/G of every weight matrix, once) and meet
// at three grid-wide barriers where the chain needs whole rows: after W_proj (LayerNorm 1 needs the row), after FFN1 (FFN2
// contracts over the whole hidden row), after FFN2 (LayerNorm 2). Rows travel between the stages through HBM/L2 (they
// are the tensors the backward pass reads anyway); the LayerNorms are computed where they are consumed. 64 x 256 x
// (256 + 1024 + 1024) MACs spread over 16 CUs is ~1 us of MFMA; the launch is three barrier latencies plus four L2 round
// trips. Arithmetic, rounding points and dropout counters are those of mst_gemm_nt / mst_layernorm_fwd on the same rows
// (counter = physical row * N + column), so the backward pass regenerates the same masks.
//
// One translation unit, kernels in headers: row_tail.hpp (what both kernels share: how rows cross a grid barrier — ONE claimed
// XCD, write-through stores to its L2, first-touch loads behind the barrier — the join, the riders, the row helpers),
// row_tail_fwd.hpp and row_tail_bwd.hpp (a kernel each). This file is the host side: the form query, the two launches and
// the entry points. (One unit on purpose: tail_shadow_ticket is reached from both kernels, and what the compiler makes of
// them depends on which share its module — docs/kernel_notes.md.)
#include "row_tail.hpp"
#include "row_tail_fwd.hpp"
#include "row_tail_bwd.hpp"

using namespace mst;

#ifdef MST_TAIL_STAMPS
extern "C" int mst_debug_tail_stamps(uint32_t* host_out) {  // diagnostic builds only: 32 realtime stamps of the last tail launch
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mst::g_tail_stamps), sizeof(uint32_t) * 32) == hipSuccess ? 0 : -1;
}
#endif

// a rider GEMM: what tail_ride's tile code takes — whole 128 x 128 tiles, 64-deep K stages, the fast epilogue (16-bit C, bias and / or
// residual, row remaps whose groups are whole tiles)
static int check_rider(const char* who, const mst_gemm_args& g, int dtype) {
  MST_CHECK_ARG(g.dtype == dtype && g.M > 0 && g.N > 0 && g.K > 0 && g.A && g.B && g.C, "%s: rider: bad GEMM", who);
  MST_CHECK_ARG(g.M % 128 == 0 && g.N % 128 == 0 && g.K % 64 == 0 && g.lda % 8 == 0 && g.ldb % 8 == 0 && g.ldc % 8 == 0 && g.M * (g.N / 128) < (1ll << 30),
                "%s: rider: M and N must be multiples of 128, K of 64 (got %lld, %lld, %lld)", who, (long long)g.M, (long long)g.N, (long long)g.K);
  MST_CHECK_ARG(!g.c_f32 && !g.a_u8 && !g.gate && !g.rowadd && !g.grpadd && g.act == MST_ACT_NONE && g.dropout_p == 0.f && !g.self_resid,
                "%s: rider: bias, alpha, a residual and row remaps only", who);
  MST_CHECK_ARG((g.a_rows_per_group <= 0 || g.a_rows_per_group % 128 == 0) && (g.c_rows_per_group <= 0 || g.c_rows_per_group % 128 == 0),
                "%s: rider: row-remap groups must be whole 128-row tiles", who);
  const int64_t phys_rows = g.c_rows_per_group > 0 ? (g.M / g.c_rows_per_group) * g.c_group_stride + g.c_group_offset : g.M;
  MST_CHECK_ARG((uint64_t)phys_rows * (uint64_t)g.N < (1ull << 32) && (!g.resid || (g.ldr % 8 == 0 && (uintptr_t)g.resid % 16 == 0)) &&
                ((uintptr_t)g.A | (uintptr_t)g.B | (uintptr_t)g.C) % 16 == 0 && (!g.bias || (uintptr_t)g.bias % 16 == 0),
                "%s: rider: operands must be 16-byte aligned and the output below 2^32 elements", who);
  return MST_OK;
}
// Grid of a launch with riders: G x over workgroups dealt round-robin over the 8 XCDs, 7/8 of them riders. As few as give every
// tile a rider of its own (+ one per XCD to spare), at most 16 x G: the launch pays ~0.6 us per 16 extra 1024-thread workgroups
// (measured: a one-tile rider costs the forward tail +0.6 / +1.3 / +3.5 us at over = 9 / 12 / 16).
static unsigned ride_grid(int64_t G, int tiles) {
  int64_t over = (((int64_t)tiles * 8 + 6) / 7 + G - 1) / G + 1;
  if (over < 9) over = 9;
  if (over > 16) over = 16;
  return (unsigned)(G * over);
}
// (tile rows, dynamic LDS) of a rider: 256-row tiles when the 128-row ones would need a second round of the ~7 x 32 riding workgroups
static void ride_shape(const mst_gemm_args& g, int& tiles_signed, size_t& lds) {
  const int64_t t128 = (g.M / 128) * (g.N / 128);
  const bool big = t128 > 7 * 32 - 16 && g.M % 256 == 0 && (g.a_rows_per_group <= 0 || g.a_rows_per_group % 256 == 0) &&
                   (g.c_rows_per_group <= 0 || g.c_rows_per_group % 256 == 0);
  if (big) { tiles_signed = -(int)((g.M / 256) * (g.N / 128)); lds = (size_t)2 * (256 + 128) * 64 * 2; }  // (the split epilogue stages 64 rows: 34 KB)
  else { tiles_signed = (int)t128; lds = (size_t)128 * (128 + 4) * 4; }  // the epilogue's fp32 staging tile (> the 64 KB of the two K stages)
  // (negative: 256-row tiles)
}

// What a valid call launches (the entries of mst_row_tail_form, include/mst_hip.h): kernel index = (D == 256 ? 0 : 1) + (no rider: 0,
// 128-row rider tiles: 2, 256-row: 4) in both directions. The launches below validate their arguments and take everything else from here.
struct TailForm { int kernel, ride_rows, tiles; unsigned grid; size_t lds; int tickets; };
static int tail_form_common(const char* who, const char* who_ride, int dtype, int64_t D, const mst_gemm_args* rider, TailForm& f) {
  MST_CHECK_ARG(D == 128 || D == 256, "%s: width must be 128 or 256 (got %lld)", who, (long long)D);
  if (const int rc = dispatch_act(dtype, [](auto) -> int { return MST_OK; })) return rc;  // (another type: the launch's own refusal)
  f = TailForm{D == 256 ? 0 : 1, 0, 0, (unsigned)((D / 16) * TAIL_OVERSUBSCRIBE), 0, 0};
  if (rider) {
    if (const int rc = check_rider(who_ride, *rider, dtype)) return rc;
    int tiles;
    ride_shape(*rider, tiles, f.lds);
    f.ride_rows = tiles < 0 ? 256 : 128;
    f.tiles = tiles < 0 ? -tiles : tiles;
    f.kernel += tiles < 0 ? 4 : 2;
    f.grid = ride_grid(D / 16, f.tiles);
  }
  return MST_OK;
}
static int row_tail_fwd_form(int dtype, int64_t D, const mst_gemm_args* rider, int64_t sh_tiles, TailForm& f) {
  if (const int rc = tail_form_common("mst_row_tail_fwd", "mst_row_tail_fwd_ride", dtype, D, rider, f)) return rc;
  MST_CHECK_ARG(sh_tiles == 0 || (rider && sh_tiles > 0 && sh_tiles < (1ll << 30)), "mst_row_tail_fwd_ride_shadows: shadow tiles need a rider (got %lld)",
                (long long)sh_tiles);
  f.tickets = (int)((sh_tiles + 15) / 16);  // sixteen shadow tiles per ticket
  if (f.tickets > 0 && f.lds < (size_t)16 * 32 * 33 * 4) f.lds = (size_t)16 * 32 * 33 * 4;
  return MST_OK;
}
static int row_tail_bwd_form(int dtype, int64_t D, const mst_gemm_args* rider, TailForm& f) {
  if (const int rc = tail_form_common("mst_row_tail_bwd", "mst_row_tail_bwd_ride", dtype, D, rider, f)) return rc;
  // (a workgroup is a participant or a rider: one region)
  const size_t lds = (size_t)2 * 64 * ((size_t)D + 8) * 2 + (size_t)16 * 2 * D * 4 + (size_t)4 * 64 * 16 * 4 + (size_t)2 * D * 4;
  if (lds > f.lds) f.lds = lds;
  return MST_OK;
}
extern "C" int mst_row_tail_form(int backward, int dtype, int64_t D, const mst_gemm_args* rider, int64_t sh_tiles, int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_row_tail_form: null form");
  MST_CHECK_ARG(!backward || sh_tiles == 0, "mst_row_tail_form: the backward tail takes no shadow tiles");
  TailForm f;
  if (const int rc = backward ? row_tail_bwd_form(dtype, D, rider, f) : row_tail_fwd_form(dtype, D, rider, sh_tiles, f)) return rc;
  form[0] = f.kernel; form[1] = f.ride_rows; form[2] = f.tiles; form[3] = f.grid; form[4] = (int64_t)f.lds; form[5] = f.tickets;
  return MST_OK;
}

static int row_tail_fwd_impl(const mst_row_tail_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream,
                             const TailShadow& shadow = TailShadow{}) {
  MST_CHECK_ARG(args != nullptr, "mst_row_tail_fwd: null args");
  const mst_row_tail_args& q = *args;
  MST_CHECK_ARG(q.B > 0 && q.B <= 64, "mst_row_tail_fwd: 1..64 rows (got %lld)", (long long)q.B);
  MST_CHECK_ARG(q.att && q.resid && q.Wp && q.bp && q.g1 && q.be1 && q.W1 && q.b1 && q.W2 && q.b2 && q.g2 && q.be2 && q.h1 && q.x1 && q.a &&
                q.h2 && q.x2 && q.mean1 && q.rstd1 && q.mean2 && q.rstd2 && q.sync, "mst_row_tail_fwd: null pointer");
  MST_CHECK_ARG(q.rs_att % 8 == 0 && q.rs_res % 8 == 0 && q.rs_d % 8 == 0 && q.rs_a % 8 == 0 && q.ldwp % 8 == 0 && q.ldw1 % 8 == 0 &&
                q.ldw2 % 8 == 0, "mst_row_tail_fwd: strides must be multiples of 8 elements");
  MST_CHECK_ARG((((uintptr_t)q.att | (uintptr_t)q.resid | (uintptr_t)q.Wp | (uintptr_t)q.W1 | (uintptr_t)q.W2 | (uintptr_t)q.h1 | (uintptr_t)q.x1 |
                  (uintptr_t)q.a | (uintptr_t)q.h2 | (uintptr_t)q.x2 | (uintptr_t)q.bp | (uintptr_t)q.b1 | (uintptr_t)q.b2) % 16) == 0,
                "mst_row_tail_fwd: operands must be 16-byte aligned");
  MST_CHECK_ARG(q.dropout_p >= 0.f && q.dropout_p < 1.f && q.phys_stride > 0 && q.stat_stride > 0, "mst_row_tail_fwd: bad dropout / strides");
  TailForm f;
  if (const int rc = row_tail_fwd_form(q.dtype, q.D, rider, shadow.tiles, f)) return rc;
  TailShadow sh = shadow;
  sh.n_groups = f.tickets;
  hipStream_t s = (hipStream_t)stream;
  const mst_gemm_args none = {};
  return dispatch_act(q.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    typedef void (*kern_t)(mst_row_tail_args, mst_gemm_args, int, uint32_t*, TailShadow);
    const kern_t fns[6] = {&row_tail_fwd_kernel<T, 256>,      &row_tail_fwd_kernel<T, 128>,      &row_tail_fwd_kernel<T, 256, 128>,
                           &row_tail_fwd_kernel<T, 128, 128>, &row_tail_fwd_kernel<T, 256, 256>, &row_tail_fwd_kernel<T, 128, 256>};
    static size_t granted[6] = {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024};
    if (const int rc = lds_opt_in(reinterpret_cast<const void*>(fns[f.kernel]), f.lds, &granted[f.kernel], "row_tail_fwd_kernel (riders)")) return rc;
    hipLaunchKernelGGL(fns[f.kernel], dim3(f.grid), dim3(1024), f.lds, s, q, rider ? *rider : none, f.tiles, rider ? queue : (uint32_t*)nullptr, sh);
    MST_CHECK_LAUNCH("row_tail_fwd_kernel");
    return MST_OK;
  });
}
extern "C" int mst_row_tail_fwd(const mst_row_tail_args* args, mst_stream_t stream) { return row_tail_fwd_impl(args, nullptr, nullptr, stream); }
extern "C" int mst_row_tail_fwd_ride(const mst_row_tail_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream) {
  MST_CHECK_ARG(rider != nullptr && queue != nullptr, "mst_row_tail_fwd_ride: null rider / queue word");
  return row_tail_fwd_impl(args, rider, queue, stream);
}
extern "C" int mst_row_tail_fwd_ride_shadows(const mst_row_tail_args* args, const mst_gemm_args* rider, uint32_t* queue, int sh_dtype,
                                             const float* sh_w, void* sh_wt16, const int64_t* sh_desc, const int64_t* sh_prefix, int64_t sh_n_mat,
                                             int64_t sh_tiles, mst_stream_t stream) {
  MST_CHECK_ARG(args != nullptr && rider != nullptr && queue != nullptr, "mst_row_tail_fwd_ride_shadows: null args / rider / queue word");
  MST_CHECK_ARG(sh_w && sh_wt16 && sh_desc && sh_prefix && sh_n_mat > 0 && sh_tiles > 0 && sh_tiles < (1ll << 30) && sh_dtype == args->dtype,
                "mst_row_tail_fwd_ride_shadows: bad shadow list (mst_transpose_shadows' arguments, in the tail's activation type)");
  TailShadow sh;
  sh.w = sh_w; sh.wt16 = sh_wt16; sh.desc = sh_desc; sh.prefix = sh_prefix; sh.n_mat = (int)sh_n_mat; sh.tiles = sh_tiles;
  sh.n_groups = 0;  // (row_tail_fwd_form: the tickets)
  return row_tail_fwd_impl(args, rider, queue, stream, sh);
}

static int row_tail_bwd_impl(const mst_row_tail_bwd_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream) {
  MST_CHECK_ARG(args != nullptr, "mst_row_tail_bwd: null args");
  const mst_row_tail_bwd_args& q = *args;
  MST_CHECK_ARG(q.B > 0 && q.B <= 64, "mst_row_tail_bwd: 1..64 rows (got %lld)", (long long)q.B);
  MST_CHECK_ARG(q.dy && q.h2 && q.h1 && q.a && q.mean1 && q.rstd1 && q.mean2 && q.rstd2 && q.g1 && q.g2 && q.W2t && q.W1t && q.Wpt && q.dh &&
                q.dhm && q.dx1 && q.dh1m && q.dpre && q.dh1 && q.datt && q.dg1 && q.db1 && q.dg2 && q.db2 && q.sync, "mst_row_tail_bwd: null pointer");
  MST_CHECK_ARG(q.rs_dy % 8 == 0 && q.rs_d % 8 == 0 && q.rs_a % 8 == 0 && q.rs_c % 8 == 0 && q.rs_dpre % 8 == 0 && q.rs_dh1 % 8 == 0 &&
                q.rs_datt % 8 == 0 && q.ldw2t % 8 == 0 && q.ldw1t % 8 == 0 && q.ldwpt % 8 == 0, "mst_row_tail_bwd: strides must be multiples of 8 elements");
  MST_CHECK_ARG((((uintptr_t)q.dy | (uintptr_t)q.h2 | (uintptr_t)q.h1 | (uintptr_t)q.a | (uintptr_t)q.W2t | (uintptr_t)q.W1t | (uintptr_t)q.Wpt |
                  (uintptr_t)q.dh | (uintptr_t)q.dhm | (uintptr_t)q.dx1 | (uintptr_t)q.dh1m | (uintptr_t)q.dpre | (uintptr_t)q.dh1 | (uintptr_t)q.datt) % 16) == 0,
                "mst_row_tail_bwd: operands must be 16-byte aligned");
  MST_CHECK_ARG(q.dropout_p >= 0.f && q.dropout_p < 1.f && q.phys_stride > 0 && q.stat_stride > 0, "mst_row_tail_bwd: bad dropout / strides");
  TailForm f;
  if (const int rc = row_tail_bwd_form(q.dtype, q.D, rider, f)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const mst_gemm_args none = {};
  return dispatch_act(q.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    static size_t granted[6] = {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024};
    typedef void (*kern_t)(mst_row_tail_bwd_args, mst_gemm_args, int, uint32_t*);
    const kern_t fns[6] = {&row_tail_bwd_kernel<T, 256>, &row_tail_bwd_kernel<T, 128>, &row_tail_bwd_kernel<T, 256, 128>, &row_tail_bwd_kernel<T, 128, 128>,
                           &row_tail_bwd_kernel<T, 256, 256>, &row_tail_bwd_kernel<T, 128, 256>};
    if (const int rc = lds_opt_in(reinterpret_cast<const void*>(fns[f.kernel]), f.lds, &granted[f.kernel], "row_tail_bwd_kernel")) return rc;
    hipLaunchKernelGGL(fns[f.kernel], dim3(f.grid), dim3(1024), f.lds, s, q, rider ? *rider : none, f.tiles, rider ? queue : (uint32_t*)nullptr);
    MST_CHECK_LAUNCH("row_tail_bwd_kernel");
    return MST_OK;
  });
}
extern "C" int mst_row_tail_bwd(const mst_row_tail_bwd_args* args, mst_stream_t stream) { return row_tail_bwd_impl(args, nullptr, nullptr, stream); }
extern "C" int mst_row_tail_bwd_ride(const mst_row_tail_bwd_args* args, const mst_gemm_args* rider, uint32_t* queue, mst_stream_t stream) {
  MST_CHECK_ARG(rider != nullptr && queue != nullptr, "mst_row_tail_bwd_ride: null rider / queue word");
  return row_tail_bwd_impl(args, rider, queue, stream);
}

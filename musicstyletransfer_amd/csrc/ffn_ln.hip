// ffn_ln.hip — the feed-forward block of a Transformer layer in one launch (ffn_ln.hpp: ffn_ln_body, where the design is described):
// mst_ffn_ln_fwd / mst_ffn_ln_bwd, with the attention output projection in front (mst_proj_ffn_ln_fwd) or the layer's leading LayerNorm
// backward in front (mst_ffn_ln_bwd_lead), and with the K | Q | V input gradient of the layer above in front of that (mst_kqv_ffn_ln_bwd).
#include "ffn_ln.hpp"
#include "gemm_checks.hpp"

namespace mst {

template <typename T, int BN, int WGM, int WGN, int MODE, bool LEAD, bool FULL, bool EXTRA = false>
__global__ __launch_bounds__(WGM * WGN * 64) void ffn_ln_kernel(mst_gemm_args g1, mst_gemm_args g2, mst_ln_args ln, mst_ln_bwd_in lead,
                                                                mst_gemm_args gx, mst_ln_args lnx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  ffn_ln_body<T, BN, WGM, WGN, MODE, LEAD, FULL, EXTRA>(smem, g1, g2, ln, lead, gx, lnx, nullptr, [] {});
}

template <typename T, int BN>
static int launch_ffn_ln(const mst_gemm_args& g1, const mst_gemm_args& g2, const mst_ln_args& ln, const mst_ln_bwd_in* lead, hipStream_t s,
                         const mst_gemm_args* gx = nullptr, const mst_ln_args* lnx = nullptr) {
  constexpr int BM = 64;
  const int ex = gx ? 1 : 0;
  const size_t lds_loop = (size_t)2 * BN * 64 * 2 + (size_t)2 * BM * (BN + 8) * 2 + (size_t)g1.N * 4 + (size_t)6 * BN * 4;
  const size_t lds_epi = (size_t)BM * (BN + 4) * 4;
  const size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  const int full = g1.M % BM == 0 ? 1 : 0;
  // [forward | backward | backward with the leading LayerNorm] x [row guards | whole tiles], then the forward form with the projection
  // head, then the backward form with the leading LayerNorm and the K | Q | V dgrad head
  const int mi = ex ? (ln.mode == 2 ? 8 : 6) + full : (lead ? 2 : (ln.mode == 2 ? 1 : 0)) * 2 + full;
  typedef void (*kern_t)(mst_gemm_args, mst_gemm_args, mst_ln_args, mst_ln_bwd_in, mst_gemm_args, mst_ln_args);
  const kern_t fns[10] = {&ffn_ln_kernel<T, BN, 2, 4, 1, false, false>, &ffn_ln_kernel<T, BN, 2, 4, 1, false, true>,
                         &ffn_ln_kernel<T, BN, 2, 4, 2, false, false>, &ffn_ln_kernel<T, BN, 2, 4, 2, false, true>,
                         &ffn_ln_kernel<T, BN, 2, 4, 2, true, false>, &ffn_ln_kernel<T, BN, 2, 4, 2, true, true>,
                         &ffn_ln_kernel<T, BN, 2, 4, 1, false, false, true>, &ffn_ln_kernel<T, BN, 2, 4, 1, false, true, true>,
                          &ffn_ln_kernel<T, BN, 2, 4, 2, true, false, true>, &ffn_ln_kernel<T, BN, 2, 4, 2, true, true, true>};
  static size_t granted[10] = {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024};
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(fns[mi]), lds, &granted[mi], "ffn_ln_kernel")) return rc;
  const mst_ln_bwd_in none = {};
  const mst_gemm_args no_gemm = {};
  const mst_ln_args no_ln = {};
  hipLaunchKernelGGL(fns[mi], dim3((unsigned)cdiv(g1.M, BM)), dim3(512), lds, s, g1, g2, ln, lead ? *lead : none,
                     gx ? *gx : no_gemm, lnx ? *lnx : no_ln);
  MST_CHECK_LAUNCH("ffn_ln_kernel");
  return MST_OK;
}

// the argument checks of the feed-forward block's launches (no HIP call)
int check_ffn_ln(const char* who, const mst_gemm_args* first, const mst_gemm_args* second, const mst_ln_args* ln, int mode,
                 const mst_ln_bwd_in* lead, const mst_gemm_args* extra, const mst_ln_args* extra_ln) {
  MST_CHECK_ARG(first != nullptr && second != nullptr && ln != nullptr, "%s: null args", who);
  const mst_gemm_args& a = *first;
  const mst_gemm_args& b = *second;
  const mst_ln_args& l = *ln;
  int rc = check_gemm_common(a);
  if (rc) return rc;
  rc = check_gemm_common(b);
  if (rc) return rc;
  MST_CHECK_ARG(a.dtype == b.dtype && a.M == b.M, "%s: the two GEMMs must share dtype and M", who);
  MST_CHECK_ARG((b.N == 256 || b.N == 128) && a.K == b.N, "%s: the model width (first K = second N) must be 128 or 256 (got %lld, %lld)", who,
                (long long)a.K, (long long)b.N);
  MST_CHECK_ARG(a.N == b.K && a.N % b.N == 0, "%s: the hidden width (first N = second K) must be a multiple of the model width", who);
  MST_CHECK_ARG(b.A == a.C && b.lda == a.ldc, "%s: the second GEMM's A operand must be the first one's output (it is consumed on chip)", who);
  MST_CHECK_ARG(!a.c_f32 && !b.c_f32 && !b.gate && !a.rowadd && !b.rowadd && !a.grpadd && !b.grpadd && !a.resid && !a.self_resid &&
                b.act == MST_ACT_NONE && a.c_rows_per_group <= 0 && b.a_rows_per_group <= 0 && b.c_rows_per_group <= 0,
                "%s: fp32 outputs, row-indexed adds, row remaps, a gate or activation on the second GEMM and a residual on the first are not supported", who);
  // ... except the first GEMM's A remap, which stands for the whole block: its M rows are rows [offset, offset + rows_per_group)
  // of every `stride` physical rows, in every operand of the launch (groups and M in whole 64-row tiles)
  MST_CHECK_ARG(a.a_rows_per_group <= 0 || (a.a_rows_per_group % 64 == 0 && a.M % a.a_rows_per_group == 0 && a.a_group_offset >= 0 &&
                                            a.a_group_stride >= a.a_rows_per_group + a.a_group_offset && a.M < (1ll << 31)),
                "%s: row groups must be whole 64-row tiles (rows per group %lld, stride %lld, offset %lld, M %lld)", who,
                (long long)a.a_rows_per_group, (long long)a.a_group_stride, (long long)a.a_group_offset, (long long)a.M);
  MST_CHECK_ARG(a.lda % 8 == 0 && a.ldc % 8 == 0 && a.ldc >= a.N && b.ldc % 8 == 0 && b.ldc >= b.N, "%s: leading dimensions must be multiples of 8", who);
  MST_CHECK_ARG((uint64_t)a.N * (uint64_t)a.ldb < (1ull << 32) && (uint64_t)b.N * (uint64_t)b.ldb < (1ull << 32), "%s: weight matrices too large", who);
  MST_CHECK_ARG(!b.resid || (b.ldr % 8 == 0 && b.ldr >= b.N && (uintptr_t)b.resid % 16 == 0), "%s: bad residual layout", who);
  MST_CHECK_ARG(!a.bias || (uintptr_t)a.bias % 16 == 0, "%s: the first GEMM's bias must be 16-byte aligned", who);
  MST_CHECK_ARG(a.dropout_p == 0.f || a.N % 4 == 0, "%s: dropout needs widths that are multiples of 4", who);
  MST_CHECK_ARG(l.mode == mode && l.gamma && l.mean && l.rstd, "%s: LayerNorm arguments of the wrong form", who);
  if (mode == 1) {
    MST_CHECK_ARG(!a.gate, "%s: a gate belongs to the backward form", who);
    MST_CHECK_ARG(l.beta && l.out && l.ld_out % 8 == 0 && l.ld_out >= b.N && (uintptr_t)l.out % 16 == 0,
                  "%s: the LayerNorm arguments are those of mst_gemm_nt_ln's forward form", who);
  } else {
    MST_CHECK_ARG(a.gate && a.ldg % 8 == 0 && a.ldg >= a.N && (uintptr_t)a.gate % 16 == 0, "%s: the first GEMM needs the forward activation as its gate", who);
    MST_CHECK_ARG(a.act == MST_ACT_NONE && a.dropout_p == 0.f && !b.self_resid, "%s: activation / dropout / self_resid belong to the forward form", who);
    MST_CHECK_ARG(l.x && l.ld_x % 8 == 0 && (uintptr_t)l.x % 16 == 0 && (l.partials || (l.dgamma && l.dbeta)) && (uintptr_t)l.partials % 16 == 0,
                  "%s: backward needs x and dgamma + dbeta (or partials)", who);
    MST_CHECK_ARG(l.mask_mode >= 0 && l.mask_mode <= 2 &&
                  (l.mask_mode != 1 || (l.out && l.ld_out % 8 == 0 && l.ld_out >= b.N && (uintptr_t)l.out % 16 == 0)),
                  "%s: mask_mode must be 0, 1 (with out) or 2", who);
  }
  if (lead) {
    const mst_ln_bwd_in& q = *lead;
    MST_CHECK_ARG(mode == 2, "%s: a leading LayerNorm belongs to the backward form", who);
    const bool dy_on_chip = extra != nullptr;  // (the head computes dy: q.dy is not read)
    MST_CHECK_ARG((q.dy || dy_on_chip) && q.x && q.gamma && q.mean && q.rstd && q.dx && (q.partials || (q.dgamma && q.dbeta)),
                  "%s: leading LayerNorm: null pointer", who);
    MST_CHECK_ARG((dy_on_chip || (q.ld_dy % 8 == 0 && q.ld_dy >= b.N)) && q.ld_x % 8 == 0 && q.ld_dx % 8 == 0 && q.ld_x >= b.N && q.ld_dx >= b.N &&
                  ((uintptr_t)q.dy | (uintptr_t)q.x | (uintptr_t)q.dx | (uintptr_t)q.partials) % 16 == 0, "%s: leading LayerNorm: bad layout", who);
    MST_CHECK_ARG(q.mask_mode == 0 || (q.mask_mode == 1 && q.dx_masked && q.ld_dxm % 8 == 0 && q.ld_dxm >= b.N && (uintptr_t)q.dx_masked % 16 == 0),
                  "%s: leading LayerNorm: mask_mode must be 0 or 1 (with dx_masked)", who);
    MST_CHECK_ARG(q.dropout_p >= 0.f && q.dropout_p < 1.f, "%s: leading LayerNorm: dropout_p must be in [0,1)", who);
    const void* tile = q.mask_mode == 1 ? q.dx_masked : q.dx;
    const int64_t tile_ld = q.mask_mode == 1 ? q.ld_dxm : q.ld_dx;
    MST_CHECK_ARG(a.A == tile && a.lda == tile_ld, "%s: the first GEMM's A operand must be the leading LayerNorm's (masked) output", who);
  }
  if (extra && mode == 2) {
    // the K | Q | V dgrad head: mst_kqv_ffn_ln_bwd takes this path only with a head its form rule accepted (kqv_head_form: shape,
    // layout, a residual and no other epilogue feature) — nothing is left to check here
  } else if (extra) {
    const mst_gemm_args& x = *extra;
    rc = check_gemm_common(x);
    if (rc) return rc;
    MST_CHECK_ARG(x.dtype == a.dtype && x.M == a.M && x.N == b.N && x.K == b.N, "%s: the extra GEMM is width x width on the same rows", who);
    MST_CHECK_ARG(!x.c_f32 && !x.gate && !x.rowadd && !x.grpadd && x.act == MST_ACT_NONE && x.a_rows_per_group <= 0 && x.c_rows_per_group <= 0 &&
                  x.ldc % 8 == 0 && x.ldc >= x.N && (uint64_t)x.N * (uint64_t)x.ldb < (1ull << 32),
                  "%s: the extra GEMM takes no gate, activation, row-indexed add or row remap", who);
    MST_CHECK_ARG(mode == 1 && extra_ln != nullptr, "%s: the projection (with its LayerNorm) rides in front of the forward form", who);
    const mst_ln_args& q = *extra_ln;
    MST_CHECK_ARG(q.mode == 1 && q.gamma && q.beta && q.mean && q.rstd && q.out == a.A && q.ld_out == a.lda,
                  "%s: the leading LayerNorm's output must be the first GEMM's A operand", who);
    MST_CHECK_ARG(!x.resid || (x.ldr % 8 == 0 && x.ldr >= x.N && (uintptr_t)x.resid % 16 == 0), "%s: bad residual layout", who);
  }
  return MST_OK;
}

}  // namespace mst

using namespace mst;

static int ffn_ln_impl(const char* who, const mst_gemm_args* first, const mst_gemm_args* second, const mst_ln_args* ln, int mode,
                       mst_stream_t stream, const mst_ln_bwd_in* lead = nullptr, const mst_gemm_args* extra = nullptr,
                       const mst_ln_args* extra_ln = nullptr) {
  const int rc = check_ffn_ln(who, first, second, ln, mode, lead, extra, extra_ln);
  if (rc) return rc;
  const mst_gemm_args &a = *first, &b = *second;
  const mst_ln_args& l = *ln;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_act(a.dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    if (b.N == 256) return launch_ffn_ln<T, 256>(a, b, l, lead, s, extra, extra_ln);
    return launch_ffn_ln<T, 128>(a, b, l, lead, s, extra, extra_ln);
  });
}

extern "C" int mst_proj_ffn_ln_fwd(const mst_gemm_args* proj, const mst_ln_args* ln1, const mst_gemm_args* ff1, const mst_gemm_args* ff2,
                                   const mst_ln_args* ln2, mst_stream_t stream) {
  MST_CHECK_ARG(proj != nullptr && ln1 != nullptr, "mst_proj_ffn_ln_fwd: null args");
  return ffn_ln_impl("mst_proj_ffn_ln_fwd", ff1, ff2, ln2, 1, stream, nullptr, proj, ln1);
}

extern "C" int mst_ffn_ln_bwd_lead(const mst_ln_bwd_in* lead, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                                   const mst_ln_args* ln, mst_stream_t stream) {
  MST_CHECK_ARG(lead != nullptr, "mst_ffn_ln_bwd_lead: null args");
  return ffn_ln_impl("mst_ffn_ln_bwd_lead", ff2_dgrad, ff1_dgrad, ln, 2, stream, lead);
}

// mst_kqv_ffn_ln_bwd: does the K | Q | V input gradient run as the head of the feed-forward backward launch (1), or as the GEMM
// launch in front of mst_ffn_ln_bwd_lead (0)? From the arguments alone (pointers: NULL and alignment only); the one decision the
// launch and mst_kqv_ffn_ln_bwd_form share. The head exists for the plain K = 3 width dgrad with a residual on whole-width rows:
// anything mst_gemm_nt would do beyond that (a bias, alpha, a gate, row-indexed adds, remaps, an fp32 or 4-column-aligned C, a
// residual it would read element by element) keeps the GEMM launch.
static int kqv_head_form(const mst_gemm_args& x, const mst_gemm_args& a, const mst_gemm_args& b) {
  const bool shape = (b.N == 256 || b.N == 128) && x.N == b.N && x.K == 3 * b.N && x.M == a.M && x.dtype == a.dtype;
  const bool plain = !x.c_f32 && !x.a_u8 && !x.bias && !x.gate && !x.rowadd && !x.grpadd && x.act == MST_ACT_NONE && x.alpha == 1.f &&
                     x.dropout_p == 0.f && !x.self_resid && x.a_rows_per_group <= 0 && x.c_rows_per_group <= 0 && a.a_rows_per_group <= 0;
  const bool layout = x.resid && ((uintptr_t)x.A | (uintptr_t)x.B | (uintptr_t)x.resid | (uintptr_t)x.C) % 16 == 0 && x.lda % 8 == 0 &&
                      x.lda >= x.K && x.ldb % 8 == 0 && x.ldb >= x.K && x.ldr % 8 == 0 && x.ldr >= x.N &&
                      (!x.C || (x.ldc % 8 == 0 && x.ldc >= x.N)) && (uint64_t)x.N * (uint64_t)x.ldb < (1ull << 32);
  return shape && plain && layout ? 1 : 0;
}

static int check_kqv_head_call(const char* who, const mst_gemm_args* head, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad) {
  MST_CHECK_ARG(head != nullptr && ff2_dgrad != nullptr && ff1_dgrad != nullptr, "%s: null args", who);
  MST_CHECK_ARG(head->M > 0 && head->N > 0 && head->K > 0, "%s: the head's M,N,K must be positive (got %lld,%lld,%lld)", who,
                (long long)head->M, (long long)head->N, (long long)head->K);
  MST_CHECK_ARG(head->A && head->B, "%s: the head's A and B operands are missing", who);
  MST_CHECK_ARG(head->M == ff2_dgrad->M && head->N == ff1_dgrad->N, "%s: the head's result is the block's incoming gradient: M x width (got %lld x %lld)",
                who, (long long)head->M, (long long)head->N);
  return MST_OK;
}

extern "C" int mst_kqv_ffn_ln_bwd_form(const mst_gemm_args* kqv_dgrad, const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad,
                                       int64_t* form) {
  MST_CHECK_ARG(form != nullptr, "mst_kqv_ffn_ln_bwd_form: null form");
  if (const int rc = check_kqv_head_call("mst_kqv_ffn_ln_bwd_form", kqv_dgrad, ff2_dgrad, ff1_dgrad)) return rc;
  form[0] = kqv_head_form(*kqv_dgrad, *ff2_dgrad, *ff1_dgrad);
  return MST_OK;
}

extern "C" int mst_kqv_ffn_ln_bwd(const mst_gemm_args* kqv_dgrad, const mst_ln_bwd_in* lead, const mst_gemm_args* ff2_dgrad,
                                  const mst_gemm_args* ff1_dgrad, const mst_ln_args* ln, mst_stream_t stream) {
  if (const int rc = check_kqv_head_call("mst_kqv_ffn_ln_bwd", kqv_dgrad, ff2_dgrad, ff1_dgrad)) return rc;
  MST_CHECK_ARG(lead != nullptr, "mst_kqv_ffn_ln_bwd: null args");
  MST_CHECK_ARG(lead->dy == kqv_dgrad->C && (!lead->dy || lead->ld_dy == kqv_dgrad->ldc),
                "mst_kqv_ffn_ln_bwd: lead->dy is the head's C (both NULL: the gradient is not stored)");
  if (kqv_head_form(*kqv_dgrad, *ff2_dgrad, *ff1_dgrad))
    return ffn_ln_impl("mst_kqv_ffn_ln_bwd", ff2_dgrad, ff1_dgrad, ln, 2, stream, lead, kqv_dgrad);
  // the two launches; every argument is checked before the first one is issued
  MST_CHECK_ARG(kqv_dgrad->C != nullptr, "mst_kqv_ffn_ln_bwd: this shape runs the GEMM launch first and needs the head's C");
  if (const int rc = check_ffn_ln("mst_kqv_ffn_ln_bwd", ff2_dgrad, ff1_dgrad, ln, 2, lead)) return rc;
  if (const int f = mst_gemm_nt_form(kqv_dgrad); f < 0) return f;  // (mst_gemm_nt's own checks and message)
  if (const int rc = mst_gemm_nt(kqv_dgrad, stream)) return rc;
  return ffn_ln_impl("mst_kqv_ffn_ln_bwd", ff2_dgrad, ff1_dgrad, ln, 2, stream, lead);
}

extern "C" int mst_ffn_ln_fwd(const mst_gemm_args* ff1, const mst_gemm_args* ff2, const mst_ln_args* ln, mst_stream_t stream) {
  return ffn_ln_impl("mst_ffn_ln_fwd", ff1, ff2, ln, 1, stream);
}
extern "C" int mst_ffn_ln_bwd(const mst_gemm_args* ff2_dgrad, const mst_gemm_args* ff1_dgrad, const mst_ln_args* ln, mst_stream_t stream) {
  return ffn_ln_impl("mst_ffn_ln_bwd", ff2_dgrad, ff1_dgrad, ln, 2, stream);
}

#ifdef MST_FFN_STAMPS
extern "C" int mst_debug_ffn_stamps(uint64_t* host_out) {  // diagnostic builds only
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mst::g_ffn_stamps), sizeof(uint64_t) * (8 + 48 * 4)) == hipSuccess ? 0 : -1;
}
#endif

// gemm_checks.hpp — the argument checks (no HIP call) that more than one unit of the GEMM family runs: a fused launch checks each of its
// parts with the check of the launch that part replaces. Each is defined once, in the unit that owns it.
#pragma once
#include "common.hpp"

namespace mst {

int check_gemm_common(const mst_gemm_args& a);                     // gemm_nt.hip
int check_gemm_ln(const mst_gemm_args& a, const mst_ln_args& l);   // gemm_ln.hip
int check_gemm_bce(const mst_gemm_args& a, const mst_bce_args& q); // gemm_bce.hip
// the feed-forward block's launches (ffn_ln.hip)
int check_ffn_ln(const char* who, const mst_gemm_args* first, const mst_gemm_args* second, const mst_ln_args* ln, int mode,
                 const mst_ln_bwd_in* lead = nullptr, const mst_gemm_args* extra = nullptr, const mst_ln_args* extra_ln = nullptr);

}  // namespace mst

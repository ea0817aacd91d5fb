// attention_forms.hpp — host side of key-row attention that its units share: the launch forms attention.hip chooses (the codes of
// mst_attn_fwd_form / mst_attn_bwd_form, include/mst_hip.h), the slice constants its form rules need, and the launchers of the
// two kernel units. A launcher switches on the form it is given and decides nothing.
#pragma once
#include <type_traits>
#include "attention.hpp"

namespace mst {

enum { ATT_FWD_RES3 = 0, ATT_FWD_RES2 = 1, ATT_FWD_CHUNKED = 2, ATT_FWD_FUSED = 3, ATT_FWD_STREAM = 4 };
enum { ATT_BWD_RES = 0, ATT_BWD_STREAM_CHUNKQ = 1, ATT_BWD_STREAM = 2 };
struct AttnFwdForm { int path, waves; size_t lds; int lone, restage; int64_t grid_stats, grid_out; };
struct AttnBwdForm { int path, waves; size_t lds; int sparse, lone, dq_chunks, dq_waves; int proj; size_t lds_proj; };
constexpr int ATT_DQ_OBM = 4, ATT_DQ_NW = 8;  // chunked dQ: owner blocks per wave, waves per workgroup

constexpr int QKV_KC = 64;            // qkv_prologue (attention_fwd.hip): contraction slice staged per step
constexpr int DOP_KC = 64;            // dout_prologue (attention_bwd.hip): contraction slice staged per step
constexpr int DOP_LDS = DOP_KC + 8;   // row stride (elements) of a staged slice: 144-byte rows

// dh has passed the entry point's checks (attention.hip); a: complete but for what the form sets (restage)
int attn_launch_fwd(int dtype, int64_t dh, const AttnArgs& a, const AttnFwdForm& f, hipStream_t s);   // attention_fwd.hip
int attn_launch_bwd(int dtype, int64_t dh, const AttnArgs& a, const AttnBwdForm& f, hipStream_t s);   // attention_bwd.hip (f.proj: mst_attn_proj_bwd's)

// f(activation type tag, std::integral_constant<int, head size>): the one head-size ladder of the attention units
template <typename F> static inline int dispatch_attn(int dtype, int64_t dh, F&& f) {
  return dispatch_act(dtype, [&](auto tag) -> int {
    if (dh == 16) return f(tag, std::integral_constant<int, 16>{});
    if (dh == 32) return f(tag, std::integral_constant<int, 32>{});
    return f(tag, std::integral_constant<int, 64>{});
  });
}

}  // namespace mst

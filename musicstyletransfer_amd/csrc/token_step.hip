// token_step.hip — the token ends' draw of a position with temperature, top-k and nucleus (top-p) cuts: mst_token_step, the token
// counterpart of mst_frame_step. One wave per sequence reads the position's LOGITS (16-bit) once and draws; the seed is a device
// word, so the launch sits in the position's captured graph behind the output layer's GEMM (decode.TokenSampling).
//
// x = logit / tau is non-decreasing in the stored 16-bit logit, so both cuts are cuts on the stored value itself, taken as an
// order-preserving 16-bit integer key (sign-magnitude bits -> unsigned order; -0 is +0):
//   top-k : c_k = the k-th largest key with multiplicity = the largest c with #{key >= c} >= k; survivors are key >= c_k (a tie group
//           at the cut survives whole, whatever its columns);
//   top-p : among the survivors, with mass e = exp(x - max x): c_p = the largest c with mass{key >= c} >= top_p * mass{survivors}.
// Each cut is a 16-step bisection over the key, one bit per step: a per-lane partial count / mass and one wave sum. The mass of a
// candidate cut is formed by ONE fixed summation (lane chunk in column order, then the wave tree, left-out terms as zeros), so it is
// monotone in the cut and mass{key >= c_k} is bitwise the survivors' mass: c_p >= c_k, and the arg-max group is always kept.
// The draw is mst_sample_step's inverse CDF over the kept tokens in column order; the score is the MODEL's -log softmax(logit)[token]
// (temperature 1, unfiltered), so every decoder's score is the same quantity.
#include <math.h>
#include "common.hpp"

namespace mst {

template <int CTRL> __device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
// wave_sum's levels on an integer (a count of up to V tokens is exact at any V)
__device__ __forceinline__ int wave_sum_i(int v) {
  v += dpp_mov_i<0xB1>(v);
  v += dpp_mov_i<0x4E>(v);
  v += dpp_mov_i<0x141>(v);
  v += dpp_mov_i<0x140>(v);
  v += __builtin_amdgcn_ds_swizzle(v, 0x401F);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// stored 16-bit float -> integer with the same order (both 16-bit types are sign-magnitude)
__device__ __forceinline__ int order_key(uint16_t b) {
  if ((b & 0x7FFFu) == 0u) return 0x8000;
  return (b & 0x8000u) ? (int)(uint16_t)~b : (int)(b | 0x8000u);
}

constexpr int TOKEN_OWN = 8;  // a lane's ceil(V / 64) tokens stay in registers up to V = 512 (the model's vocabulary is 293: 5)

// lane l owns the contiguous columns [l chunk, (l + 1) chunk) as in sample_step_kernel. REGS: keys and masses in registers; otherwise
// the chunk is walked from memory again in every pass (the row is then in L1 / L2).
//
// HELD (mst_token_step_held): where hold[n, i] != 0 the token is given[n, i] instead of a draw — written whatever the sequence's state,
// charged to held_scores[n] (the model's own -log softmax, as for a drawn token) unless the sequence is finished, counted in
// active[i] by the usual rule, kept_out[n] = 0. The branch is wave-uniform and leaves before the cuts; it costs the five bytes of
// hold and given per sequence. A given token outside [0, V) is never used as an index: PAD is written and nothing is charged.
template <typename T, bool REGS, bool HELD>
__global__ __launch_bounds__(256) void token_step_kernel(int64_t N, int64_t V, int64_t i, int64_t L, const uint16_t* __restrict__ logits,
                                                         int64_t ldl, float tau, int32_t top_k, float top_p,
                                                         const uint64_t* __restrict__ seed_ptr, int32_t* __restrict__ seqs,
                                                         float* __restrict__ scores, int32_t* __restrict__ word, int32_t* __restrict__ active,
                                                         int32_t* __restrict__ kept_out, int32_t eos, int32_t pad,
                                                         const int32_t* __restrict__ given, const uint8_t* __restrict__ hold,
                                                         float* __restrict__ held_scores) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;  // (a whole wave)
  const int32_t last = seqs[n * L + i - 1];
  const bool fin = (last == eos) || (last == pad && i > 1);
  const uint16_t* __restrict__ row = logits + n * ldl;
  const int chunk = (int)((V + 63) / 64);
  const int64_t lo64 = (int64_t)lane * chunk;
  const int lo = (int)(lo64 < V ? lo64 : V), hi = (int)(lo64 + chunk < V ? lo64 + chunk : V), cnt = hi - lo;

  // ---- the row, once: maximum, the model's normaliser (temperature 1), keys and sampling masses
  int key[TOKEN_OWN];
  float e[TOKEN_OWN];
  float vmax = -INFINITY;
  if constexpr (REGS) {
#pragma unroll
    for (int c = 0; c < TOKEN_OWN; ++c) {
      const uint16_t b = c < cnt ? row[lo + c] : (uint16_t)0;
      key[c] = c < cnt ? order_key(b) : -1;  // (-1: below every cut)
      e[c] = bits_to_f32<T>(b);
      if (c < cnt) vmax = fmaxf(vmax, e[c]);
    }
  } else {
    for (int w = lo; w < hi; ++w) vmax = fmaxf(vmax, bits_to_f32<T>(row[w]));
  }
  vmax = wave_max(vmax);
  const float xmax = vmax / tau;
  float psum = 0.f;
  if constexpr (REGS) {
#pragma unroll
    for (int c = 0; c < TOKEN_OWN; ++c) {
      const float v = e[c];
      if (c < cnt) psum += expf(v - vmax);
      e[c] = c < cnt ? expf(v / tau - xmax) : 0.f;
    }
  } else {
    for (int w = lo; w < hi; ++w) psum += expf(bits_to_f32<T>(row[w]) - vmax);
  }
  psum = wave_sum(psum);

  if constexpr (HELD) {
    if (hold[n * L + i] != 0) {  // (the same for the whole wave)
      if (lane == 0) {
        const int32_t g = given[n * L + i];
        const bool ok = g >= 0 && (int64_t)g < V;
        const int32_t w = ok ? g : pad;
        seqs[n * L + i] = w;
        word[n] = w;
        if (ok && !fin) held_scores[n] += -logf(fmaxf(expf(bits_to_f32<T>(row[g]) - vmax) / fmaxf(psum, 1e-30f), 1e-30f));
        if (active && w != eos && w != pad) atomicAdd(active + i, 1);
        if (kept_out) kept_out[n] = 0;
      }
      return;
    }
  }

  // f(key, mass, column) over this lane's tokens in column order
  auto each = [&](auto&& f) {
    if constexpr (REGS) {
#pragma unroll
      for (int c = 0; c < TOKEN_OWN; ++c)
        if (c < cnt) f(key[c], e[c], lo + c);
    } else {
      for (int w = lo; w < hi; ++w) {
        const uint16_t b = row[w];
        f(order_key(b), expf(bits_to_f32<T>(b) / tau - xmax), w);
      }
    }
  };
  auto mass_from = [&](int c) {
    float part = 0.f;
    each([&](int k, float m, int) { part += k >= c ? m : 0.f; });
    return part;
  };

  // ---- top-k: the k-th largest key
  int cut = 0;
  if (top_k > 0 && (int64_t)top_k < V) {
    for (int bit = 15; bit >= 0; --bit) {
      const int t = cut | (1 << bit);
      int c = 0;
      each([&](int k, float, int) { c += k >= t ? 1 : 0; });
      if (wave_sum_i(c) >= top_k) cut = t;
    }
  }
  // ---- top-p among the survivors
  if (top_p < 1.f) {
    const float need = top_p * wave_sum(mass_from(cut));
    int cp = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const int t = cp | (1 << bit);
      if (wave_sum(mass_from(t > cut ? t : cut)) >= need) cp = t;
    }
    cut = cp > cut ? cp : cut;
  }

  // ---- the draw: inverse CDF over the kept tokens in column order
  float part = 0.f;
  int n_kept = 0, last_kept = -1;
  each([&](int k, float m, int w) {
    if (k >= cut) { part += m; ++n_kept; last_kept = w; }
  });
  n_kept = wave_sum_i(n_kept);
  float incl = part;  // inclusive scan over the lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const float total = __shfl(incl, 63, 64);
  const uint32_t h = dropout_hash(seed_ptr[0], (uint32_t)i, (uint64_t)n);
  const float target = ((float)(h >> 8) + 1.0f) * (1.0f / 16777216.0f) * total;  // in (0, total]
  const bool mine = (incl >= target) && (incl - part < target);
  int tok = -1;
  if (mine) {
    float acc = incl - part;
    tok = last_kept;  // (the walk ending short by rounding: this chunk's last kept token)
    bool found = false;
    each([&](int k, float m, int w) {
      if (k >= cut && !found) {
        acc += m;
        if (acc >= target) { tok = w; found = true; }
      }
    });
  }
  // exactly one lane owns the draw; rounding at a chunk boundary could leave none: the LAST KEPT token of the row then takes it
  const unsigned long long owners = __ballot(mine && tok >= 0);
  const unsigned long long holders = __ballot(last_kept >= 0);
  int chosen = owners ? tok : last_kept;
  const int src_lane = owners ? (int)__builtin_ctzll(owners) : (holders ? 63 - (int)__builtin_clzll(holders) : 0);
  chosen = __shfl(chosen, src_lane, 64);
  if (chosen < 0 || chosen >= (int)V) chosen = (int)V - 1;  // (index safety only: the kept set holds the arg-max group, so is not empty)
  if (lane == 0) {
    const int32_t w = fin ? pad : chosen;
    seqs[n * L + i] = w;
    word[n] = w;
    if (!fin) scores[n] += -logf(fmaxf(expf(bits_to_f32<T>(row[chosen]) - vmax) / fmaxf(psum, 1e-30f), 1e-30f));
    if (active && w != eos && w != pad) atomicAdd(active + i, 1);
    if (kept_out) kept_out[n] = n_kept;
  }
}

}  // namespace mst

using namespace mst;

// the checks and the launch of both entry points (`name`: the one that was called; held: given / hold / held_scores are used)
static int token_step_launch(const char* name, bool held, int dtype, int64_t N, int64_t V, int64_t i, int64_t L, const void* logits, int64_t ldl,
                             float tau, int32_t top_k, float top_p, const uint64_t* seed_ptr, int32_t* seqs, float* scores, int32_t* word,
                             int32_t* active, int32_t* kept_out, int32_t eos, int32_t pad, const int32_t* given, const uint8_t* hold,
                             float* held_scores, mst_stream_t stream) {
  MST_CHECK_ARG(N > 0 && V > 0 && L > 1 && V <= (1ll << 30), "%s: sizes must be positive (L >= 2, V <= 2^30)", name);
  MST_CHECK_ARG(i >= 1 && i < L, "%s: position i outside [1, L)", name);
  MST_CHECK_ARG(tau > 0.f && tau <= 3.0e38f, "%s: tau must be positive and finite", name);
  MST_CHECK_ARG(top_k >= 0, "%s: top_k must be 0 (off) or at least 1", name);
  MST_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "%s: top_p outside (0, 1]", name);
  MST_CHECK_ARG(logits && seed_ptr && seqs && scores && word, "%s: null pointer (logits, seed word, seqs, scores, word)", name);
  MST_CHECK_ARG(ldl >= V, "%s: a row stride below V", name);
  if (held) MST_CHECK_ARG(given && hold && held_scores, "%s: null pointer (given, hold, held_scores)", name);
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, N, V, i, L, (const uint16_t*)logits, ldl, tau,
                         top_k, top_p, seed_ptr, seqs, scores, word, active, kept_out, eos, pad, given, hold, held_scores);
    };
    const bool regs = V <= 64 * TOKEN_OWN;
    if (regs && held) launch(token_step_kernel<T, true, true>);
    else if (regs) launch(token_step_kernel<T, true, false>);
    else if (held) launch(token_step_kernel<T, false, true>);
    else launch(token_step_kernel<T, false, false>);
    MST_CHECK_LAUNCH("token_step_kernel");
    return MST_OK;
  });
}

extern "C" int mst_token_step(int dtype, int64_t N, int64_t V, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int32_t top_k,
                              float top_p, const uint64_t* seed_ptr, int32_t* seqs, float* scores, int32_t* word, int32_t* active,
                              int32_t* kept_out, int32_t eos, int32_t pad, mst_stream_t stream) {
  return token_step_launch("mst_token_step", false, dtype, N, V, i, L, logits, ldl, tau, top_k, top_p, seed_ptr, seqs, scores, word, active,
                           kept_out, eos, pad, nullptr, nullptr, nullptr, stream);
}

extern "C" int mst_token_step_held(int dtype, int64_t N, int64_t V, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau,
                                   int32_t top_k, float top_p, const uint64_t* seed_ptr, int32_t* seqs, float* scores, int32_t* word,
                                   int32_t* active, int32_t* kept_out, int32_t eos, int32_t pad, const int32_t* given, const uint8_t* hold,
                                   float* held_scores, mst_stream_t stream) {
  return token_step_launch("mst_token_step_held", true, dtype, N, V, i, L, logits, ldl, tau, top_k, top_p, seed_ptr, seqs, scores, word,
                           active, kept_out, eos, pad, given, hold, held_scores, stream);
}

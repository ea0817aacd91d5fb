// beam.hip — one position of beam search on the device (reference VarAutoEncoder/sampler.py:198-257, token ends):
//   mst_beam_step   : per sample, the K best of its K x V continuations (score = summed -log p; a finished hypothesis continues
//                     with PAD only, at no cost: sampler.py:218-221), the re-ranked token rows, the words fed to the next position
//   mst_beam_gather : the decoder layers' K | Q | V cache rows of the re-ranked hypotheses (sampler.py:236-238)
//   mst_sample_step / mst_frame_step(_held) : ancestral sampling's draw of a position — a token by inverse CDF, a piano-roll frame by a
//                     Bernoulli draw (or a threshold) per pitch from the position's logits
// With these two the whole position — decoder step, ranking, cache reorder — is device work inside ONE captured graph; the host
// version spent 98 % of a position in its own top-k over beam x V and the copies around it (2.6 ms against 55 us of device time).
// Ranking is deterministic: candidates are ordered by (score, hypothesis * V + word), i.e. the stable argsort of the host form.
#include <math.h>
#include "common.hpp"

namespace mst {

struct BeamArgs {
  int64_t B, K, V, i, L;
  const float* probs; int64_t ldp;
  const float* scores_in; float* scores_out;
  const int32_t* seqs_in; int32_t* seqs_out;
  int32_t* hyp_src; int32_t* word; int32_t* active;
  int32_t eos, pad;
};

constexpr int BEAM_MAXK = 16;

// one 256-thread workgroup per sample
__global__ __launch_bounds__(256) void beam_step_kernel(BeamArgs q) {
  __shared__ float s_score[BEAM_MAXK];
  __shared__ int s_fin[BEAM_MAXK];
  __shared__ float s_val[BEAM_MAXK];
  __shared__ int s_idx[BEAM_MAXK];
  __shared__ float r_val[4];
  __shared__ int r_idx[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int K = (int)q.K, V = (int)q.V;
  if (tid < K) {
    const int64_t h = b * K + tid;
    s_score[tid] = q.scores_in[h];
    const int32_t last = q.seqs_in[h * q.L + q.i - 1];
    s_fin[tid] = (last == q.eos) || (last == q.pad && q.i > 1);
  }
  __syncthreads();
  const int n_cand = K * V;
  // every candidate's score ONCE (the K selection rounds below used to recompute the logarithm and the c / V division of all
  // K V candidates each: 15.9 us per position); a thread keeps its candidates c = tid + 256 j in registers when they fit
  constexpr int OWN = 8;  // K V <= 2048 candidates: beam 4 x 293 tokens = 5 per thread
  const bool in_regs = n_cand <= OWN * 256;
  float own[OWN];
  uint32_t done = 0u;  // this thread's candidates already selected
  auto score = [&](int c) {
    const int k = c / V, w = c - k * V;
    if (s_fin[k]) return (w == q.pad) ? s_score[k] : INFINITY;
    const float v = s_score[k] - logf(fmaxf(q.probs[(b * K + k) * q.ldp + w], 1e-30f));
    return v == v ? v : INFINITY;  // a NaN (from a NaN score or probability) never wins and never leaves the selection without a winner
  };
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
      const int c = tid + 256 * j;
      own[j] = c < n_cand ? score(c) : INFINITY;
    }
  }
  for (int r = 0; r < K; ++r) {
    float best = INFINITY;
    int best_i = 0x7fffffff;
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < OWN; ++j) {  // (the general loop's rule, ties included: an all-infinite remainder still yields a valid index)
        const int c = tid + 256 * j;
        if (c < n_cand && !((done >> j) & 1u) && (own[j] < best || (own[j] == best && c < best_i))) { best = own[j]; best_i = c; }
      }
    } else {
      for (int c = tid; c < n_cand; c += 256) {
        bool taken = false;
        for (int u = 0; u < r; ++u) taken |= (s_idx[u] == c);
        if (taken) continue;
        const float val = score(c);
        if (val < best || (val == best && c < best_i)) { best = val; best_i = c; }
      }
    }
    // workgroup argmin by (value, index)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(best_i, off, 64);
      if (ov < best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    if (lane == 0) { r_val[wave] = best; r_idx[wave] = best_i; }
    __syncthreads();
    if (tid == 0) {
      float bv = r_val[0]; int bi = r_idx[0];
      for (int wv = 1; wv < 4; ++wv)
        if (r_val[wv] < bv || (r_val[wv] == bv && r_idx[wv] < bi)) { bv = r_val[wv]; bi = r_idx[wv]; }
      // (with NaN mapped to +inf above some candidate always wins, ties included; the clamp keeps the index arithmetic below
      // inside seqs / hyp_src whatever happens)
      s_val[r] = bv; s_idx[r] = ((unsigned)bi < (unsigned)n_cand) ? bi : 0;
    }
    __syncthreads();
    if (in_regs) {  // the winner leaves its owner's registers
      const int won = s_idx[r];
#pragma unroll
      for (int j = 0; j < OWN; ++j)
        if (tid + 256 * j == won) done |= 1u << j;
    }
  }
  // the re-ranked rows: new hypothesis r continues hypothesis s_idx[r] / V with word s_idx[r] % V
  int alive = 0;
  for (int r = 0; r < K; ++r) {
    const int c = s_idx[r];
    const int k = c / V, w = c - k * V;
    const int64_t dst = b * K + r, src = b * K + k;
    for (int64_t col = tid; col < q.i; col += 256) q.seqs_out[dst * q.L + col] = q.seqs_in[src * q.L + col];
    if (tid == 0) {
      q.seqs_out[dst * q.L + q.i] = w;
      q.scores_out[dst] = s_val[r];
      q.hyp_src[dst] = (int32_t)src;
      q.word[dst] = w;
      alive += (w != q.eos && w != q.pad) ? 1 : 0;
    }
  }
  if (tid == 0 && q.active && alive) atomicAdd(q.active + q.i, alive);
}

// out[j, r, :] = in[src[j], r, :] for r < n_rows; rows of row_bytes bytes (a multiple of 16), t_max rows per hypothesis
// (skip_begin, skip_bytes: a byte range of every row that is NOT copied — the Q third of a K | Q | V cache row: a past position's
// query is never read again, attn_decode_kernel takes q from the newest row only)
__global__ __launch_bounds__(256) void beam_gather_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ src,
                                                          int64_t N, int64_t n_rows, int64_t row_bytes, int64_t t_max, int64_t skip_begin,
                                                          int64_t skip_bytes) {
  const int64_t pieces = (row_bytes - skip_bytes) / 16, total = N * n_rows * pieces, skip_pc = skip_begin / 16, skip_n = skip_bytes / 16;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    int64_t pc = p % pieces;
    const int64_t rr = (p / pieces) % n_rows, j = p / (pieces * n_rows);
    if (pc >= skip_pc) pc += skip_n;
    const int64_t s = src[j];
    reinterpret_cast<u32x4*>(out + (j * t_max + rr) * row_bytes)[pc] = reinterpret_cast<const u32x4*>(in + (s * t_max + rr) * row_bytes)[pc];
  }
}

// Ancestral sampling (sampler.py:155-190): one wave per sequence draws the next token from its distribution by inverse CDF —
// u = counter hash of (seed, position, sequence) in (0, 1] times the row sum; lane l owns the contiguous chunk of ceil(V / 64)
// tokens, a wave scan of the chunk sums finds the owning lane, which walks its chunk. A finished sequence (last token EOS, or
// PAD from position 2 on) continues with PAD at no cost. score += -log max(p[token], 1e-30); active[i] counts running sequences.
__global__ __launch_bounds__(256) void sample_step_kernel(int64_t N, int64_t V, int64_t i, int64_t L, const float* __restrict__ probs, int64_t ldp,
                                                          int32_t* __restrict__ seqs, float* __restrict__ scores, int32_t* __restrict__ word,
                                                          int32_t* __restrict__ active, uint64_t seed, int32_t eos, int32_t pad) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int32_t last = seqs[n * L + i - 1];
  const bool fin = (last == eos) || (last == pad && i > 1);
  const float* row = probs + n * ldp;
  const int chunk = (int)((V + 63) / 64);
  const int lo = lane * chunk, hi = (lo + chunk < V) ? lo + chunk : (int)V;
  float part = 0.f;
  for (int w = lo; w < hi; ++w) part += row[w];
  float incl = part;  // inclusive scan over the lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const float total = __shfl(incl, 63, 64);
  const uint32_t h = dropout_hash(seed, (uint32_t)i, (uint64_t)n);
  const float target = ((float)(h >> 8) + 1.0f) * (1.0f / 16777216.0f) * total;  // in (0, total]
  const bool mine = (incl >= target) && (incl - part < target);
  int tok = -1;
  if (mine) {
    float acc = incl - part;
    tok = hi - 1;
    for (int w = lo; w < hi; ++w) {
      acc += row[w];
      if (acc >= target) { tok = w; break; }
    }
  }
  // exactly one lane owns the draw (rounding at a chunk boundary could leave none: token V - 1 then takes it, whatever its mass)
  const unsigned long long owners = __ballot(mine && tok >= 0);
  int chosen = tok;
  if (owners == 0ull) chosen = (int)V - 1;
  const int src_lane = owners ? (int)__builtin_ctzll(owners) : 0;
  chosen = __shfl(chosen, src_lane, 64);
  if (lane == 0) {
    const int32_t w = fin ? pad : chosen;
    seqs[n * L + i] = w;
    word[n] = w;
    if (!fin) scores[n] += -logf(fmaxf(row[chosen] / fmaxf(total, 1e-30f), 1e-30f));
    if (active && w != eos && w != pad) atomicAdd(active + i, 1);
  }
}

// The piano-roll ends' draw (sampler.py:155-190 with a Bernoulli per pitch): one wave per sequence walks the P logits of the position.
// x = logit / tau; p = sigmoid(x) and 1 - p = sigmoid(-x) are each formed from their own exponential, so the score of an unlikely
// frame does not lose its digits in 1 - p. mode 0 draws frame = u < p with u = (dropout_hash(seed, i, n * P + j) >> 8) * 2^-24 in
// [0, 1); mode 1 thresholds x > thr_logit (no random number). The frame goes to frames[n, :P] (the next position's input) and to
// roll[n, i - 1, :P]; scores[n] += -sum_j log max(frame ? p : 1 - p, 1e-30) (one wave owns a sequence: no atomics, a fixed order).
//
// HELD (mst_frame_step_held): a cell with hold[n, i - 1, j] != 0 is not drawn — its frame is given[n, i - 1, j] != 0, and its
// -log p goes to held_scores[n] instead of scores[n]. A free cell is computed exactly as above, its random number still indexed by
// (seed, i, n P + j), so what it draws does not depend on which other cells are held; with nothing held the free sum has the same
// terms in the same order. Two more bytes are read per cell; still one wave per sequence and no atomics.
template <typename T, bool HELD>
__global__ __launch_bounds__(256) void frame_step_kernel(int64_t N, int64_t P, int64_t i, int64_t L, const T* __restrict__ logits, int64_t ldl,
                                                         float tau, int mode, float thr_logit, const uint64_t* __restrict__ seed_ptr,
                                                         uint8_t* __restrict__ frames, int64_t ldf, uint8_t* __restrict__ roll, int64_t ldr,
                                                         float* __restrict__ scores, float* __restrict__ probs_out,
                                                         const uint8_t* __restrict__ given, int64_t ldg, const uint8_t* __restrict__ hold,
                                                         int64_t ldh, float* __restrict__ held_scores) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const uint64_t seed = mode == 0 ? seed_ptr[0] : 0ull;
  const T* __restrict__ row = logits + n * ldl;
  uint8_t* __restrict__ fr = frames + n * ldf;
  uint8_t* __restrict__ rl = roll + (n * L + (i - 1)) * ldr;
  float* __restrict__ po = probs_out ? probs_out + (n * L + (i - 1)) * P : nullptr;
  const uint8_t* __restrict__ gv = HELD ? given + (n * L + (i - 1)) * ldg : nullptr;
  const uint8_t* __restrict__ hd = HELD ? hold + (n * L + (i - 1)) * ldh : nullptr;
  float nll = 0.f, held_nll = 0.f;
  for (int64_t j = lane; j < P; j += 64) {
    // (both bytes are loaded beside the logit, whatever hold says: a load of given behind the test of hold would put a second
    // memory round trip — to rows no launch has touched before — into a launch that is all latency)
    uint8_t hold_j = 0, given_j = 0;
    if constexpr (HELD) {
      hold_j = hd[j];
      given_j = gv[j];
    }
    const float x = to_f32(row[j]) / tau;
    const float p = 1.f / (1.f + expf(-x)), q = 1.f / (1.f + expf(x));
    bool on;
    if (mode == 0) {
      const float u = (float)(dropout_hash(seed, (uint32_t)i, (uint64_t)(n * P + j)) >> 8) * (1.0f / 16777216.0f);
      on = u < p;
    } else {
      on = x > thr_logit;
    }
    bool held = false;
    if constexpr (HELD) {
      held = hold_j != 0;
      if (held) on = given_j != 0;
    }
    const uint8_t f = on ? 1 : 0;
    fr[j] = f;
    rl[j] = f;
    if (po) po[j] = p;
    const float cost = logf(fmaxf(on ? p : q, 1e-30f));
    if (held) held_nll -= cost;
    else nll -= cost;
  }
  nll = wave_sum(nll);
  if constexpr (HELD) held_nll = wave_sum(held_nll);
  if (lane == 0) {
    scores[n] += nll;
    if constexpr (HELD) held_scores[n] += held_nll;
  }
}

}  // namespace mst

using namespace mst;

// the checks and the launch of both entry points (`name`: the one that was called; held: given / hold / held_scores are used)
static int frame_step_launch(const char* name, bool held, int dtype, int64_t N, int64_t P, int64_t i, int64_t L, const void* logits, int64_t ldl,
                             float tau, int mode, float thr, const uint64_t* seed_ptr, uint8_t* frames, int64_t ldf, uint8_t* roll, int64_t ldr,
                             float* scores, float* probs_out, const uint8_t* given, int64_t ldg, const uint8_t* hold, int64_t ldh,
                             float* held_scores, mst_stream_t stream) {
  MST_CHECK_ARG(N > 0 && P > 0 && L > 1, "%s: sizes must be positive (L >= 2)", name);
  MST_CHECK_ARG(i >= 1 && i < L, "%s: position i outside [1, L)", name);
  MST_CHECK_ARG(tau > 0.f && tau <= 3.0e38f, "%s: tau must be positive and finite", name);
  MST_CHECK_ARG(mode == 0 || mode == 1, "%s: mode must be 0 (draw) or 1 (threshold)", name);
  MST_CHECK_ARG(mode == 0 || (thr > 0.f && thr < 1.f), "%s: thr outside (0, 1)", name);
  MST_CHECK_ARG(logits && frames && roll && scores && (mode == 1 || seed_ptr), "%s: null pointer (draw mode needs the seed word)", name);
  MST_CHECK_ARG(ldl >= P && ldf >= P && ldr >= P, "%s: a row stride below P", name);
  if (held) {
    MST_CHECK_ARG(given && hold && held_scores, "%s: null pointer (given, hold, held_scores)", name);
    MST_CHECK_ARG(ldg >= P && ldh >= P, "%s: a row stride below P (given, hold)", name);
  }
  const float thr_logit = mode == 1 ? (float)log((double)thr / (1.0 - (double)thr)) : 0.f;
  return dispatch_act(dtype, [&](auto tag) -> int {
    typedef decltype(tag) T;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, N, P, i, L, (const T*)logits, ldl, tau, mode,
                         thr_logit, seed_ptr, frames, ldf, roll, ldr, scores, probs_out, given, ldg, hold, ldh, held_scores);
    };
    if (held) launch(frame_step_kernel<T, true>);
    else launch(frame_step_kernel<T, false>);
    MST_CHECK_LAUNCH("frame_step_kernel");
    return MST_OK;
  });
}

extern "C" int mst_frame_step(int dtype, int64_t N, int64_t P, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int mode,
                              float thr, const uint64_t* seed_ptr, uint8_t* frames, int64_t ldf, uint8_t* roll, int64_t ldr, float* scores,
                              float* probs_out, mst_stream_t stream) {
  return frame_step_launch("mst_frame_step", false, dtype, N, P, i, L, logits, ldl, tau, mode, thr, seed_ptr, frames, ldf, roll, ldr, scores,
                           probs_out, nullptr, 0, nullptr, 0, nullptr, stream);
}

extern "C" int mst_frame_step_held(int dtype, int64_t N, int64_t P, int64_t i, int64_t L, const void* logits, int64_t ldl, float tau, int mode,
                                   float thr, const uint64_t* seed_ptr, uint8_t* frames, int64_t ldf, uint8_t* roll, int64_t ldr,
                                   float* scores, float* probs_out, const uint8_t* given, int64_t ldg, const uint8_t* hold, int64_t ldh,
                                   float* held_scores, mst_stream_t stream) {
  return frame_step_launch("mst_frame_step_held", true, dtype, N, P, i, L, logits, ldl, tau, mode, thr, seed_ptr, frames, ldf, roll, ldr,
                           scores, probs_out, given, ldg, hold, ldh, held_scores, stream);
}

extern "C" int mst_sample_step(int64_t N, int64_t V, int64_t i, int64_t L, const float* probs, int64_t ldp, int32_t* seqs, float* scores,
                               int32_t* word, int32_t* active, uint64_t seed, int32_t eos, int32_t pad, mst_stream_t stream) {
  MST_CHECK_ARG(N > 0 && V > 0 && i >= 1 && i < L && probs && seqs && scores && word && ldp >= V, "mst_sample_step: bad argument");
  hipLaunchKernelGGL(sample_step_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, N, V, i, L, probs, ldp, seqs, scores, word,
                     active, seed, eos, pad);
  MST_CHECK_LAUNCH("sample_step_kernel");
  return MST_OK;
}

extern "C" int mst_beam_step(int64_t B, int64_t K, int64_t V, int64_t i, int64_t L, const float* probs, int64_t ldp, const float* scores_in,
                             float* scores_out, const int32_t* seqs_in, int32_t* seqs_out, int32_t* hyp_src, int32_t* word, int32_t* active,
                             int32_t eos, int32_t pad, mst_stream_t stream) {
  MST_CHECK_ARG(B > 0 && K > 0 && K <= BEAM_MAXK && V > 0 && i >= 1 && i < L && K * V < (1ll << 30), "mst_beam_step: bad sizes (beam <= %d)", BEAM_MAXK);
  MST_CHECK_ARG(probs && scores_in && scores_out && seqs_in && seqs_out && hyp_src && word && ldp >= V, "mst_beam_step: null pointer or ldp < V");
  MST_CHECK_ARG(seqs_in != seqs_out && scores_in != scores_out, "mst_beam_step: the re-ranked rows need buffers of their own");
  BeamArgs q = {B, K, V, i, L, probs, ldp, scores_in, scores_out, seqs_in, seqs_out, hyp_src, word, active, eos, pad};
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, q);
  MST_CHECK_LAUNCH("beam_step_kernel");
  return MST_OK;
}

extern "C" int mst_beam_gather_cols(const void* in, void* out, const int32_t* src, int64_t N, int64_t n_rows, int64_t row_bytes, int64_t t_max,
                                    int64_t skip_begin, int64_t skip_bytes, mst_stream_t stream) {
  MST_CHECK_ARG(in && out && src && in != out && N > 0 && n_rows > 0 && n_rows <= t_max && row_bytes > 0 && row_bytes % 16 == 0,
                "mst_beam_gather: bad argument (rows of a multiple of 16 bytes, distinct buffers)");
  MST_CHECK_ARG(((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0), "mst_beam_gather: buffers must be 16-byte aligned");
  MST_CHECK_ARG(skip_begin >= 0 && skip_bytes >= 0 && skip_begin % 16 == 0 && skip_bytes % 16 == 0 && skip_begin + skip_bytes <= row_bytes &&
                    skip_bytes < row_bytes,
                "mst_beam_gather_cols: the skipped range must be whole 16-byte pieces inside the row and leave something to copy");
  const int64_t total = N * n_rows * ((row_bytes - skip_bytes) / 16);
  int64_t grid = cdiv(total, 256 * 4);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(beam_gather_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)in, (uint8_t*)out, src, N,
                     n_rows, row_bytes, t_max, skip_begin, skip_bytes);
  MST_CHECK_LAUNCH("beam_gather_kernel");
  return MST_OK;
}
extern "C" int mst_beam_gather(const void* in, void* out, const int32_t* src, int64_t N, int64_t n_rows, int64_t row_bytes, int64_t t_max,
                               mst_stream_t stream) {
  return mst_beam_gather_cols(in, out, src, N, n_rows, row_bytes, t_max, 0, 0, stream);
}

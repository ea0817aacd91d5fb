// step_begin.hpp — the bookkeeping at the top of every training step (mst_step_begin): advances the RNG state, advances Adam's step
// counter and bias-corrected learning rate (and, asked to, the step's training-schedule block: KL weight, free bits, lr factor), draws eps, writes the two padding masks from the sequence lengths (SequenceMask,
// model.py:246-247; the encoder's for the piano-roll ends) and clears the loss sums and the gradient bucket. A launch of its own
// (util.hip) or extra workgroups of the step's first GEMM launch (mst_gemm_nt_pair_begin, gemm_nt.hip): every kernel in the captured
// graph costs ~4.7 us however small, and nothing in the embedding GEMMs depends on this.
#pragma once
#include <math.h>
#include "common.hpp"

namespace mst {

constexpr int SB_THREADS = 1024;  // threads of the stand-alone launch
__device__ __forceinline__ uint64_t step_seed(uint64_t base, uint64_t step) {
  uint64_t x = base ^ (step * 0x9E3779B97F4A7C15ull);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

struct StepBegin {  // mst_step_begin_args with the zero lists in 16-byte units and the number of bookkeeping workgroups
  uint64_t* rng_state; int32_t* adam_state; double lr, beta1, beta2;
  float* eps_out; int64_t n_eps; uint32_t eps_site; int64_t eps_index0;
  const int32_t* lens; int64_t B; uint8_t* mask_e; int64_t Se; int32_t add_e; uint8_t* mask_d; int64_t Sd; int32_t add_d;
  u32x4* zero_a; int64_t n16_a; u32x4* zero_b; int64_t n16_b; int n_state;
  // optional transposed-shadow refresh hosted by the same launch (mst_step_begin_args.sh_*; sh_w == nullptr: none)
  const float* sh_w; void* sh_wt16; const int64_t* sh_desc; const int64_t* sh_prefix; int sh_n_mat; int64_t sh_tiles;
  // optional training schedules (mst_step_begin_args.sched*; sched == nullptr: none)
  float* sched; float kl_weight, kl_free_bits; int32_t kl_warmup, kl_cycle, lr_warmup;
  // optional decoder-input dropout (mst_step_begin_args.in_*; in_keep == nullptr: none) — only step_begin_wg<NT, true> reads these
  uint8_t* in_keep; int64_t in_n; float in_p; uint32_t in_site; int64_t in_index0;
  const uint8_t* in_src; int64_t in_ld_src; uint8_t* in_dst; int64_t in_ld_dst; int64_t in_chunks;  // (8-byte chunks of a row)
};

// The training schedules, pure functions of Adam's step count t (1-based), in double: the learning-rate warm-up factor f_lr and the
// (cyclical) KL warm-up ramp. W = 0 switches a warm-up off; C > 0 restarts the KL ramp every C steps.
__host__ __device__ inline double sched_lr_factor(int t, int W_lr) {
  return W_lr > 0 ? fmin(1.0, (double)t / (double)W_lr) : 1.0;
}
__host__ __device__ inline double sched_kl_ramp(int t, int W_b, int C) {
  const int u = C > 0 ? (t - 1) % C + 1 : t;
  return W_b > 0 ? fmin(1.0, (double)u / (double)W_b) : 1.0;
}

// Workgroup `wg` of `nwg` (NT threads each). Every workgroup derives the new seed itself from (base seed, step counter + 1); the
// state is written back by the workgroup that ARRIVES LAST at rng_state[3], i.e. after every other workgroup has read the old
// counter. Workgroups [0, n_state) do the bookkeeping (and take part in the arrival count); the rest only help clearing the two
// buffers — the gradient bucket is most of the bytes and has no business waiting on 64 workgroups' worth of store bandwidth.
// IN: the launch carries a decoder-input dropout job (q.in_*; include/mst_hip.h). Its draw needs the new seed, so it is work of the
// bookkeeping workgroups; the flag keeps its code out of every launch that cannot carry one (gemm_nt_pair_kernel: the decoder's tiles
// of that launch would read the masked frames while these workgroups write them).
template <int NT, bool IN = false>
__device__ __forceinline__ void step_begin_wg(const StepBegin& q, int wg, int nwg) {
  const u32x4 z4 = {0u, 0u, 0u, 0u};
  {
    const int64_t zid = (int64_t)wg * NT + threadIdx.x, zsz = (int64_t)nwg * NT;
    for (int64_t i = zid; i < q.n16_a; i += zsz) q.zero_a[i] = z4;
    for (int64_t i = zid; i < q.n16_b; i += zsz) q.zero_b[i] = z4;
  }
  if (wg >= q.n_state) return;
  const int64_t gid = (int64_t)wg * NT + threadIdx.x, gsz = (int64_t)q.n_state * NT;
  uint64_t step = 0, s = 0;
  if (q.rng_state) {
    step = q.rng_state[1] + 1;
    s = step_seed(q.rng_state[2], step);
  }
  if (wg == 0 && threadIdx.x == 0 && q.adam_state) {  // nobody else in this launch touches the Adam state
    const int t = q.adam_state[0] + 1;
    q.adam_state[0] = t;
    const double c1 = 1.0 - pow(q.beta1, (double)t), c2 = 1.0 - pow(q.beta2, (double)t);  // double, like the reference
    double lr = q.lr;
    if (q.sched) {
      // the schedule block {beta_t, tau, f_lr, t} of this step: the latent block's backward launch and the step-closing bookkeeping
      // read it in place of their kl_weight constant (a captured graph replays with the weight of ITS step)
      const double f_lr = sched_lr_factor(t, q.lr_warmup);
      lr = q.lr * f_lr;
      q.sched[0] = (float)((double)q.kl_weight * sched_kl_ramp(t, q.kl_warmup, q.kl_cycle));
      q.sched[1] = q.kl_free_bits;
      q.sched[2] = (float)f_lr;
      q.sched[3] = (float)t;
    }
    reinterpret_cast<float*>(q.adam_state)[1] = (float)(lr * sqrt(c2) / c1);
  }
  if (q.eps_out) {
    for (int64_t i = gid; i < (q.n_eps + 1) / 2; i += gsz) {
      const uint32_t a = dropout_hash(s, q.eps_site, (uint64_t)(q.eps_index0 + 2 * i));
      const uint32_t b = dropout_hash(s, q.eps_site, (uint64_t)(q.eps_index0 + 2 * i + 1));
      const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);
      const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
      const float r = sqrtf(-2.0f * logf(u1));
      float sn, cs;
      sincosf(6.283185307179586f * u2, &sn, &cs);
      q.eps_out[2 * i] = r * cs;
      if (2 * i + 1 < q.n_eps) q.eps_out[2 * i + 1] = r * sn;
    }
  }
  // (32-bit quotients: B * S < 2^31 is checked on the host; each thread handles about one element of each mask, and the
  // 64-bit division it used to start with was several hundred instructions)
  if (q.mask_e)
    for (int64_t i = gid; i < q.B * q.Se; i += gsz) {
      const uint32_t b = (uint32_t)i / (uint32_t)q.Se, r = (uint32_t)i - b * (uint32_t)q.Se;
      q.mask_e[i] = ((int64_t)r < (int64_t)q.lens[b] + q.add_e) ? 1 : 0;
    }
  if (q.mask_d)
    for (int64_t i = gid; i < q.B * q.Sd; i += gsz) {
      const uint32_t b = (uint32_t)i / (uint32_t)q.Sd, r = (uint32_t)i - b * (uint32_t)q.Sd;
      q.mask_d[i] = ((int64_t)r < (int64_t)q.lens[b] + q.add_d) ? 1 : 0;
    }
  if constexpr (IN) {
    // keep[r] = dropout_keep(seed of this step, site, index0 + r, p): one byte per decoder input position ...
    for (int64_t r = gid; r < q.in_n; r += gsz) q.in_keep[r] = dropout_keep(s, q.in_site, (uint64_t)(q.in_index0 + r), q.in_p) ? 1 : 0;
    if (q.in_src) {
      // ... and the frames with the dropped rows zeroed, 8 bytes per thread (every thread draws for its own row again: the byte
      // above may be another workgroup's). Two divisions per thread: the (row, chunk) pair advances by a constant.
      const int64_t cpr = q.in_chunks, dr = gsz / cpr, dc = gsz - dr * cpr;
      int64_t r = gid / cpr, c = gid - r * cpr;
      while (r < q.in_n) {
        u32x2 v = {0u, 0u};
        if (dropout_keep(s, q.in_site, (uint64_t)(q.in_index0 + r), q.in_p)) v = *reinterpret_cast<const u32x2*>(q.in_src + r * q.in_ld_src + c * 8);
        *reinterpret_cast<u32x2*>(q.in_dst + r * q.in_ld_dst + c * 8) = v;
        r += dr; c += dc;
        if (c >= cpr) { c -= cpr; ++r; }
      }
    }
  }
  if (q.rng_state) {
    __syncthreads();  // every thread of this workgroup has read the old counter
    if (threadIdx.x == 0) {
      __threadfence();
      const unsigned long long arrived = atomicAdd(reinterpret_cast<unsigned long long*>(q.rng_state + 3), 1ull);
      if (arrived == (unsigned long long)q.n_state - 1) {
        q.rng_state[3] = 0;
        q.rng_state[1] = step;
        q.rng_state[0] = s;
      }
    }
  }
}

// host: validate mst_step_begin_args and pack them; *grid = workgroups of a stand-alone launch (callers hosting the work in another
// launch use min(*grid, what fits)). Returns MST_OK or a status with mst_last_error() set.
static inline int pack_step_begin(const mst_step_begin_args& a, StepBegin& q, int64_t* grid) {
  MST_CHECK_ARG((!a.zero_a || ((uintptr_t)a.zero_a % 16 == 0 && a.zero_a_bytes % 16 == 0)) &&
                    (!a.zero_b || ((uintptr_t)a.zero_b % 16 == 0 && a.zero_b_bytes % 16 == 0)),
                "mst_step_begin: zero buffers must be 16-byte aligned with sizes that are multiples of 16");
  MST_CHECK_ARG(!a.eps_out || (a.rng_state && a.n_eps > 0), "mst_step_begin: eps needs the rng state");
  MST_CHECK_ARG(a.eps_index0 >= 0 && a.eps_index0 % 2 == 0, "mst_step_begin: eps_index0 must be even (Box-Muller pairs)");
  MST_CHECK_ARG((!a.mask_e && !a.mask_d) || (a.lens && a.B > 0), "mst_step_begin: masks need the lengths");
  MST_CHECK_ARG((!a.mask_e || (a.Se > 0 && a.B * a.Se < (1ll << 31))) && (!a.mask_d || (a.Sd > 0 && a.B * a.Sd < (1ll << 31))),
                "mst_step_begin: B * S must stay below 2^31");
  int64_t in_chunks = 0;
  if (a.in_keep) {  // decoder-input dropout (the semantics: include/mst_hip.h)
    MST_CHECK_ARG(a.rng_state, "mst_step_begin: input dropout needs the rng state");
    MST_CHECK_ARG(a.in_p >= 0.f && a.in_p <= 1.f, "mst_step_begin: in_p must lie in [0, 1]");
    MST_CHECK_ARG(a.in_n > 0 && a.in_n < (1ll << 31), "mst_step_begin: in_n must be positive (and below 2^31)");
    MST_CHECK_ARG(a.in_index0 >= 0 && a.in_index0 < (1ll << 31) && a.in_index0 + a.in_n < (1ll << 31),
                  "mst_step_begin: in_index0 must not be negative and in_index0 + in_n must stay below 2^31");
    MST_CHECK_ARG(!a.in_src == !a.in_dst, "mst_step_begin: in_src and in_dst come together");
    if (a.in_src) {
      MST_CHECK_ARG(a.in_row_bytes > 0 && a.in_row_bytes % 8 == 0 && a.in_ld_src % 8 == 0 && a.in_ld_dst % 8 == 0,
                    "mst_step_begin: in_row_bytes, in_ld_src and in_ld_dst must be (positive) multiples of 8");
      MST_CHECK_ARG(a.in_ld_src >= a.in_row_bytes && a.in_ld_dst >= a.in_row_bytes,
                    "mst_step_begin: in_ld_src and in_ld_dst must be at least in_row_bytes");
      MST_CHECK_ARG((uintptr_t)a.in_src % 8 == 0 && (uintptr_t)a.in_dst % 8 == 0, "mst_step_begin: in_src and in_dst must be 8-byte aligned");
      in_chunks = a.in_row_bytes / 8;
    }
  }
  int64_t work = a.n_eps / 2;
  if (a.in_keep && a.in_n > work) work = a.in_n;
  if (in_chunks > 0 && (a.in_n * in_chunks) / 2 > work) work = (a.in_n * in_chunks) / 2;  // (16 bytes of the copy weigh like one mask byte)
  if (a.mask_e && a.B * a.Se > work) work = a.B * a.Se;
  if (a.mask_d && a.B * a.Sd > work) work = a.B * a.Sd;
  const int64_t n16_a = a.zero_a ? a.zero_a_bytes / 16 : 0, n16_b = a.zero_b ? a.zero_b_bytes / 16 : 0;
  if (n16_a > work) work = n16_a;
  if (n16_b > work) work = n16_b;
  // few, fat workgroups: every workgroup ends with one atomic on the SAME arrival counter, and same-address atomics
  // are serialised at ~40 ns each (512 workgroups measured 20 us for this launch)
  int64_t n_state = cdiv(work > 0 ? work : 1, SB_THREADS * 4);
  if (n_state > 64) n_state = 64;
  // (+ workgroups that only clear: 16 KiB of the zero lists each, one per CU at most)
  int64_t g = cdiv(n16_a + n16_b, SB_THREADS);
  if (g > 256) g = 256;
  if (g < n_state) g = n_state;
  *grid = g;
  q = StepBegin{a.rng_state, a.adam_state, a.lr, a.beta1, a.beta2, a.eps_out, a.n_eps, a.eps_site, a.eps_index0, a.lens, a.B,
                a.mask_e, a.Se, a.add_e, a.mask_d, a.Sd, a.add_d, (u32x4*)a.zero_a, n16_a, (u32x4*)a.zero_b, n16_b, (int)n_state,
                nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0.f, 0.f, 0, 0, 0,
                nullptr, 0, 0.f, 0u, 0, nullptr, 0, nullptr, 0, 0};
  if (a.in_keep) {
    q.in_keep = a.in_keep; q.in_n = a.in_n; q.in_p = a.in_p; q.in_site = a.in_site; q.in_index0 = a.in_index0;
    if (in_chunks > 0) { q.in_src = a.in_src; q.in_ld_src = a.in_ld_src; q.in_dst = a.in_dst; q.in_ld_dst = a.in_ld_dst; q.in_chunks = in_chunks; }
  }
  if (a.sched) {
    MST_CHECK_ARG(a.adam_state, "mst_step_begin: the schedule block is a function of Adam's step count (adam_state)");
    MST_CHECK_ARG(a.sched_kl_warmup >= 0 && a.sched_kl_cycle >= 0 && a.sched_lr_warmup >= 0 && a.sched_kl_free_bits >= 0.f,
                  "mst_step_begin: schedule lengths and the free bits must not be negative");
    MST_CHECK_ARG(a.sched_kl_cycle == 0 || (a.sched_kl_warmup > 0 && a.sched_kl_warmup <= a.sched_kl_cycle),
                  "mst_step_begin: a KL cycle needs a warm-up no longer than the cycle");
    q.sched = a.sched; q.kl_weight = a.sched_kl_weight; q.kl_free_bits = a.sched_kl_free_bits;
    q.kl_warmup = a.sched_kl_warmup; q.kl_cycle = a.sched_kl_cycle; q.lr_warmup = a.sched_lr_warmup;
  }
  if (a.sh_w) {
    MST_CHECK_ARG(a.sh_wt16 && a.sh_desc && a.sh_prefix && a.sh_n_mat > 0 && a.sh_tiles > 0 && a.sh_tiles < (1ll << 30),
                  "mst_step_begin: the shadow refresh needs w, wt16, the matrix table and its tile prefix sums");
    q.sh_w = a.sh_w; q.sh_wt16 = a.sh_wt16; q.sh_desc = a.sh_desc; q.sh_prefix = a.sh_prefix; q.sh_n_mat = (int)a.sh_n_mat; q.sh_tiles = a.sh_tiles;
  }
  return MST_OK;
}

}  // namespace mst

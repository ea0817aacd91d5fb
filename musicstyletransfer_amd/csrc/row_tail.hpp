// row_tail.hpp — what the two position-0 tail kernels (row_tail_fwd.hpp, row_tail_bwd.hpp; one translation unit: row_tail.hip)
// share: the grid barrier and the visibility protocol, the join onto one XCD, the riders, and the row helpers.
//
// HOW ROWS CROSS A GRID BARRIER. A tail is D / 16 workgroups that meet at grid-wide barriers and hand rows to each other
// through memory. Each XCD has an L2 of its own, not coherent with the others', so:
//   - ONE XCD. The kernels launch 12 x more workgroups than they need and let them JOIN (tail_join): the first arrival
//     claims its XCD (s_getreg XCC_ID) with a compare-and-swap, workgroups on that XCD take the roles 0..G-1 in arrival
//     order, everybody else leaves at once (or rides, below). All participants then share one L2.
//   - WRITE-THROUGH TO THAT L2. The bytes that cross a barrier are written through the CU's L1 (sc0 stores: store8_l2 /
//     store4_l2) and are complete — s_waitcnt vmcnt(0), the first thing grid_sync does — before the workgroup arrives.
//   - FIRST-TOUCH LOADS BEHIND IT. What makes the loads behind the barrier safe is NOT a cache-bypass bit (a polling loop
//     of sc0 loads was tried for the barrier counter and kept reading its first value: the L1 serves repeats) but that every
//     such line is read by a CU for the FIRST time since the L1 invalidate at kernel start — each stage's operand rows are
//     new to the workgroup that loads them, and the L1 does not allocate on the write-through of a partial line (the 32-byte
//     column slices a workgroup itself stored: parity tests cover exactly that) — so the load misses and is served by the
//     shared L2.
//   - THE COUNTER STAYS AGENT-SCOPE. ONE lane per workgroup adds to it and polls it with relaxed agent-scope loads (bounded),
//     and the workgroup barriers again before anyone loads.
// Correct for ANY dispatch order (participants share an XCD by construction; a launch that put fewer than G workgroups on the
// claimed XCD would leave the bounded barrier spin and fail the step's parity, not hang). Weights, att and the residual come
// from earlier launches and are read with plain loads.
// Two forms came before and are gone. With fences (a release is a write-back of the XCD's L2, an acquire an invalidate of
// the CU's L1) a barrier cost ~8 us, 38 us in all — the five launches took 43. Without fences but with the G workgroups dealt
// round-robin over the eight XCDs, every crossing byte was an agent-scope (sc1) store or load, served BEHIND the L2s: 8 us
// over the fabric for the 128 KB of stage 3, 3-5 us per barrier waiting for write-through acknowledgements from memory.
#pragma once
#include <math.h>
#include "common.hpp"
#include "gemm_tile.hpp"
#include "shadows.hpp"

namespace mst {

// Status bits left in the caller's sticky device word (mst_row_tail_*_args.status, optional) when a launch could not do its work:
//   1 / 2   a grid barrier of the forward / backward kernel gave up waiting (fewer than G workgroups of the launch were placed
//           on the claimed XCD — CU masks, another partition mode, a co-tenant holding the CUs — so the rows behind it are stale)
// A launch in which NOBODY got a role (sync words not zeroed) cannot flag itself; it leaves its barrier counter short, which is
// what the step guard of the optimizer launch checks (mst_step_metrics.expect_ptr: MST_STEP_INCOMPLETE).
// The optimizer launch of the same step reads the word and leaves parameters, moments and the step count untouched when it is
// set (mst_step_metrics.status), and the host switches to the five-launch form: a failed tail costs skipped batches, never a
// silently wrong update.
// (MST_TAIL_SPIN_FWD / _BWD of include/mst_hip.h)
#ifndef MST_TAIL_SPIN_TICKS
#define MST_TAIL_SPIN_TICKS 20000000ull /* 0.2 s of the 100 MHz s_memrealtime clock; a healthy barrier waits microseconds */
#endif

__device__ __forceinline__ void grid_sync(uint32_t* ctr, uint32_t target, uint32_t* status, uint32_t spin_bit) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's write-through stores have completed
  __syncthreads();
  if (threadIdx.x == 0) {
    // (agent-scope counter operations even though the participants share an XCD: an atomic add without scope bits + sc0 polling
    // loads was tried and is NOT reliable — most launches sat out the spin bound)
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t spins = 0;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 255u) == 0u) {  // (a healthy barrier waits microseconds and never gets here)
        // a run that is ALREADY flagged (this launch's earlier barrier, or a step before it that the host has not looked at
        // yet) does not sit out the bound again at every barrier of every following step: its result is discarded anyway
        if (status && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > MST_TAIL_SPIN_TICKS) {
          // never in a correct launch; a bound instead of a hung GPU — and a flag instead of a silently wrong step
          if (status) __hip_atomic_fetch_or(status, spin_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
  }
  __syncthreads();
}

// The accesses of the bytes that cross a grid barrier: write-through stores, and loads WITHOUT the wait hipcc would put behind
// each (sixteen rows read one after the other were sixteen exposed L2 round trips: 4.8 us of stage 2): issue a batch with
// *_nowait, then l2_wait on the destinations — the values may be used only behind that wait (its "+v" operands make every use
// depend on it).
__device__ __forceinline__ void store8_l2(void* p, u32x2 v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc0" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store4_l2(void* p, uint32_t v) {
  asm volatile("global_store_dword %0, %1, off sc0" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void load16_l2_nowait(u32x4& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off sc0" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void load8_l2_nowait(u32x2& dst, const void* p) {
  asm volatile("global_load_dwordx2 %0, %1, off sc0" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void load4_l2_nowait(uint32_t& dst, const void* p) {
  asm volatile("global_load_dword %0, %1, off sc0" : "=v"(dst) : "v"(p) : "memory");
}
template <typename V, int N>
__device__ __forceinline__ void l2_wait(V (&r)[N]) {  // the *_nowait destinations may be used only behind this
  static_assert(N == 1 || N == 2 || N == 4 || N == 8, "batch size");
  if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]) : : "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]), "+v"(r[1]) : : "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : : "memory");
}
// the one agent-scope (sc1) load left: tail_drain's early look at the rider queue, whose atomics live behind the L2s
__device__ __forceinline__ void load4_sc1_nowait(uint32_t& dst, const void* p) {
  asm volatile("global_load_dword %0, %1, off sc1" : "=v"(dst) : "v"(p) : "memory");
}

template <typename T>
__device__ __forceinline__ typename Act<T>::vec8 frag16(const T* p, bool ok) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (ok) v = *reinterpret_cast<const u32x4*>(p);
  return __builtin_bit_cast(typename Act<T>::vec8, v);
}

// wave_sum of N independent values at once: the six cross-lane steps of all of them interleaved. One after the other
// (16 rows x 2 sums x 6 dependent permutes, alone on its SIMD) the LayerNorm of 16 rows took 8.7 us.
template <int N>
__device__ __forceinline__ void wave_sum_batch(float (&v)[N]) {
  // level by level over all N values (DPP adds, one swizzle, one permute each: common.hpp group_sum), so that the N chains overlap
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0xB1>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x4E>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x141>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x140>(v[i]);
  float t[N];
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = lane_xor16(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += t[i];
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = __shfl_xor(v[i], 32, 64);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += t[i];
}

// diagnostic build only (-DMST_TAIL_STAMPS): workgroup 0 leaves s_memrealtime stamps (100 MHz) in a device array of its own, read
// back with mst_debug_tail_stamps (they used to go behind the caller's three sync words, i.e. out of bounds for any caller but
// the stamp tools)
#ifdef MST_TAIL_STAMPS
__device__ uint32_t g_tail_stamps[32];
#define TAIL_STAMP(i) do { if (g == 0 && threadIdx.x == 0 && (i) < 32) g_tail_stamps[(i)] = (uint32_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TAIL_STAMP(i) do { } while (0)
#endif

// The join onto one XCD (the protocol at the top of this file).
// sync: [0] barrier counter, [1] claimed XCD + 1, [2] roles handed out (all zero at launch).
constexpr int TAIL_OVERSUBSCRIBE = 12;  // 8 is exact under round-robin dispatch; measured 8 / 10 / 12 / 16: 0.7245 / 0.7234 / 0.7256 / 0.7256 ms per step
__device__ __forceinline__ int tail_join(uint32_t* sync, int G) {
  __shared__ int role;
  if (threadIdx.x == 0) {
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc = (xcc & 0xFu) + 1u;
    uint32_t seen = 0u;
    __hip_atomic_compare_exchange_strong(sync + 1, &seen, xcc, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t claimed = seen == 0u ? xcc : seen;
    int r = -1;  // -1: another XCD (free to do riding work), -2: the claimed XCD without a role (leaves: its L2 is the chain's)
    if (claimed == xcc) {
      const uint32_t k = __hip_atomic_fetch_add(sync + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r = k < (uint32_t)G ? (int)k : -2;
    }
    role = r;
  }
  __syncthreads();
  return role;
}

// RIDERS. A tail launch keeps ONE XCD busy for ~26 us of dependent round trips while seven idle. Work that nothing in the chain
// waits for can use them: the workgroups that join on another XCD, instead of leaving, take 128 x 128 tiles of ONE GEMM
// (mst_gemm_args `g`: the decoder's K | Q | V projection of rows 1..T behind the forward tail, the input gradient of that
// projection behind the backward tail — both were launches of their own in the step's dependent chain, 12 and 10 us) from a
// work queue (`counter`: a zeroed device word in a cache line of its OWN — next to the barrier words, the riders' first 224 ticket
// atomics queued in front of the chain's barrier arrivals: +3 us on the launch) until it is empty. 16 waves as a 2 x 8 grid of 64 x 16 wave tiles, the
// tile code of gemm_nt.hip (gemm_tile.hpp); the tails' own participants never touch it. A tile's result does not depend on who
// computes it or when, so the launch stays deterministic; and the chain's own participants pass by the queue when they are done
// (normally empty by then), so every tile is computed by the end of the launch even if NO workgroup landed on another XCD.
// BM = 256 (4 x 4 waves of 64 x 32, the epilogue staged one 64-row block at a time): for GEMMs with more 128 x 128 tiles than riders —
// a tile is a chain of dependent latencies (~9 us whatever its size) and a 16-wave workgroup has a CU to itself, so ONE round of
// bigger tiles ends long before two rounds of small ones (the decoder projection: 192 tiles on 224 riders instead of 384).
// ... and BEHIND the GEMM's tiles in the same queue (forward tail only): the step's transposed 16-bit shadow refresh (shadows.hpp; the
// matrices only the backward pass reads — nothing in this launch reads them), sixteen 32 x 32 tiles per ticket, four per 256 threads with
// their loads requested together (68 KB of the rider's LDS; at four tiles per ticket the refresh was two rounds of round trips and the
// chain's participants met an unfinished queue). On the
// step's first launch they were 4.9 us of its 24; here they run on compute units that have nothing else to do until the chain ends.
struct TailShadow {
  const float* w; void* wt16; const int64_t* desc; const int64_t* prefix; int n_mat; int n_groups; int64_t tiles;
};
// (a function of its own, not inlined: inside the tail kernel its index arithmetic raised the kernel's register pressure and the
// allocator spilled 49 registers instead of 18 — some of them in the chain's stages: forward tail 34 -> 42 us)
template <typename T>
__device__ __attribute__((noinline)) void tail_shadow_ticket(const TailShadow& sh, int grp, unsigned char* smem) {
  const int quarter = threadIdx.x >> 8;
  shadow_tile_quad<T>(sh.w, reinterpret_cast<T*>(sh.wt16), sh.desc, sh.prefix, sh.n_mat, (int64_t)grp * 16 + 4 * quarter, sh.tiles,
                      reinterpret_cast<float(*)[32][33]>(smem) + 4 * quarter, threadIdx.x & 255);
}
template <typename T, int BM>
__device__ __forceinline__ void tail_ride_bm(const mst_gemm_args& g, int n_tiles, uint32_t* counter, unsigned char* smem, const TailShadow& sh) {
  constexpr int BN = 128, WGM = BM == 256 ? 4 : 2, WGN = 16 / WGM, PATH = BM == 256 ? 4 : 1;
  __shared__ int s_tile;
  for (;;) {
    if (threadIdx.x == 0) s_tile = (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int tile = s_tile;
    if (tile >= n_tiles) {
      const int grp = tile - n_tiles;
      if (grp >= sh.n_groups) return;
      tail_shadow_ticket<T>(sh, grp, smem);
      __syncthreads();  // (the tile buffers and s_tile are rewritten)
      continue;
    }
    f32x4 acc[(BN / WGN) / 16][(BM / WGM) / 16];
    int64_t m0, n0;
    float bias_pre[8];
    gemm_bias_preload<BM, BN>(g, bias_pre, tile);
    gemm_mainloop<T, BM, BN, WGM, WGN, 64, true, false>(g, smem, acc, m0, n0, tile);
    gemm_epilogue<T, BM, BN, WGM, WGN, false, true, PATH, false>(g, smem, acc, m0, n0, bias_pre);
    __syncthreads();  // (the epilogue's staging tile is the next tile's first K stage; s_tile is rewritten)
  }
}

// The chain's participants at the end of their kernel: every tile of the rider must have been HANDED OUT by then (whoever took one
// finishes it before the launch ends). The queue counter is looked at with a load requested at the START of the chain's last stage
// (`seen`, thread 0; sc1: the riders' atomics live behind the L2s) — normally it already shows an empty queue and the participants
// leave without another round trip (an atomic here cost the launch ~2 us); if it does not — or if no workgroup ever landed on
// another XCD, so that nobody rode — they take tiles themselves until the queue is empty.
template <typename T, int BM>
__device__ __forceinline__ void tail_drain(const mst_gemm_args& g, int n_tiles, uint32_t* counter, uint32_t& seen, unsigned char* smem,
                                           const TailShadow& sh) {
  __shared__ int s_drain;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(seen) : : "memory");
    s_drain = seen < (uint32_t)(n_tiles + sh.n_groups);
  }
  __syncthreads();
  if (s_drain) tail_ride_bm<T, BM>(g, n_tiles, counter, smem, sh);
}

// Sixteen waves per workgroup (four per SIMD): every stage is a chain of dependent L2 round trips, and with one wave per
// SIMD nothing ran under them (four waves: forward 30 us, backward 43 us against 39 for its five launches). Wave (mi, wq):
// row block mi = wave & 3 (rows 16 mi .. 16 mi + 15 in the MFMA stages), quarter wq = wave >> 2 — the 64-column slices are
// split by 16-column block, the 16-column slices by quarter of K (partial accumulators meet in LDS); the LayerNorms take
// four rows per wave.
constexpr int TAIL_WAVES = 16;
// partial 16-column accumulators of the four K quarters -> their sum on the waves of quarter 0 (sP: [4][64][16] floats)
__device__ __forceinline__ f32x4 quarter_sum(float* sP, const f32x4& part, int wq, int m, int lq) {
  *reinterpret_cast<f32x4*>(sP + (wq * 64 + m) * 16 + 4 * lq) = part;
  __syncthreads();
  f32x4 acc = part;
  if (wq == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(sP + (w * 64 + m) * 16 + 4 * lq);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += o[e];
    }
  }
  return acc;
}

// E consecutive 16-bit elements of a row as one word: E = 4 (u32x2) is a lane's share of a D = 256 row in the LayerNorms and a
// lane's four output columns of an MFMA stage, E = 2 (uint32_t) a lane's share of a D = 128 row. The kernels are
// allocator-sensitive: each use of these was checked to leave the device code as it was, and the few sites that spell the
// same thing out say so. (pack_bits takes its elements by value: taking the array by reference changed code generation.)
template <int E> using row_raw = typename std::conditional<E == 4, u32x2, uint32_t>::type;
__device__ __forceinline__ uint32_t pack_bits(uint16_t b0, uint16_t b1) { return (uint32_t)b0 | ((uint32_t)b1 << 16); }
__device__ __forceinline__ u32x2 pack_bits(uint16_t b0, uint16_t b1, uint16_t b2, uint16_t b3) {
  return u32x2{(uint32_t)b0 | ((uint32_t)b1 << 16), (uint32_t)b2 | ((uint32_t)b3 << 16)};
}
template <typename T, int E>
__device__ __forceinline__ row_raw<E> row_pack(const float (&v)[E]) {
  if constexpr (E == 4) return u32x2{(uint32_t)f32_to_bits<T>(v[0]) | ((uint32_t)f32_to_bits<T>(v[1]) << 16),
                                     (uint32_t)f32_to_bits<T>(v[2]) | ((uint32_t)f32_to_bits<T>(v[3]) << 16)};
  else return (uint32_t)f32_to_bits<T>(v[0]) | ((uint32_t)f32_to_bits<T>(v[1]) << 16);
}
template <typename T, int E>
__device__ __forceinline__ void row_unpack(row_raw<E> t, float (&v)[E]) {
  if constexpr (E == 4) {
    v[0] = bits_to_f32<T>((uint16_t)(t[0] & 0xffff)); v[1] = bits_to_f32<T>((uint16_t)(t[0] >> 16));
    v[2] = bits_to_f32<T>((uint16_t)(t[1] & 0xffff)); v[3] = bits_to_f32<T>((uint16_t)(t[1] >> 16));
  } else {
    v[0] = bits_to_f32<T>((uint16_t)(t & 0xffff)); v[1] = bits_to_f32<T>((uint16_t)(t >> 16));
  }
}
template <typename T, int E>
__device__ __forceinline__ void row_load_l2_nowait(row_raw<E>& dst, const T* p) {
  if constexpr (E == 4) load8_l2_nowait(dst, p);
  else load4_l2_nowait(dst, p);
}
template <typename T, int E>
__device__ __forceinline__ void row_store(T* dst, row_raw<E> v, bool through) {  // `through`: another workgroup reads it behind a grid barrier
  if constexpr (E == 4) { if (through) store8_l2(dst, v); else *reinterpret_cast<u32x2*>(dst) = v; }
  else { if (through) store4_l2(dst, v); else *reinterpret_cast<uint32_t*>(dst) = v; }
}

}  // namespace mst

// The placement sort on the device: which robot sits in which slot of the next launch, from the iteration counts
// of the last one -- as launches of their own (placement_hist_kernel, placement_kernel) and as extra wavefronts in the shadow of
// a placed balance launch (placement_wave, called from balance_coop_body.hpp).  Included by balance_kernel.hip alone, whose
// translation unit these kernels belong to; the host side -- their launches and the public entry -- is at the end.
#pragma once

#include "balance_coop.hpp"
#include "context.hpp"

#include <type_traits>

namespace {
using namespace qlamd;
using namespace qlamd::rt;

// Placement of the robots into the slots of the next launch from the iteration counts of the last one
// (qlamd_placement_from_iterations): a stable counting sort by iteration count, hardest first (ties by robot index), then
// the slot of each rank by policy:
//   throughput  slot = rank: four neighbours of the sorted list share a wavefront.  The union of four similar add / drop
//               sequences is the shortest there is, which is what counts once every SIMD holds several wavefronts, and the
//               long wavefronts start first.
//   latency     the hardest quarter one per wavefront (row 0 of wavefront r = rank r), each joined by the three easiest
//               robots still to be had (rank B-1-e sits in row 1 + e % 3 of wavefront e / 3): a launch of one wavefront
//               per SIMD lasts as long as its slowest wavefront, and next to three robots that finish early a hard robot
//               runs at the speed it has alone (finished rows ride along as ghost rows, force_qp_coop.hpp).
// It sits between two control steps of a caller that wants the hint used at once, so it is built for latency: one
// workgroup of 1024 lanes takes 1024 G consecutive robots, robot g * 1024 + lane in its round g.  A robot's ordinal among
// the robots of its wavefront and round with the same count is the return value of ONE LDS atomic on the counter
// [bin][round][wavefront] (the lanes of one instruction that meet on an address are served in lane order); an exclusive
// scan over the 512 G counters in (bin, round, wavefront) order turns them into first ranks; rank -> slot -> one store.
// Batches beyond 4096 robots take several workgroups, which need the counts of the other workgroups per bin: a first
// launch (placement_hist_kernel) leaves them in the context's scratch.
constexpr int kPlaceThreads = 1024, kPlaceWaves = kPlaceThreads / 64, kPlaceBins = 24, kPlaceRounds = 4;
__device__ __forceinline__ int place_bin(int v) { // bin 0 = hardest (the clamp compiles to one v_med3_i32)
  const int h = v < 0 ? 0 : (v >= kPlaceBins ? kPlaceBins - 1 : v);
  return kPlaceBins - 1 - h;
}
// The launches of their own also know a robot's CLASS when the caller's support flags are at hand (`support`: [B][4] bytes
// read as one word per robot; NULL: one class): robots on more than two legs first, then the robots on at most two --
// whose wavefronts then take the 6-variable form of the QP (balance_coop.hpp, "support legs first": a wavefront takes it
// only when all four of its robots can).  Key = class * kPlaceBins + bin; sorted placement only (placing the hardest
// robots one per wavefront mixes the classes by design).
constexpr int kPlaceKeys = 2 * kPlaceBins;
__device__ __forceinline__ int place_class(uint32_t support_word) { return support_legs(support_word) <= 2 ? kPlaceBins : 0; }
__device__ __forceinline__ int place_key(int v, const uint32_t *__restrict__ support, int64_t i) {
  int key = place_bin(v);
  if (support) {
    key += place_class(support[i]);
  }
  return key;
}
__global__ __launch_bounds__(kPlaceThreads) void placement_hist_kernel(const int32_t *__restrict__ iters, int64_t B, int64_t per_block,
                                                                      const uint32_t *__restrict__ support,
                                                                      uint32_t *__restrict__ blockhist) {
  __shared__ uint32_t h[kPlaceKeys];
  if (threadIdx.x < kPlaceKeys) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < B ? lo + per_block : B;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kPlaceThreads) atomicAdd(&h[place_key(iters[i], support, i)], 1u);
  __syncthreads();
  if (threadIdx.x < kPlaceKeys) blockhist[(int64_t)blockIdx.x * kPlaceKeys + threadIdx.x] = h[threadIdx.x];
}
template <int G>
__global__ __launch_bounds__(kPlaceThreads) void placement_kernel(const int32_t *__restrict__ iters, int64_t B, int throughput,
                                                                 const uint32_t *__restrict__ support,
                                                                 const uint32_t *__restrict__ blockhist, int32_t *__restrict__ order) {
  constexpr int kN = kPlaceKeys * G * kPlaceWaves, kPer = (kN + kPlaceThreads - 1) / kPlaceThreads; // counters, counters per lane in the scan
  __shared__ uint32_t cnt[kN];
  __shared__ uint32_t wtot[kPlaceWaves];
  __shared__ uint32_t bin_base[kPlaceKeys];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t first = (int64_t)blockIdx.x * (kPlaceThreads * G);
  int v[G];
#pragma unroll
  for (int g = 0; g < G; g++) { // all loads in flight before the first atomic
    const int64_t i = first + g * kPlaceThreads + t;
    v[g] = i < B ? place_key(iters[i], support, i) : -1;
  }
#pragma unroll
  for (int k = 0; k < kPer; k++)
    if (t + k * kPlaceThreads < kN) cnt[t + k * kPlaceThreads] = 0;
  __shared__ uint32_t tot[kPlaceKeys], before[kPlaceKeys];
  if (gridDim.x > 1) {
    // several workgroups: robots of the harder bins anywhere, and of my bin in the workgroups before mine
    if (t < kPlaceKeys) { tot[t] = 0; before[t] = 0; }
    __syncthreads();
    for (unsigned e = t; e < gridDim.x * kPlaceKeys; e += kPlaceThreads) {
      const unsigned blk = e / kPlaceKeys, b = e - blk * kPlaceKeys;
      const uint32_t c = blockhist[e];
      atomicAdd(&tot[b], c);
      if (blk < blockIdx.x) atomicAdd(&before[b], c);
    }
    __syncthreads();
    if (t < kPlaceKeys) {
      uint32_t harder = 0;
      for (int b = 0; b < kPlaceKeys; b++) harder += b < t ? tot[b] : 0u;
      bin_base[t] = harder + before[t];
    }
  }
  __syncthreads();
  uint32_t ord[G];
#pragma unroll
  for (int g = 0; g < G; g++) ord[g] = v[g] >= 0 ? atomicAdd(&cnt[(v[g] * G + g) * kPlaceWaves + wave], 1u) : 0u;
  __syncthreads();
  // exclusive scan of the counters in place: kPer consecutive counters per lane, then lanes, then wavefronts
  uint32_t c[kPer], mine = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) { c[k] = t * kPer + k < kN ? cnt[t * kPer + k] : 0u; mine += c[k]; }
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    incl += lane >= d ? o : 0u;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint32_t run = incl - mine;
#pragma unroll
  for (int w = 0; w < kPlaceWaves; w++) run += w < wave ? wtot[w] : 0u;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    if (t * kPer + k < kN) cnt[t * kPer + k] = run;
    run += c[k];
  }
  __syncthreads();
  const int64_t W = (B + 3) / 4;
#pragma unroll
  for (int g = 0; g < G; g++) {
    if (v[g] < 0) continue;
    int64_t r = cnt[(v[g] * G + g) * kPlaceWaves + wave] + ord[g];
    if (gridDim.x > 1) r += (int64_t)bin_base[v[g]] - cnt[v[g] * G * kPlaceWaves]; // my workgroup's harder bins come off
    int64_t slot = r;
    if (!throughput) {
      const int64_t e = B - 1 - r;
      slot = r < W ? 4 * r : 4 * (e / 3) + 1 + e % 3;
    }
    order[slot] = (int32_t)(first + g * kPlaceThreads + t);
  }
}

// The same placement inside a placed launch, for the extra workgroups it carries when the caller asks for the next launch's
// placement (qlamd_placement::next_robot_order): they run in the shadow of the solve -- a launch of a few thousand robots
// lasts 9-24 us, one of these wavefronts a few us for its 1024 robots -- instead of as launches of their own between two
// control steps (6-9 us).  One wavefront (= workgroup) per `chunk` robots, the first workgroups of the grid:
// rounds of 64 robots; counters [key][round] in the workgroup's LDS (the solve's 13.5 KB).  Pass 1 counts (LDS atomics
// without a return value), an exclusive scan in (key, round) order turns the counters into first ranks within the chunk,
// pass 2 takes each robot's rank as the return value of one more atomic on its counter (lanes that meet on a counter are
// served in lane order: rank order = index order within a key).  With several chunks a wavefront needs the others' counts
// per key between the scan and pass 2: each leaves its own in the context's scratch and they meet at a barrier in global
// memory (arrivals + generation, agent scope; the workgroups in front of a grid are dispatched first and all at once, so
// they can wait for each other; the barrier resets itself, so a hipGraph can replay the launch).  Keys: the iteration
// count's bin, and with a sorted placement also the robot's class (place_key: robots on more than two legs first).
// A lone wavefront issues one instruction per ~5.5 cycles and waits out every memory round trip, so the loop bodies are
// counted in instructions (32-bit index arithmetic, the division by 3 as a multiplication, one clamp per count),
// kShadowChunk rounds have their loads in flight together, and the last, ragged rounds are the only ones that check
// indices.  Measured and dropped (profiles/r5/placed_probe.txt): ONE atomic pass whose return values are kept until the
// scan is done -- in registers (13 000 instructions of unrolled code), as bytes in LDS (16 us at 4096 robots: sub-word LDS
// stores) or as words of four rounds (14.6 us, and 16 KB of LDS per workgroup cost every placed launch 0.3 us).
constexpr int kShadowLdsBytes = (4 * kTabPerLeg + 4 * coop::kCoopLdsDoubles + coop::kCoopNrmDoubles) * 8;
// robots per shadow wavefront.  Below the throughput form's batches: 1024 with a warm start (4096 robots: 4 wavefronts, 6 us
// -- shorter than the shortest solve, a warm-started calm batch's 9.5 us), 2048 without (8 us against the 13.4 us of a calm
// batch solved cold: every shadow wavefront shares a SIMD with a wavefront that solves, and two of them cost the placed
// loop of 4096 robots 0.3 us less than four: profiles/r5/ab_shadow_blocks.txt).  4096 from there (65 536 robots: 16
// wavefronts, 13 us of a 70 us launch; with 64 of them every one reads 64 x 48 counts and the launch is 3-5 us longer).
constexpr int kShadowChunkWarm = 1024, kShadowChunkCold = 2048, kShadowChunkLarge = 4096, kShadowMaxBlocks = 256;
static_assert((kShadowChunkLarge / 64) * kPlaceKeys * 4 + kPlaceKeys * 4 <= kShadowLdsBytes, "the shadow wavefront's counters live in the solve's LDS");
constexpr int kShadowChunk = 16; // rounds whose loads are in flight together: a chunk's 1024 robots
typedef __attribute__((address_space(3))) uint32_t lds_u32; // (a generic pointer would turn the atomics into flat ones)
template <bool kThroughput>
__device__ __forceinline__ uint32_t place_slot(uint32_t rk, uint32_t B, uint32_t W) {
  if constexpr (kThroughput) return rk;
  const uint32_t e = B - 1u - rk, q = __umulhi(e, 0xAAAAAAABu) >> 1; // e / 3
  return rk < W ? 4u * rk : 4u * q + 1u + (e - 3u * q);
}
// sidx of S: my chunk; support: the robots' support flags when the keys carry the class (sorted placement), else NULL
__device__ __forceinline__ void placement_wave(const int32_t *__restrict__ iters, int64_t B64, int throughput,
                                               int32_t *__restrict__ order, lds_u32 *cnt, uint32_t sidx, uint32_t S,
                                               uint32_t chunk, const uint32_t *__restrict__ support, uint32_t *__restrict__ ghist,
                                               uint32_t *__restrict__ gsync, uint32_t max_polls) {
  const uint32_t lane = threadIdx.x & 63u, B = (uint32_t)B64, W = (B + 3u) >> 2;
  const uint32_t lo = sidx * chunk;
  const uint32_t n = lo >= B ? 0u : (B - lo < chunk ? B - lo : chunk); // my robots
  const uint32_t R = (n + 63u) >> 6, full = n >> 6;      // rounds, rounds without a missing robot
  const bool classes = throughput && support != nullptr;
  const uint32_t nkeys = classes ? kPlaceKeys : kPlaceBins, N = nkeys * R; // counters
  lds_u32 *adj = cnt + N;                                // what turns a rank within the chunk into the rank of the batch, per key
  for (uint32_t k = lane; k < N + nkeys; k += 64) cnt[k] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const auto run = [&](auto Classes, auto Thr) {
    constexpr bool kClasses = decltype(Classes)::value, kThr = decltype(Thr)::value;
    const auto key_of = [&](int v, uint32_t w) -> uint32_t {
      uint32_t key = (uint32_t)place_bin(v);
      if constexpr (kClasses) key += (uint32_t)place_class(w);
      return key;
    };
    // one pass over my robots: kPass 1 counts, kPass 2 ranks and stores
    const auto pass = [&](auto Pass) {
      constexpr int kPass = decltype(Pass)::value;
      for (uint32_t r0 = 0; r0 < R; r0 += kShadowChunk) {
        if (r0 + kShadowChunk <= full) {
          int v[kShadowChunk];
          uint32_t w[kShadowChunk], rk[kShadowChunk];
#pragma unroll
          for (int k = 0; k < kShadowChunk; k++) {
            v[k] = iters[lo + (r0 + k) * 64u + lane];
            w[k] = kClasses ? support[lo + (r0 + k) * 64u + lane] : 0u;
          }
#pragma unroll
          for (int k = 0; k < kShadowChunk; k++) {
            const uint32_t key = key_of(v[k], w[k]);
            w[k] = key;
            lds_u32 *c = cnt + key * R + (r0 + k);
            if constexpr (kPass == 1) (void)__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else rk[k] = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          if constexpr (kPass == 2) {
#pragma unroll
            for (int k = 0; k < kShadowChunk; k++)
              order[place_slot<kThr>(rk[k] + adj[w[k]], B, W)] = (int32_t)(lo + (r0 + k) * 64u + lane);
          }
        } else {
          for (uint32_t r = r0; r < R && r < r0 + kShadowChunk; r++) {
            const uint32_t i = r * 64u + lane;
            if (i < n) {
              const uint32_t key = key_of(iters[lo + i], kClasses ? support[lo + i] : 0u);
              lds_u32 *c = cnt + key * R + r;
              if constexpr (kPass == 1) (void)__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              else {
                const uint32_t rk = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                order[place_slot<kThr>(rk + adj[key], B, W)] = (int32_t)(lo + i);
              }
            }
          }
        }
      }
    };
    pass(std::integral_constant<int, 1>{});
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // ---- exclusive scan in (key, round) order: `per` consecutive counters per lane
    {
      const uint32_t per = (N + 63u) >> 6, k0 = lane * per, k1 = k0 + per < N ? k0 + per : N;
      uint32_t mine = 0;
      for (uint32_t k = k0; k < k1; k++) mine += cnt[k];
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        incl += lane >= (uint32_t)d ? o : 0u;
      }
      uint32_t running = incl - mine;
      for (uint32_t k = k0; k < k1; k++) { const uint32_t c = cnt[k]; cnt[k] = running; running += c; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (S > 1) {
      // ---- the other chunks: lane k < nkeys owns key k.  My count of it goes to the scratch, the barrier, then
      //      rank of the batch = robots of harder keys anywhere + robots of my key in the chunks before mine + rank in my chunk
      const uint32_t start = (lane < nkeys && R > 0) ? cnt[lane * R] : 0u;
      const uint32_t next = (lane + 1u < nkeys && R > 0) ? cnt[(lane + 1u) * R] : n;
      if (lane < nkeys) __hip_atomic_store(ghist + sidx * kPlaceKeys + lane, R > 0 ? next - start : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      // The barrier: arrivals in gsync[0], its state in gsync[1].  A launch finds the state at an even value g and leaves it at
      // g + 2 (everybody arrived: the last one says so) or at g + 4 (somebody gave up waiting -- g + 1, odd -- and the last one
      // to arrive closed the launch).  Both transitions away from g are compare-and-swaps, so a launch has ONE outcome, and
      // every wavefront can tell which whenever it looks (odd: given up; g + 2: complete; g + 4: given up and closed).  The
      // waiting is bounded (a second or two: a device shared with something that keeps these wavefronts from running together
      // must not hang), and a launch that gives up writes the identity order -- a valid placement, which costs the next launch
      // time, never a result.
      int gave_up = 0;
      if (lane == 0) {
        const uint32_t g = __hip_atomic_load(gsync + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t arrived = __hip_atomic_fetch_add(gsync, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = arrived == S - 1u;
        if (last) __hip_atomic_store(gsync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g & 1u) { // somebody gave up before I got here
          gave_up = 1;
          if (last) __hip_atomic_store(gsync + 1, g + 3u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else if (last) {
          uint32_t now = g;
          if (!__hip_atomic_compare_exchange_strong(gsync + 1, &now, g + 2u, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) {
            __hip_atomic_store(gsync + 1, g + 4u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            gave_up = 1;
          }
        } else {
          uint32_t now = g;
          for (unsigned spin = 0;; spin++) {
            now = __hip_atomic_load(gsync + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (now != g) break;
            if (spin >= max_polls) {
              if (__hip_atomic_compare_exchange_strong(gsync + 1, &now, g + 1u, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) now = g + 1u;
              break; // (lost the exchange: `now` holds what the winner wrote)
            }
            __builtin_amdgcn_s_sleep(4);
          }
          gave_up = now != g + 2u ? 1 : 0;
        }
      }
      gave_up = __builtin_amdgcn_readfirstlane(gave_up);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      if (gave_up) {
        for (uint32_t i = lane; i < n; i += 64) order[lo + i] = (int32_t)(lo + i);
        if (sidx == 0 && lane == 0) atomicAdd(gsync + kSyncGiveUps, 1u); // one count per launch (QLAMD_COUNTER_PLACEMENT_GIVE_UPS)
        return;
      }
      uint32_t total = 0, before = 0;
      if (lane < nkeys) {
        for (uint32_t b = 0; b < S; b++) {
          const uint32_t h = __hip_atomic_load(ghist + b * kPlaceKeys + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          total += h;
          before += b < sidx ? h : 0u;
        }
      }
      uint32_t incl = total;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        incl += lane >= (uint32_t)d ? o : 0u;
      }
      if (lane < nkeys) adj[lane] = (incl - total) + before - start;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    pass(std::integral_constant<int, 2>{});
  };
  if (classes) run(std::true_type{}, std::true_type{});
  else if (throughput) run(std::false_type{}, std::true_type{});
  else run(std::false_type{}, std::false_type{});
}

// ---- the host side: the launches on device pointers, for entries that hold the context's guard (qlamd::rt::placement_launch,
// declared in context.hpp), and the public qlamd_placement_from_iterations
// qlamd_placement_from_iterations on device pointers (the caller holds the context's guard)
// d_support: the robots' support flags ([B][4] bytes, device) or NULL -- the class of the sorted placement (place_key)
int launch_placement(qlamd_context *ctx, const int32_t *d_it, int64_t batch, int throughput, int32_t *d_ord, hipStream_t st,
                     const uint8_t *d_support = nullptr) {
  const uint32_t *sup = throughput ? reinterpret_cast<const uint32_t *>(d_support) : nullptr;
  if (batch <= kPlaceRounds * kPlaceThreads)
    hipLaunchKernelGGL(placement_kernel<kPlaceRounds>, dim3(1), dim3(kPlaceThreads), 0, st, d_it, batch, throughput, sup, nullptr, d_ord);
  else {
    // several workgroups (the LDS atomics of one compute unit serve about one robot per cycle: 4096 robots per workgroup
    // keep a launch at 3-4 us whatever the batch): their counts per bin go through the context's placement scratch
    // (sized for 1 M robots when the context is created; growing it is an allocation, which a stream capture cannot take)
    const int64_t per_block = (int64_t)kPlaceRounds * kPlaceThreads;
    const unsigned nb = (unsigned)((batch + per_block - 1) / per_block);
    const size_t need = (size_t)nb * kPlaceKeys * sizeof(uint32_t);
    if (ctx->place_ws_bytes < need) {
      if (CallGuard::capturing(st)) return QLAMD_ERR_NEEDS_RESERVE;
      if (hipStreamSynchronize(st) != hipSuccess) return QLAMD_ERR_HIP;
      if (ctx->place_ws) (void)hipFree(ctx->place_ws);
      ctx->place_ws = nullptr;
      ctx->place_ws_bytes = 0;
      if (hipMalloc(&ctx->place_ws, need) != hipSuccess) return QLAMD_ERR_OUT_OF_MEMORY;
      ctx->place_ws_bytes = need;
    }
    hipLaunchKernelGGL(placement_hist_kernel, dim3(nb), dim3(kPlaceThreads), 0, st, d_it, batch, per_block, sup, (uint32_t *)ctx->place_ws);
    hipLaunchKernelGGL(placement_kernel<kPlaceRounds>, dim3(nb), dim3(kPlaceThreads), 0, st, d_it, batch, throughput, sup,
                       (const uint32_t *)ctx->place_ws, d_ord);
  }
  return hipGetLastError() == hipSuccess ? QLAMD_OK : QLAMD_ERR_HIP;
}
bool throughput_policy(int policy, int64_t batch) {
  return policy == QLAMD_PLACEMENT_THROUGHPUT || (policy == QLAMD_PLACEMENT_AUTO && batch >= QLAMD_THROUGHPUT_BATCH);
}
__global__ void identity_order_kernel(int32_t *order, int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < B) order[i] = (int32_t)i;
}
} // namespace

int qlamd::rt::placement_launch(qlamd_context *ctx, const int32_t *d_iterations, int64_t batch, int policy, int32_t *d_order,
                                hipStream_t st, const uint8_t *d_support) {
  if (policy == QLAMD_PLACEMENT_NONE) { // the batch order
    hipLaunchKernelGGL(identity_order_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, d_order, batch);
    return hipGetLastError() == hipSuccess ? QLAMD_OK : QLAMD_ERR_HIP;
  }
  return launch_placement(ctx, d_iterations, batch, throughput_policy(policy, batch) ? 1 : 0, d_order, st, d_support);
}

// (the public entry; balance_kernel.hip's host-buffer calls come here for a next_robot_order as well)
extern "C" int qlamd_placement_from_iterations(qlamd_context *ctx, const int32_t *iterations, int64_t batch, int policy,
                                               int32_t *robot_order, int memory, void *stream) {
  if (!ctx || !iterations || !robot_order || batch < 0 || batch > INT32_MAX) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!valid_policy(policy)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (policy == QLAMD_PLACEMENT_NONE) { // the batch order
    if (memory == QLAMD_MEM_HOST) {
      for (int64_t i = 0; i < batch; i++) robot_order[i] = (int32_t)i;
      return QLAMD_OK;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
    QL_ENTER(ctx, (hipStream_t)stream);
    return placement_launch(ctx, nullptr, batch, QLAMD_PLACEMENT_NONE, robot_order, (hipStream_t)stream);
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(iterations, B * 4);
  sg.out(robot_order, B * 4);
  if (const int rc = sg.upload(ctx, st)) return rc;
  if (const int rc = launch_placement(ctx, iterations, batch, throughput_policy(policy, batch) ? 1 : 0, robot_order, st)) return rc;
  return sg.finish(st);
}

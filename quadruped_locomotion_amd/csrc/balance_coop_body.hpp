// The body of balance_coop_kernel and balance_table_kernel (balance_kernel.hip), included into both: text, not a function,
// because the existing kernels' code is to stay what it was instruction for instruction (as an inlined function template the
// same statements come out 20-30 instructions shorter and scheduled differently).  In scope: the kernel's parameters Pp, s, B,
// tau, grf, status; its LDS block `lds`; the flags kPerLeg, kMinWaves, kPlaced, kWarm, kTable.
  double *tab = lds, *rows = lds + 4 * kTabPerLeg, *nrm = rows + 4 * kCoopWaves * coop::kCoopLdsDoubles;
  const DeviceParams &P = *Pp;
  const int row = threadIdx.x >> 4, wave = threadIdx.x >> 6;
  unsigned block = blockIdx.x;
  QL_BLOCK_STAMP(0);
  if constexpr (kPlaced) {
    // the first workgroups of a launch that also places the next one (they start first and have the whole launch to finish in)
    if (s.shadow_blocks) {
      if (block < (unsigned)s.shadow_blocks) {
        placement_wave(s.prev_iterations, B, s.place_throughput, s.next_order, (lds_u32 *)lds, block, (uint32_t)s.shadow_blocks,
                       (uint32_t)s.shadow_chunk, s.place_throughput ? reinterpret_cast<const uint32_t *>(s.stance) : nullptr, s.place_hist, s.place_sync,
                       s.place_wait);
        return;
      }
      block -= (unsigned)s.shadow_blocks;
      // the wavefronts that solve go first wherever one of them shares a SIMD with a shadow wavefront (which has the whole
      // launch to finish in): without it the placed loop of 4096 robots is 0.4 us longer with four shadow wavefronts than
      // with one (profiles/r5/ab_shadow_blocks.txt)
      __builtin_amdgcn_s_setprio(3);
    }
  }
  // (the slot's robot: coop::slot_robot's statements with the next order's write between them, written out -- see there)
  int64_t i = (int64_t)block * (4 * kCoopWaves) + row;
  bool live = i < B;
  if (!live) i = B - 1;
  if constexpr (kPlaced) {
    if constexpr (kMinWaves == 2) { // (QLAMD_PLACEMENT_NONE: the batch order; the 168-register form has no register for it -- a launch of its own there)
      if (s.shadow_blocks == 0 && s.next_order && live && (threadIdx.x & 15) == 0) s.next_order[i] = (int32_t)i;
    }
    if (s.order) {
      const int64_t o = s.order[i];
      live = live && o >= 0 && o < B;
      i = live ? o : B - 1;
    }
  }
  // (coop_ptrs' fold by name, written out: as a call on the kernel's own parameter the placed kernels come out differently)
  coop::CoopPtrs cp{};
  cp.q = s.q; cp.pos = s.pos; cp.quat = s.quat; cp.linvel = s.linvel; cp.angvel = s.angvel;
  cp.dpos = s.dpos; cp.dquat = s.dquat; cp.dlinvel = s.dlinvel; cp.dangvel = s.dangvel;
  cp.stance = s.stance; cp.normals = s.normals;
  cp.wrench = s.wrench; cp.live = s.live; cp.support_only = s.support_only;
  if constexpr (kPlaced) cp.iterations = s.iterations;
  if constexpr (kWarm) { cp.prev_working_set = s.prev_working_set; cp.working_set = s.working_set; cp.warm_retries = s.warm_retries; }
  cp.record_doubles = s.record_doubles;
  if constexpr (kTable) cp.set_memory = s.set_memory;
  // the form: a placed launch carries the 6-variable form of the QP; the 168-register form (kMinWaves 3) installs a warm start's
  // rows one after the other and, solving cold and placed, parks its inputs in LDS
  using Form = coop::CoopForm<coop::PerLegNormals<kPerLeg>, coop::BlockLanes<64 * kCoopWaves>, coop::WarmStart<kWarm>, coop::FromTable<kTable>,
                              coop::SmallForm<kPlaced>, coop::ThroughputForm<kMinWaves == 3>, coop::ParkInputs<kMinWaves == 3 && !kWarm && kPlaced>>;
#ifdef QLAMD_STAMPS
#pragma unroll 1
  for (int rep = 0; rep < 2; rep++) // second pass runs with a warm instruction cache
#endif
  // (inputs parked in LDS across the first form of the QP: the 168-register form solving cold -- no scratch then, 1-2 % on 65 536
  // to a million robots; the warm-started kernel is 3 % faster with them in registers and 20 bytes of scratch around the loop)
  {
    const bool rejected = coop::coop_robot<Form>(
        P, cp, i, live, tab, rows + row * coop::kCoopLdsDoubles, nrm + wave * coop::kCoopNrmDoubles, tau, grf, status);
    QL_BLOCK_STAMP(3);
    if constexpr (kWarm) {
      // A warm start must never cost an answer (balance_coop.hpp): the rows whose warm start was rejected are solved again, cold,
      // by this wavefront -- the plain kernel's body behind a scalar branch, everything it needs fetched again from the argument
      // segment (coop::kernel_arguments_again), the other rows riding along empty; the robot's working set comes back 0 (its slot of the table holds 0 already).
      if (__builtin_expect(P.warm_fallback && __builtin_amdgcn_ballot_w64(rejected) != 0ull, 0)) {
        __syncthreads(); // (one wavefront: the first attempt's LDS reads are done before the table is staged again)
        if constexpr (kTable) balance_table_retry<kPerLeg, kMinWaves>(coop::kernel_arguments_again<BalanceCoopArgs>(), lds, rejected);
        else balance_cold_retry<kPerLeg, kMinWaves>(coop::kernel_arguments_again<BalanceCoopArgs>(), lds, rejected);
      }
    }
  }

// HIP kernels (gfx950) of the batched balance-controller step and their part of the
// C-ABI of include/qlamd.h, plus the context.  See DESIGN.md for the data layout and launch geometry.
#include "balance_coop.hpp"
#include "params_build.hpp"
#include "context.hpp"
#include "launch_form.hpp"
#include "placement.hpp" // the placement sort: its kernels, the shadow wavefronts of a placed launch, its launches and entry

#include <type_traits>

using namespace qlamd;
using namespace qlamd::rt;

namespace {

struct StatePtrs {
  const double *q, *pos, *quat, *linvel, *angvel, *dpos, *dquat, *dlinvel, *dangvel;
  const uint8_t *stance;
  const double *normals;
  const double *wrench; // [B][6] or NULL
  const uint8_t *live;  // [B] or NULL: 0 = robot left alone (nothing written)
  int support_only;     // whole tick: only the support legs' efforts are written (the swing branch, which writes the
                        // others, runs beside this kernel on another stream)
  const int32_t *order; // [B] or NULL: slot s of the launch (row s % 4 of wavefront s / 4) takes robot order[s]
  int32_t *iterations;  // [B] or NULL: outer iterations of each robot's QP
  // the placement of the NEXT launch, made by extra wavefronts in the shadow of this one (placement_wave, placement.hpp)
  const int32_t *prev_iterations; // [B]: the counts it is made from (the previous launch's `iterations`)
  int32_t *next_order;            // [B] or NULL: where it goes.  With shadow_blocks == 0: QLAMD_PLACEMENT_NONE -- every slot writes its own
                                  // index here (no field of its own: one more pointer in the arguments cost the 168-register form 1 % at 65 536 robots)
  int place_throughput;           // policy: 0 latency, 1 throughput
  const uint32_t *prev_working_set; // [B] or NULL: warm start (kWarm instantiations)
  uint32_t *working_set;            // [B] or NULL
  int shadow_blocks, shadow_chunk;  // workgroups in front of the launch that make next_order, and the robots each of them takes
  uint32_t *place_hist;             // [shadow_blocks][kPlaceKeys]: their counts per key, for each other (the context's scratch)
  uint32_t *place_sync;             // two words, zero when the context is created: arrivals, state (their barrier)
  uint32_t place_wait;              // polls they wait for each other before they give up (QLAMD_OPT_PLACEMENT_WAIT)
  uint32_t *warm_retries;           // the context's count of rejected warm starts (kWarm instantiations)
  int record_doubles;               // 0, or the record length of QLAMD_STATE_RECORDS (lane-cooperative kernels, device memory)
  uint32_t *set_memory;             // [B][4] or NULL: a working set per support set (kTable instantiations), instead of prev_working_set
};

__device__ __forceinline__ void load_robot(const StatePtrs &s, int64_t i, RobotIn &in) {
  // 96-byte (q), 32-byte (quat) and 24-byte records: each lane reads its own
  // contiguous record; neighbouring lanes share cache lines, every fetched byte is used.
  const double2 *q2 = reinterpret_cast<const double2 *>(s.q + 12 * i);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double2 v = q2[k];
    in.q[2 * k] = v.x;
    in.q[2 * k + 1] = v.y;
  }
  const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
  const double2 *b2 = reinterpret_cast<const double2 *>(s.dquat + 4 * i);
  double2 v = a2[0]; in.quat[0] = v.x; in.quat[1] = v.y;
  v = a2[1]; in.quat[2] = v.x; in.quat[3] = v.y;
  v = b2[0]; in.dquat[0] = v.x; in.dquat[1] = v.y;
  v = b2[1]; in.dquat[2] = v.x; in.dquat[3] = v.y;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    in.pos[k] = s.pos[3 * i + k];
    in.linvel[k] = s.linvel[3 * i + k];
    in.angvel[k] = s.angvel[3 * i + k];
    in.dpos[k] = s.dpos[3 * i + k];
    in.dlinvel[k] = s.dlinvel[3 * i + k];
    in.dangvel[k] = s.dangvel[3 * i + k];
  }
  const uint32_t m = *reinterpret_cast<const uint32_t *>(s.stance + 4 * i);
  in.stance = support_mask(m);
  in.has_wrench = s.wrench != nullptr;
  if (in.has_wrench) {
#pragma unroll
    for (int k = 0; k < 6; k++) in.wrench[k] = s.wrench[6 * i + k];
  }
}

// StatePtrs -> what coop_robot takes, by the pointer groups the caller uses (the others stay NULL / 0): the iteration counts; the
// warm start's sets and counter; the table; what only the context-wide entries and the whole tick have (an external wrench, the
// live flags, support_only, the record layout).  In the order of CoopPtrs' members: the order the kernels fetch them in.
enum : unsigned { kUseIterations = 1u, kUseWarm = 2u, kUseTable = 4u, kUseWrenchLive = 8u };
template <unsigned kUse>
__device__ __forceinline__ coop::CoopPtrs coop_ptrs(const StatePtrs &s) {
  coop::CoopPtrs c{};
  c.q = s.q; c.pos = s.pos; c.quat = s.quat; c.linvel = s.linvel; c.angvel = s.angvel;
  c.dpos = s.dpos; c.dquat = s.dquat; c.dlinvel = s.dlinvel; c.dangvel = s.dangvel; c.stance = s.stance; c.normals = s.normals;
  if constexpr (kUse & kUseWrenchLive) { c.wrench = s.wrench; c.live = s.live; c.support_only = s.support_only; }
  if constexpr (kUse & kUseIterations) c.iterations = s.iterations;
  if constexpr (kUse & kUseWarm) { c.prev_working_set = s.prev_working_set; c.working_set = s.working_set; c.warm_retries = s.warm_retries; }
  if constexpr (kUse & kUseWrenchLive) c.record_doubles = s.record_doubles;
  if constexpr (kUse & kUseTable) c.set_memory = s.set_memory;
  return c;
}

// One wavefront per workgroup, RPW robots per wavefront (64, 16 or 4).  A small batch is spread
// over more SIMDs by lowering RPW: at 4096 robots the step is latency-bound, not throughput-bound.
//   phase A  lanes = (robot, leg) pairs: FK + Jacobian + gravity torque       -> LDS
//   phase B  lanes = robots: wrench, QP assembly, Cholesky, active-set QP      -> LDS
//   phase C  lanes = (robot, leg) pairs: tau = J'(-f) + G(q), clamp            -> HBM
// Loads and stores of phases A and C are contiguous across lanes (24-byte records in
// (robot, leg) order); phase B reads its 26 base-state doubles as per-robot records.
template <int RPW, bool kPerLeg>
__global__ __launch_bounds__(64) void balance_step_kernel(const DeviceParams *__restrict__ Pp, const StatePtrs s,
                                                          int64_t B, double *__restrict__ tau,
                                                          double *__restrict__ grf, int32_t *__restrict__ status) {
  extern __shared__ double lds[];
  double *tab = lds;                 // 256 doubles: leg model table
  double *scratch = lds + 4 * kTabPerLeg; // [kScratchDoubles][RPW]
  const DeviceParams &P = *Pp;
  const int lane = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * RPW;

#pragma unroll
  for (int i = lane; i < 4 * kTabPerLeg; i += 64) tab[i] = P.legtab[i];
  __syncthreads();

  // ---- phase A
#pragma unroll 1
  for (int item = lane; item < 4 * RPW; item += 64) {
    const int rb = item >> 2, leg = item & 3;
    const int64_t i = base + rb;
    if (i < B && (!s.live || s.live[i])) {
      const bool support = s.stance[4 * i + leg] != 0;
      const double q3[3] = {s.q[12 * i + 3 * leg], s.q[12 * i + 3 * leg + 1], s.q[12 * i + 3 * leg + 2]};
      const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
      const double2 v0 = a2[0], v1 = a2[1];
      const double quat[4] = {v0.x, v0.y, v1.x, v1.y};
      LdsScratch scr{scratch + rb, RPW};
      phase_a_leg(LdsTab{tab + kTabPerLeg * leg}, leg, support, q3, quat, P.grav, scr);
    }
  }
  __syncthreads();

  // ---- phase B
  {
    const int64_t i = base + lane;
    if (lane < RPW && i < B && (!s.live || s.live[i])) {
      RobotIn in;
      load_robot(s, i, in);
      double nw[12];
      if (kPerLeg) {
#pragma unroll
        for (int k = 0; k < 12; k++) nw[k] = s.normals[12 * i + k];
      }
      LdsScratch scr{scratch + lane, RPW};
      const QpResult r = phase_b_robot<kPerLeg>(P, in, nw, scr);
      scr.at(kScrStatus) = (double)r.status;
      status[i] = r.status;
    }
  }
  __syncthreads();

  // ---- phase C
#pragma unroll 1
  for (int item = lane; item < 4 * RPW; item += 64) {
    const int rb = item >> 2, leg = item & 3;
    const int64_t i = base + rb;
    if (i < B && (!s.live || s.live[i])) {
      LdsScratch scr{scratch + rb, RPW};
      if (P.keep_on_failure && scr.at(kScrStatus) != 0.0) continue;
      if (s.support_only && s.stance[4 * i + leg] == 0) continue;
      const bool live = (s.stance[4 * i + leg] != 0) && (scr.at(kScrStatus) == 0.0);
      double t[3], f[3];
      phase_c_leg(leg, live, P.tau_max, scr, t, f);
      double *to = tau + 12 * i + 3 * leg;
      to[0] = t[0]; to[1] = t[1]; to[2] = t[2];
      if (grf) {
        double *go = grf + 12 * i + 3 * leg;
        go[0] = f[0]; go[1] = f[1]; go[2] = f[2];
      }
    }
  }
}

// The second attempt of the rows whose warm start was rejected (balance_coop_kernel<..., kWarm = true>, below): the plain kernel's
// body as a function of its own that ENDS THE WAVEFRONT -- nothing of the caller's is live across the call -- and takes what it
// needs from the kernel's argument segment again (coop::kernel_arguments_again: the caller passes the segment's address -- a
// function that is not a kernel has none of its own -- and keeps nothing else for it).
// (BalanceCoopArgs mirrors the parameters of balance_coop_kernel by hand: the checks behind the kernel tie the two together)
struct BalanceCoopArgs { const DeviceParams *Pp; StatePtrs s; int64_t B; double *tau, *grf; int32_t *status; }; // the kernel's parameters
template <bool kPerLeg, int kMinWaves>
__device__ __forceinline__ void cold_retry_body(const BalanceCoopArgs *args, double *lds, bool rejected) {
  const BalanceCoopArgs &a = *args;
  double *tab = lds, *rows = lds + 4 * kTabPerLeg, *nrm = rows + 4 * coop::kCoopLdsDoubles;
  const int row = threadIdx.x >> 4;
  const unsigned blk = blockIdx.x - (unsigned)a.s.shadow_blocks;
  // (coop::slot_robot's statements, written out: see there)
  int64_t ir = (int64_t)blk * 4 + row;
  const bool inside = ir < a.B;
  if (!inside) ir = a.B - 1;
  if (a.s.order) {
    const int64_t o = a.s.order[ir];
    ir = (inside && o >= 0 && o < a.B) ? o : a.B - 1;
  }
  const coop::CoopPtrs cold = coop_ptrs<kUseIterations | kUseWrenchLive>(a.s);
  using Cold = coop::CoopForm<coop::PerLegNormals<kPerLeg>, coop::ParkInputs<kMinWaves == 3>>;
  (void)coop::coop_robot<Cold>(*a.Pp, cold, ir, rejected, tab, rows + row * coop::kCoopLdsDoubles, nrm, a.tau, a.grf, a.status);
  if (rejected && (threadIdx.x & 15) == 0 && a.s.working_set) a.s.working_set[ir] = 0u;
}
template <bool kPerLeg, int kMinWaves>
__device__ __attribute__((noinline, noreturn)) void balance_cold_retry(const BalanceCoopArgs *args, double *lds, bool rejected) {
  cold_retry_body<kPerLeg, kMinWaves>(args, lds, rejected);
  __builtin_amdgcn_endpgm();
}
// ... of the kernels that start from the table (balance_table_kernel): the same body -- the first attempt has written the table's
// word already -- as a function of its own, because a function with two callers saves what it would clobber: 40-136 bytes more
// scratch in every warm-started launch
template <bool kPerLeg, int kMinWaves>
__device__ __attribute__((noinline, noreturn)) void balance_table_retry(const BalanceCoopArgs *args, double *lds, bool rejected) {
  cold_retry_body<kPerLeg, kMinWaves>(args, lds, rejected);
  __builtin_amdgcn_endpgm();
}

// Latency form: 16 lanes per robot, 4 robots per wavefront (balance_coop.hpp), kCoopWaves wavefronts per workgroup.
// One wavefront per workgroup is the measured optimum: four (one workgroup per compute unit, the model table in LDS
// shared) costs 2.3 us at 4096 robots and 20 % at 65536 -- the barrier behind the table ties the start of four
// wavefronts together and workgroups leave their compute unit only when their slowest wavefront has finished.
constexpr int kCoopWaves = 1;
// (from which batch the three-wavefront form runs: QLAMD_THROUGHPUT_BATCH, QLAMD_THREE_WAVE_WARM_BATCH, launch_form.hpp)
// kMinWaves wavefronts per SIMD at least: 2 (at most 256 registers: the large-batch throughput halves without it) for the
// latency form, 3 (at most 168 registers; 12 wavefronts x 13 056 bytes of LDS fit a compute unit) for the throughput form
// that large batches take (QLAMD_THROUGHPUT_BATCH): two wavefronts of dependent instruction streams cannot fill a SIMD's
// issue port (2 x one instruction per 5.5 cycles against one per 4), three can.
// kPlaced: the caller says which robot sits in which slot of the launch (qlamd_balance_solve_placed_batch): the four robots
// of a wavefront run in lockstep, so a wavefront lasts as long as the union of their passes, and a launch of a few
// thousand robots as long as its slowest wavefront -- WHO shares a wavefront decides both.  The slot's
// robot index is one more load in front of the robot's own (a dependent round trip at the head of the launch), which is
// why the plain entry keeps a kernel without it.  An entry outside [0, B) leaves its row empty.
// kWarm (with kPlaced): every robot's QP starts from the working set the caller hands in (force_qp_coop.hpp).
// kTable (with kWarm; balance_table_kernel): ... from the word of its support set in the caller's table of four, s.set_memory
// (balance_coop.hpp).
constexpr int kCoopLdsTotal = 4 * kTabPerLeg + 4 * kCoopWaves * coop::kCoopLdsDoubles + kCoopWaves * coop::kCoopNrmDoubles;
static_assert(kCoopLdsTotal * sizeof(double) >= kShadowLdsBytes || kCoopWaves != 1, "the shadow wavefronts' counters live in the solve's LDS");
template <bool kPerLeg, int kMinWaves, bool kPlaced = false, bool kWarm = false>
__global__ __launch_bounds__(64 * kCoopWaves, kMinWaves) void balance_coop_kernel(const DeviceParams *__restrict__ Pp, const StatePtrs s,
                                                                      int64_t B, double *__restrict__ tau,
                                                                      double *__restrict__ grf, int32_t *__restrict__ status) {
  __shared__ double lds[kCoopLdsTotal];
  constexpr bool kTable = false;
#include "balance_coop_body.hpp"
}
// placed, warm-started from the table (qlamd_placement::set_memory): a kernel of its own, so that a launch without the table
// runs what it ran before the table existed
template <bool kPerLeg, int kMinWaves>
__global__ __launch_bounds__(64 * kCoopWaves, kMinWaves) void balance_table_kernel(const DeviceParams *__restrict__ Pp, const StatePtrs s,
                                                                       int64_t B, double *__restrict__ tau,
                                                                       double *__restrict__ grf, int32_t *__restrict__ status) {
  __shared__ double lds[kCoopLdsTotal];
  constexpr bool kPlaced = true, kWarm = true, kTable = true;
#include "balance_coop_body.hpp"
}
// balance_cold_retry reads the kernel's arguments through BalanceCoopArgs laid over the argument segment: same members, same
// types, same places as the parameters of the kernels (every instantiation of the two has the one signature)
using CoopKernelLayout = KernargLayout<decltype(&balance_coop_kernel<false, 2, true, true>)>;
QL_KERNARG_MIRROR(CoopKernelLayout, BalanceCoopArgs, true, Pp, s, B, tau, grf, status);
static_assert(std::is_same<decltype(&balance_coop_kernel<false, 2, true, true>), decltype(&balance_table_kernel<true, 3>)>::value,
              "balance_table_kernel takes the parameters of balance_coop_kernel");

// Controller parameters per robot (qlamd_balance_solve_robot_params_batch): the body of coop_robot with every parameter of the
// controller taken from the robot's own record (robot_params [B] of QLAMD_ROBOT_PARAMS_DOUBLES doubles) instead of *Pp, whose
// leg model table, gravity and options still hold.  Kernels of their own -- one more parameter, 1 KB more LDS (the four rows'
// staged records, behind the block of the other kernels) -- so that a launch without per-robot parameters runs what it ran
// before they existed.  Always the two-wavefront form, always with a placement's robot_order (NULL: the batch order) and the
// 6-variable form for wavefronts whose robots stand on two legs (results bit for bit those of the 12-variable form); no shadow
// wavefronts: the entry refuses prev_iterations / next_robot_order.
constexpr int kRobotParamsLdsTotal = kCoopLdsTotal + 4 * kCoopWaves * QLAMD_ROBOT_PARAMS_DOUBLES;
static_assert(kCoopWaves == 1, "balance_robot_params_kernel is written for one wavefront per workgroup");
static_assert(kCoopLdsTotal % 2 == 0, "the staged records start on a 16-byte boundary");
static_assert(2 * 4 * kRobotParamsLdsTotal * sizeof(double) <= 160 * 1024, "two wavefronts per SIMD fit a compute unit's LDS");
static_assert(sizeof(qlamd_robot_params) == QLAMD_ROBOT_PARAMS_DOUBLES * sizeof(double) && QLAMD_ROBOT_PARAMS_DOUBLES == 2 * 16,
              "a row's 16 lanes fetch the record two doubles each");
struct RobotParamsArgs { const DeviceParams *Pp; StatePtrs s; int64_t B; double *tau, *grf; int32_t *status; const double *robot_params; };
template <bool kPerLeg, bool kWarm, bool kTable>
__device__ __forceinline__ bool robot_params_rows(const DeviceParams &P, const StatePtrs &s, int64_t B, double *tau, double *grf,
                                                  int32_t *status, const double *robot_params, double *lds, bool cold, bool only) {
  double *tab = lds, *rows = lds + 4 * kTabPerLeg, *nrm = rows + 4 * coop::kCoopLdsDoubles, *rp = lds + kCoopLdsTotal;
  const int row = threadIdx.x >> 4;
  bool live;
  const int64_t i = coop::slot_robot((int64_t)blockIdx.x * 4 + row, B, s.order, live);
  const coop::CoopPtrs cp = coop_ptrs<kUseIterations | (kWarm ? kUseWarm : 0u) | (kTable ? kUseTable : 0u)>(s);
  using Form = coop::CoopForm<coop::PerLegNormals<kPerLeg>, coop::WarmStart<kWarm>, coop::FromTable<kTable>, coop::RobotParams<true>>;
  return coop::coop_robot<Form>(P, cp, i, live && only, tab, rows + row * coop::kCoopLdsDoubles, nrm, tau, grf, status, cold, robot_params,
                                rp + row * QLAMD_ROBOT_PARAMS_DOUBLES);
}
// the second attempt of its rejected rows (as balance_cold_retry: a function that ends the wavefront, one per calling kernel)
template <bool kPerLeg, bool kTable>
__device__ __attribute__((noinline, noreturn)) void balance_robot_params_retry(const RobotParamsArgs *args, double *lds, bool rejected) {
  const RobotParamsArgs &a = *args;
  (void)robot_params_rows<kPerLeg, false, false>(*a.Pp, a.s, a.B, a.tau, a.grf, a.status, a.robot_params, lds, true, rejected);
  if (rejected && (threadIdx.x & 15) == 0 && a.s.working_set) {
    // (the rejected row's robot, as robot_params_rows found it)
    int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 4);
    if (a.s.order) i = a.s.order[i];
    a.s.working_set[i] = 0u;
  }
  __builtin_amdgcn_endpgm();
}
template <bool kPerLeg, bool kWarm, bool kTable>
__global__ __launch_bounds__(64, 2) void balance_robot_params_kernel(const DeviceParams *__restrict__ Pp, const StatePtrs s, int64_t B,
                                                                     double *__restrict__ tau, double *__restrict__ grf,
                                                                     int32_t *__restrict__ status,
                                                                     const double *__restrict__ robot_params) {
  __shared__ __attribute__((aligned(16))) double lds[kRobotParamsLdsTotal]; // (the staged records are stored 16 bytes a lane)
  const DeviceParams &P = *Pp;
  const bool rejected = robot_params_rows<kPerLeg, kWarm, kTable>(P, s, B, tau, grf, status, robot_params, lds, false, true);
  if constexpr (kWarm) {
    if (__builtin_expect(P.warm_fallback && __builtin_amdgcn_ballot_w64(rejected) != 0ull, 0)) {
      __syncthreads(); // (one wavefront: the first attempt's LDS reads are done before the table is staged again)
      balance_robot_params_retry<kPerLeg, kTable>(coop::kernel_arguments_again<RobotParamsArgs>(), lds, rejected);
    }
  }
}
using RobotParamsKernelLayout = KernargLayout<decltype(&balance_robot_params_kernel<false, true, true>)>;
QL_KERNARG_MIRROR(RobotParamsKernelLayout, RobotParamsArgs, true, Pp, s, B, tau, grf, status, robot_params);
static_assert(std::is_same<decltype(&balance_robot_params_kernel<false, true, true>), decltype(&balance_robot_params_kernel<true, false, false>)>::value,
              "every balance_robot_params_kernel has the one signature");

__global__ __launch_bounds__(64) void virtual_wrench_kernel(const DeviceParams *__restrict__ Pp, const StatePtrs s,
                                                            int64_t B, double *__restrict__ wrench) {
  const DeviceParams &P = *Pp;
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  RobotIn in; // only the base state enters the wrench (joint positions and stance flags are not read)
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
    const double2 *b2 = reinterpret_cast<const double2 *>(s.dquat + 4 * i);
    double2 v = a2[0]; in.quat[0] = v.x; in.quat[1] = v.y;
    v = a2[1]; in.quat[2] = v.x; in.quat[3] = v.y;
    v = b2[0]; in.dquat[0] = v.x; in.dquat[1] = v.y;
    v = b2[1]; in.dquat[2] = v.x; in.dquat[3] = v.y;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      in.pos[k] = s.pos[3 * i + k]; in.linvel[k] = s.linvel[3 * i + k]; in.angvel[k] = s.angvel[3 * i + k];
      in.dpos[k] = s.dpos[3 * i + k]; in.dlinvel[k] = s.dlinvel[3 * i + k]; in.dangvel[k] = s.dangvel[3 * i + k];
    }
    in.stance = 0; in.has_wrench = false;
  }
  double Rm[9], gB[3], b[6];
  quat_to_matrix(in.quat, Rm);
  const double gW[3] = {0.0, 0.0, -P.grav};
  irot(Rm, gW, gB);
  virtual_wrench(P, in, Rm, gB, b);
#pragma unroll
  for (int k = 0; k < 6; k++) wrench[6 * i + k] = b[k];
}

__global__ __launch_bounds__(64) void leg_kinematics_kernel(const DeviceParams *__restrict__ Pp,
                                                            const double *__restrict__ q,
                                                            const double *__restrict__ quat, int64_t B,
                                                            double *__restrict__ foot, double *__restrict__ jac,
                                                            double *__restrict__ grav) {
  // one lane per (robot, leg)
  __shared__ double tab[4 * kTabPerLeg];
  const DeviceParams &P = *Pp;
  TabStage ts;
  ts.issue(P);
  const int64_t t0 = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = t0 < 4 * B;
  const int64_t t = live ? t0 : 4 * B - 1;
  const int64_t i = t >> 2;
  const int leg = (int)(t & 3);
  double ql[3];
  load3(q, t, ql);
  const double qq[4] = {quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3]};
  ts.commit(tab);
  double Rm[9], gB[3];
  quat_to_matrix(qq, Rm);
  const double gW[3] = {0.0, 0.0, -P.grav};
  irot(Rm, gW, gB);
  double F[3], J[9], Gq[3];
  leg_kinematics(LdsTab{tab + kTabPerLeg * leg}, ql, gB, F, J, Gq);
  if (!live) return;
  if (foot) { foot[3 * t] = F[0]; foot[3 * t + 1] = F[1]; foot[3 * t + 2] = F[2]; }
  if (jac) {
#pragma unroll
    for (int k = 0; k < 9; k++) jac[9 * t + k] = J[k];
  }
  if (grav) { grav[3 * t] = Gq[0]; grav[3 * t + 1] = Gq[1]; grav[3 * t + 2] = Gq[2]; }
}

template <int RPW>
hipError_t launch_balance(const qlamd_context *ctx, const StatePtrs &s, int64_t B, double *tau, double *grf,
                          int32_t *status, hipStream_t st) {
  const size_t lds = ((size_t)RPW * kScratchDoubles + 4 * kTabPerLeg) * sizeof(double);
  const unsigned grid = (unsigned)((B + RPW - 1) / RPW);
  const auto k = s.normals ? balance_step_kernel<RPW, true> : balance_step_kernel<RPW, false>;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, ctx->d_params, s, B, tau, grf, status);
  return hipGetLastError();
}

} // namespace

extern "C" {

void qlamd_balance_default_params(qlamd_balance_params *p) { if (p) default_balance_params(p); }
void qlamd_default_robot_model(qlamd_robot_model *m) { if (m) default_robot_model(m); }
int qlamd_version(void) { return QLAMD_VERSION_MAJOR * 1000 + QLAMD_VERSION_MINOR; }
unsigned qlamd_set_memory_slot(unsigned support_mask) { return QLAMD_SET_MEMORY_SLOT(support_mask); }

const char *qlamd_strerror(int code) {
  switch (code) {
    case QLAMD_OK: return "ok";
    case QLAMD_ERR_INVALID_ARGUMENT: return "invalid argument";
    case QLAMD_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case QLAMD_ERR_HIP: return "HIP runtime error";
    case QLAMD_ERR_NOT_LOADED: return "parameters not loaded";
    case QLAMD_ERR_OUT_OF_MEMORY: return "out of device memory";
    case QLAMD_ERR_BUSY: return "another thread is inside a call on this context";
    case QLAMD_ERR_NEEDS_RESERVE: return "device scratch would have to grow inside a stream capture: call qlamd_reserve first";
    default: return "unknown error";
  }
}

int qlamd_context_create(const qlamd_balance_params *params, const qlamd_robot_model *model, int device,
                         qlamd_context **out) {
  if (!out) return QLAMD_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!params) return QLAMD_ERR_NOT_LOADED;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return QLAMD_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return QLAMD_ERR_INVALID_ARGUMENT;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return QLAMD_ERR_HIP;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QLAMD_ERR_NO_DEVICE;
  qlamd_context *ctx = new (std::nothrow) qlamd_context(); // (value-initialised: every pointer NULL, every count and flag 0)
  if (!ctx) return QLAMD_ERR_OUT_OF_MEMORY;
  ctx->device = device;
  ctx->num_cu = prop.multiProcessorCount;
  ctx->placement_wait = 1u << 13;
  ctx->on_failure = QLAMD_ON_FAILURE_ZERO;
  ctx->dynamics_form = QLAMD_DYNAMICS_AUTO;
  qlamd_robot_model m;
  if (model) m = *model; else default_robot_model(&m);
  build_device_params(*params, m, &ctx->params);
  {
    // base_link inertia moved from its centre of mass to the base origin: I + m (|c|^2 1 - c c')
    const double bm = m.base_mass, *c = m.base_com, *I = m.base_inertia, cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    ctx->base_m = bm;
    for (int a = 0; a < 3; a++) ctx->base_h[a] = bm * c[a];
    ctx->base_I[0] = I[0] + bm * (cc - c[0] * c[0]); ctx->base_I[1] = I[1] - bm * c[0] * c[1]; ctx->base_I[2] = I[2] - bm * c[0] * c[2];
    ctx->base_I[3] = I[3] + bm * (cc - c[1] * c[1]); ctx->base_I[4] = I[4] - bm * c[1] * c[2];
    ctx->base_I[5] = I[5] + bm * (cc - c[2] * c[2]);
  }
  // (the placement scratch for batches up to 1 M robots comes with the context: 48 KB, and no placement call of a
  // sensible size ever has to allocate inside a stream capture)
  const size_t place_bytes = (size_t)256 * kPlaceKeys * sizeof(uint32_t);
  if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&ctx->d_params, sizeof(DeviceParams)) != hipSuccess ||
      hipMemcpy(ctx->d_params, &ctx->params, sizeof(DeviceParams), hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc(&ctx->place_ws, place_bytes) != hipSuccess || hipMalloc(&ctx->place_sync, 256) != hipSuccess ||
      hipMemset(ctx->place_sync, 0, 256) != hipSuccess) {
    if (ctx->d_params) (void)hipFree(ctx->d_params);
    if (ctx->place_ws) (void)hipFree(ctx->place_ws);
    if (ctx->place_sync) (void)hipFree(ctx->place_sync);
    delete ctx;
    return QLAMD_ERR_HIP;
  }
  ctx->place_ws_bytes = place_bytes;
  *out = ctx;
  return QLAMD_OK;
}

void qlamd_context_destroy(qlamd_context *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->wire_tpl) (void)hipFree(ctx->wire_tpl);
  if (ctx->tick_ws) (void)hipFree(ctx->tick_ws);
  if (ctx->place_ws) (void)hipFree(ctx->place_ws);
  if (ctx->place_sync) (void)hipFree(ctx->place_sync);
  if (ctx->d_params) (void)hipFree(ctx->d_params);
  if (ctx->done_event) (void)hipEventDestroy(ctx->done_event);
  delete ctx;
}

int qlamd_set_robots_per_wave(qlamd_context *ctx, int rpw) {
  if (!ctx || !(rpw == 0 || rpw == 4 || rpw == 16 || rpw == 64)) return QLAMD_ERR_INVALID_ARGUMENT;
  ctx->rpw_override = rpw;
  return QLAMD_OK;
}

int qlamd_set_option(qlamd_context *ctx, int option, int value) {
  if (!ctx) return QLAMD_ERR_INVALID_ARGUMENT;
  QL_ENTER_NO_STREAM(ctx);
  switch (option) {
    case QLAMD_OPT_ON_FAILURE:
      if (value != QLAMD_ON_FAILURE_ZERO && value != QLAMD_ON_FAILURE_KEEP) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->on_failure = value;
      ctx->params.keep_on_failure = value == QLAMD_ON_FAILURE_KEEP;
      break;
    case QLAMD_OPT_REFINE_PASSES:
      if (value < 0 || value > 4) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->params.refine_passes = value;
      break;
    case QLAMD_OPT_DYNAMICS_FORM:
      if (value < QLAMD_DYNAMICS_AUTO || value > QLAMD_DYNAMICS_ROW) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->dynamics_form = (int)value;
      return QLAMD_OK;
    case QLAMD_OPT_PLACEMENT_WAIT:
      if (value < 0) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->placement_wait = (unsigned)value;
      return QLAMD_OK;
    case QLAMD_OPT_STATE_LAYOUT:
      if (value != QLAMD_STATE_FIELDS && value != QLAMD_STATE_RECORDS) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->state_record_doubles = value == QLAMD_STATE_RECORDS ? QLAMD_STATE_RECORD_DOUBLES : 0;
      return QLAMD_OK;
    case QLAMD_OPT_WARM_FALLBACK:
      if (value < 0 || value > 2) return QLAMD_ERR_INVALID_ARGUMENT;
      ctx->params.warm_fallback = value;
      break;
    default: return QLAMD_ERR_INVALID_ARGUMENT;
  }
  // the device copy of the parameters: after everything already queued on the context has read the old one
  if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(ctx->d_params, &ctx->params, sizeof(DeviceParams), hipMemcpyHostToDevice) != hipSuccess)
    return QLAMD_ERR_HIP;
  return QLAMD_OK;
}

int qlamd_get_counter(qlamd_context *ctx, int counter, int64_t *value) {
  if (!ctx || !value || (counter != QLAMD_COUNTER_PLACEMENT_GIVE_UPS && counter != QLAMD_COUNTER_WARM_RETRIES)) return QLAMD_ERR_INVALID_ARGUMENT;
  QL_ENTER_NO_STREAM(ctx);
  uint32_t v = 0;
  const uint32_t *src = (const uint32_t *)ctx->place_sync + (counter == QLAMD_COUNTER_PLACEMENT_GIVE_UPS ? kSyncGiveUps : kSyncWarmRetries);
  if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&v, src, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
    return QLAMD_ERR_HIP;
  *value = (int64_t)v;
  return QLAMD_OK;
}

} // extern "C"

namespace {
// The launch's StatePtrs from the caller's state and placement (arrays on the device); the context's counter of rejected warm
// starts.  What only some launches have -- wrench, live flags, record layout, the shadow wavefronts -- is theirs to add.
StatePtrs state_ptrs(const qlamd_context *ctx, const qlamd_state_batch &in, const qlamd_placement &pl) {
  StatePtrs s{};
  s.q = in.joint_position; s.pos = in.base_position; s.quat = in.base_orientation;
  s.linvel = in.base_linear_velocity; s.angvel = in.base_angular_velocity;
  s.dpos = in.desired_position; s.dquat = in.desired_orientation;
  s.dlinvel = in.desired_linear_velocity; s.dangvel = in.desired_angular_velocity;
  s.stance = in.support_leg; s.normals = in.surface_normal;
  s.order = pl.robot_order; s.iterations = pl.iterations;
  s.prev_working_set = pl.prev_working_set; s.working_set = pl.working_set; s.set_memory = pl.set_memory;
  s.warm_retries = (uint32_t *)ctx->place_sync + kSyncWarmRetries;
  return s;
}
// the kernel of a form (every instantiation of the two families has the one signature: the static_asserts behind them)
using CoopKernel = decltype(&balance_coop_kernel<false, 2, true, true>);
template <bool kPerLeg, int kMinWaves>
CoopKernel coop_kernel_of(const LaunchForm &f) {
  if (f.table) return balance_table_kernel<kPerLeg, kMinWaves>;
  if (f.warm) return balance_coop_kernel<kPerLeg, kMinWaves, true, true>;
  if (f.placed) return balance_coop_kernel<kPerLeg, kMinWaves, true>;
  return balance_coop_kernel<kPerLeg, kMinWaves, false>;
}
CoopKernel coop_kernel_of(const LaunchForm &f) {
  if (f.per_leg) return coop_kernel_of<true, 2>(f);
  return f.waves == 3 ? coop_kernel_of<false, 3>(f) : coop_kernel_of<false, 2>(f);
}
} // namespace

int qlamd::rt::balance_launch(qlamd_context *ctx, const qlamd_state_batch &in, int layout, const double *wrench, const uint8_t *live,
                              int support_only, const qlamd_placement &pl, int64_t batch, double *d_tau, double *d_grf,
                              int32_t *d_status, hipStream_t st) {
  // (table: instead of prev_working_set, the entries have checked that; prev_working_set == working_set is fine: a robot's set is
  // read and written by its own 16 lanes only -- updated in place)
  const LaunchForm form = balance_launch_form(in.surface_normal != nullptr, batch, pl.prev_working_set || pl.working_set, pl.set_memory != nullptr,
                                              pl.robot_order || pl.iterations || pl.next_robot_order);
  const int policy = pl.next_robot_order ? effective_policy(pl.policy, batch, form.warm) : QLAMD_PLACEMENT_NONE;
  StatePtrs s = state_ptrs(ctx, in, pl);
  s.wrench = wrench; s.live = live; s.support_only = support_only;
  s.record_doubles = layout == QLAMD_STATE_RECORDS ? QLAMD_STATE_RECORD_DOUBLES : 0;
  // the next launch's placement: by extra wavefronts in front of this launch
  const int chunk = batch >= QLAMD_THROUGHPUT_BATCH ? kShadowChunkLarge : (form.warm ? kShadowChunkWarm : kShadowChunkCold);
  const int64_t shadows = (batch + chunk - 1) / chunk;
  if (pl.next_robot_order && policy == QLAMD_PLACEMENT_NONE) {
    if (form.waves != 3) s.next_order = pl.next_robot_order; // (shadow_blocks stays 0: written by the slots themselves)
  } else if (pl.next_robot_order && shadows <= kShadowMaxBlocks && pick_rpw(ctx, batch) == 4) {
    s.prev_iterations = pl.prev_iterations;
    s.next_order = pl.next_robot_order;
    s.place_throughput = policy == QLAMD_PLACEMENT_THROUGHPUT ? 1 : 0;
    s.shadow_blocks = (int)shadows;
    s.shadow_chunk = chunk;
    s.place_hist = (uint32_t *)ctx->place_ws;
    s.place_sync = (uint32_t *)ctx->place_sync;
    s.place_wait = ctx->placement_wait;
  }

  hipError_t e;
  switch (pick_rpw(ctx, batch)) {
    case 4: {
      const unsigned grid = (unsigned)((batch + 4 * kCoopWaves - 1) / (4 * kCoopWaves)) + (unsigned)s.shadow_blocks;
      hipLaunchKernelGGL(coop_kernel_of(form), dim3(grid), dim3(64 * kCoopWaves), 0, st, ctx->d_params, s, batch, d_tau, d_grf, d_status);
      e = hipGetLastError();
      break;
    }
    case 16: e = launch_balance<16>(ctx, s, batch, d_tau, d_grf, d_status, st); break;
    default: e = launch_balance<64>(ctx, s, batch, d_tau, d_grf, d_status, st); break;
  }
  if (e != hipSuccess) return QLAMD_ERR_HIP;
  // a next placement the launch did not make itself (QLAMD_PLACEMENT_NONE in the three-wavefront form, more robots than the
  // shadow wavefronts take): launches of their own
  if (pl.next_robot_order && !s.next_order)
    return placement_launch(ctx, pl.prev_iterations, batch, policy, pl.next_robot_order, st, s.stance);
  return QLAMD_OK;
}

namespace {
// One launch of balance_robot_params_kernel on device arrays (the entry has checked its arguments): cold, warm-started from
// prev_working_set, or from the table, with or without per-leg normals -- always the two-wavefront form, whatever the batch
int robot_params_launch(qlamd_context *ctx, const qlamd_state_batch &in, const qlamd_placement &pl, const double *d_robot_params,
                        int64_t batch, double *d_tau, double *d_grf, int32_t *d_status, hipStream_t st) {
  const bool table = pl.set_memory != nullptr;
  const bool warm = pl.prev_working_set || pl.working_set || table;
  const StatePtrs s = state_ptrs(ctx, in, pl);
  const unsigned grid = (unsigned)((batch + 3) / 4);
  const auto kernel = s.normals ? (table  ? balance_robot_params_kernel<true, true, true>
                                   : warm ? balance_robot_params_kernel<true, true, false>
                                          : balance_robot_params_kernel<true, false, false>)
                                : (table  ? balance_robot_params_kernel<false, true, true>
                                   : warm ? balance_robot_params_kernel<false, true, false>
                                          : balance_robot_params_kernel<false, false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, st, ctx->d_params, s, batch, d_tau, d_grf, d_status, d_robot_params);
  return hipGetLastError() == hipSuccess ? QLAMD_OK : QLAMD_ERR_HIP;
}

// The public balance / force-distribution entries: the checks of their arguments, the host buffers' staging, then
// balance_launch.  pl: the placed entries' placement (NULL otherwise), in the memory space of the call; per_robot: the call is
// qlamd_balance_solve_robot_params_batch and robot_params [B] its records (in the memory space of the call)
int balance_entry(qlamd_context *ctx, const qlamd_state_batch *in_user, const double *wrench, int64_t batch, const qlamd_placement *pl,
                  double *joint_effort, double *contact_force, int32_t *status, int memory, void *stream, bool per_robot = false,
                  const qlamd_robot_params *robot_params = nullptr) {
  if (!ctx || !in_user || batch < 0 || !joint_effort || !status) return QLAMD_ERR_INVALID_ARGUMENT;
  qlamd_placement p;
  memset(&p, 0, sizeof(p));
  if (pl) p = *pl;
  if (!placement_ok(p)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (per_robot) {
    // records or nothing; the lane-cooperative kernels only; no placement made inside the launch (no shadow wavefronts in
    // these kernels: qlamd_placement_from_iterations makes it); 16-byte loads of the records
    if (!robot_params || (memory == QLAMD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(robot_params) & 15u)) || pick_rpw(ctx, batch) != 4 || p.prev_iterations ||
        p.next_robot_order || batch > INT32_MAX)
      return QLAMD_ERR_INVALID_ARGUMENT;
    if (memory == QLAMD_MEM_DEVICE && ctx->state_record_doubles) return QLAMD_ERR_INVALID_ARGUMENT; // (QLAMD_STATE_RECORDS: not taken)
  }
  // the table takes the place of prev_working_set, and its robots' four words are one 16-byte load
  if (p.set_memory && (p.prev_working_set || (reinterpret_cast<uintptr_t>(p.set_memory) & 15u))) return QLAMD_ERR_INVALID_ARGUMENT;
  const bool warm = p.prev_working_set || p.working_set || p.set_memory;
  if (warm && memory != QLAMD_MEM_DEVICE) return QLAMD_ERR_INVALID_ARGUMENT; // (a host-buffer call is bound by its copies)
  const bool placed = p.robot_order || p.iterations || p.next_robot_order || warm;
  // the one-lane kernels of qlamd_set_robots_per_wave know no placement (a lane is a robot there: nothing is shared)
  if (placed && pick_rpw(ctx, batch) != 4) return QLAMD_ERR_INVALID_ARGUMENT;
  if (placed && batch > INT32_MAX) return QLAMD_ERR_INVALID_ARGUMENT;
  if (p.robot_order && memory == QLAMD_MEM_HOST) {
    // host memory can be checked: every robot exactly once
    std::vector<uint8_t> seen((size_t)batch, 0);
    for (int64_t k = 0; k < batch; k++) {
      const int32_t o = p.robot_order[k];
      if (o < 0 || o >= batch || seen[(size_t)o]) return QLAMD_ERR_INVALID_ARGUMENT;
      seen[(size_t)o] = 1;
    }
  }
  qlamd_state_batch in = *in_user;
  if (!in.joint_position || !in.base_orientation || !in.support_leg) return QLAMD_ERR_INVALID_ARGUMENT;
  if (wrench) {
    // force distribution only: the base pose / twist fields are not read for arithmetic; point
    // them at valid memory of sufficient size (joint_position is [B][12])
    in.base_position = in.base_linear_velocity = in.base_angular_velocity = in.joint_position;
    in.desired_position = in.desired_linear_velocity = in.desired_angular_velocity = in.joint_position;
    in.desired_orientation = in.base_orientation;
  } else if (!in.base_position || !in.base_linear_velocity || !in.base_angular_velocity || !in.desired_position ||
             !in.desired_orientation || !in.desired_linear_velocity || !in.desired_angular_velocity) {
    return QLAMD_ERR_INVALID_ARGUMENT;
  }
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  // records instead of per-field arrays: the lane-cooperative kernels only (and never with an external wrench, whose entry
  // points the unused pose fields at joint_position); host-buffer calls take per-field arrays whatever the option says
  const int layout = memory == QLAMD_MEM_DEVICE && ctx->state_record_doubles ? QLAMD_STATE_RECORDS : QLAMD_STATE_FIELDS;
  if (layout == QLAMD_STATE_RECORDS && (pick_rpw(ctx, batch) != 4 || wrench)) return QLAMD_ERR_INVALID_ARGUMENT;
  qlamd_placement dp = p;
  if (memory == QLAMD_MEM_HOST) dp.prev_iterations = dp.next_robot_order = nullptr; // made on the host, behind the launch
  // host buffers: inputs, then outputs.  QLAMD_ON_FAILURE_KEEP: a failed robot's entries are not written by the kernel, and
  // the outputs are copied back whole -- so the caller's efforts / forces go up with the inputs and come back untouched.
  // (with an external wrench the pose / twist fields alias the head of joint_position)
  const size_t B = (size_t)batch;
  const bool keep = ctx->params.keep_on_failure != 0;
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(in.joint_position, B * 96); sg.in(in.base_position, B * 24); sg.in(in.base_orientation, B * 32);
  sg.in(in.base_linear_velocity, B * 24); sg.in(in.base_angular_velocity, B * 24);
  sg.in(in.desired_position, B * 24); sg.in(in.desired_orientation, B * 32);
  sg.in(in.desired_linear_velocity, B * 24); sg.in(in.desired_angular_velocity, B * 24);
  sg.in(in.support_leg, B * 4); sg.in(in.surface_normal, B * 96); sg.in(wrench, B * 48); sg.in(dp.robot_order, B * 4);
  sg.in(robot_params, B * sizeof(qlamd_robot_params));
  sg.out(joint_effort, B * 96, keep); sg.out(contact_force, B * 96, keep);
  sg.out(status, B * 4); sg.out(dp.iterations, B * 4);
  int rc = sg.upload(ctx, st);
  if (rc != QLAMD_OK) return rc;
  if (per_robot)
    rc = robot_params_launch(ctx, in, dp, reinterpret_cast<const double *>(robot_params), batch, joint_effort, contact_force, status, st);
  else
    rc = balance_launch(ctx, in, layout, wrench, nullptr, 0, dp, batch, joint_effort, contact_force, status, st);
  if (rc == QLAMD_OK) rc = sg.finish(st);
  if (rc == QLAMD_OK && memory == QLAMD_MEM_HOST && p.next_robot_order)
    rc = qlamd_placement_from_iterations(ctx, p.prev_iterations, batch, p.policy, p.next_robot_order, QLAMD_MEM_HOST, stream);
  return rc;
}
// the force-distribution entries' state: the four arrays they read
qlamd_state_batch wrench_state(const double *joint_position, const double *base_orientation, const uint8_t *support_leg,
                               const double *surface_normal) {
  qlamd_state_batch in;
  memset(&in, 0, sizeof(in));
  in.joint_position = joint_position;
  in.base_orientation = base_orientation;
  in.support_leg = support_leg;
  in.surface_normal = surface_normal;
  return in;
}
} // namespace

extern "C" {

int qlamd_balance_solve_batch(qlamd_context *ctx, const qlamd_state_batch *in, int64_t batch, double *joint_effort,
                              double *contact_force, int32_t *status, int memory, void *stream) {
  return balance_entry(ctx, in, nullptr, batch, nullptr, joint_effort, contact_force, status, memory, stream);
}

int qlamd_force_distribution_batch(qlamd_context *ctx, const double *joint_position, const double *base_orientation,
                                   const uint8_t *support_leg, const double *surface_normal,
                                   const double *virtual_wrench, int64_t batch, double *joint_effort,
                                   double *contact_force, int32_t *status, int memory, void *stream) {
  if (!virtual_wrench) return QLAMD_ERR_INVALID_ARGUMENT;
  const qlamd_state_batch in = wrench_state(joint_position, base_orientation, support_leg, surface_normal);
  return balance_entry(ctx, &in, virtual_wrench, batch, nullptr, joint_effort, contact_force, status, memory, stream);
}

int qlamd_balance_solve_placed_batch(qlamd_context *ctx, const qlamd_state_batch *in, int64_t batch, const qlamd_placement *placement,
                                     double *joint_effort, double *contact_force, int32_t *status, int memory, void *stream) {
  return balance_entry(ctx, in, nullptr, batch, placement, joint_effort, contact_force, status, memory, stream);
}

int qlamd_balance_solve_robot_params_batch(qlamd_context *ctx, const qlamd_state_batch *in, const qlamd_robot_params *robot_params,
                                           int64_t batch, const qlamd_placement *placement, double *joint_effort,
                                           double *contact_force, int32_t *status, int memory, void *stream) {
  return balance_entry(ctx, in, nullptr, batch, placement, joint_effort, contact_force, status, memory, stream, true, robot_params);
}

int qlamd_robot_params_fill(const qlamd_balance_params *params, int64_t count, qlamd_robot_params *out) {
  if (!params || !out || count < 0) return QLAMD_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < count; i++) fold_robot_params(params[i], &out[i]);
  return QLAMD_OK;
}

int qlamd_force_distribution_placed_batch(qlamd_context *ctx, const double *joint_position, const double *base_orientation,
                                          const uint8_t *support_leg, const double *surface_normal,
                                          const double *virtual_wrench, int64_t batch, const qlamd_placement *placement,
                                          double *joint_effort, double *contact_force, int32_t *status, int memory, void *stream) {
  if (!virtual_wrench) return QLAMD_ERR_INVALID_ARGUMENT;
  const qlamd_state_batch in = wrench_state(joint_position, base_orientation, support_leg, surface_normal);
  return balance_entry(ctx, &in, virtual_wrench, batch, placement, joint_effort, contact_force, status, memory, stream);
}

int qlamd_place_next_call(qlamd_context *ctx, const qlamd_placement *placement) {
  if (!ctx) return QLAMD_ERR_INVALID_ARGUMENT;
  QL_ENTER_NO_STREAM(ctx);
  ctx->has_next_placement = false;
  if (!placement) return QLAMD_OK;
  // (the table of the balance step: the whole-body step keeps two words per robot, the dense entries start cold)
  if (!placement_ok(*placement) || placement->set_memory) return QLAMD_ERR_INVALID_ARGUMENT;
  ctx->next_placement = *placement;
  ctx->has_next_placement = true;
  return QLAMD_OK;
}

int qlamd_virtual_wrench_batch(qlamd_context *ctx, const qlamd_state_batch *in, int64_t batch, double *wrench,
                               int memory, void *stream) {
  if (!ctx || !in || batch < 0 || !wrench) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->base_position || !in->base_orientation || !in->base_linear_velocity || !in->base_angular_velocity ||
      !in->desired_position || !in->desired_orientation || !in->desired_linear_velocity || !in->desired_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  StatePtrs s = state_ptrs(ctx, *in, qlamd_placement{}); // only the base state enters the wrench (virtual_wrench_kernel)
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(s.pos, B * 24); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.dpos, B * 24); sg.in(s.dquat, B * 32); sg.in(s.dlinvel, B * 24); sg.in(s.dangvel, B * 24);
  sg.out(wrench, B * 48);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((batch + 63) / 64);
  hipLaunchKernelGGL(virtual_wrench_kernel, dim3(grid), dim3(64), 0, st, ctx->d_params, s, batch, wrench);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

int qlamd_leg_kinematics_batch(qlamd_context *ctx, const double *joint_position, const double *base_orientation,
                               int64_t batch, double *foot_position, double *jacobian, double *gravity_torque,
                               int memory, void *stream) {
  if (!ctx || !joint_position || !base_orientation || batch < 0) return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(joint_position, B * 96); sg.in(base_orientation, B * 32);
  sg.out(foot_position, B * 96); sg.out(jacobian, B * 288); sg.out(gravity_torque, B * 96);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((4 * batch + 63) / 64);
  hipLaunchKernelGGL(leg_kinematics_kernel, dim3(grid), dim3(64), 0, st, ctx->d_params, joint_position, base_orientation, batch,
                     foot_position, jacobian, gravity_torque);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps)
QLAMD_BLOCK_STAMPS_ACCESSOR(qlamd_debug_block_stamps)

// HIP kernel (gfx950) of the whole-body plant step -- contact-constrained forward dynamics and the state update -- and its
// entry of the C-ABI of include/qlamd.h.  The arithmetic is csrc/plant_coop.hpp's; the lane layout, the failure rule, the tail
// and the entry's checks and staging are csrc/plant_step_body.hpp's, shared with the plant steps with contacts.
#include "plant_step_body.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// One robot per 16-lane row.  Everything is loaded before the first use and stored after the last: the outputs may alias the inputs.
// TWIN OF the load prologues of plant_contact_kernel (plant_contact_kernel.hip), plant_friction_kernel (plant_friction_kernel.hip) and
// anchored_plant_body (contact_anchor_kernel.hip), which add their own loads: the prologue stays text of each kernel because the
// compiler pairs multiplications and additions downstream of it differently once the loads come out of a function of their own
// (profiles/r17/refactor_checks.md).  A fix to one belongs in the others.
__global__ __launch_bounds__(64) void plant_step_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const PlantIn s, int64_t B,
                                                        double dt, const PlantOut o) {
  using namespace coop;
  __shared__ double tab[4 * kTabPerLeg];
  const DeviceParams &P = *Pp;
  TabStage ts;
  ts.issue(P);
  const PlantLane ln = plant_lane(B);
  const int leg = ln.leg, c = ln.c, jq = ln.jq;
  const int64_t i = ln.i;
  const bool comp = ln.comp;
  const bool step = o.q != nullptr;
  double quat[4], linvel[3], angvel[3], pos[3] = {0.0, 0.0, 0.0}, ge[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
    double2 v = a2[0]; quat[0] = v.x; quat[1] = v.y;
    v = a2[1]; quat[2] = v.x; quat[3] = v.y;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { linvel[k] = s.linvel[3 * i + k]; angvel[k] = s.angvel[3 * i + k]; }
  const double qj = s.q[12 * i + jq], qdj = s.qd[12 * i + jq], tauj = s.tau[12 * i + jq];
  const uint32_t sm = s.stance ? *reinterpret_cast<const uint32_t *>(s.stance + 4 * i) : 0u;
  double gej = 0.0;
  if (s.gext) {
#pragma unroll
    for (int k = 0; k < 6; k++) ge[k] = s.gext[18 * i + k];
    gej = s.gext[18 * i + 6 + jq];
  }
  if (step) {
#pragma unroll
    for (int k = 0; k < 3; k++) pos[k] = s.pos[3 * i + k];
  }
  ts.commit(tab);
  const bool on = ((support_mask(sm) >> leg) & 1u) != 0u;

  // ---- dynamics on the quad lanes (wholebody_kernel.hip)
  double Rm[9], gB[3], vB[3];
  quat_to_matrix(quat, Rm);
  const double gW[3] = {0.0, 0.0, -W.grav};
  irot(Rm, gW, gB);
  irot(Rm, linvel, vB);
  double sj, cj;
  sincos_reduced(qj, sj, cj);
  WbLink L;
  wb_link(CoopTab{tab + kTabPerLeg * leg}, c, sj, cj, L);
  const double V0[6] = {angvel[0], angvel[1], angvel[2], vB[0], vB[1], vB[2]};
  const double A0[6] = {0.0, 0.0, 0.0, -gB[0], -gB[1], -gB[2]};
  WbInertia T;
  double Fcol[6], Mleg[3];
  wb_crba(W, L, c, T, Fcol, Mleg);
  double hj, hb[6], gam[3];
  const double qd_l = comp ? qdj : 0.0;
  wb_inverse_dynamics(W, L, c, V0, A0, qd_l, 0.0, hj, hb);
  plant_foot_bias(L, c, V0, qd_l, gam);
  PlantSolution x;
  plant_solve(L, leg, c, T, Fcol, Mleg, hb, hj, gam, ge, comp ? tauj + gej : 0.0, on, x);

  // ---- outputs, and the state integrated from nu
  if (!plant_store_status(o.status, ln, x.ok ? kStatusOk : kStatusNotPd, P)) return;
  const double nu[6] = {vB[0], vB[1], vB[2], angvel[0], angvel[1], angvel[2]};
  plant_store_tail(o, ln, quat, linvel, angvel, pos, qj, qdj, Rm, x.ok, dt, nu, qdj, x.nub, x.nuj, x.f);
}

} // namespace

extern "C" {

int qlamd_wholebody_forward_dynamics_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *joint_effort,
                                           const double *generalized_force, const double *base_position, double gravity, double dt,
                                           int64_t batch, double *acceleration, double *contact_force, const qlamd_plant_next *next,
                                           int32_t *status, int memory, void *stream) {
  if (const int rc = plant_check(ctx, in, joint_effort, base_position, false, dt, batch, next, status, memory)) return rc;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  PlantCall k = plant_call(in, joint_effort, generalized_force, next ? base_position : nullptr, acceleration, contact_force, next,
                           nullptr, status);
  Staged sg(memory == QLAMD_MEM_HOST);
  plant_stage(sg, k, (size_t)batch, ctx->params.keep_on_failure != 0);
  if (const int rc = sg.upload(ctx, st)) return rc;
  // (this kernel's arguments have no room for the contact arrays, which are NULL here)
  const PlantIn s{k.s.q, k.s.qd, k.s.quat, k.s.linvel, k.s.angvel, k.s.stance, k.s.tau, k.s.gext, k.s.pos};
  const PlantOut o{k.o.acc, k.o.force, k.o.q, k.o.qd, k.o.pos, k.o.quat, k.o.linvel, k.o.angvel, k.o.status};
  hipLaunchKernelGGL(plant_step_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, st, ctx->d_params, plant_params(ctx, gravity),
                     s, batch, dt, o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps_plant)

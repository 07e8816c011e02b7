// HIP kernel (gfx950) of the plant step with touchdown impacts, contact stabilisation and the contact report, and its entry of
// the C-ABI (include/qlamd_plant_contacts.h, which qlamd.h includes).  The arithmetic is csrc/plant_contact_coop.hpp's: the KKT
// system of plant_coop.hpp, factored once and applied twice.  The lane layout, the failure rule, the tail and the entry's checks
// and staging are csrc/plant_step_body.hpp's.
#include "plant_step_body.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// TWIN OF anchored_plant_body<false> (contact_anchor_kernel.hip), which adds the anchors, and in its load prologue of
// plant_step_kernel (plant_kernel.hip): from the prologue to the status this stays text of each kernel, because the compiler pairs
// multiplications and additions differently once the same text stands in a function that several kernels call, and the results
// move in their last bits (profiles/r17/refactor_checks.md).  A fix to one belongs in the others.
// One robot per 16-lane row.  Everything is loaded before the first use and stored after the last: the outputs may alias the inputs.
// Robots with and without a touchdown share wavefronts: a robot without one runs the impact with a zero right-hand side and keeps
// its velocity by a select.
__global__ __launch_bounds__(64) void plant_contact_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const PlantContactIn s,
                                                           int64_t B, double dt, double kv, double mu, const PlantContactOut o) {
  using namespace coop;
  __shared__ double tab[4 * kTabPerLeg];
  const DeviceParams &P = *Pp;
  TabStage ts;
  ts.issue(P);
  const PlantLane ln = plant_lane(B);
  const int lr = ln.lr, leg = ln.leg, c = ln.c, jq = ln.jq;
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
  const uint32_t pm = s.prev ? *reinterpret_cast<const uint32_t *>(s.prev + 4 * i) : 0xFFFFFFFFu;
  double nW[3] = {0.0, 0.0, 1.0};
  if (s.normals) {
#pragma unroll
    for (int k = 0; k < 3; k++) nW[k] = s.normals[12 * i + 3 * leg + k];
  }
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
  const unsigned now = support_mask(sm), touch = now & ~support_mask(pm);
  const bool on = ((now >> leg) & 1u) != 0u, row_on = comp && on;
  const bool project = touch != 0u; // the same on all lanes of the row

  // ---- kinematics and the factors: q alone
  double Rm[9], gB[3], vB[3];
  quat_to_matrix(quat, Rm);
  const double gW[3] = {0.0, 0.0, -W.grav};
  irot(Rm, gW, gB);
  irot(Rm, linvel, vB);
  double sj, cj;
  sincos_reduced(qj, sj, cj);
  WbLink L;
  wb_link(CoopTab{tab + kTabPerLeg * leg}, c, sj, cj, L);
  PlantFactors F;
  {
    WbInertia T;
    double Fcol[6], Mleg[3];
    wb_crba(W, L, c, T, Fcol, Mleg);
    plant_factor(L, leg, c, T, Fcol, Mleg, on, F);
  }
  double jcol[3], jrow[3], Jb[6];
  plant_js_row(L, c, row_on, jcol, jrow, Jb);
  const double qd_l = comp ? qdj : 0.0;

  // ---- the impact: nu+ = nu + M^-1 Js' p, Js nu+ = 0 over all flagged feet
  const double nu0[6] = {vB[0], vB[1], vB[2], angvel[0], angvel[1], angvel[2]};
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  PlantApplied imp;
  plant_apply<false>(F, c, on, jcol, jrow, Jb, zero6, 0.0, project ? -plant_js_dot(Jb, jrow, row_on, nu0, qd_l) : 0.0, imp);
  double nup[6];
#pragma unroll
  for (int a = 0; a < 6; a++) nup[a] = project ? nu0[a] + imp.xb[a] : nu0[a];
  const double qdp = project ? qd_l + imp.xj : qd_l;
  const double p = project ? imp.y : 0.0;

  // ---- the dynamics at nu+
  const double V0[6] = {nup[3], nup[4], nup[5], nup[0], nup[1], nup[2]};
  const double A0[6] = {0.0, 0.0, 0.0, -gB[0], -gB[1], -gB[2]};
  double hj, hb[6], gam[3];
  wb_inverse_dynamics(W, L, c, V0, A0, qdp, 0.0, hj, hb);
  plant_foot_bias(L, c, V0, qdp, gam);
  double rb[6];
#pragma unroll
  for (int a = 0; a < 6; a++) rb[a] = ge[a] - hb[a];
  plant_js_row(L, c, row_on, jcol, jrow, Jb);
  PlantApplied x;
  plant_apply<true>(F, c, on, jcol, jrow, Jb, rb, comp ? (tauj + gej) - hj : 0.0,
                    -(pick3(gam, c) + kv * plant_js_dot(Jb, jrow, row_on, nup, qdp)), x);
  const double f = x.y;
  const bool ok = !row_any(!(F.ok && plant_applied_finite(imp, comp) && plant_applied_finite(x, comp)));

  // ---- outputs.  A failed robot's nu+ is nu as it came
  if (!plant_store_status(o.status, ln, ok ? kStatusOk : kStatusNotPd, P)) return;
  const int64_t jo = 3 * leg + c; // my joint / my force component (lanes c < 3)
  if (o.nu_plus) {
    if (comp) o.nu_plus[18 * i + 6 + jo] = ok ? qdp : qdj;
    if (lr < 6) {
      double v = ok ? nup[0] : nu0[0];
#pragma unroll
      for (int b = 1; b < 6; b++) v = sel(lr == b, ok ? nup[b] : nu0[b], v);
      o.nu_plus[18 * i + lr] = v;
    }
  }
  if (o.impulse && comp) o.impulse[12 * i + jo] = ok ? p : 0.0;
  if (o.report) {
    double nB[3] = {0.0, 0.0, 1.0}; // no normals: the base's z axis (n_W = R z, as in the control-step state batch)
    if (s.normals) irot(Rm, nW, nB);
    const double fl[3] = {quad_bc<0>(f), quad_bc<1>(f), quad_bc<2>(f)};
    const unsigned bits = plant_contact_bits(fl, nB, mu) | (((touch >> leg) & 1u) ? 4u : 0u);
    if (c == 0) o.report[4 * i + leg] = (uint8_t)((ok && on) ? bits : 0u);
  }
  plant_store_tail(o, ln, quat, linvel, angvel, pos, qj, qdj, Rm, ok, dt, nup, qdp, x.xb, x.xj, f);
}

} // namespace

extern "C" {

int qlamd_wholebody_plant_step_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *joint_effort,
                                     const double *generalized_force, const double *base_position, double gravity, double dt,
                                     int64_t batch, double *acceleration, double *contact_force, const qlamd_plant_next *next,
                                     const qlamd_plant_contacts *contacts, int32_t *status, int memory, void *stream) {
  if (!contacts)
    return qlamd_wholebody_forward_dynamics_batch(ctx, in, joint_effort, generalized_force, base_position, gravity, dt, batch,
                                                  acceleration, contact_force, next, status, memory, stream);
  if (const int rc = plant_check(ctx, in, joint_effort, base_position, false, dt, batch, next, status, memory)) return rc;
  const double kv = contacts->velocity_gain, mu = contacts->friction_coefficient;
  if (!(kv >= 0.0) || !(kv - kv == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (contacts->contact_report && (!(mu >= 0.0) || !(mu - mu == 0.0))) return QLAMD_ERR_INVALID_ARGUMENT; // (read for the report only)
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  PlantCall k = plant_call(in, joint_effort, generalized_force, next ? base_position : nullptr, acceleration, contact_force, next,
                           contacts, status);
  Staged sg(memory == QLAMD_MEM_HOST);
  plant_stage(sg, k, (size_t)batch, ctx->params.keep_on_failure != 0);
  if (const int rc = sg.upload(ctx, st)) return rc;
  hipLaunchKernelGGL(plant_contact_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, st, ctx->d_params, plant_params(ctx, gravity),
                     static_cast<const PlantContactIn &>(k.s), batch, dt, kv, mu, static_cast<const PlantContactOut &>(k.o));
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps_plant_contact)

// HIP kernel (gfx950) of the plant step with friction -- contact impulses and forces as the minimisers of the plant's own quadratic
// over the friction pyramid -- and its entry of the C-ABI (include/qlamd_plant_friction.h, which qlamd.h includes).  The arithmetic
// is csrc/plant_friction_coop.hpp's: plant_contact_coop.hpp's factors, and force_qp_coop.hpp's active-set method in the place of
// the multiplier step, once for the impulse and once for the force.
#include "plant_friction_coop.hpp"
#include "context.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// (no __restrict__ anywhere: the next state may be written over the state it was computed from)
struct FrictionIn {
  const double *q, *qd, *quat, *linvel, *angvel;
  const uint8_t *stance;           // or NULL: free flight
  const uint8_t *prev;             // or NULL: no touchdown
  const double *normals;           // or NULL: the base's z axis
  const double *tau, *gext, *pos;  // gext, pos: or NULL
};
struct FrictionOut {
  double *acc, *force;                           // or NULL
  double *nu_plus, *impulse;                     // or NULL
  uint8_t *report;                               // or NULL
  double *q, *qd, *pos, *quat, *linvel, *angvel; // all NULL: no state update
  int32_t *status;
  int32_t *iterations;                           // or NULL: [B][2]
};

// TWIN OF plant_contact_kernel (plant_contact_kernel.hip): the load prologue, the kinematics and factors, the output and
// state-update tail, and the entry's checks and staging below repeat that file's (that unit keeps its text, so nothing is shared
// through it).  A fix to one belongs in the other.
// One robot per 16-lane row.  Everything is loaded before the first use and stored after the last: the outputs may alias the inputs.
// Robots with and without a touchdown share wavefronts: a robot without one runs the impulse QP with a zero linear term (it ends
// at its first selection) and keeps its velocity by a select; a wavefront without any touchdown does not run it.
// More than 256 registers: one wavefront per SIMD.
constexpr int kFrictionLdsDoubles = 4 * kTabPerLeg + 4 * coop::kCoopLdsDoubles + coop::kForceQpNrmRows * 64;
__global__ __launch_bounds__(64) void plant_friction_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const FrictionIn s, int64_t B,
                                                            double dt, double kv, double mu, const FrictionOut o) {
  using namespace coop;
  __shared__ double lds[kFrictionLdsDoubles];
  double *tab = lds, *rows = lds + 4 * kTabPerLeg, *nrm = rows + 4 * kCoopLdsDoubles;
  const DeviceParams &P = *Pp;
  TabStage ts;
  ts.issue(P);
  const int row = threadIdx.x >> 4, lr = threadIdx.x & 15, leg = lr >> 2, c = lr & 3;
  const int64_t i0 = (int64_t)blockIdx.x * 4 + row;
  const bool live = i0 < B;
  const int64_t i = live ? i0 : B - 1;
  const bool comp = c < 3;
  const int jq = 3 * leg + (comp ? c : 2);
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
  // the pyramid of my leg, and what both QPs share
  ForceQp Q;
  double nB[3] = {0.0, 0.0, 1.0}; // no normals: the base's z axis (n_W = R z, as in the control-step state batch)
  if (s.normals) irot(Rm, nW, nB);
  const bool pyramid_ok = plant_pyramid(Rm, nB, c, mu, Q) || !on;
  Q.on = on; Q.comp = comp; Q.nS = __popc(now); Q.refine_passes = 1;
  Q.jrow[0] = Q.jrow[1] = Q.jrow[2] = 0.0; Q.jcol[0] = Q.jcol[1] = Q.jcol[2] = 0.0; Q.tq_up = 0.0; Q.tq_lo = 0.0;
  Q.warm = 0ull; Q.stance = now; Q.build_set = false;
  const bool bad = row_any(!(F.ok && pyramid_ok)); // (the same on all lanes of the row: such a row leaves both QPs at once)
  double *lds_row = rows + kCoopLdsDoubles * row;

  // ---- the impact: p = argmin over the pyramid of 1/2 p'H0 p + p'(Js nu), nu+ = nu + M^-1 Js' p
  const double nu0[6] = {vB[0], vB[1], vB[2], angvel[0], angvel[1], angvel[2]};
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  PlantFree rest;
  plant_free<false>(F, c, on, jrow, Jb, zero6, 0.0, 0.0, rest);
  PlantApplied imp;
  int st_p = kStatusOk, it_p = 0;
  {
    double pq = 0.0;
    unsigned set_p = 0u;
    if (__builtin_amdgcn_ballot_w64(project) != 0ull) {
      st_p = plant_cone_qp(Q, F, bad, project ? plant_js_dot(Jb, jrow, row_on, nu0, qd_l) : 0.0, lds_row, nrm, pq, it_p, set_p);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (the force QP writes the blocks this one has just read)
    }
    st_p = project ? st_p : kStatusOk;
    it_p = project ? it_p : 0;
    plant_lift(F, jcol, (project && row_on && st_p == kStatusOk) ? pq : 0.0, rest, imp);
  }
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
  // f = argmin over the pyramid of 1/2 f'H0 f - f'(r - Js x_0), nu' = x_0 + M^-1 Js' f
  PlantFree x0;
  plant_free<true>(F, c, on, jrow, Jb, rb, comp ? (tauj + gej) - hj : 0.0,
                   -(pick3(gam, c) + kv * plant_js_dot(Jb, jrow, row_on, nup, qdp)), x0);
  PlantApplied x;
  int st_f = kStatusOk, it_f = 0;
  unsigned set_f = 0u;
  {
    double fq = 0.0;
    st_f = plant_cone_qp(Q, F, bad, -x0.cv, lds_row, nrm, fq, it_f, set_f);
    plant_lift(F, jcol, (row_on && st_f == kStatusOk) ? fq : 0.0, x0, x);
  }
  const double f = x.y;
  // the QP's own status (the impulse's first); a value that is not finite is QLAMD_STATUS_NOT_PD as in the hard-contact entry
  int st = bad ? kStatusNotPd : (st_p != kStatusOk ? st_p : st_f);
  st = (st == kStatusOk && row_any(!(plant_applied_finite(imp, comp) && plant_applied_finite(x, comp)))) ? kStatusNotPd : st;
  const bool ok = st == kStatusOk;

  // ---- outputs.  A failed robot: zeros, nu and its state as they came, or (QLAMD_ON_FAILURE_KEEP) nothing but its status
  if (lr == 0 && live) o.status[i] = st;
  if (!live || (!ok && P.keep_on_failure)) return;
  if (o.iterations && lr < 2) o.iterations[2 * i + lr] = lr == 0 ? it_p : it_f;
  const int64_t jo = 3 * leg + c; // my joint / my force component (lanes c < 3)
  if (o.acc) {
    if (comp) o.acc[18 * i + 6 + jo] = ok ? x.xj : 0.0;
    if (lr < 6) {
      double v = x.xb[0];
#pragma unroll
      for (int b = 1; b < 6; b++) v = sel(lr == b, x.xb[b], v);
      o.acc[18 * i + lr] = ok ? v : 0.0;
    }
  }
  if (o.force && comp) o.force[12 * i + jo] = ok ? f : 0.0;
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
    const unsigned bits = plant_friction_bits(set_f, leg) | (((touch >> leg) & 1u) ? 4u : 0u);
    if (c == 0) o.report[4 * i + leg] = (uint8_t)((ok && on) ? bits : 0u);
  }
  if (!step) return;
  // semi-implicit Euler from nu+ (include/qlamd.h has the rule)
  double qn[4] = {quat[0], quat[1], quat[2], quat[3]}, pn[3] = {pos[0], pos[1], pos[2]};
  double ln[3] = {linvel[0], linvel[1], linvel[2]}, wn[3] = {angvel[0], angvel[1], angvel[2]};
  double qdn = qdj, qjn = qj;
  if (ok) {
    qdn = qdp + dt * x.xj;
    qjn = qj + dt * qdn;
    double vn[3], phi[3], dv[3], Rn[9];
#pragma unroll
    for (int a = 0; a < 3; a++) { vn[a] = nup[a] + dt * x.xb[a]; wn[a] = nup[3 + a] + dt * x.xb[3 + a]; phi[a] = dt * wn[a]; }
    plant_quat_step(quat, phi, qn);
    rot(Rm, vn, dv);
#pragma unroll
    for (int a = 0; a < 3; a++) pn[a] = pos[a] + dt * dv[a];
    quat_to_matrix(qn, Rn);
    rot(Rn, vn, ln);
  }
  if (comp) { o.q[12 * i + jo] = qjn; o.qd[12 * i + jo] = qdn; }
  if (lr < 4) {
    double v = qn[0];
#pragma unroll
    for (int b = 1; b < 4; b++) v = sel(lr == b, qn[b], v);
    o.quat[4 * i + lr] = v;
  }
  if (lr < 3) {
    o.pos[3 * i + lr] = sel(lr == 2, pn[2], sel(lr == 1, pn[1], pn[0]));
    o.linvel[3 * i + lr] = sel(lr == 2, ln[2], sel(lr == 1, ln[1], ln[0]));
    o.angvel[3 * i + lr] = sel(lr == 2, wn[2], sel(lr == 1, wn[1], wn[0]));
  }
}

} // namespace

extern "C" {

int qlamd_wholebody_plant_step_friction_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *joint_effort,
                                              const double *generalized_force, const double *base_position, double gravity, double dt,
                                              int64_t batch, double *acceleration, double *contact_force, const qlamd_plant_next *next,
                                              const qlamd_plant_contacts *contacts, const qlamd_plant_friction *friction,
                                              int32_t *status, int memory, void *stream) {
  if (!friction)
    return qlamd_wholebody_plant_step_batch(ctx, in, joint_effort, generalized_force, base_position, gravity, dt, batch, acceleration,
                                            contact_force, next, contacts, status, memory, stream);
  if (!ctx || !in || batch < 0 || !joint_effort || !status || !contacts) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (next) {
    if (!base_position || !(dt > 0.0) || !(dt - dt == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
    if (!next->joint_position || !next->joint_velocity || !next->base_position || !next->base_orientation ||
        !next->base_linear_velocity || !next->base_angular_velocity)
      return QLAMD_ERR_INVALID_ARGUMENT;
  }
  const double kv = contacts->velocity_gain, mu = contacts->friction_coefficient;
  if (!(kv >= 0.0) || !(kv - kv == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!(mu > 0.0) || !(mu - mu == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT; // (read with or without a report: it is the constraint)
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  FrictionIn s{in->joint_position, in->joint_velocity, in->base_orientation, in->base_linear_velocity, in->base_angular_velocity,
              in->support_leg, contacts->previous_support_leg, in->surface_normal, joint_effort, generalized_force,
              next ? base_position : nullptr};
  FrictionOut o{};
  o.acc = acceleration; o.force = contact_force; o.status = status;
  o.iterations = friction->iterations;
  o.nu_plus = contacts->post_impact_velocity; o.impulse = contacts->impulse; o.report = contacts->contact_report;
  if (next) {
    o.q = next->joint_position; o.qd = next->joint_velocity; o.pos = next->base_position; o.quat = next->base_orientation;
    o.linvel = next->base_linear_velocity; o.angvel = next->base_angular_velocity;
  }
  const bool keep = ctx->params.keep_on_failure != 0; // entries the kernel leaves alone come back as they went up
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.stance, B * 4); sg.in(s.prev, B * 4); sg.in(s.normals, B * 96); sg.in(s.tau, B * 96); sg.in(s.gext, B * 144);
  sg.in(s.pos, B * 24);
  sg.out(o.acc, B * 144, keep); sg.out(o.force, B * 96, keep);
  sg.out(o.nu_plus, B * 144, keep); sg.out(o.impulse, B * 96, keep); sg.out(o.report, B * 4, keep);
  sg.out(o.q, B * 96, keep); sg.out(o.qd, B * 96, keep); sg.out(o.pos, B * 24, keep); sg.out(o.quat, B * 32, keep);
  sg.out(o.linvel, B * 24, keep); sg.out(o.angvel, B * 24, keep); sg.out(o.iterations, B * 8, keep); sg.out(o.status, B * 4);
  if (const int rc = sg.upload(ctx, st)) return rc;
  coop::WbParamsDev W;
  W.base_m = ctx->base_m;
  for (int a = 0; a < 3; a++) W.base_h[a] = ctx->base_h[a];
  for (int a = 0; a < 6; a++) W.base_I[a] = ctx->base_I[a];
  W.w_tau = 0.0; W.tau_max = 0.0; W.grav = gravity;
  hipLaunchKernelGGL(plant_friction_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, st, ctx->d_params, W, s, batch, dt, kv, mu, o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps_plant_friction)

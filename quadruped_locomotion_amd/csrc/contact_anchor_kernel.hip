// HIP kernels (gfx950) of the contact anchors -- where each flagged foot is held -- and their entries of the C-ABI
// (include/qlamd_contact_anchor.h, which qlamd.h includes): the contact update that keeps the anchors, and the plant step, with
// hard contacts or with friction, whose constraint right-hand side carries the position term -k_p e.  The update is the body of
// csrc/contact_update_body.hpp with kAnchored, where the anchor rule is; the error is below, between the lane layout, the failure
// rule and the tail of csrc/plant_step_body.hpp.  The arithmetic is csrc/plant_contact_coop.hpp's and csrc/plant_friction_coop.hpp's.
#include "plant_step_body.hpp"
#include "contact_update_body.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

__global__ __launch_bounds__(kUpdateBlock) void anchored_contact_update_kernel(const DeviceParams *Pp, const UpdateIn s, const UpdateGrid G,
                                                                               const ContactRule rule, unsigned reanchor, int64_t B,
                                                                               const AnchoredUpdateOut o) {
  __shared__ double tab[4 * kTabPerLeg];
  contact_update_body<true>(tab, Pp, s, G, rule, reanchor, B, o);
}

// TWIN OF plant_contact_kernel (plant_contact_kernel.hip; kFriction false) AND OF plant_friction_kernel (plant_friction_kernel.hip;
// kFriction true): the load prologue, the kinematics and factors, the impact, the dynamics at nu+ and the contact outputs repeat
// those files' in their order; the lane layout, the failure rule and the tail are csrc/plant_step_body.hpp's, as theirs.  From the
// prologue to the status the text is not shared with them, because the compiler pairs multiplications and additions differently
// once it stands in a function that they call as well, and their results move in their last bits
// (profiles/r17/refactor_checks.md).  A fix to one belongs in the others.  What is added: the anchor of my leg among the
// prologue's loads, the clamped error of my row next to the factors -- one live register until r is formed -- its term in r, its
// finiteness in the status, and position_error.
// One robot per 16-lane row, lane 4 * leg + c.  Everything is loaded before the first use and stored after the last.
template <bool kFriction>
__device__ __forceinline__ void anchored_plant_body(double *lds, const DeviceParams *Pp, const coop::WbParamsDev &W, const AnchoredPlantIn &s,
                                                    int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                    const AnchoredPlantOut &o) {
  using namespace coop;
  double *tab = lds;
  const DeviceParams &P = *Pp;
  TabStage ts;
  ts.issue(P);
  const PlantLane ln = plant_lane(B);
  const int row = ln.row, lr = ln.lr, leg = ln.leg, c = ln.c, jq = ln.jq;
  const int64_t i = ln.i;
  const bool comp = ln.comp;
  double quat[4], linvel[3], angvel[3], pos[3], anc[3], ge[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
#pragma unroll
  for (int k = 0; k < 3; k++) { pos[k] = s.pos[3 * i + k]; anc[k] = s.anchor[12 * i + 3 * leg + k]; }
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
  // the error of my foot against its anchor, base coordinates: e = r - R'(a - pos), clamped to length emax; my lane keeps
  // component c.  An unflagged leg's anchor is never looked at (selects); a flagged leg's that is not finite fails the robot.
  double ehat;
  bool anchor_ok;
  {
    const double dW[3] = {anc[0] - pos[0], anc[1] - pos[1], anc[2] - pos[2]};
    double dB[3];
    irot(Rm, dW, dB);
    const double e[3] = {L.pf[0] - dB[0], L.pf[1] - dB[1], L.pf[2] - dB[2]};
    const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const double scale = len > emax ? emax / len : 1.0; // (|e| = 0: e itself)
    const double ec = pick3(e, c) * scale;
    anchor_ok = !on || (__builtin_isfinite(e[0]) && __builtin_isfinite(e[1]) && __builtin_isfinite(e[2]) && __builtin_isfinite(ec));
    ehat = (row_on && anchor_ok) ? ec : 0.0;
  }
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
  const double nu0[6] = {vB[0], vB[1], vB[2], angvel[0], angvel[1], angvel[2]};
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double nB[3] = {0.0, 0.0, 1.0}; // no normals: the base's z axis (n_W = R z, as in the control-step state batch)
  if (s.normals) irot(Rm, nW, nB);

  PlantApplied imp, x;
  int st = kStatusOk, it_p = 0, it_f = 0;
  unsigned set_f = 0u;
  double nup[6], qdp, p, hj, hb[6], gam[3], rb[6];
  if constexpr (kFriction) {
    double *rows = lds + 4 * kTabPerLeg, *nrm = rows + 4 * kCoopLdsDoubles;
    // the pyramid of my leg, and what both QPs share
    ForceQp Q;
    const bool pyramid_ok = plant_pyramid(Rm, nB, c, mu, Q) || !on;
    Q.on = on; Q.comp = comp; Q.nS = __popc(now); Q.refine_passes = 1;
    Q.jrow[0] = Q.jrow[1] = Q.jrow[2] = 0.0; Q.jcol[0] = Q.jcol[1] = Q.jcol[2] = 0.0; Q.tq_up = 0.0; Q.tq_lo = 0.0;
    Q.warm = 0ull; Q.stance = now; Q.build_set = false;
    const bool bad = row_any(!(F.ok && pyramid_ok && anchor_ok)); // (the same on all lanes of the row: such a row leaves both QPs at once)
    double *lds_row = rows + kCoopLdsDoubles * row;

    // ---- the impact: p = argmin over the pyramid of 1/2 p'H0 p + p'(Js nu), nu+ = nu + M^-1 Js' p
    PlantFree rest;
    plant_free<false>(F, c, on, jrow, Jb, zero6, 0.0, 0.0, rest);
    int st_p = kStatusOk;
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
#pragma unroll
    for (int a = 0; a < 6; a++) nup[a] = project ? nu0[a] + imp.xb[a] : nu0[a];
    qdp = project ? qd_l + imp.xj : qd_l;
    p = project ? imp.y : 0.0;

    // ---- the dynamics at nu+
    const double V0[6] = {nup[3], nup[4], nup[5], nup[0], nup[1], nup[2]};
    const double A0[6] = {0.0, 0.0, 0.0, -gB[0], -gB[1], -gB[2]};
    wb_inverse_dynamics(W, L, c, V0, A0, qdp, 0.0, hj, hb);
    plant_foot_bias(L, c, V0, qdp, gam);
#pragma unroll
    for (int a = 0; a < 6; a++) rb[a] = ge[a] - hb[a];
    plant_js_row(L, c, row_on, jcol, jrow, Jb);
    // f = argmin over the pyramid of 1/2 f'H0 f - f'(r - Js x_0), nu' = x_0 + M^-1 Js' f, with r = -gamma - k_v Js nu+ - k_p e
    PlantFree x0;
    plant_free<true>(F, c, on, jrow, Jb, rb, comp ? (tauj + gej) - hj : 0.0,
                     -(pick3(gam, c) + kv * plant_js_dot(Jb, jrow, row_on, nup, qdp) + kp * ehat), x0);
    int st_f = kStatusOk;
    {
      double fq = 0.0;
      st_f = plant_cone_qp(Q, F, bad, -x0.cv, lds_row, nrm, fq, it_f, set_f);
      plant_lift(F, jcol, (row_on && st_f == kStatusOk) ? fq : 0.0, x0, x);
    }
    // the QP's own status (the impulse's first); a value that is not finite is QLAMD_STATUS_NOT_PD as in the hard-contact entry
    st = bad ? kStatusNotPd : (st_p != kStatusOk ? st_p : st_f);
    st = (st == kStatusOk && row_any(!(plant_applied_finite(imp, comp) && plant_applied_finite(x, comp)))) ? kStatusNotPd : st;
  } else {
    // ---- the impact: nu+ = nu + M^-1 Js' p, Js nu+ = 0 over all flagged feet
    plant_apply<false>(F, c, on, jcol, jrow, Jb, zero6, 0.0, project ? -plant_js_dot(Jb, jrow, row_on, nu0, qd_l) : 0.0, imp);
#pragma unroll
    for (int a = 0; a < 6; a++) nup[a] = project ? nu0[a] + imp.xb[a] : nu0[a];
    qdp = project ? qd_l + imp.xj : qd_l;
    p = project ? imp.y : 0.0;

    // ---- the dynamics at nu+, with r = -gamma - k_v Js nu+ - k_p e
    const double V0[6] = {nup[3], nup[4], nup[5], nup[0], nup[1], nup[2]};
    const double A0[6] = {0.0, 0.0, 0.0, -gB[0], -gB[1], -gB[2]};
    wb_inverse_dynamics(W, L, c, V0, A0, qdp, 0.0, hj, hb);
    plant_foot_bias(L, c, V0, qdp, gam);
#pragma unroll
    for (int a = 0; a < 6; a++) rb[a] = ge[a] - hb[a];
    plant_js_row(L, c, row_on, jcol, jrow, Jb);
    plant_apply<true>(F, c, on, jcol, jrow, Jb, rb, comp ? (tauj + gej) - hj : 0.0,
                      -(pick3(gam, c) + kv * plant_js_dot(Jb, jrow, row_on, nup, qdp) + kp * ehat), x);
    st = row_any(!(F.ok && anchor_ok && plant_applied_finite(imp, comp) && plant_applied_finite(x, comp))) ? kStatusNotPd : kStatusOk;
  }
  const double f = x.y;
  const bool ok = st == kStatusOk;

  // ---- outputs.  A failed robot's nu+ is nu as it came
  if (!plant_store_status(o.status, ln, st, P)) return;
  if constexpr (kFriction) {
    if (o.iterations && lr < 2) o.iterations[2 * i + lr] = lr == 0 ? it_p : it_f;
  }
  const int64_t jo = 3 * leg + c; // my joint / my force component (lanes c < 3)
  if (o.perr && comp) o.perr[12 * i + jo] = ok ? ehat : 0.0;
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
    unsigned bits;
    if constexpr (kFriction) {
      bits = plant_friction_bits(set_f, leg);
    } else {
      const double fl[3] = {quad_bc<0>(f), quad_bc<1>(f), quad_bc<2>(f)};
      bits = plant_contact_bits(fl, nB, mu);
    }
    bits |= ((touch >> leg) & 1u) ? 4u : 0u;
    if (c == 0) o.report[4 * i + leg] = (uint8_t)((ok && on) ? bits : 0u);
  }
  plant_store_tail(o, ln, quat, linvel, angvel, pos, qj, qdj, Rm, ok, dt, nup, qdp, x.xb, x.xj, f);
}

__global__ __launch_bounds__(64) void anchored_plant_contact_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const AnchoredPlantIn s,
                                                                    int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                                    const AnchoredPlantOut o) {
  __shared__ double lds[4 * kTabPerLeg];
  anchored_plant_body<false>(lds, Pp, W, s, B, dt, kv, mu, kp, emax, o);
}

// More than 256 registers: one wavefront per SIMD, as without anchors.
__global__ __launch_bounds__(64) void anchored_plant_friction_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const AnchoredPlantIn s,
                                                                     int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                                     const AnchoredPlantOut o) {
  __shared__ double lds[kFrictionLdsDoubles];
  anchored_plant_body<true>(lds, Pp, W, s, B, dt, kv, mu, kp, emax, o);
}

} // namespace

extern "C" {

int qlamd_wholebody_contact_update_anchored_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *base_position,
                                                  const qlamd_contact_update *update, const qlamd_contact_anchors *anchors,
                                                  int64_t batch, int32_t *status, int memory, void *stream) {
  if (!anchors) return qlamd_wholebody_contact_update_batch(ctx, in, base_position, update, batch, status, memory, stream);
  if (!anchors->anchor) return QLAMD_ERR_INVALID_ARGUMENT;
  if (const int rc = contact_update_check(ctx, in, base_position, update, batch, status, memory)) return rc;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  UpdateCall k = contact_update_call(in, base_position, update, status, anchors->anchor);
  Staged sg(memory == QLAMD_MEM_HOST);
  contact_update_stage(sg, k, update->heightfield, (size_t)batch, ctx->params.keep_on_failure != 0);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((4 * batch + kUpdateBlock - 1) / kUpdateBlock);
  hipLaunchKernelGGL(anchored_contact_update_kernel, dim3(grid), dim3(kUpdateBlock), 0, st, ctx->d_params, k.s, k.G, k.rule,
                     (unsigned)anchors->reanchor_mask, batch, k.o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

int qlamd_wholebody_plant_step_anchored_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *joint_effort,
                                              const double *generalized_force, const double *base_position, double gravity, double dt,
                                              int64_t batch, double *acceleration, double *contact_force, const qlamd_plant_next *next,
                                              const qlamd_plant_contacts *contacts, const qlamd_plant_friction *friction,
                                              const qlamd_plant_anchor *anchor, int32_t *status, int memory, void *stream) {
  if (!anchor)
    return qlamd_wholebody_plant_step_friction_batch(ctx, in, joint_effort, generalized_force, base_position, gravity, dt, batch,
                                                     acceleration, contact_force, next, contacts, friction, status, memory, stream);
  if (!contacts || !anchor->anchor) return QLAMD_ERR_INVALID_ARGUMENT;
  // (the base position with or without `next`: the error is measured from it)
  if (const int rc = plant_check(ctx, in, joint_effort, base_position, true, dt, batch, next, status, memory)) return rc;
  const double kv = contacts->velocity_gain, mu = contacts->friction_coefficient;
  const double kp = anchor->position_gain, emax = anchor->max_error;
  if (!(kv >= 0.0) || !(kv - kv == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (friction) {
    if (!(mu > 0.0) || !(mu - mu == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT; // (read with or without a report: it is the constraint)
  } else if (contacts->contact_report && (!(mu >= 0.0) || !(mu - mu == 0.0))) {
    return QLAMD_ERR_INVALID_ARGUMENT;
  }
  if (!(kp >= 0.0) || !(kp - kp == 0.0) || !(emax > 0.0)) return QLAMD_ERR_INVALID_ARGUMENT; // (emax = +infinity: no clamp)
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  PlantCall k = plant_call(in, joint_effort, generalized_force, base_position, acceleration, contact_force, next, contacts, status);
  k.s.anchor = anchor->anchor;
  k.o.iterations = friction ? friction->iterations : nullptr;
  k.o.perr = anchor->position_error;
  Staged sg(memory == QLAMD_MEM_HOST);
  plant_stage(sg, k, (size_t)batch, ctx->params.keep_on_failure != 0);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const coop::WbParamsDev W = plant_params(ctx, gravity);
  const dim3 grid((unsigned)((batch + 3) / 4));
  if (friction)
    hipLaunchKernelGGL(anchored_plant_friction_kernel, grid, dim3(64), 0, st, ctx->d_params, W, k.s, batch, dt, kv, mu, kp, emax, k.o);
  else
    hipLaunchKernelGGL(anchored_plant_contact_kernel, grid, dim3(64), 0, st, ctx->d_params, W, k.s, batch, dt, kv, mu, kp, emax, k.o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps_contact_anchor)

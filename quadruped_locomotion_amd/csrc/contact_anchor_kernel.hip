// HIP kernels (gfx950) of the contact anchors -- where each flagged foot is held -- and their entries of the C-ABI
// (include/qlamd_contact_anchor.h, which qlamd.h includes): the contact update that keeps the anchors, and the plant step, with
// hard contacts or with friction, whose constraint right-hand side carries the position term -k_p e.  The arithmetic is
// csrc/contact_update_core.hpp's, csrc/plant_contact_coop.hpp's and csrc/plant_friction_coop.hpp's; the anchor rule and the error
// are below.
#include "plant_friction_coop.hpp"
#include "contact_update_core.hpp"
#include "context.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// ---------------------------------------------------------------------------------------------------------------- the update

// (no __restrict__ anywhere: support_next may be the array the current flags are read from)
struct AnchorUpdateIn {
  const double *q, *qd, *quat, *linvel, *angvel, *pos;
  const uint8_t *stance;   // or NULL: no foot is flagged
  const uint8_t *report;   // or NULL
  const double *plane;     // or NULL
  const double *heights;   // or NULL; with plane NULL as well: the ground z = 0
};
struct AnchorUpdateGrid { double ox, oy, inv_res; int nx, ny; };
struct AnchorUpdateOut {
  uint8_t *next, *sensor, *events;    // each or NULL
  double *gap, *normal, *fpos, *fvel; // each or NULL
  int32_t *status;
  double *anchor;                     // never read
};

constexpr int kUpdateBlock = 256; // 64 robots per block: the model table is staged once for 256 lanes, two loads each
constexpr unsigned kEventReanchored = 8;

// the bytes of a quad's four lanes, each in its own byte of the word, OR-ed into one word that all four lanes hold
__device__ __forceinline__ uint32_t quad_or(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true); // quad_perm [1, 0, 3, 2]
  x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true); // quad_perm [2, 3, 0, 1]
  return x;
}

// TWIN OF contact_update_kernel (contact_update_kernel.hip): the loads, the geometry, the flags and the outputs repeat that
// file's (that unit keeps its text, so nothing is shared through it); the anchor rule and its three stores are added.  A fix to
// one belongs in the other.
// One lane per (robot, leg), 16 robots per wavefront.  Everything is loaded before the first store; the anchors are only written:
// 336 bytes read and up to 432 written per robot with every array given.
__global__ __launch_bounds__(kUpdateBlock) void anchored_contact_update_kernel(const DeviceParams *Pp, const AnchorUpdateIn s,
                                                                               const AnchorUpdateGrid G, const ContactRule rule,
                                                                               unsigned reanchor, int64_t B, const AnchorUpdateOut o) {
  __shared__ double tab[4 * kTabPerLeg];
  const DeviceParams &P = *Pp;
  const int second = (int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg ? (int)threadIdx.x + kUpdateBlock : 4 * kTabPerLeg - 1;
  const double tab0 = P.legtab[threadIdx.x], tab1 = P.legtab[second];
  const int64_t t0 = (int64_t)blockIdx.x * kUpdateBlock + threadIdx.x;
  const bool live = t0 < 4 * B; // a quad is live or dead as a whole
  const int64_t t = live ? t0 : 4 * B - 1;
  const int64_t i = t >> 2;
  const int leg = (int)(t & 3);
  double q[3], qd[3], quat[4], linvel[3], angvel[3], pos[3];
  load3(s.q, t, q); load3(s.qd, t, qd);
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
    double2 v = a2[0]; quat[0] = v.x; quat[1] = v.y;
    v = a2[1]; quat[2] = v.x; quat[3] = v.y;
  }
  load3(s.linvel, i, linvel); load3(s.angvel, i, angvel); load3(s.pos, i, pos);
  const uint32_t sw = s.stance ? *reinterpret_cast<const uint32_t *>(s.stance + 4 * i) : 0u;
  const uint32_t rw = s.report ? *reinterpret_cast<const uint32_t *>(s.report + 4 * i) : 0u;
  double pl[4] = {0.0, 0.0, 1.0, 0.0};
  if (s.plane) {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.plane + 4 * i);
    double2 v = a2[0]; pl[0] = v.x; pl[1] = v.y;
    v = a2[1]; pl[2] = v.x; pl[3] = v.y;
  }
  tab[threadIdx.x] = tab0;
  if ((int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg) tab[threadIdx.x + kUpdateBlock] = tab1;
  __syncthreads();

  double Rm[9], p[3], u[3], n[3], gap;
  quat_to_matrix(quat, Rm);
  cu_foot_world(LdsTab{tab + kTabPerLeg * leg}, q, qd, Rm, pos, linvel, angvel, p, u);
  bool good = cu_finite3(q) && cu_finite3(qd) && cu_finite3(linvel) && cu_finite3(angvel) && cu_finite3(pos) && cu_finite3(p) &&
              cu_finite3(u) && cu_finite(quat[0]) && cu_finite(quat[1]) && cu_finite(quat[2]) && cu_finite(quat[3]);
  if (s.heights) { // (the same on every lane: a kernel argument)
    int ci, cj;
    double alpha, beta;
    cu_cell(p[0], G.ox, G.inv_res, G.nx, ci, alpha);
    cu_cell(p[1], G.oy, G.inv_res, G.ny, cj, beta);
    const double *h = s.heights + ((int64_t)cj * G.nx + ci); // cell (ci, cj) and its three neighbours: inside [ny][nx]
    const double h00 = h[0], h10 = h[1], h01 = h[G.nx], h11 = h[G.nx + 1];
    cu_patch(h00, h10, h01, h11, alpha, beta, G.inv_res, p[2], n, gap);
    good = good && cu_finite(h00) && cu_finite(h10) && cu_finite(h01) && cu_finite(h11);
  } else {
    good = cu_plane(pl, p, n, gap) && good && cu_finite(pl[0]) && cu_finite(pl[1]) && cu_finite(pl[2]) && cu_finite(pl[3]);
  }
  good = good && cu_finite(gap) && cu_finite3(n);
  const bool ok = quad_or(good ? 0u : 1u) == 0u;

  bool next, sensor;
  unsigned events;
  const bool cur = ((sw >> (8 * leg)) & 0xFFu) != 0u;
  const unsigned report = (rw >> (8 * leg)) & 0xFFu; // (0 without a report: no leg is re-anchored then)
  cu_flags(rule, cur, report, gap, dot3(n, u), next, events, sensor);
  // the anchor rule: a foot that stays held keeps its anchor unless the report says it slid
  const bool moved = next && cur && (report & reanchor) != 0u;
  const bool kept = next && cur && !moved;
  events |= moved ? kEventReanchored : 0u;
  const uint32_t next_w = quad_or((next ? 1u : 0u) << (8 * leg)), sensor_w = quad_or((sensor ? 1u : 0u) << (8 * leg)),
                 events_w = quad_or(events << (8 * leg));

  // ---- outputs.  A failed robot: its current flags and zeros, or (QLAMD_ON_FAILURE_KEEP) nothing but its status; its anchors
  // stay as they are either way
  if (!live) return;
  if (leg == 0) o.status[i] = ok ? kStatusOk : kStatusNotPd;
  if (!ok && P.keep_on_failure) return;
  if (leg == 0) {
    if (o.next) *reinterpret_cast<uint32_t *>(o.next + 4 * i) = ok ? next_w : sw;
    if (o.sensor) *reinterpret_cast<uint32_t *>(o.sensor + 4 * i) = ok ? sensor_w : 0u;
    if (o.events) *reinterpret_cast<uint32_t *>(o.events + 4 * i) = ok ? events_w : 0u;
  }
  if (o.gap) o.gap[t] = ok ? gap : 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (o.normal) o.normal[3 * t + a] = ok ? n[a] : 0.0;
    if (o.fpos) o.fpos[3 * t + a] = ok ? p[a] : 0.0;
    if (o.fvel) o.fvel[3 * t + a] = ok ? u[a] : 0.0;
  }
  if (ok && !kept) {
    // a foot held from now on: its projection on the terrain's tangent plane; a free foot: where it is
#pragma unroll
    for (int a = 0; a < 3; a++) o.anchor[3 * t + a] = next ? p[a] - gap * n[a] : p[a];
  }
}

// ------------------------------------------------------------------------------------------------------------ the plant steps

// (no __restrict__ anywhere: the next state may be written over the state it was computed from)
struct AnchorPlantIn {
  const double *q, *qd, *quat, *linvel, *angvel;
  const uint8_t *stance;           // or NULL: free flight
  const uint8_t *prev;             // or NULL: no touchdown
  const double *normals;           // or NULL: the base's z axis
  const double *tau, *gext, *pos;  // gext: or NULL
  const double *anchor;
};
struct AnchorPlantOut {
  double *acc, *force;                           // or NULL
  double *nu_plus, *impulse;                     // or NULL
  uint8_t *report;                               // or NULL
  double *q, *qd, *pos, *quat, *linvel, *angvel; // all NULL: no state update
  int32_t *status;
  int32_t *iterations;                           // or NULL: [B][2] (the friction form)
  double *perr;                                  // or NULL
};

constexpr int kAnchorFrictionLdsDoubles = 4 * kTabPerLeg + 4 * coop::kCoopLdsDoubles + coop::kForceQpNrmRows * 64;

// TWIN OF plant_contact_kernel (plant_contact_kernel.hip; kFriction false) AND OF plant_friction_kernel (plant_friction_kernel.hip;
// kFriction true): the load prologue, the kinematics and factors, the impact, the dynamics at nu+, the output and state-update
// tail repeat those files' in their order (those units keep their text, so nothing is shared through them).  A fix to one belongs
// in the others.  What is added: the anchor of my leg among the prologue's loads, the clamped error of my row next to the
// factors -- one live register until r is formed -- its term in r, its finiteness in the status, and position_error.
// One robot per 16-lane row, lane 4 * leg + c.  Everything is loaded before the first use and stored after the last.
template <bool kFriction>
__device__ __forceinline__ void anchored_plant_body(double *lds, const DeviceParams *Pp, const coop::WbParamsDev &W, const AnchorPlantIn &s,
                                                    int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                    const AnchorPlantOut &o) {
  using namespace coop;
  double *tab = lds;
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

  // ---- outputs.  A failed robot: zeros, nu and its state as they came, or (QLAMD_ON_FAILURE_KEEP) nothing but its status
  if (lr == 0 && live) o.status[i] = st;
  if (!live || (!ok && P.keep_on_failure)) return;
  if constexpr (kFriction) {
    if (o.iterations && lr < 2) o.iterations[2 * i + lr] = lr == 0 ? it_p : it_f;
  }
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

__global__ __launch_bounds__(64) void anchored_plant_contact_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const AnchorPlantIn s,
                                                                    int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                                    const AnchorPlantOut o) {
  __shared__ double lds[4 * kTabPerLeg];
  anchored_plant_body<false>(lds, Pp, W, s, B, dt, kv, mu, kp, emax, o);
}

// More than 256 registers: one wavefront per SIMD, as its twin.
__global__ __launch_bounds__(64) void anchored_plant_friction_kernel(const DeviceParams *Pp, const coop::WbParamsDev W, const AnchorPlantIn s,
                                                                     int64_t B, double dt, double kv, double mu, double kp, double emax,
                                                                     const AnchorPlantOut o) {
  __shared__ double lds[kAnchorFrictionLdsDoubles];
  anchored_plant_body<true>(lds, Pp, W, s, B, dt, kv, mu, kp, emax, o);
}

} // namespace

extern "C" {

int qlamd_wholebody_contact_update_anchored_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *base_position,
                                                  const qlamd_contact_update *update, const qlamd_contact_anchors *anchors,
                                                  int64_t batch, int32_t *status, int memory, void *stream) {
  if (!anchors) return qlamd_wholebody_contact_update_batch(ctx, in, base_position, update, batch, status, memory, stream);
  // (the checks and the staging of that entry, which keeps its text)
  if (!ctx || !in || !base_position || !update || !status || batch < 0 || !anchors->anchor) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  const qlamd_heightfield *hf = update->heightfield;
  if (update->plane && hf) return QLAMD_ERR_INVALID_ARGUMENT;
  if (hf && (hf->nx < 2 || hf->ny < 2 || !(hf->resolution > 0.0) || !cu_finite(hf->resolution) || !hf->heights))
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (!cu_finite(update->touchdown_distance) || !cu_finite(update->approach_speed) || !cu_finite(update->liftoff_distance) ||
      !cu_finite(update->sensor_distance) || update->liftoff_distance < update->touchdown_distance)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  AnchorUpdateIn s{in->joint_position, in->joint_velocity, in->base_orientation, in->base_linear_velocity, in->base_angular_velocity,
                   base_position, in->support_leg, update->contact_report, update->plane, hf ? hf->heights : nullptr};
  AnchorUpdateGrid G{0.0, 0.0, 1.0, 2, 2};
  if (hf) G = AnchorUpdateGrid{hf->origin_x, hf->origin_y, 1.0 / hf->resolution, hf->nx, hf->ny};
  const ContactRule rule{update->touchdown_distance, update->approach_speed, update->liftoff_distance, update->sensor_distance,
                         update->release_mask};
  AnchorUpdateOut o{update->support_next, update->contact_sensor, update->events, update->gap, update->surface_normal,
                    update->foot_position, update->foot_velocity, status, anchors->anchor};
  const bool keep = ctx->params.keep_on_failure != 0; // entries the kernel leaves alone come back as they went up
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.pos, B * 24); sg.in(s.stance, B * 4); sg.in(s.report, B * 4); sg.in(s.plane, B * 32);
  sg.in(s.heights, hf ? (size_t)hf->nx * (size_t)hf->ny * 8 : 0);
  sg.out(o.next, B * 4, keep); sg.out(o.sensor, B * 4, keep); sg.out(o.events, B * 4, keep); sg.out(o.gap, B * 32, keep);
  sg.out(o.normal, B * 96, keep); sg.out(o.fpos, B * 96, keep); sg.out(o.fvel, B * 96, keep); sg.out(o.status, B * 4);
  sg.inout(o.anchor, B * 96); // (kept anchors come back as they went up)
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((4 * batch + kUpdateBlock - 1) / kUpdateBlock);
  hipLaunchKernelGGL(anchored_contact_update_kernel, dim3(grid), dim3(kUpdateBlock), 0, st, ctx->d_params, s, G, rule,
                     (unsigned)anchors->reanchor_mask, batch, o);
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
  // (the checks and the staging of the two entries underneath, which keep their text)
  if (!ctx || !in || batch < 0 || !joint_effort || !status || !contacts || !base_position || !anchor->anchor)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (next) {
    if (!(dt > 0.0) || !(dt - dt == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
    if (!next->joint_position || !next->joint_velocity || !next->base_position || !next->base_orientation ||
        !next->base_linear_velocity || !next->base_angular_velocity)
      return QLAMD_ERR_INVALID_ARGUMENT;
  }
  const double kv = contacts->velocity_gain, mu = contacts->friction_coefficient;
  const double kp = anchor->position_gain, emax = anchor->max_error;
  if (!(kv >= 0.0) || !(kv - kv == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (friction) {
    if (!(mu > 0.0) || !(mu - mu == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT; // (read with or without a report: it is the constraint)
  } else if (contacts->contact_report && (!(mu >= 0.0) || !(mu - mu == 0.0))) {
    return QLAMD_ERR_INVALID_ARGUMENT;
  }
  if (!(kp >= 0.0) || !(kp - kp == 0.0) || !(emax > 0.0)) return QLAMD_ERR_INVALID_ARGUMENT; // (emax = +infinity: no clamp)
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  const size_t B = (size_t)batch;
  AnchorPlantIn s{in->joint_position, in->joint_velocity, in->base_orientation, in->base_linear_velocity, in->base_angular_velocity,
                  in->support_leg, contacts->previous_support_leg, in->surface_normal, joint_effort, generalized_force,
                  base_position, anchor->anchor};
  AnchorPlantOut o{};
  o.acc = acceleration; o.force = contact_force; o.status = status;
  o.iterations = friction ? friction->iterations : nullptr;
  o.perr = anchor->position_error;
  o.nu_plus = contacts->post_impact_velocity; o.impulse = contacts->impulse; o.report = contacts->contact_report;
  if (next) {
    o.q = next->joint_position; o.qd = next->joint_velocity; o.pos = next->base_position; o.quat = next->base_orientation;
    o.linvel = next->base_linear_velocity; o.angvel = next->base_angular_velocity;
  }
  const bool keep = ctx->params.keep_on_failure != 0; // entries the kernel leaves alone come back as they went up
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.stance, B * 4); sg.in(s.prev, B * 4); sg.in(s.normals, B * 96); sg.in(s.tau, B * 96); sg.in(s.gext, B * 144);
  sg.in(s.pos, B * 24); sg.in(s.anchor, B * 96);
  sg.out(o.acc, B * 144, keep); sg.out(o.force, B * 96, keep);
  sg.out(o.nu_plus, B * 144, keep); sg.out(o.impulse, B * 96, keep); sg.out(o.report, B * 4, keep);
  sg.out(o.q, B * 96, keep); sg.out(o.qd, B * 96, keep); sg.out(o.pos, B * 24, keep); sg.out(o.quat, B * 32, keep);
  sg.out(o.linvel, B * 24, keep); sg.out(o.angvel, B * 24, keep); sg.out(o.iterations, B * 8, keep); sg.out(o.perr, B * 96, keep);
  sg.out(o.status, B * 4);
  if (const int rc = sg.upload(ctx, st)) return rc;
  coop::WbParamsDev W;
  W.base_m = ctx->base_m;
  for (int a = 0; a < 3; a++) W.base_h[a] = ctx->base_h[a];
  for (int a = 0; a < 6; a++) W.base_I[a] = ctx->base_I[a];
  W.w_tau = 0.0; W.tau_max = 0.0; W.grav = gravity;
  const dim3 grid((unsigned)((batch + 3) / 4));
  if (friction)
    hipLaunchKernelGGL(anchored_plant_friction_kernel, grid, dim3(64), 0, st, ctx->d_params, W, s, batch, dt, kv, mu, kp, emax, o);
  else
    hipLaunchKernelGGL(anchored_plant_contact_kernel, grid, dim3(64), 0, st, ctx->d_params, W, s, batch, dt, kv, mu, kp, emax, o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

QLAMD_STAMPS_ACCESSOR(qlamd_debug_stamps_contact_anchor)

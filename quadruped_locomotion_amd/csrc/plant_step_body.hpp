// What the five plant kernels (plant_kernel.hip, plant_contact_kernel.hip, plant_friction_kernel.hip, contact_anchor_kernel.hip)
// and their four entries have in common, once: the kernel arguments, the lane layout, the failure rule, the output and
// state-update tail, and what the entries check, fill and stage.  What lies between the lane layout and the failure rule -- the
// loads and the arithmetic of csrc/plant_coop.hpp, csrc/plant_contact_coop.hpp and csrc/plant_friction_coop.hpp -- is each
// kernel's own text.
#pragma once
#include "plant_friction_coop.hpp"
#include "context.hpp"

namespace qlamd {
namespace rt {

// ---- kernel arguments (no __restrict__ anywhere: the next state may be written over the state it was computed from)
struct PlantIn {
  const double *q, *qd, *quat, *linvel, *angvel;
  const uint8_t *stance;           // or NULL: free flight
  const double *tau, *gext, *pos;  // gext, pos: or NULL
};
struct PlantOut {
  double *acc, *force;                           // or NULL
  double *q, *qd, *pos, *quat, *linvel, *angvel; // all NULL: accelerations only
  int32_t *status;
};
struct PlantContactIn {
  const double *q, *qd, *quat, *linvel, *angvel;
  const uint8_t *stance;           // or NULL: free flight
  const uint8_t *prev;             // or NULL: no touchdown
  const double *normals;           // or NULL: the base's z axis
  const double *tau, *gext, *pos;  // gext: or NULL; pos: or NULL without anchors
};
struct AnchoredPlantIn : PlantContactIn {
  const double *anchor;
};
struct PlantContactOut {
  double *acc, *force;                           // or NULL
  double *nu_plus, *impulse;                     // or NULL
  uint8_t *report;                               // or NULL
  double *q, *qd, *pos, *quat, *linvel, *angvel; // all NULL: no state update
  int32_t *status;
};
struct PlantFrictionOut : PlantContactOut {
  int32_t *iterations;                           // or NULL: [B][2]
};
struct AnchoredPlantOut : PlantFrictionOut {
  double *perr;                                  // or NULL
};

constexpr int kFrictionLdsDoubles = 4 * kTabPerLeg + 4 * coop::kCoopLdsDoubles + coop::kForceQpNrmRows * 64;

// ---- the head and the tail of every plant kernel

// One robot per 16-lane row, lane 4 * leg + c; lanes c < 3 hold joint (leg, c) and force component (leg, c).  A row past the
// batch works on the last robot and stores nothing.
struct PlantLane {
  int row, lr, leg, c, jq;
  bool comp, live;
  int64_t i;
};
__device__ __forceinline__ PlantLane plant_lane(int64_t B) {
  PlantLane ln;
  ln.row = threadIdx.x >> 4; ln.lr = threadIdx.x & 15; ln.leg = ln.lr >> 2; ln.c = ln.lr & 3;
  const int64_t i0 = (int64_t)blockIdx.x * 4 + ln.row;
  ln.live = i0 < B;
  ln.i = ln.live ? i0 : B - 1;
  ln.comp = ln.c < 3;
  ln.jq = 3 * ln.leg + (ln.comp ? ln.c : 2);
  return ln;
}

// The failure rule.  A failed robot: zeros and its state as it came, or (QLAMD_ON_FAILURE_KEEP) nothing but its status.  False:
// this lane stores nothing more.
__device__ __forceinline__ bool plant_store_status(int32_t *status, const PlantLane &ln, int st, const DeviceParams &P) {
  if (ln.lr == 0 && ln.live) status[ln.i] = st;
  return ln.live && (st == kStatusOk || !P.keep_on_failure);
}

// The tail: the accelerations accb, accj and the force component f, then semi-implicit Euler from the velocity nu = (v_B, w),
// qd_from (include/qlamd.h has the rule): nu+ = nu + dt nu', q+ = q + dt qd+, quat+ = normalise(quat (x) exp(dt w+)),
// pos+ = pos + dt R(quat) v+, world linear velocity+ = R(quat+) v+.  (qd_from of a lane c = 3 is stored nowhere.)
template <class Out>
__device__ __forceinline__ void plant_store_tail(const Out &o, const PlantLane &ln, const double quat[4], const double linvel[3],
                                                 const double angvel[3], const double pos[3], double qj, double qdj, const double Rm[9],
                                                 bool ok, double dt, const double nu[6], double qd_from, const double accb[6], double accj,
                                                 double f) {
  const int64_t i = ln.i;
  const int lr = ln.lr;
  using coop::sel;
  const int64_t jo = 3 * ln.leg + ln.c; // my joint / my force component (lanes c < 3)
  if (o.acc) {
    if (ln.comp) o.acc[18 * i + 6 + jo] = ok ? accj : 0.0;
    if (lr < 6) {
      double v = accb[0];
#pragma unroll
      for (int b = 1; b < 6; b++) v = sel(lr == b, accb[b], v);
      o.acc[18 * i + lr] = ok ? v : 0.0;
    }
  }
  if (o.force && ln.comp) o.force[12 * i + jo] = ok ? f : 0.0;
  if (o.q == nullptr) return;
  double qn[4] = {quat[0], quat[1], quat[2], quat[3]}, pn[3] = {pos[0], pos[1], pos[2]};
  double lvn[3] = {linvel[0], linvel[1], linvel[2]}, wn[3] = {angvel[0], angvel[1], angvel[2]};
  double qdn = qdj, qjn = qj;
  if (ok) {
    qdn = qd_from + dt * accj;
    qjn = qj + dt * qdn;
    double vn[3], phi[3], dv[3], Rn[9];
#pragma unroll
    for (int a = 0; a < 3; a++) { vn[a] = nu[a] + dt * accb[a]; wn[a] = nu[3 + a] + dt * accb[3 + a]; phi[a] = dt * wn[a]; }
    coop::plant_quat_step(quat, phi, qn);
    rot(Rm, vn, dv);
#pragma unroll
    for (int a = 0; a < 3; a++) pn[a] = pos[a] + dt * dv[a];
    quat_to_matrix(qn, Rn);
    rot(Rn, vn, lvn);
  }
  if (ln.comp) { o.q[12 * i + jo] = qjn; o.qd[12 * i + jo] = qdn; }
  if (lr < 4) {
    double v = qn[0];
#pragma unroll
    for (int b = 1; b < 4; b++) v = sel(lr == b, qn[b], v);
    o.quat[4 * i + lr] = v;
  }
  if (lr < 3) {
    o.pos[3 * i + lr] = sel(lr == 2, pn[2], sel(lr == 1, pn[1], pn[0]));
    o.linvel[3 * i + lr] = sel(lr == 2, lvn[2], sel(lr == 1, lvn[1], lvn[0]));
    o.angvel[3 * i + lr] = sel(lr == 2, wn[2], sel(lr == 1, wn[1], wn[0]));
  }
}

// ---- the host side of the four plant entries

// What every plant entry refuses.  base_position is needed with `next`; pos_always: and without it (the anchored step).
inline int plant_check(const qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *joint_effort, const double *base_position,
                       bool pos_always, double dt, int64_t batch, const qlamd_plant_next *next, const int32_t *status, int memory) {
  if (!ctx || !in || batch < 0 || !joint_effort || !status || (pos_always && !base_position)) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (next) {
    if (!base_position || !(dt > 0.0) || !(dt - dt == 0.0)) return QLAMD_ERR_INVALID_ARGUMENT;
    if (!next->joint_position || !next->joint_velocity || !next->base_position || !next->base_orientation ||
        !next->base_linear_velocity || !next->base_angular_velocity)
      return QLAMD_ERR_INVALID_ARGUMENT;
  }
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  return QLAMD_OK;
}

// The kernel arguments of one call, in their widest form: an entry fills what it has, leaves the rest NULL and hands its kernel
// the part that kernel takes.  pos: the base position if the kernel is to load it; next, contacts: or NULL.
struct PlantCall {
  AnchoredPlantIn s;
  AnchoredPlantOut o;
};
inline PlantCall plant_call(const qlamd_wholebody_batch *in, const double *joint_effort, const double *generalized_force, const double *pos,
                            double *acceleration, double *contact_force, const qlamd_plant_next *next,
                            const qlamd_plant_contacts *contacts, int32_t *status) {
  PlantCall k{};
  k.s.q = in->joint_position; k.s.qd = in->joint_velocity; k.s.quat = in->base_orientation; k.s.linvel = in->base_linear_velocity;
  k.s.angvel = in->base_angular_velocity; k.s.stance = in->support_leg; k.s.tau = joint_effort; k.s.gext = generalized_force;
  k.s.pos = pos;
  k.o.acc = acceleration; k.o.force = contact_force; k.o.status = status;
  if (contacts) {
    k.s.prev = contacts->previous_support_leg; k.s.normals = in->surface_normal;
    k.o.nu_plus = contacts->post_impact_velocity; k.o.impulse = contacts->impulse; k.o.report = contacts->contact_report;
  }
  if (next) {
    k.o.q = next->joint_position; k.o.qd = next->joint_velocity; k.o.pos = next->base_position; k.o.quat = next->base_orientation;
    k.o.linvel = next->base_linear_velocity; k.o.angvel = next->base_angular_velocity;
  }
  return k;
}

// Binds every array of the call (a NULL one stages nothing, but takes one of Staged's slots: an array added to the list below
// is counted here).  keep: entries the kernel leaves alone come back as they went up.
constexpr int kPlantStagedItems = 12 + 14; // inputs + outputs
static_assert(kPlantStagedItems <= Staged::kMaxItems, "plant_stage binds more arrays than Staged::upload() accepts");
inline void plant_stage(Staged &sg, PlantCall &k, size_t B, bool keep) {
  AnchoredPlantIn &s = k.s;
  AnchoredPlantOut &o = k.o;
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.stance, B * 4); sg.in(s.prev, B * 4); sg.in(s.normals, B * 96); sg.in(s.tau, B * 96); sg.in(s.gext, B * 144);
  sg.in(s.pos, B * 24); sg.in(s.anchor, B * 96);
  sg.out(o.acc, B * 144, keep); sg.out(o.force, B * 96, keep);
  sg.out(o.nu_plus, B * 144, keep); sg.out(o.impulse, B * 96, keep); sg.out(o.report, B * 4, keep);
  sg.out(o.q, B * 96, keep); sg.out(o.qd, B * 96, keep); sg.out(o.pos, B * 24, keep); sg.out(o.quat, B * 32, keep);
  sg.out(o.linvel, B * 24, keep); sg.out(o.angvel, B * 24, keep); sg.out(o.iterations, B * 8, keep); sg.out(o.perr, B * 96, keep);
  sg.out(o.status, B * 4);
}

inline coop::WbParamsDev plant_params(const qlamd_context *ctx, double gravity) {
  coop::WbParamsDev W;
  W.base_m = ctx->base_m;
  for (int a = 0; a < 3; a++) W.base_h[a] = ctx->base_h[a];
  for (int a = 0; a < 6; a++) W.base_I[a] = ctx->base_I[a];
  W.w_tau = 0.0; W.tau_max = 0.0; W.grav = gravity;
  return W;
}

} // namespace rt
} // namespace qlamd

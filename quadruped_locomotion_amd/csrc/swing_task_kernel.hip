// HIP kernel (gfx950) of the swing-foot task -- schedule and footholds in, desired joint accelerations and the solve's support
// flags out, one swing record per leg kept in device memory -- and its entries of the C-ABI (include/qlamd_swing_task.h, which
// qlamd.h brings in).  The arithmetic is csrc/swing_task_core.hpp's; the launch shape, the table staging and the quad-wide vote
// are the contact update's (csrc/contact_update_body.hpp).
#include <cmath>

#include "contact_update_body.hpp"
#include "swing_task_core.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// (no __restrict__ anywhere: support may be the array the detected flags are read from)
struct SwingIn {
  const double *q, *qd, *quat, *linvel, *angvel, *pos;
  const double *ades;      // or NULL: 0
  const uint8_t *stance;   // or NULL: no foot is flagged
  const uint8_t *want;
  const double *foothold;
  const double *normal;    // or NULL: e_z
};
struct SwingOut {
  double *state;           // in/out
  double *qdd;
  uint8_t *support, *events; // each or NULL
  double *ref;             // or NULL
  int32_t *status;
};

// One lane per (robot, leg), 16 robots per wavefront, as the contact update: the four legs of a robot are independent, only the
// status is the robot's (a quad-wide vote).  Everything is loaded before the first store.  Per robot 672 bytes read with every
// input given (the state 296, the flags 4, the desired base acceleration 48, the schedule 4, footholds and normals 96 each, the
// records 128) and up to 524 written.  A failed robot's stores are masked by `ok`, and nothing
// branches around the table's barrier.
__global__ __launch_bounds__(kUpdateBlock) void swing_task_kernel(const DeviceParams *Pp, const SwingIn s, const SwingRule rule,
                                                                  int64_t B, const SwingOut o) {
  __shared__ double tab[4 * kTabPerLeg];
  const DeviceParams &P = *Pp;
  const int second = (int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg ? (int)threadIdx.x + kUpdateBlock : 4 * kTabPerLeg - 1;
  const double tab0 = P.legtab[threadIdx.x], tab1 = P.legtab[second];
  const int64_t t0 = (int64_t)blockIdx.x * kUpdateBlock + threadIdx.x;
  const bool live = t0 < 4 * B; // a quad is live or dead as a whole
  const int64_t t = live ? t0 : 4 * B - 1;
  const int64_t i = t >> 2;
  const int leg = (int)(t & 3);
  double q[3], qd[3], quat[4], linvel[3], angvel[3], pos[3], target[3], st[4];
  double ades[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 1.0};
  load3(s.q, t, q); load3(s.qd, t, qd);
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
    double2 v = a2[0]; quat[0] = v.x; quat[1] = v.y;
    v = a2[1]; quat[2] = v.x; quat[3] = v.y;
  }
  load3(s.linvel, i, linvel); load3(s.angvel, i, angvel); load3(s.pos, i, pos);
  if (s.ades) { load3(s.ades, 2 * i, ades); load3(s.ades, 2 * i + 1, ades + 3); } // (the same on every lane: a kernel argument)
  const uint32_t sw = s.stance ? *reinterpret_cast<const uint32_t *>(s.stance + 4 * i) : 0u;
  const uint32_t ww = *reinterpret_cast<const uint32_t *>(s.want + 4 * i);
  load3(s.foothold, t, target);
  if (s.normal) load3(s.normal, t, n);
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(o.state + 4 * t);
    double2 v = a2[0]; st[0] = v.x; st[1] = v.y;
    v = a2[1]; st[2] = v.x; st[3] = v.y;
  }
  tab[threadIdx.x] = tab0;
  if ((int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg) tab[threadIdx.x + kUpdateBlock] = tab1;
  __syncthreads();

  double Rm[9], qdd[3], ref[9], next[4];
  bool support;
  unsigned events;
  quat_to_matrix(quat, Rm);
  const bool cur = ((sw >> (8 * leg)) & 0xFFu) != 0u, want = ((ww >> (8 * leg)) & 0xFFu) != 0u;
  bool good = swing_task_leg(LdsTab{tab + kTabPerLeg * leg}, rule, q, qd, Rm, pos, linvel, angvel, ades, want, cur, st, target, n, qdd,
                             ref, next, support, events);
  good = good && cu_finite(quat[0]) && cu_finite(quat[1]) && cu_finite(quat[2]) && cu_finite(quat[3]);
  const bool ok = quad_or(good ? 0u : 1u) == 0u;
  const uint32_t support_w = quad_or((support ? 1u : 0u) << (8 * leg)), events_w = quad_or(events << (8 * leg));

  // ---- outputs.  A failed robot: zeros and its detected flags, or (QLAMD_ON_FAILURE_KEEP) nothing but its status; its records
  // stay as they are either way
  if (!live) return;
  if (leg == 0) o.status[i] = ok ? kStatusOk : kStatusNotPd;
  if (!ok && P.keep_on_failure) return;
  if (leg == 0) {
    if (o.support) *reinterpret_cast<uint32_t *>(o.support + 4 * i) = ok ? support_w : sw;
    if (o.events) *reinterpret_cast<uint32_t *>(o.events + 4 * i) = ok ? events_w : 0u;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) o.qdd[3 * t + a] = ok ? qdd[a] : 0.0;
  if (o.ref) {
#pragma unroll
    for (int a = 0; a < 9; a++) o.ref[9 * t + a] = ok ? ref[a] : 0.0;
  }
  if (ok) {
    double2 *a2 = reinterpret_cast<double2 *>(o.state + 4 * t);
    a2[0] = make_double2(next[0], next[1]);
    a2[1] = make_double2(next[2], next[3]);
  }
}

bool in_range(double x, bool positive, bool may_be_infinite) {
  if (x != x) return false;
  if (!may_be_infinite && !cu_finite(x)) return false;
  return positive ? x > 0.0 : x >= 0.0;
}

} // namespace

extern "C" {

void qlamd_swing_task_default(qlamd_swing_task *t) {
  if (!t) return;
  memset(t, 0, sizeof(*t)); // (the padding too)
  t->swing_leg = nullptr; t->foothold = nullptr; t->surface_normal = nullptr;
  t->swing_duration = 0.45; t->profile_height = 0.08; t->touchdown_speed = 0.0; t->touchdown_phase = 0.0;
  t->position_gain = 0.0; t->velocity_gain = 0.0; t->max_error = INFINITY; t->damping = 0.0; t->max_joint_acceleration = INFINITY;
  t->dt = 0.0;
  t->swing_state = nullptr; t->desired_joint_acceleration = nullptr; t->support_solve = nullptr; t->foot_reference = nullptr;
  t->swing_events = nullptr;
}

int qlamd_wholebody_swing_task_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *base_position,
                                     const qlamd_swing_task *task, int64_t batch, int32_t *status, int memory, void *stream) {
  if (!ctx || !in || !base_position || !task || !status || batch < 0) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (!task->swing_leg || !task->foothold || !task->swing_state || !task->desired_joint_acceleration) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in_range(task->swing_duration, true, false) || !in_range(task->profile_height, false, false) ||
      !in_range(task->touchdown_speed, false, false) || !in_range(task->touchdown_phase, false, false) || task->touchdown_phase > 1.0 ||
      !in_range(task->position_gain, false, false) || !in_range(task->velocity_gain, false, false) ||
      !in_range(task->max_error, true, true) || !in_range(task->damping, false, false) ||
      !in_range(task->max_joint_acceleration, true, true) || !in_range(task->dt, true, false))
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  SwingIn s{in->joint_position, in->joint_velocity, in->base_orientation, in->base_linear_velocity, in->base_angular_velocity,
            base_position, in->desired_base_acceleration, in->support_leg, task->swing_leg, task->foothold, task->surface_normal};
  SwingOut o{task->swing_state, task->desired_joint_acceleration, task->support_solve, task->swing_events, task->foot_reference, status};
  const SwingRule rule = swing_rule(task->swing_duration, task->profile_height, task->touchdown_speed, task->touchdown_phase,
                                    task->position_gain, task->velocity_gain, task->max_error, task->damping,
                                    task->max_joint_acceleration, task->dt);
  const size_t B = (size_t)batch;
  const bool keep = ctx->params.keep_on_failure != 0;
  Staged sg(memory == QLAMD_MEM_HOST);
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.pos, B * 24); sg.in(s.ades, B * 48); sg.in(s.stance, B * 4); sg.in(s.want, B * 4); sg.in(s.foothold, B * 96);
  sg.in(s.normal, B * 96);
  sg.inout(o.state, B * 128); // a failed robot's records come back as they went up
  sg.out(o.qdd, B * 96, keep); sg.out(o.support, B * 4, keep); sg.out(o.events, B * 4, keep); sg.out(o.ref, B * 288, keep);
  sg.out(o.status, B * 4);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((4 * batch + kUpdateBlock - 1) / kUpdateBlock);
  hipLaunchKernelGGL(swing_task_kernel, dim3(grid), dim3(kUpdateBlock), 0, st, ctx->d_params, s, rule, batch, o);
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"

// The swing-foot task from C++, beside contact_detection.hpp: before the whole-body step of a tick, swing_task() turns the
// tick's swing schedule and footholds into the desired joint accelerations and the support flags that step runs with
// (qlamd_wholebody_swing_task_batch of qlamd_swing_task.h, which qlamd.h brings in), and keeps the swing records.  Needs qlamd.h only.
#pragma once

#include "qlamd/contact_detection.hpp"

#ifndef QLAMD_HAS_SWING_TASK
#error "this qlamd.h has no qlamd_wholebody_swing_task_batch"
#endif

namespace qlamd {
namespace host {

// The parameters of the task with the library's defaults, and what the task keeps and gives for a batch, owned: the swing
// records (zeros: no leg is in a swing), the desired joint accelerations and the flags for the solve.  Set `task.dt`, the gains
// and whatever else differs from the defaults before the first call; the pointers of `task` are set by swing_task().
struct SwingTask {
  explicit SwingTask(int64_t batch)
      : swing_state((size_t)batch * 16), desired_joint_acceleration((size_t)batch * 12), support_solve((size_t)batch * 4) {
    qlamd_swing_task_default(&task);
  }
  qlamd_swing_task task;
  std::vector<double> swing_state;                // [B][4][4] start x y z, clock
  std::vector<double> desired_joint_acceleration; // [B][12]
  std::vector<uint8_t> support_solve;             // [B][4]
};

// One tick of the task on the state `s` (s.support_leg: the detected flags): swing_leg [B][4] the schedule, foothold [B][4][3],
// desired_base_acceleration [B][6] or NULL, surface_normal [B][4][3] or NULL.  After a call that returns QLAMD_OK,
// k.desired_joint_acceleration and k.support_solve are what in->desired_joint_acceleration and in->support_leg of
// qlamd_wholebody_solve_batch take; the plant keeps s.support_leg.  swing_events [B][4] and foot_reference [B][4][9] or NULL.
inline int swing_task(qlamd_context *ctx, const PlantState &s, SwingTask &k, const uint8_t *swing_leg, const double *foothold,
                      int32_t *status, const double *desired_base_acceleration = nullptr, const double *surface_normal = nullptr,
                      uint8_t *swing_events = nullptr, double *foot_reference = nullptr) {
  qlamd_wholebody_batch in = s.batch();
  in.desired_base_acceleration = desired_base_acceleration;
  qlamd_swing_task t = k.task;
  t.swing_leg = swing_leg;
  t.foothold = foothold;
  t.surface_normal = surface_normal;
  t.swing_state = k.swing_state.data();
  t.desired_joint_acceleration = k.desired_joint_acceleration.data();
  t.support_solve = k.support_solve.data();
  t.swing_events = swing_events;
  t.foot_reference = foot_reference;
  return qlamd_wholebody_swing_task_batch(ctx, &in, s.base_position.data(), &t, s.size(), status, QLAMD_MEM_HOST, nullptr);
}

} // namespace host
} // namespace qlamd

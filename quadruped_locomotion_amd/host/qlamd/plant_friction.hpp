// The plant step with friction from C++, beside plant.hpp: step_with_friction() is step_with_contacts() with the contact
// impulses and forces inside the friction pyramid (qlamd_wholebody_plant_step_friction_batch of qlamd_plant_friction.h, which
// qlamd.h includes), so a foot lifts or slides without a flag change.  Needs qlamd.h only.
#pragma once

#include "qlamd/plant.hpp"

#ifndef QLAMD_HAS_PLANT_FRICTION
#error "this qlamd.h has no qlamd_wholebody_plant_step_friction_batch"
#endif

namespace qlamd {
namespace host {

// One step of `dt` in place: step_with_contacts()'s arguments, with `friction` = mu > 0 the constraint.  contact_report [B][4]:
// QLAMD_CONTACT_TOUCHDOWN | _SEPARATING | _SLIDING per leg, what detect_contacts() takes with release_mask =
// QLAMD_CONTACT_SEPARATING; iterations [B][2]: outer iterations of the impulse QP and of the force QP.  Either may be NULL.
// After a call that returns QLAMD_OK the state remembers this step's flags.
inline int step_with_friction(qlamd_context *ctx, PlantState &s, const double *joint_effort, double gravity, double dt, double k_v,
                              double friction, int32_t *status, double *contact_force = nullptr, uint8_t *contact_report = nullptr,
                              int32_t *iterations = nullptr, const double *generalized_force = nullptr) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_plant_next next = s.next();
  const qlamd_plant_contacts contacts = plant_contacts(s, k_v, friction, contact_report);
  qlamd_plant_friction fr{};
  fr.iterations = iterations;
  const int rc = qlamd_wholebody_plant_step_friction_batch(ctx, &in, joint_effort, generalized_force, s.base_position.data(), gravity,
                                                           dt, s.size(), nullptr, contact_force, &next, &contacts, &fr, status,
                                                           QLAMD_MEM_HOST, nullptr);
  if (rc == QLAMD_OK) s.previous_support_leg = s.support_leg;
  return rc;
}

} // namespace host
} // namespace qlamd

// Contact anchors from C++, beside plant_friction.hpp and contact_detection.hpp: detect_contacts_anchored() is detect_contacts()
// that also keeps where each flagged foot is held, and step_anchored() is step_with_contacts() / step_with_friction() that holds
// it there (qlamd_wholebody_contact_update_anchored_batch and qlamd_wholebody_plant_step_anchored_batch of
// qlamd_contact_anchor.h, which qlamd.h brings in).  Needs qlamd.h only.
#pragma once

#include <limits>

#include "qlamd/contact_detection.hpp"
#include "qlamd/plant_friction.hpp"

#ifndef QLAMD_HAS_CONTACT_ANCHORS
#error "this qlamd.h has no qlamd_wholebody_plant_step_anchored_batch"
#endif

namespace qlamd {
namespace host {

// The anchors of a batch, [B][4][3] in the world, with the gain and the clamp the plant step holds them with.  The first anchors
// come from init_anchors(): every foot where it is, on or under the terrain as well.
struct ContactAnchors {
  explicit ContactAnchors(int64_t batch) : anchor((size_t)batch * 12, 0.0) {}
  std::vector<double> anchor;
  double position_gain = 0.0;                                  // k_p, 1/s^2
  double max_error = std::numeric_limits<double>::infinity();  // e_max, metres
  uint8_t reanchor_mask = 0;                                   // report bits that move a held foot's anchor
};

// detect_contacts() with the anchors kept: a foot that touches down is anchored at its projection on the terrain, a foot that
// stays held keeps its anchor (unless its report has a bit of a.reanchor_mask), a free foot's anchor follows the foot.
inline int detect_contacts_anchored(qlamd_context *ctx, PlantState &s, const ContactDetector &d, ContactAnchors &a,
                                    const uint8_t *contact_report, int32_t *status) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_contact_update u = contact_update(s, d, contact_report);
  qlamd_contact_anchors ca{};
  ca.anchor = a.anchor.data();
  ca.reanchor_mask = a.reanchor_mask;
  return qlamd_wholebody_contact_update_anchored_batch(ctx, &in, s.base_position.data(), &u, &ca, s.size(), status, QLAMD_MEM_HOST,
                                                       nullptr);
}

// The first anchors of a loop: every foot where it is, no flag read or written.  An update without flags treats every foot as
// unflagged, and one that its rule takes would be a touchdown, anchored at its projection on the terrain; so this call runs with
// a rule that takes no foot (no approach speed is low enough), which leaves anchor = p on every leg whatever the terrain.
inline int init_anchors(qlamd_context *ctx, const PlantState &s, const ContactDetector &d, ContactAnchors &a, int32_t *status) {
  qlamd_wholebody_batch in = s.batch();
  in.support_leg = nullptr;
  qlamd_contact_update u = d.update;
  u.contact_report = nullptr;
  u.approach_speed = std::numeric_limits<double>::lowest();
  u.support_next = nullptr; u.contact_sensor = nullptr; u.events = nullptr; u.gap = nullptr;
  u.surface_normal = nullptr; u.foot_position = nullptr; u.foot_velocity = nullptr;
  qlamd_contact_anchors ca{};
  ca.anchor = a.anchor.data();
  return qlamd_wholebody_contact_update_anchored_batch(ctx, &in, s.base_position.data(), &u, &ca, s.size(), status, QLAMD_MEM_HOST,
                                                       nullptr);
}

// One step of `dt` in place with the held feet pulled to their anchors: step_with_friction()'s arguments; friction > 0 with
// `cone` the constraint, else hard contacts (friction is then read for the report only).  position_error [B][4][3] or NULL.
// After a call that returns QLAMD_OK the state remembers this step's flags.
inline int step_anchored(qlamd_context *ctx, PlantState &s, const ContactAnchors &a, const double *joint_effort, double gravity,
                         double dt, double k_v, double friction, bool cone, int32_t *status, double *contact_force = nullptr,
                         uint8_t *contact_report = nullptr, double *position_error = nullptr, int32_t *iterations = nullptr,
                         const double *generalized_force = nullptr) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_plant_next next = s.next();
  const qlamd_plant_contacts contacts = plant_contacts(s, k_v, friction, contact_report);
  qlamd_plant_friction fr{};
  fr.iterations = iterations;
  qlamd_plant_anchor pa{};
  pa.anchor = a.anchor.data();
  pa.position_gain = a.position_gain;
  pa.max_error = a.max_error;
  pa.position_error = position_error;
  const int rc = qlamd_wholebody_plant_step_anchored_batch(ctx, &in, joint_effort, generalized_force, s.base_position.data(), gravity,
                                                           dt, s.size(), nullptr, contact_force, &next, &contacts, cone ? &fr : nullptr,
                                                           &pa, status, QLAMD_MEM_HOST, nullptr);
  if (rc == QLAMD_OK) s.previous_support_leg = s.support_leg;
  return rc;
}

} // namespace host
} // namespace qlamd

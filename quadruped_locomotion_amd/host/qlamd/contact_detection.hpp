// Ground contact detection from C++, beside plant.hpp: after step_with_contacts() has moved a PlantState, detect_contacts()
// decides which feet are on the ground and writes the flags of the next step into it (qlamd_wholebody_contact_update_batch of
// qlamd_contact_detection.h, which qlamd.h includes).  Needs qlamd.h only.
#pragma once

#include "qlamd/plant.hpp"

#ifndef QLAMD_HAS_CONTACT_DETECTION
#error "this qlamd.h has no qlamd_wholebody_contact_update_batch"
#endif

namespace qlamd {
namespace host {

// The thresholds of the flag rule and the terrain: a qlamd_contact_update with the library's defaults (the ground z = 0, every
// distance and the speed 0, a pulling foot is released) and no output.  Set `plane` ([B][4]) or `heightfield`, the thresholds and
// whatever outputs are wanted on `update` before the call.
struct ContactDetector {
  ContactDetector() { qlamd_contact_update_default(&update); }
  qlamd_contact_update update;
};

// d.update for one call on `s`: with that plant step's report (or NULL), the next flags written over the state's own
inline qlamd_contact_update contact_update(PlantState &s, const ContactDetector &d, const uint8_t *contact_report) {
  qlamd_contact_update u = d.update;
  u.contact_report = contact_report;
  u.support_next = s.support_leg.data();
  return u;
}

// The flags of the next step from the state `s` as the plant left it, in place: s.support_leg holds the flags the plant ran with
// when the call is made and the next step's flags after a call that returns QLAMD_OK.  (step_with_contacts() has copied the
// flags it ran with to s.previous_support_leg already, which is what the next step's impact needs.)  contact_report [B][4]: the
// report of that plant step or NULL.  Outputs set on d.update are written as well.
inline int detect_contacts(qlamd_context *ctx, PlantState &s, const ContactDetector &d, const uint8_t *contact_report, int32_t *status) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_contact_update u = contact_update(s, d, contact_report);
  return qlamd_wholebody_contact_update_batch(ctx, &in, s.base_position.data(), &u, s.size(), status, QLAMD_MEM_HOST, nullptr);
}

} // namespace host
} // namespace qlamd

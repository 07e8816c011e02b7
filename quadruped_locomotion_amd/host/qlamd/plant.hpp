// The plant step from C++: the state of a batch of robots on the host and qlamd_wholebody_forward_dynamics_batch on it, in
// place -- what a simulation loop calls after the controller (balance_controller/WholeBodyController.hpp gives the efforts of
// one robot, qlamd_wholebody_solve_batch those of a batch).  The contacts are hard constraints on the flagged feet: no contact
// detection, no friction limit, no drift stabilisation (include/qlamd.h) -- for forward_dynamics() and step().  With a
// qlamd.h that has qlamd_wholebody_plant_step_batch (QLAMD_HAS_PLANT_CONTACTS), step_with_contacts() is the step for a closed loop: a plastic impact at
// every touchdown, a velocity term that keeps held feet at rest, and a report of pulling and sliding feet; which feet
// to flag for the next step is detect_contacts()'s to say (qlamd/contact_detection.hpp).  Needs qlamd.h only.
#pragma once

#include <cstdint>
#include <vector>

#include "qlamd.h"

#ifndef QLAMD_HAS_PLANT_STEP
#error "this qlamd.h has no qlamd_wholebody_forward_dynamics_batch"
#endif

namespace qlamd {
namespace host {

// The arrays of qlamd_wholebody_batch that describe a state, with the base position, owned
struct PlantState {
  explicit PlantState(int64_t batch)
      : joint_position((size_t)batch * 12), joint_velocity((size_t)batch * 12), base_position((size_t)batch * 3),
        base_orientation((size_t)batch * 4), base_linear_velocity((size_t)batch * 3), base_angular_velocity((size_t)batch * 3),
        support_leg((size_t)batch * 4) {
    for (int64_t i = 0; i < batch; i++) base_orientation[(size_t)i * 4] = 1.0;
#ifdef QLAMD_HAS_PLANT_CONTACTS
    previous_support_leg.assign((size_t)batch * 4, 0);
#endif
  }
  int64_t size() const { return (int64_t)(joint_position.size() / 12); }
  // the state as the input of any whole-body entry (desired_* and surface_normal stay NULL: the plant step ignores them)
  qlamd_wholebody_batch batch() const {
    qlamd_wholebody_batch in{};
    in.joint_position = joint_position.data();
    in.joint_velocity = joint_velocity.data();
    in.base_orientation = base_orientation.data();
    in.base_linear_velocity = base_linear_velocity.data();
    in.base_angular_velocity = base_angular_velocity.data();
    in.support_leg = support_leg.data();
    return in;
  }
  // the state as the output of a plant step: the step is taken in place
  qlamd_plant_next next() {
    qlamd_plant_next out;
    out.joint_position = joint_position.data();
    out.joint_velocity = joint_velocity.data();
    out.base_position = base_position.data();
    out.base_orientation = base_orientation.data();
    out.base_linear_velocity = base_linear_velocity.data();
    out.base_angular_velocity = base_angular_velocity.data();
    return out;
  }
  std::vector<double> joint_position, joint_velocity;          // [B][12]
  std::vector<double> base_position;                           // [B][3] world
  std::vector<double> base_orientation;                        // [B][4] (w, x, y, z)
  std::vector<double> base_linear_velocity, base_angular_velocity; // [B][3] world / base
  std::vector<uint8_t> support_leg;                            // [B][4] the feet held by the contact constraints
#ifdef QLAMD_HAS_PLANT_CONTACTS
  std::vector<uint8_t> previous_support_leg;                   // [B][4] support_leg of the step before (step_with_contacts keeps
                                                               // it; zeros at the start: the first step projects every held foot)
#endif
};

// nu' [B][18] and f [B][12] for the efforts joint_effort [B][12] (either output may be NULL); the library's return code
inline int forward_dynamics(qlamd_context *ctx, const PlantState &s, const double *joint_effort, double gravity, double *acceleration,
                            double *contact_force, int32_t *status, const double *generalized_force = nullptr) {
  const qlamd_wholebody_batch in = s.batch();
  return qlamd_wholebody_forward_dynamics_batch(ctx, &in, joint_effort, generalized_force, nullptr, gravity, 0.0, s.size(), acceleration,
                                                contact_force, nullptr, status, QLAMD_MEM_HOST, nullptr);
}

// One semi-implicit Euler step of `dt` in place (include/qlamd.h has the rule); contact_force [B][12] or NULL
inline int step(qlamd_context *ctx, PlantState &s, const double *joint_effort, double gravity, double dt, int32_t *status,
                double *contact_force = nullptr, const double *generalized_force = nullptr) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_plant_next next = s.next();
  return qlamd_wholebody_forward_dynamics_batch(ctx, &in, joint_effort, generalized_force, s.base_position.data(), gravity, dt, s.size(),
                                                nullptr, contact_force, &next, status, QLAMD_MEM_HOST, nullptr);
}

#ifdef QLAMD_HAS_PLANT_CONTACTS
// The contacts struct of every step with contacts: the state's previous flags, k_v, mu and the report (or NULL); no other output
inline qlamd_plant_contacts plant_contacts(const PlantState &s, double k_v, double friction, uint8_t *contact_report) {
  qlamd_plant_contacts contacts{};
  contacts.previous_support_leg = s.previous_support_leg.data();
  contacts.velocity_gain = k_v;
  contacts.friction_coefficient = friction;
  contacts.contact_report = contact_report;
  return contacts;
}

// One step of `dt` in place with contacts (qlamd_wholebody_plant_step_batch): the impact over the held feet of every robot one of
// whose feet is flagged now and was not in the step before, the dynamics at nu+ with the velocity term k_v (1/s; 1/dt brings a held
// foot to rest within the step), the state update from nu+.  contact_force [B][12] and contact_report [B][4] (QLAMD_CONTACT_* bits
// for the friction coefficient `friction`) or NULL.  After a call that returns QLAMD_OK the state remembers this step's flags.
inline int step_with_contacts(qlamd_context *ctx, PlantState &s, const double *joint_effort, double gravity, double dt, double k_v,
                              int32_t *status, double *contact_force = nullptr, uint8_t *contact_report = nullptr,
                              double friction = 0.0, const double *generalized_force = nullptr) {
  const qlamd_wholebody_batch in = s.batch();
  const qlamd_plant_next next = s.next();
  const qlamd_plant_contacts contacts = plant_contacts(s, k_v, friction, contact_report);
  const int rc = qlamd_wholebody_plant_step_batch(ctx, &in, joint_effort, generalized_force, s.base_position.data(), gravity, dt,
                                                  s.size(), nullptr, contact_force, &next, &contacts, status, QLAMD_MEM_HOST, nullptr);
  if (rc == QLAMD_OK) s.previous_support_leg = s.support_leg;
  return rc;
}
#endif

} // namespace host
} // namespace qlamd

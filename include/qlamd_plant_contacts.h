/* qlamd_plant_contacts.h -- the plant step with touchdown impacts, contact stabilisation and a contact report.
 * Part of the C-ABI of qlamd.h in a file of its own: same library, same conventions, plain C.  qlamd.h includes this file at its
 * end, so a caller includes qlamd.h and tests QLAMD_HAS_PLANT_CONTACTS; including this file directly works as well.
 * "The old entry" below is qlamd_wholebody_forward_dynamics_batch of qlamd.h, whose comment has the equations of the plant step,
 * its arguments and the rule of the state update. */
#ifndef QLAMD_PLANT_CONTACTS_H
#define QLAMD_PLANT_CONTACTS_H

#include "qlamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The plant step with touchdown impacts, contact stabilisation and a contact report: what a closed loop calls (the old entry
 * holds the ACCELERATION of a flagged foot at zero and says nothing about its velocity, so a foot flagged while it moves keeps
 * moving).  Arguments, next, statuses, memory spaces, streams, QLAMD_ERR_BUSY and capture as for
 * qlamd_wholebody_forward_dynamics_batch (qlamd.h); with contacts == NULL the call IS that entry (it calls it: the same kernel, bit for
 * bit).  With contacts, per robot, S = the legs flagged in in->support_leg and Js the rows of Jc of those feet:
 *   1. impact.  T = the legs of S that are not flagged in previous_support_leg (NULL: T is empty; an array of zeros: every
 *      flagged leg touches down).  If T is not empty,
 *          M (nu+ - nu) = Js' p,   Js nu+ = 0      over ALL of S
 *      (a plastic impact at one foot changes the velocity of the others, and the hard constraint that follows must start
 *      from feet at rest); otherwise nu+ = nu, bit for bit, and p = 0.
 *   2. dynamics at nu+.   M nu' - Js' f = [0 ; tau] + g_ext - h(q, nu+),   Js nu' = -gamma(q, nu+) - k_v Js nu+
 *      so that in the world each held foot obeys a_foot = -k_v v_foot (Js nu+ = v + w x r + J_leg qd at nu+).
 *   3. state update.  next keeps the old entry's rule, starting from nu+:  nu_next = nu+ + dt nu', and so on.
 *   4. report.  For a flagged leg the QLAMD_CONTACT_* bits, from f and the unit normal n in base coordinates: n = R' n_W with
 *      in->surface_normal given (this entry reads it; the old entry ignores it), the base's z axis with NULL, as in the
 *      control-step state batch.  An unflagged leg reports 0.
 * No contact detection in this entry, no friction limit as a constraint (qlamd_wholebody_plant_step_friction_batch of
 * qlamd_plant_friction.h has it), no position-level drift correction
 * (qlamd_wholebody_plant_step_anchored_batch of qlamd_contact_anchor.h has it): the report gives
 * what it takes to drop a flag -- qlamd_wholebody_contact_update_batch (qlamd_contact_detection.h) reads it and does, on the device.
 * A robot whose status is not QLAMD_STATUS_OK (a pivot not positive or a value not finite, nu+ and p included): nu as it came
 * in post_impact_velocity, zeros in impulse, contact_report, acceleration and contact_force, its state unchanged in next; or
 * (QLAMD_ON_FAILURE_KEEP) all of them untouched.
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: what the old entry refuses; velocity_gain negative or not
 * finite; contact_report given with friction_coefficient negative or not finite. */
#define QLAMD_HAS_PLANT_CONTACTS 1 /* (the feature test: the version number did not move with this entry) */
typedef struct qlamd_plant_contacts {
  const uint8_t *previous_support_leg; /* [B][4] or NULL: the flags of the step before */
  double velocity_gain;                /* k_v >= 0 in 1/s; 0 = none */
  double friction_coefficient;         /* mu >= 0; read only with contact_report */
  double *post_impact_velocity;        /* [B][18] or NULL out: nu+ in the order of nu, base coordinates */
  double *impulse;                     /* [B][12] or NULL out: p by leg, base coordinates, N s; 0 on an unflagged leg */
  uint8_t *contact_report;             /* [B][4]  or NULL out: QLAMD_CONTACT_* bits per leg */
} qlamd_plant_contacts;
#define QLAMD_CONTACT_PULLS 1         /* f . n < 0 */
#define QLAMD_CONTACT_OUTSIDE_CONE 2  /* |f - (f . n) n| > mu max(f . n, 0) */
#define QLAMD_CONTACT_TOUCHDOWN 4     /* flagged now, not in previous_support_leg */

int qlamd_wholebody_plant_step_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *joint_effort /*[B][12]*/, const double *generalized_force /*[B][18] or NULL*/,
        const double *base_position /*[B][3], needed only with next*/, double gravity, double dt,
        int64_t batch, double *acceleration /*[B][18] or NULL*/, double *contact_force /*[B][12] or NULL*/,
        const qlamd_plant_next *next /*or NULL*/, const qlamd_plant_contacts *contacts /*or NULL*/,
        int32_t *status, int memory, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QLAMD_PLANT_CONTACTS_H */

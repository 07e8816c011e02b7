/* qlamd_plant_friction.h -- the plant step with friction: contact impulses and contact forces inside the friction pyramid.
 * Part of the C-ABI of qlamd.h in a file of its own: same library, same conventions, plain C.  qlamd.h includes this file at its
 * end, behind qlamd_plant_contacts.h and qlamd_contact_detection.h, so a caller includes qlamd.h and tests
 * QLAMD_HAS_PLANT_FRICTION; including this file directly works as well.
 * "The hard entry" below is qlamd_wholebody_plant_step_batch of qlamd_plant_contacts.h, whose comment has S, Js, nu, M, h, gamma,
 * k_v, previous_support_leg, T and the state update. */
#ifndef QLAMD_PLANT_FRICTION_H
#define QLAMD_PLANT_FRICTION_H

#include "qlamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The hard entry holds a flagged foot with an equality: its force may pull and may lie anywhere outside the friction cone, and
 * the entry only reports that.  Here the impulse and the force are the minimisers of the plant's own quadratic over the friction
 * pyramid, so a foot whose hold would need a pulling force lifts and one whose hold would need a force outside the cone slides,
 * without a flag change.
 * The pyramid.  Per flagged leg, with mu = contacts->friction_coefficient and n the unit normal in base coordinates as the hard
 * entry's report forms it (n = R' n_W with in->surface_normal given, else the base's z axis):
 *     t1 = normalise(n x y_B) with y_B = R' e_y,   t2 = normalise(n x t1)
 * -- the control step's rule, so the controller's pyramid and the plant's have the same faces -- and K is the set of
 * y in R^(3|S|) with, per leg,   n . y_l >= 0,   mu n . y_l +- t1 . y_l >= 0,   mu n . y_l +- t2 . y_l >= 0.
 * With H0 = Js M^-1 Js':
 *   1. impact, only if T is not empty:   p = argmin_{p in K} 1/2 p'H0 p + p'(Js nu),   nu+ = nu + M^-1 Js' p.
 *      If T is empty, nu+ = nu bit for bit and p = 0 exactly, as in the hard entry.
 *   2. dynamics at nu+:   x0 = M^-1 ([0 ; tau] + g_ext - h(q, nu+)),   r = -gamma(q, nu+) - k_v Js nu+,   c = r - Js x0,
 *          f = argmin_{f in K} 1/2 f'H0 f - f'c,   nu' = x0 + M^-1 Js' f.
 *      This is Gauss' principle restricted to the cone.  When no row of K is active, f and nu' are the hard entry's; otherwise
 *      Js nu' - r = C' lambda with lambda >= 0 over the active rows C.  Both minimisers are unique (H0 is positive definite).
 *   3. state update: the hard entry's rule from nu+, unchanged.
 *   4. report, per flagged leg, from the final working set of the force QP:
 *          QLAMD_CONTACT_TOUCHDOWN   as in the hard entry;
 *          QLAMD_CONTACT_SEPARATING  the row n . f >= 0 holds with equality: the leg's force is at the apex (f_l = 0);
 *          QLAMD_CONTACT_SLIDING     a friction face is active and the leg is not separating;
 *      neither of the last two: the foot sticks.  QLAMD_CONTACT_PULLS and QLAMD_CONTACT_OUTSIDE_CONE are never set by this
 *      entry.  The bits share the report byte of qlamd_plant_contacts, so qlamd_wholebody_contact_update_batch releases a
 *      separating foot with release_mask = QLAMD_CONTACT_SEPARATING.
 * Known property: this is the convex relaxation of the contact problem (the pyramid's faces couple the tangential and the normal
 * direction), so a sliding foot may also gain normal acceleration.
 * Each QP is solved by the dual active-set method of the control step (Goldfarb-Idnani, from the unconstrained minimiser).
 * With friction == NULL the call IS the hard entry (it calls it: bit for bit).  With friction, contacts must be given: it
 * carries the previous flags, k_v, mu and the nu+, impulse and report outputs.
 * status per robot: the QP's own -- QLAMD_STATUS_MAX_ITER at the iteration guard; QLAMD_STATUS_NOT_PD for a pivot not positive or
 * a value not finite (a normal parallel to y_B, which has no tangents, ends there).  QLAMD_STATUS_INFEASIBLE cannot occur: 0 is in
 * K.  A failed robot gets the outputs of the hard entry's failure rule (and iterations as far as they went), or
 * (QLAMD_ON_FAILURE_KEEP) nothing but its status; its neighbours in the wavefront are not disturbed.
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: what the hard entry refuses; contacts == NULL; friction_coefficient
 * not finite or <= 0 (with or without a report: it is the constraint).
 * Memory spaces, streams, QLAMD_ERR_BUSY and capture as for the hard entry; next may alias the state.
 * Position-level drift correction of a held foot is qlamd_wholebody_plant_step_anchored_batch (qlamd_contact_anchor.h, which this
 * file includes at its end).  Not built: a round cone, mu = 0, warm starts of the plant's QPs. */
#define QLAMD_HAS_PLANT_FRICTION 1 /* (the feature test: the version number did not move with this entry) */
#define QLAMD_CONTACT_SEPARATING 8 /* n . f = 0 is active: the force is at the apex of its pyramid */
#define QLAMD_CONTACT_SLIDING 16   /* a friction face is active, and the leg is not separating */
struct qlamd_plant_contacts; /* qlamd_plant_contacts.h's (declared here as well: that header may be the one that brought this one in) */
typedef struct qlamd_plant_friction {
  int32_t *iterations; /* [B][2] or NULL out: outer iterations of the impulse QP and of the force QP */
} qlamd_plant_friction;

int qlamd_wholebody_plant_step_friction_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *joint_effort /*[B][12]*/, const double *generalized_force /*[B][18] or NULL*/,
        const double *base_position /*[B][3], needed only with next*/, double gravity, double dt,
        int64_t batch, double *acceleration /*[B][18] or NULL*/, double *contact_force /*[B][12] or NULL*/,
        const qlamd_plant_next *next /*or NULL*/, const struct qlamd_plant_contacts *contacts,
        const qlamd_plant_friction *friction /*or NULL*/, int32_t *status, int memory, void *stream);

#ifdef __cplusplus
}
#endif

/* contact anchors (QLAMD_HAS_CONTACT_ANCHORS, qlamd_wholebody_plant_step_anchored_batch and
 * qlamd_wholebody_contact_update_anchored_batch): part of this interface, kept in a file of its own that ships beside this one */
#include "qlamd_contact_anchor.h"

#endif /* QLAMD_PLANT_FRICTION_H */

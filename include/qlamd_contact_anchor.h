/* qlamd_contact_anchor.h -- contact anchors for the plant: where each flagged foot is supposed to stand, kept by the contact update
 * and held by the plant step with a position term in its constraint.
 * Part of the C-ABI of qlamd.h in a file of its own: same library, same conventions, plain C.  qlamd.h brings this file in at its
 * end, behind qlamd_plant_friction.h (that header, the last qlamd.h includes, includes this one at its own end), so a caller
 * includes qlamd.h and tests QLAMD_HAS_CONTACT_ANCHORS; including this file directly works as well.
 * "The update" below is qlamd_wholebody_contact_update_batch of qlamd_contact_detection.h, "the friction entry"
 * qlamd_wholebody_plant_step_friction_batch of qlamd_plant_friction.h and "the hard entry" qlamd_wholebody_plant_step_batch of
 * qlamd_plant_contacts.h; their comments have p, n, gap, the flag rule, S, Js, nu+, gamma, k_v, K and the state update.
 *
 * Why: the plant's contact constraint is on acceleration plus a velocity term, Js nu' = -gamma - k_v Js nu+.  The position error
 * that the first-order integrator and a touchdown leave is never taken back: a held foot drifts, and a foot taken at gap <= 0
 * while it still moves stays under the ground.  An anchor per leg says where the foot stands; the plant step adds -k_p e.
 *
 * The closed loop on the device, three launches per tick as before:
 *   the first anchors come from one anchored update with in->support_leg == NULL: no foot is flagged, so a foot the rule takes
 *   (gap <= touchdown_distance, not leaving) is a touchdown and is anchored at its projection p - gap n, every other foot at p.
 *   For anchors at the feet whatever the terrain, make that call with a rule that takes no foot (approach_speed = -DBL_MAX);
 *   tick k solves, the anchored plant step runs with flags_k and the anchors, the anchored update on the state the plant left
 *   gives flags_{k+1} and moves the anchors of the legs whose contact changed. */
#ifndef QLAMD_CONTACT_ANCHOR_H
#define QLAMD_CONTACT_ANCHOR_H

#include "qlamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QLAMD_HAS_CONTACT_ANCHORS 1 /* (the feature test: the version number did not move with these entries) */
/* the siblings' structs (declared here as well: one of those headers may be the one that brought this one in) */
struct qlamd_contact_update;
struct qlamd_plant_contacts;
struct qlamd_plant_friction;

/* The anchored contact update.  With anchors == NULL the call IS the update (it calls it: the same kernel, bit for bit).
 * Otherwise everything the update computes is unchanged, and per leg, with p, n, gap of the update, cur = the leg's current
 * flag and nxt = the flag the update decides:
 *   nxt and not cur (touchdown)                anchor = p - gap n: the foot's projection on the terrain's tangent plane;
 *   nxt and cur and (report & reanchor_mask)   anchor = p - gap n, so that a sliding foot keeps only its normal error, and
 *                                              QLAMD_CONTACT_EVENT_REANCHORED is set in events;
 *   nxt and cur otherwise                      the anchor is not stored: it keeps its value bit for bit;
 *   not nxt                                    anchor = p, so that a foot flagged later by decree starts with no error.
 * Without a contact report no leg is re-anchored.  The anchors are never read: a QLAMD_MEM_HOST call stages the array as in/out,
 * so that kept entries come back as they went up.  A failed robot's anchors stay untouched, with or without
 * QLAMD_ON_FAILURE_KEEP.
 * With in->support_leg == NULL cur is 0 on every leg, so only the first and the last row apply: that call gives a loop its first
 * anchors (see above for a call that anchors every foot where it is).
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: what the update refuses; anchors->anchor NULL. */
typedef struct qlamd_contact_anchors {
  double *anchor;        /* [B][4][3] world, in/out: where each flagged foot is held */
  uint8_t reanchor_mask; /* report bits that move a held foot's anchor to where the foot is now */
} qlamd_contact_anchors;
#define QLAMD_CONTACT_EVENT_REANCHORED 8

int qlamd_wholebody_contact_update_anchored_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *base_position /*[B][3]*/, const struct qlamd_contact_update *update,
        const qlamd_contact_anchors *anchors /*or NULL*/, int64_t batch, int32_t *status, int memory, void *stream);

/* The anchored plant step.  With anchor == NULL the call IS the friction entry (it calls it: bit for bit), which in turn is the
 * hard entry with friction == NULL.  Otherwise, per flagged leg l, with r_l the foot in base coordinates, R = R(base_orientation),
 * a_l the leg's anchor and pos = base_position:
 *     e_l = r_l - R'(a_l - pos),      e^_l = e_l min(1, e_max / |e_l|)      (e^ = 0 where |e| = 0)
 * and the constraint right-hand side of step 2 of both entries becomes
 *     r = -gamma(q, nu+) - k_v Js nu+ - k_p e^
 * so that in the world each held foot obeys a_foot = -k_v v_foot - k_p e^.  With friction the same r enters c = r - Js x0 of the
 * force QP.  The impact, the state update and the report are unchanged.
 * The gain is the caller's and the error is clamped for a reason: k_p = 1 / dt^2 with k_v = 1 / dt is a deadbeat correction, which
 * the hard constraint answers with pulling forces wherever a foot was taken under the ground (DESIGN.md 4.6g has the figures); a
 * tenth of that with e_max at the size of a touchdown's penetration takes the error back over some ten ticks.
 * base_position is required, with or without next.  The anchor of an unflagged leg is never looked at (a NaN there changes
 * nothing).  A value that is not finite in a flagged leg's anchor gives that robot QLAMD_STATUS_NOT_PD under the entries'
 * failure rule, with zeros in position_error; its neighbours in the wavefront are not disturbed.
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: contacts NULL; anchor->anchor or base_position NULL; position_gain
 * negative or not finite; max_error not > 0 (NaN included); what the entry underneath refuses.
 * Memory spaces, streams, QLAMD_ERR_BUSY and capture as for the hard entry; next may alias the state.
 * Not built: anchors that follow a moving terrain, a rotational anchor (a foot is a point here). */
typedef struct qlamd_plant_anchor {
  const double *anchor;   /* [B][4][3] world */
  double position_gain;   /* k_p >= 0, 1/s^2 */
  double max_error;       /* e_max > 0 in metres; +infinity = no clamp */
  double *position_error; /* [B][4][3] or NULL out: the clamped error, base coordinates; 0 on an unflagged leg */
} qlamd_plant_anchor;

int qlamd_wholebody_plant_step_anchored_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *joint_effort /*[B][12]*/, const double *generalized_force /*[B][18] or NULL*/,
        const double *base_position /*[B][3]*/, double gravity, double dt,
        int64_t batch, double *acceleration /*[B][18] or NULL*/, double *contact_force /*[B][12] or NULL*/,
        const qlamd_plant_next *next /*or NULL*/, const struct qlamd_plant_contacts *contacts,
        const struct qlamd_plant_friction *friction /*or NULL*/, const qlamd_plant_anchor *anchor /*or NULL*/,
        int32_t *status, int memory, void *stream);

#ifdef __cplusplus
}
#endif

/* the swing-foot task (QLAMD_HAS_SWING_TASK, qlamd_wholebody_swing_task_batch): part of this interface, kept in a file of its own
 * that ships beside this one */
#include "qlamd_swing_task.h"

#endif /* QLAMD_CONTACT_ANCHOR_H */

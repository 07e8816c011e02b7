/* qlamd_contact_detection.h -- ground contact detection for the plant: where the feet are in the world, what terrain lies under
 * them, and the support flags of the next tick, in one launch.
 * Part of the C-ABI of qlamd.h in a file of its own: same library, same conventions, plain C.  qlamd.h includes this file at its
 * end, behind qlamd_plant_contacts.h, so a caller includes qlamd.h and tests QLAMD_HAS_CONTACT_DETECTION; including this file
 * directly works as well.
 *
 * The closed loop on the device, three launches per tick and no copy to the host:
 *   tick k solves (qlamd_wholebody_solve_batch) with flags_k and normals_k in support_leg and surface_normal;
 *   the plant steps (qlamd_wholebody_plant_step_batch) with flags_k and previous_support_leg = flags_{k-1};
 *   the update below, on the state the plant left and the plant's report, gives flags_{k+1}, normals_{k+1} and the sensors. */
#ifndef QLAMD_CONTACT_DETECTION_H
#define QLAMD_CONTACT_DETECTION_H

#include "qlamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QLAMD_HAS_CONTACT_DETECTION 1 /* (the feature test: the version number did not move with this entry) */

/* A height field: one grid shared by the whole batch.  The struct itself is always read on the host; `heights` lies in the
 * memory space of the call. */
typedef struct qlamd_heightfield {
  double origin_x, origin_y; /* world x, y of cell (0, 0) */
  double resolution;         /* > 0, metres per cell */
  int32_t nx, ny;            /* >= 2 each */
  const double *heights;     /* [ny][nx], x fastest, world z */
} qlamd_heightfield;

/* qlamd_wholebody_contact_update_batch reads joint_position, joint_velocity, base_orientation, base_linear_velocity (world),
 * base_angular_velocity (base) and support_leg of `in`; everything else in `in` is ignored.  support_leg holds the CURRENT
 * flags, the ones the plant step just ran with (NULL: no foot is flagged).
 * Per leg l, with the model's leg forward kinematics and Jacobian (those of qlamd_leg_kinematics_batch), R = R(base_orientation):
 *   r = the foot in base coordinates,   p = base_position + R r,   u = v_W + R (w x r + J_l qd_l).
 * The terrain under p:
 *   plane         n = (a, b, c) / |(a, b, c)|,  gap = n . p - d / |(a, b, c)|;   plane and heightfield both NULL: n = e_z, gap = p_z.
 *   height field  s = clamp((p_x - origin_x) / resolution, 0, nx - 1), i = min(floor(s), nx - 2), alpha = s - i; the same in y
 *                 gives j and beta.  h = the bilinear patch of the four corners of cell (i, j) at (alpha, beta), (h_x, h_y) its
 *                 gradient there, n = (-h_x, -h_y, 1) / |.|, gap = n_z (p_z - h): the distance to the cell's tangent plane, the
 *                 same quantity as in plane mode.  A foot outside the grid sees the border cell's patch at the clamped point.
 * The flags:
 *   a leg flagged now stays flagged unless contact_report is given and (report & release_mask) != 0
 *   (QLAMD_CONTACT_EVENT_RELEASED_PULL) or gap > liftoff_distance (QLAMD_CONTACT_EVENT_RELEASED_GAP); both bits may be set.
 *   a leg not flagged now becomes flagged when gap <= touchdown_distance and n . u <= approach_speed
 *   (QLAMD_CONTACT_EVENT_TOUCHDOWN).
 * So a foot standing at rest on the ground is picked up, and a foot just released because it pulled is not taken back while it
 * moves away.  contact_sensor is purely geometric.
 * status: QLAMD_STATUS_OK, or QLAMD_STATUS_NOT_PD when a value read for that robot (state, plane, a height cell) or a result
 * is not finite, or the plane normal has length 0 -- as the plant step reports values that are not finite.  A failed robot:
 * support_next = its current flags and zeros in every other output; or (QLAMD_ON_FAILURE_KEEP) all of them untouched.  Its
 * neighbours are not disturbed.
 * Everything is read before anything is written: support_next may be in->support_leg.
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: ctx, in, base_position, update or status NULL; one of the five state
 * arrays NULL; plane and heightfield both given; a height field with nx or ny < 2, a resolution that is not positive or not
 * finite, or heights NULL; a distance or the speed not finite; liftoff_distance < touchdown_distance; batch < 0.
 * Memory spaces, streams, QLAMD_ERR_BUSY and capture as for qlamd_wholebody_plant_step_batch: a QLAMD_MEM_DEVICE call uses no
 * scratch of the context's and can be captured into a graph.
 * Friction as a constraint is qlamd_wholebody_plant_step_friction_batch (qlamd_plant_friction.h), whose report releases a foot with
 * release_mask = QLAMD_CONTACT_SEPARATING.  Position-level drift correction of a held foot is qlamd_contact_anchor.h:
 * qlamd_wholebody_contact_update_anchored_batch keeps an anchor per leg and qlamd_wholebody_plant_step_anchored_batch holds it. */
typedef struct qlamd_contact_update {
  /* in */
  const double *plane;                  /* [B][4] (a, b, c, d): ground a x + b y + c z = d per robot, or NULL */
  const qlamd_heightfield *heightfield; /* or NULL; both given: refused; both NULL: the ground z = 0 */
  const uint8_t *contact_report;        /* [B][4] or NULL: the plant step's QLAMD_CONTACT_* bits for the current flags */
  uint8_t release_mask;                 /* report bits that release a flagged foot */
  double touchdown_distance;            /* an unflagged foot is flagged when gap <= this ... */
  double approach_speed;                /* ... and n . u <= this */
  double liftoff_distance;              /* a flagged foot is released when gap > this; >= touchdown_distance */
  double sensor_distance;               /* contact_sensor = gap <= this */
  /* out, each may be NULL */
  uint8_t *support_next;                /* [B][4]; may alias in->support_leg */
  uint8_t *contact_sensor;              /* [B][4], what qlamd_tick_batch::contact takes */
  uint8_t *events;                      /* [B][4] QLAMD_CONTACT_EVENT_* */
  double *gap;                          /* [B][4] */
  double *surface_normal;               /* [B][4][3] world, unit: what in->surface_normal of the solve and of the plant's report take */
  double *foot_position, *foot_velocity;/* [B][4][3] world */
} qlamd_contact_update;
#define QLAMD_CONTACT_EVENT_TOUCHDOWN 1
#define QLAMD_CONTACT_EVENT_RELEASED_PULL 2
#define QLAMD_CONTACT_EVENT_RELEASED_GAP 4

/* distances and speed 0, release_mask = QLAMD_CONTACT_PULLS, every pointer NULL */
void qlamd_contact_update_default(qlamd_contact_update *u);
int qlamd_wholebody_contact_update_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *base_position /*[B][3]*/, const qlamd_contact_update *update, int64_t batch,
        int32_t *status, int memory, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QLAMD_CONTACT_DETECTION_H */

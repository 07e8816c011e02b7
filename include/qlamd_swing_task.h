/* qlamd_swing_task.h -- the swing-foot task of the closed loop: from a swing schedule and footholds to the desired joint
 * accelerations and the support flags that the whole-body step runs with, one swing record per leg kept on the device.
 * Part of the C-ABI of qlamd.h in a file of its own: same library, same conventions, plain C.  qlamd.h brings this file in at its
 * end, behind qlamd_contact_anchor.h (that header includes this one at its own end), so a caller includes qlamd.h and tests
 * QLAMD_HAS_SWING_TASK; including this file directly works as well.
 * "The update" below is qlamd_wholebody_contact_update_batch of qlamd_contact_detection.h, "the solve"
 * qlamd_wholebody_solve_batch of qlamd.h and "the plant" any of the plant steps; their comments have p, u, r, J, gamma and R.
 *
 * Why: the solve gives a leg that does not support its inverse-dynamics torque for in->desired_joint_acceleration, and nothing
 * produced that array on the device: without it no swing leg moves, and a foot the schedule wants in the air stays on the
 * ground.
 *
 * The closed loop on the device, four launches per tick and no copy to the host:
 *   the task below, on the state and the flags the update left, gives desired_joint_acceleration and support_solve;
 *   tick k solves with support_leg = support_solve and that desired_joint_acceleration;
 *   the plant steps with the DETECTED flags_k (a foot on the ground is held whatever the schedule says) and flags_{k-1};
 *   the update gives flags_{k+1}. */
#ifndef QLAMD_SWING_TASK_H
#define QLAMD_SWING_TASK_H

#include "qlamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QLAMD_HAS_SWING_TASK 1 /* (the feature test: the version number did not move with this entry) */

/* qlamd_wholebody_swing_task_batch reads joint_position, joint_velocity, base_orientation, base_linear_velocity (world),
 * base_angular_velocity (base), support_leg and desired_base_acceleration of `in`; everything else in `in` is ignored.
 * support_leg holds the detected flags `cur` of this tick (NULL: no foot is flagged), desired_base_acceleration [v'_d ; w'_d]
 * in base coordinates (NULL: 0).
 * Per leg, with want = swing_leg, c = the clock of its swing record and p, u the update's world position and velocity of the
 * foot:
 *   not want                                     idle: clock = 0, qdd = 0, support_solve = cur.  foothold, surface_normal and
 *                                                the record of such a leg are not looked at (a NaN there changes nothing).
 *   want, c == 0                                 the swing begins (QLAMD_SWING_EVENT_BEGAN): start = p, the reference at t = 0,
 *                                                clock = dt.
 *   want, c < 0                                  it landed earlier in this swing (the landing leaves c = -1): qdd = 0,
 *                                                support_solve = cur, the record stays.
 *   want, c > 0, cur, c >= touchdown_phase T     it lands (QLAMD_SWING_EVENT_LANDED): clock = -1, qdd = 0, support_solve = 1.
 *   want, c > 0 otherwise                        it swings, the reference at t = c, clock = c + dt;
 *                                                QLAMD_SWING_EVENT_LATE_LIFTOFF while cur is still set,
 *                                                QLAMD_SWING_EVENT_OVERTIME once t > T.
 * A leg that begins or swings has support_solve = 0.  An idle leg's clock of 0 is what lets its next swing begin.
 * The reference, from `start` to `target` = foothold, with s = min(t / T, 1) and sigma(x) = 10 x^3 - 15 x^4 + 6 x^5:
 *   x, y      start + (target - start) sigma(s)
 *   z         z_A = max(z_start, z_target) + profile_height;   s <= 1/2: z_start + (z_A - z_start) sigma(2 s),
 *                                                               s >  1/2: z_A + (z_target - z_A) sigma(2 s - 1)
 *   v_ref, a_ref: the exact derivatives in t (continuous at s = 1/2 up to the acceleration, zero at both ends);
 *   t > T     p_ref = target - n v_td (t - T), v_ref = -n v_td, a_ref = 0, n = the leg's surface_normal (NULL: e_z).
 * The command and its joint accelerations, R = R(base_orientation), w = base_angular_velocity, v = R' v_W:
 *   e^ = (p_ref - p) min(1, e_max / |p_ref - p|)                     (e^ = 0 where the error is 0)
 *   a_cmd = a_ref + k_d (v_ref - u) + k_p e^
 *   gamma = w x v + w x (w x r) + 2 w x (J qd) + J' qd               (the plant's, this leg's rows)
 *   c = R' a_cmd - v'_d - w'_d x r - gamma
 *   qdd = J' (J J' + lambda^2 I)^-1 c   by the LDL' factors of the 3 x 3 matrix, then each component clamped to
 *                                       +-max_joint_acceleration.
 * So with lambda = 0 and the clamps off, a base that accelerates by [v'_d ; w'_d] and joints that accelerate by qdd move the
 * foot with a_cmd in the world.
 * status: QLAMD_STATUS_OK, or QLAMD_STATUS_NOT_PD when a value read for that robot (the state, the desired base acceleration; the
 * clock of a scheduled leg; start, foothold and normal of a leg that begins or swings) or a result is not finite, or a pivot
 * of the factorisation is not positive (possible only with lambda = 0).  A failed robot: qdd = 0, support_solve = cur, zeros
 * in foot_reference and swing_events, and its swing_state untouched; or (QLAMD_ON_FAILURE_KEEP) all of them untouched.  Its
 * neighbours are not disturbed.
 * Everything is read before anything is written: support_solve may be in->support_leg.
 * Refused with QLAMD_ERR_INVALID_ARGUMENT, nothing written: ctx, in, base_position, task or status NULL; swing_leg, foothold,
 * swing_state or desired_joint_acceleration NULL; one of the five state arrays NULL; a scalar outside the range given below
 * (NaN included); batch < 0.
 * Memory spaces, streams, QLAMD_ERR_BUSY and capture as for the update: a QLAMD_MEM_DEVICE call uses no scratch of the
 * context's and can be captured into a graph; a QLAMD_MEM_HOST call stages swing_state as in/out.
 * Not built: foothold planning, other profiles (square, trapezoid), per-robot parameters. */
typedef struct qlamd_swing_task {
  /* in */
  const uint8_t *swing_leg;       /* [B][4] the schedule: 1 = this leg is to swing now */
  const double  *foothold;        /* [B][4][3] world: where the swing ends (read for scheduled legs only) */
  const double  *surface_normal;  /* [B][4][3] world unit, or NULL = e_z: direction of the touchdown descent */
  double swing_duration;          /* T > 0, s */
  double profile_height;          /* h >= 0, m */
  double touchdown_speed;         /* v_td >= 0, m/s: after T the reference keeps descending along -n */
  double touchdown_phase;         /* in [0,1]: a contact flag counts as a landing only once t >= touchdown_phase * T */
  double position_gain, velocity_gain; /* k_p, k_d >= 0 */
  double max_error;               /* e_max > 0, +inf = no clamp: |p_ref - p| is clamped to it */
  double damping;                 /* lambda >= 0 of the damped inverse */
  double max_joint_acceleration;  /* > 0, +inf = none: componentwise clamp of the result */
  double dt;                      /* > 0: what a swinging leg's clock advances by */
  /* in/out */
  double *swing_state;            /* [B][4][4]: start x y z, clock.  Zero-filled before the first tick */
  /* out, each may be NULL except desired_joint_acceleration */
  double  *desired_joint_acceleration; /* [B][12]: what in->desired_joint_acceleration of the solve takes */
  uint8_t *support_solve;         /* [B][4]: what in->support_leg of the SOLVE takes (the plant keeps the detected flags) */
  double  *foot_reference;        /* [B][4][9] world p_ref, v_ref, a_ref; zeros on a leg that does not swing */
  uint8_t *swing_events;          /* [B][4] QLAMD_SWING_EVENT_* */
} qlamd_swing_task;
#define QLAMD_SWING_EVENT_BEGAN 1
#define QLAMD_SWING_EVENT_LANDED 2
#define QLAMD_SWING_EVENT_LATE_LIFTOFF 4
#define QLAMD_SWING_EVENT_OVERTIME 8

/* T 0.45, h 0.08, touchdown_speed, touchdown_phase, the gains and the damping 0, max_error and max_joint_acceleration +infinity,
 * dt 0 (the caller's to set: the call refuses it), every pointer NULL */
void qlamd_swing_task_default(qlamd_swing_task *t);
int qlamd_wholebody_swing_task_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in,
        const double *base_position /*[B][3]*/, const qlamd_swing_task *task, int64_t batch,
        int32_t *status, int memory, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QLAMD_SWING_TASK_H */

// Arithmetic of the contact update (include/qlamd_contact_detection.h), one leg at a time, host and device: the foot in the
// world, the terrain under it, the flag rule.  csrc/contact_update_kernel.hip runs it with one lane per leg.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "balance_core.hpp"

namespace qlamd {

QL_HD bool cu_finite(double x) { return x - x == 0.0; }
QL_HD bool cu_finite3(const double v[3]) { return cu_finite(v[0]) && cu_finite(v[1]) && cu_finite(v[2]); }

// p = pos + R r,  u = v_W + R (w x r + J qd): world position and velocity of one foot.  tab: the leg's block of the model table.
template <class Tab>
QL_HD void cu_foot_world(const Tab &tab, const double q[3], const double qd[3], const double Rm[9], const double pos[3],
                         const double linvel[3], const double angvel[3], double p[3], double u[3]) {
  const double zero[3] = {0.0, 0.0, 0.0};
  double r[3], J[9], Gq[3]; // (the gravity torques of leg_kinematics are not used and fold away)
  leg_kinematics(tab, q, zero, r, J, Gq);
  double wr[3], vb[3], Rr[3], Rv[3];
  cross3(angvel, r, wr);
  QL_UNROLL for (int a = 0; a < 3; a++) vb[a] = wr[a] + (J[3 * a] * qd[0] + J[3 * a + 1] * qd[1] + J[3 * a + 2] * qd[2]);
  rot(Rm, r, Rr);
  rot(Rm, vb, Rv);
  QL_UNROLL for (int a = 0; a < 3; a++) { p[a] = pos[a] + Rr[a]; u[a] = linvel[a] + Rv[a]; }
}

// Plane a x + b y + c z = d: n = (a, b, c) / |.|, gap = n . p - d / |.|.  false: the normal has length 0 (n and gap are not set
// to anything useful then); values that are not finite come out as such and are the caller's to test.
QL_HD bool cu_plane(const double pl[4], const double p[3], double n[3], double &gap) {
  const double len2 = pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2];
  const bool ok = len2 > 0.0;
  const double inv = ql_rsqrt(ok ? len2 : 1.0);
  n[0] = pl[0] * inv; n[1] = pl[1] * inv; n[2] = pl[2] * inv;
  gap = dot3(n, p) - pl[3] * inv;
  return ok;
}

// The cell of a height field under a coordinate: s = clamp((x - origin) * inv_res, 0, n - 1), cell = min(floor(s), n - 2),
// frac = s - cell.  A coordinate that is not a number lands in cell 0 (fmax and fmin return the other operand): the index is
// inside the grid whatever comes in.
QL_HD void cu_cell(double x, double origin, double inv_res, int n, int &cell, double &frac) {
  const double s = fmin(fmax((x - origin) * inv_res, 0.0), (double)(n - 1));
  int c = (int)floor(s);
  c = c > n - 2 ? n - 2 : c;
  c = c < 0 ? 0 : c;
  cell = c;
  frac = s - (double)c;
}

// The bilinear patch of a cell with corners h00 (i, j), h10 (i + 1, j), h01 (i, j + 1), h11 at (alpha, beta):
// n = (-h_x, -h_y, 1) / |.|,  gap = n_z (p_z - h).
QL_HD void cu_patch(double h00, double h10, double h01, double h11, double alpha, double beta, double inv_res, double pz,
                    double n[3], double &gap) {
  const double a1 = 1.0 - alpha, b1 = 1.0 - beta;
  const double h = b1 * (a1 * h00 + alpha * h10) + beta * (a1 * h01 + alpha * h11);
  const double hx = (b1 * (h10 - h00) + beta * (h11 - h01)) * inv_res;
  const double hy = (a1 * (h01 - h00) + alpha * (h11 - h10)) * inv_res;
  const double inv = ql_rsqrt(hx * hx + hy * hy + 1.0);
  n[0] = -hx * inv; n[1] = -hy * inv; n[2] = inv;
  gap = inv * (pz - h);
}

struct ContactRule {
  double touchdown, speed, liftoff, sensor; // the four thresholds of qlamd_contact_update
  unsigned release;                         // its release_mask
};
constexpr unsigned kEventTouchdown = 1, kEventReleasedPull = 2, kEventReleasedGap = 4;

// The flag rule for one leg: flagged = its current flag, report = the plant's bits for it (0 without a report).
QL_HD void cu_flags(const ContactRule &rule, bool flagged, unsigned report, double gap, double nu, bool &next, unsigned &events,
                    bool &sensor) {
  const bool pull = (report & rule.release) != 0u, far = gap > rule.liftoff;
  const bool touch = gap <= rule.touchdown && nu <= rule.speed;
  events = flagged ? (pull ? kEventReleasedPull : 0u) | (far ? kEventReleasedGap : 0u) : (touch ? kEventTouchdown : 0u);
  next = flagged ? !(pull || far) : touch;
  sensor = gap <= rule.sensor;
}

} // namespace qlamd

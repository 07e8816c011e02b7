// Arithmetic of the swing-foot task (include/qlamd_swing_task.h), one leg at a time, host and device: the leg's row of the
// swing table, the reference of the foot, the command, gamma of the foot point and the damped map from the foot to the joints.
// csrc/swing_task_kernel.hip runs it with one lane per leg.
#pragma once

#include "contact_update_core.hpp"

namespace qlamd {

// The scalars of qlamd_swing_task as the leg rule reads them.  t_land = touchdown_phase * T and lam2 = lambda^2 are formed once,
// on the host, so that every build of the rule compares a clock with the same number.
struct SwingRule {
  double T, inv_T, height, v_td, t_land, kp, kd, e_max, lam2, qdd_max, dt;
};
inline SwingRule swing_rule(double T, double height, double v_td, double phase, double kp, double kd, double e_max, double lambda,
                            double qdd_max, double dt) {
  return SwingRule{T, 1.0 / T, height, v_td, phase * T, kp, kd, e_max, lambda * lambda, qdd_max, dt};
}
constexpr unsigned kSwingBegan = 1, kSwingLanded = 2, kSwingLateLiftoff = 4, kSwingOvertime = 8;

// sigma(x) = 10 x^3 - 15 x^4 + 6 x^5 and its first two derivatives
QL_HD void st_quintic(double x, double &s, double &d, double &dd) {
  const double x2 = x * x;
  s = x2 * x * (10.0 + x * (-15.0 + 6.0 * x));
  d = x2 * (30.0 + x * (-60.0 + 30.0 * x));
  dd = x * (60.0 + x * (-180.0 + 120.0 * x));
}

// ref [9] = p_ref, v_ref, a_ref of the foot at time t of a swing from `start` to `target` (the header has the profile)
QL_HD void st_reference(const SwingRule &S, const double start[3], const double target[3], const double n[3], double t,
                        double ref[9]) {
  const double s = fmin(t * S.inv_T, 1.0);
  double g, dg, ddg;
  st_quintic(s, g, dg, ddg);
  QL_UNROLL for (int a = 0; a < 2; a++) {
    const double D = target[a] - start[a];
    ref[a] = start[a] + D * g;
    ref[3 + a] = D * dg * S.inv_T;
    ref[6 + a] = D * ddg * (S.inv_T * S.inv_T);
  }
  const double zA = fmax(start[2], target[2]) + S.height;
  const bool up = s <= 0.5;
  st_quintic(up ? 2.0 * s : 2.0 * s - 1.0, g, dg, ddg);
  const double z0 = up ? start[2] : zA, D = up ? zA - start[2] : target[2] - zA;
  ref[2] = z0 + D * g;
  ref[5] = D * dg * (2.0 * S.inv_T);
  ref[8] = D * ddg * (4.0 * S.inv_T * S.inv_T);
  const bool over = t > S.T;
  const double late = t - S.T;
  QL_UNROLL for (int a = 0; a < 3; a++) {
    ref[a] = over ? target[a] - n[a] * (S.v_td * late) : ref[a];
    ref[3 + a] = over ? -n[a] * S.v_td : ref[3 + a];
    ref[6 + a] = over ? 0.0 : ref[6 + a];
  }
}

// The leg's chain once more, for what leg_kinematics does not hand out: the joint axes z [3] and origins o [3] in base
// coordinates beside the foot r -- T_seg(q) = Trans(xyz) R0 Rz(q) per segment, the fourth one fixed.  Kinematics only: no mass,
// no inertia is read, and every R0 is a full rotation.
template <class Tab>
QL_HD void st_leg_chain(const Tab &tab, const double q[3], double z[3][3], double o[3][3], double r[3]) {
  double Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double pc[3] = {0, 0, 0};
  QL_UNROLL for (int k = 0; k < 4; k++) {
    double R0[9], t[3], pn[3];
    QL_UNROLL for (int i = 0; i < 9; i++) R0[i] = tab[kTabR0 + 9 * k + i];
    QL_UNROLL for (int i = 0; i < 3; i++) t[i] = tab[kTabXyz + 3 * k + i];
    QL_UNROLL for (int i = 0; i < 3; i++) pn[i] = pc[i] + (Rc[i * 3] * t[0] + Rc[i * 3 + 1] * t[1] + Rc[i * 3 + 2] * t[2]);
    QL_UNROLL for (int i = 0; i < 3; i++) pc[i] = pn[i];
    if (k < 3) {
      double s, c, Rs[9], Rn[9];
      sincos_reduced(q[k], s, c);
      QL_UNROLL for (int i = 0; i < 3; i++) {
        Rs[i * 3 + 0] = R0[i * 3 + 0] * c + R0[i * 3 + 1] * s;
        Rs[i * 3 + 1] = R0[i * 3 + 1] * c - R0[i * 3 + 0] * s;
        Rs[i * 3 + 2] = R0[i * 3 + 2];
      }
      QL_UNROLL for (int i = 0; i < 3; i++)
        QL_UNROLL for (int j = 0; j < 3; j++)
          Rn[i * 3 + j] = Rc[i * 3] * Rs[j] + Rc[i * 3 + 1] * Rs[3 + j] + Rc[i * 3 + 2] * Rs[6 + j];
      QL_UNROLL for (int i = 0; i < 9; i++) Rc[i] = Rn[i];
      QL_UNROLL for (int i = 0; i < 3; i++) { z[k][i] = Rn[i * 3 + 2]; o[k][i] = pn[i]; }
    }
  }
  r[0] = pc[0]; r[1] = pc[1]; r[2] = pc[2];
}

// r, J (row-major, column i = z_i x (r - o_i)) and gamma = w x v + w x (w x r) + 2 w x (J qd) + J' qd of one foot point, base
// coordinates: plant_foot_bias of plant_coop.hpp on one lane, walking the leg's three joints.  With w_i = sum_{k <= i} qd_k z_k
// the angular velocity of link i against the base, z_i' = w_i x z_i and o_i' = sum_{k < i} qd_k z_k x (o_i - o_k), so
//   J' qd = sum_i qd_i (z_i' x (r - o_i) + z_i x (J qd - o_i')).
template <class Tab>
QL_HD void st_foot_bias(const Tab &tab, const double q[3], const double qd[3], const double w[3], const double v[3], double r[3],
                        double J[9], double gam[3]) {
  double z[3][3], o[3][3], d[3][3], vrel[3] = {0.0, 0.0, 0.0};
  st_leg_chain(tab, q, z, o, r);
  QL_UNROLL for (int i = 0; i < 3; i++) {
    double col[3];
    QL_UNROLL for (int a = 0; a < 3; a++) d[i][a] = r[a] - o[i][a];
    cross3(z[i], d[i], col);
    QL_UNROLL for (int a = 0; a < 3; a++) { J[3 * a + i] = col[a]; vrel[a] += col[a] * qd[i]; }
  }
  double wl[3] = {0.0, 0.0, 0.0}, jd[3] = {0.0, 0.0, 0.0};
  QL_UNROLL for (int i = 0; i < 3; i++) {
    double od[3] = {0.0, 0.0, 0.0};
    QL_UNROLL for (int k = 0; k < i; k++) {
      const double ok[3] = {o[i][0] - o[k][0], o[i][1] - o[k][1], o[i][2] - o[k][2]};
      double c[3];
      cross3(z[k], ok, c);
      QL_UNROLL for (int a = 0; a < 3; a++) od[a] += qd[k] * c[a];
    }
    QL_UNROLL for (int a = 0; a < 3; a++) wl[a] += qd[i] * z[i][a];
    double zd[3], c1[3], c2[3];
    cross3(wl, z[i], zd);
    const double dd[3] = {vrel[0] - od[0], vrel[1] - od[1], vrel[2] - od[2]};
    cross3(zd, d[i], c1);
    cross3(z[i], dd, c2);
    QL_UNROLL for (int a = 0; a < 3; a++) jd[a] += qd[i] * (c1[a] + c2[a]);
  }
  double wv[3], wr[3], wwr[3], wj[3];
  cross3(w, v, wv);
  cross3(w, r, wr);
  cross3(w, wr, wwr);
  cross3(w, vrel, wj);
  QL_UNROLL for (int a = 0; a < 3; a++) gam[a] = wv[a] + wwr[a] + 2.0 * wj[a] + jd[a];
}

// qdd = J' (J J' + lam2 I)^-1 c by the LDL' factors of the 3 x 3 matrix.  false: a pivot was not positive.
QL_HD bool st_damped_map(const double J[9], double lam2, const double c[3], double qdd[3]) {
  double A[6]; // xx xy xz yy yz zz
  {
    int e = 0;
    QL_UNROLL for (int a = 0; a < 3; a++)
      QL_UNROLL for (int b = a; b < 3; b++)
        A[e++] = J[3 * a] * J[3 * b] + J[3 * a + 1] * J[3 * b + 1] + J[3 * a + 2] * J[3 * b + 2] + (a == b ? lam2 : 0.0);
  }
  const double d0 = A[0], i0 = ql_rcp(d0);
  const double l10 = A[1] * i0, l20 = A[2] * i0;
  const double d1 = A[3] - l10 * A[1], i1 = ql_rcp(d1);
  const double t = A[4] - l10 * A[2], l21 = t * i1;
  const double d2 = A[5] - l20 * A[2] - l21 * t, i2 = ql_rcp(d2);
  const double y0 = c[0], y1 = c[1] - l10 * y0, y2 = c[2] - l20 * y0 - l21 * y1;
  const double x2 = y2 * i2, x1 = y1 * i1 - l21 * x2, x0 = y0 * i0 - l10 * x1 - l20 * x2;
  QL_UNROLL for (int j = 0; j < 3; j++) qdd[j] = J[j] * x0 + J[3 + j] * x1 + J[6 + j] * x2;
  return d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}

// One leg of the task.  want: the schedule; cur: the detected flag; st [4]: the leg's swing record (start, clock); ades [6]:
// [v'_d ; w'_d].  -> qdd [3], ref [9], next [4] = the record after the tick, support = the flag for the solve, events; the
// return value: everything read for this leg and everything produced is finite and every pivot positive (the quaternion is the
// caller's to test: Rm comes in).  The outputs of a leg that does not move are exact zeros whatever its foothold holds.
template <class Tab>
QL_HD bool swing_task_leg(const Tab &tab, const SwingRule &S, const double q[3], const double qd[3], const double Rm[9],
                          const double pos[3], const double linvel[3], const double angvel[3], const double ades[6], bool want,
                          bool cur, const double st[4], const double target[3], const double n[3], double qdd[3], double ref[9],
                          double next[4], bool &support, unsigned &events) {
  double p[3], u[3];
  cu_foot_world(tab, q, qd, Rm, pos, linvel, angvel, p, u);
  bool good = cu_finite3(q) && cu_finite3(qd) && cu_finite3(linvel) && cu_finite3(angvel) && cu_finite3(pos) && cu_finite3(p) &&
              cu_finite3(u) && cu_finite3(ades) && cu_finite3(ades + 3);
  const double c = st[3];
  const bool begin = want && c == 0.0, landed = want && c < 0.0, active = want && c > 0.0;
  const bool landing = active && cur && c >= S.t_land, swinging = active && !landing, moving = begin || swinging;
  good = good && (!want || cu_finite(c));
  const double t = begin ? 0.0 : c;
  const double start[3] = {begin ? p[0] : st[0], begin ? p[1] : st[1], begin ? p[2] : st[2]};

  double r9[9];
  st_reference(S, start, target, n, t, r9);
  double e[3] = {r9[0] - p[0], r9[1] - p[1], r9[2] - p[2]};
  const double len2 = dot3(e, e);
  const double scale = len2 > S.e_max * S.e_max ? S.e_max * ql_rsqrt(len2) : 1.0;
  double acmd[3], v[3], cb[3], r[3], J[9], gam[3], wdr[3], x[3];
  QL_UNROLL for (int a = 0; a < 3; a++) acmd[a] = r9[6 + a] + S.kd * (r9[3 + a] - u[a]) + S.kp * (e[a] * scale);
  irot(Rm, linvel, v);
  st_foot_bias(tab, q, qd, angvel, v, r, J, gam);
  irot(Rm, acmd, cb);
  cross3(ades + 3, r, wdr);
  QL_UNROLL for (int a = 0; a < 3; a++) cb[a] = cb[a] - ades[a] - wdr[a] - gam[a];
  const bool pivots = st_damped_map(J, S.lam2, cb, x);
  good = good && (!moving || (pivots && cu_finite3(start) && cu_finite3(target) && cu_finite3(n) && cu_finite3(x) && cu_finite3(r9) &&
                              cu_finite3(r9 + 3) && cu_finite3(r9 + 6)));

  QL_UNROLL for (int j = 0; j < 3; j++) qdd[j] = moving ? fmin(fmax(x[j], -S.qdd_max), S.qdd_max) : 0.0;
  QL_UNROLL for (int a = 0; a < 9; a++) ref[a] = moving ? r9[a] : 0.0;
  QL_UNROLL for (int a = 0; a < 3; a++) next[a] = start[a];
  next[3] = !want ? 0.0 : begin ? S.dt : landing ? -1.0 : swinging ? c + S.dt : c;
  support = moving ? false : landing ? true : cur;
  events = begin ? kSwingBegan : landing ? kSwingLanded : swinging ? (cur ? kSwingLateLiftoff : 0u) | (t > S.T ? kSwingOvertime : 0u) : 0u;
  return good;
}

} // namespace qlamd

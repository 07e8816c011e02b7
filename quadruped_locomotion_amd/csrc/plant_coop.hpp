// Contact-constrained forward dynamics of the 18-DoF robot (the plant step), lane-cooperative: 16 lanes per robot, 4 robots per
// wavefront, lane 4*leg + c as in wholebody_coop.hpp.  Device-only.
//
//     M nu' - Js' f = [0 ; tau] + g_ext - h,      Js nu' = -gamma      (rows of the flagged feet)
//
// M is never formed as an 18 x 18 array.  Its joint block is block-diagonal, one 3 x 3 block A_l per leg, held by the quad of
// the leg; with F_l [6][3] the leg's columns of the base rows (wb_crba's Fcol) and G_l = F_l A_l^-1:
//     S   = M_bb - sum_l G_l F_l'                         base Schur complement, 6 x 6, replicated on the row
//     E_r = Jb_r - J_leg,r G_l'                           row r = (leg, component) of Js after the joint elimination, lane r
//     Js M^-1 Js' = E S^-1 E' + blockdiag(J_leg A_l^-1 J_leg')     row r on lane r, inverted by the in-place Gauss-Jordan of
//                                                                  force_qp_coop.hpp (rows of unflagged feet: the identity)
// and M^-1 [b ; j] = [x ; A^-1 j - G' x] with x = S^-1 (b - G j).  (Featherstone 2008, section 9.4 has the elimination order.)
#pragma once

#include "wholebody_coop.hpp"

namespace qlamd {
namespace coop {

// gamma of my leg's foot point, replicated in the quad: its classical acceleration at nu' = 0, base coordinates --
// w x v + w x (w x r) + 2 w x (J_leg qd) + J_leg' qd.  It is the velocity-product part of the Newton-Euler forward pass of
// wb_inverse_dynamics (same prefix sums, no fictitious gravity term) read on the foot lane: with [w ; v] the foot link's spatial
// velocity and [aw ; av] its spatial acceleration, the point r of the link accelerates by av + aw x r + w x (v + w x r).
__device__ __forceinline__ void plant_foot_bias(const WbLink &L, int c, const double V0[6], double qd, double gam[3]) {
  double sw[3], sv[3];
  wb_joint_axis(L, c, sw, sv);
  double w[3], v[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { w[a] = V0[a] + quad_prefix(sw[a] * qd, c); v[a] = V0[3 + a] + quad_prefix(sv[a] * qd, c); }
  const double jw[3] = {sw[0] * qd, sw[1] * qd, sw[2] * qd}, jv[3] = {sv[0] * qd, sv[1] * qd, sv[2] * qd};
  double c1[3], c2[3], c3[3];
  cross3(w, jw, c1);
  cross3(w, jv, c2);
  cross3(v, jw, c3);
  double aw[3], av[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { aw[a] = quad_prefix(c1[a], c); av[a] = quad_prefix(c2[a] + c3[a], c); }
  double wr[3], ar[3], wu[3];
  cross3(w, L.pf, wr);
  cross3(aw, L.pf, ar);
  const double u[3] = {v[0] + wr[0], v[1] + wr[1], v[2] + wr[2]};
  cross3(w, u, wu);
#pragma unroll
  for (int a = 0; a < 3; a++) gam[a] = quad_bc<3>(av[a] + ar[a] + wu[a]);
}

// Inverse of the symmetric 3 x 3 block a (xx xy xz yy yz zz) through its LDL' factors, the same layout out.  Returns whether
// every pivot was positive.
__device__ __forceinline__ bool plant_inverse3(const double a[6], double inv[6]) {
  const double d0 = a[0], i0 = rcp_nr(d0);
  const double l10 = a[1] * i0, l20 = a[2] * i0;
  const double d1 = a[3] - l10 * a[1], i1 = rcp_nr(d1);
  const double t = a[4] - l10 * a[2], l21 = t * i1;
  const double d2 = a[5] - l20 * a[2] - l21 * t, i2 = rcp_nr(d2);
  const double m10 = -l10, m21 = -l21, m20 = l10 * l21 - l20; // L^-1
  inv[0] = i0 + m10 * m10 * i1 + m20 * m20 * i2;
  inv[1] = m10 * i1 + m20 * m21 * i2;
  inv[2] = m20 * i2;
  inv[3] = i1 + m21 * m21 * i2;
  inv[4] = m21 * i2;
  inv[5] = i2;
  return d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}

// In-place Gauss-Jordan inversion of a symmetric positive definite 6 x 6 matrix held in full by every lane (no pivoting: the
// pivots are those of its Cholesky factor, squared).  Returns whether every pivot was positive.
__device__ __forceinline__ bool plant_inverse6(double S[6][6]) {
  bool ok = true;
  static_for<6>([&](auto K) {
    constexpr int k = K;
    ok = ok && S[k][k] > 0.0;
    const double p = rcp_nr(S[k][k]);
    double rk[6];
#pragma unroll
    for (int j = 0; j < 6; j++) rk[j] = S[k][j] * p;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      if (i == k) continue;
      const double f = S[i][k];
#pragma unroll
      for (int j = 0; j < 6; j++)
        if (j != k) S[i][j] -= f * rk[j];
      S[i][k] = -f * p;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) S[k][j] = rk[j];
    S[k][k] = p;
  });
  return ok;
}

// In-place Gauss-Jordan inversion of a symmetric positive definite 12 x 12 matrix, row myidx = 3 leg + c on lane 4 leg + c
// (comp: c < 3): the elimination of force_qp_coop.hpp -- one v_fmac_f64_dpp per row update, the next pivot's column first --
// with the reciprocal at full precision, since nothing refines on the matrix itself afterwards but one residual pass.
__device__ __forceinline__ bool plant_inverse12(double H[12], bool comp, int myidx) {
  bool bad = false;
  double d = bcv<0>(H[0]);
  static_for<12>([&](auto K) {
    constexpr int k = K;
    bad = bad || !(d > 0.0);
    const double p = rcp_nr(d);
    const bool piv = comp && (myidx == k);
    const double f = piv ? (1.0 - p) : H[k] * p;
    const double nf = -f;
    if constexpr (k < 11) {
      fmac_bc<lane_of(k), true>(H[k + 1], H[k + 1], nf);
      d = bcv<k + 1>(H[k + 1]);
    }
    static_for<12>([&](auto J) {
      constexpr int j = J;
      if constexpr (j != k && j != k + 1) fmac_bc<lane_of(k), (k == 11 && j == 0)>(H[j], H[j], nf);
    });
    H[k] = piv ? p : nf;
  });
  return !bad;
}

// sum over j of H[j] * (v on the lane of variable j): a row of a 12 x 12 product per lane
__device__ __forceinline__ double plant_row_dot(const double H[12], double v) {
  double acc[3] = {0.0, 0.0, 0.0};
  static_for<12>([&](auto J) { constexpr int j = J; fmac_bc<lane_of(j), j == 0>(acc[j % 3], v, H[j]); });
  return (acc[0] + acc[1]) + acc[2];
}

// whether `pred` holds on any lane of my 16-lane row
__device__ __forceinline__ bool row_any(bool pred) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);
  return ((unsigned)(m >> (threadIdx.x & 48)) & 0xFFFFu) != 0u;
}

struct PlantSolution {
  double nub[6]; // base rows of nu', interface order [v' ; w'], replicated
  double nuj;    // my joint's acceleration (lanes c < 3)
  double f;      // component c of my leg's contact force (lanes c < 3; 0 on an unflagged leg)
  bool ok;       // every pivot positive, every value finite -- the same on all lanes of the row
};

// The solve.  T, Fcol, Mleg: wb_crba's; hb [6], hj: the bias forces (wb_inverse_dynamics at nu' = 0); gam: plant_foot_bias;
// rb [6] = g_ext's base rows, rj = tau + g_ext of my joint (0 on the foot lane); on: my leg is flagged.
__device__ __forceinline__ void plant_solve(const WbLink &L, int leg, int c, const WbInertia &T, const double Fcol[6],
                                            const double Mleg[3], const double hb[6], double hj, const double gam[3],
                                            const double rb[6], double rj, bool on, PlantSolution &out) {
  const bool comp = c < 3, row_on = comp && on;
  const int myidx = 3 * leg + c;
  // ---- joint block of my leg, replicated in the quad
  double A[6], Ai[6];
  A[0] = quad_bc<0>(Mleg[0]); A[1] = quad_bc<0>(Mleg[1]); A[2] = quad_bc<0>(Mleg[2]);
  A[3] = quad_bc<1>(Mleg[1]); A[4] = quad_bc<1>(Mleg[2]); A[5] = quad_bc<2>(Mleg[2]);
  const bool okA = plant_inverse3(A, Ai);
  const double r0[3] = {Ai[0], Ai[1], Ai[2]}, r1[3] = {Ai[1], Ai[3], Ai[4]}, r2[3] = {Ai[2], Ai[4], Ai[5]};
  const double arow[3] = {pick3(r0, c), pick3(r1, c), pick3(r2, c)}; // column (= row) c of A^-1; 0 on the foot lane
  // ---- G = F A^-1, my column; interface order [force ; moment]
  const double Fi[6] = {Fcol[3], Fcol[4], Fcol[5], Fcol[0], Fcol[1], Fcol[2]};
  double G[6];
#pragma unroll
  for (int b = 0; b < 6; b++) G[b] = arow[0] * quad_bc<0>(Fi[b]) + arow[1] * quad_bc<1>(Fi[b]) + arow[2] * quad_bc<2>(Fi[b]);
  // ---- base Schur complement and its inverse.  M_bb = [[m 1, -[h]x], [[h]x, I]]
  double S[6][6];
  {
    const double m = T.m, hx = T.h[0], hy = T.h[1], hz = T.h[2];
    const double Mb[6][6] = {{m, 0.0, 0.0, 0.0, hz, -hy},      {0.0, m, 0.0, -hz, 0.0, hx},       {0.0, 0.0, m, hy, -hx, 0.0},
                             {0.0, -hz, hy, T.I[0], T.I[1], T.I[2]}, {hz, 0.0, -hx, T.I[1], T.I[3], T.I[4]}, {-hy, hx, 0.0, T.I[2], T.I[4], T.I[5]}};
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++) {
        S[a][b] = Mb[a][b] - row_sum(Fi[a] * G[b]); // (the foot lanes hold F = 0)
        S[b][a] = S[a][b];
      }
  }
  const bool okS = plant_inverse6(S);
  // ---- nu'_0 = M^-1 ([0 ; tau] + g_ext - h)
  const double bj = comp ? rj - hj : 0.0;
  const double yj = arow[0] * quad_bc<0>(bj) + arow[1] * quad_bc<1>(bj) + arow[2] * quad_bc<2>(bj);
  double bb[6], xb[6];
#pragma unroll
  for (int b = 0; b < 6; b++) bb[b] = (rb[b] - hb[b]) - row_sum(Fi[b] * yj);
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) acc += S[a][b] * bb[b];
    xb[a] = acc;
  }
  double xj = yj;
#pragma unroll
  for (int b = 0; b < 6; b++) xj -= G[b] * xb[b];
  // ---- my row of Js: [e_c , -[r]x row c | J_leg row c]; my lane's joint gives COLUMN c of J_leg (wholebody_kernel.hip)
  double jcol[3], jrow[3];
  {
    const double d[3] = {L.pf[0] - L.p[0], L.pf[1] - L.p[1], L.pf[2] - L.p[2]};
    double col[3];
    cross3(L.z, d, col);
#pragma unroll
    for (int a = 0; a < 3; a++) jcol[a] = row_on ? col[a] : 0.0;
    static_for<3>([&](auto K) {
      constexpr int k = K;
      const double v[3] = {quad_bc<k>(jcol[0]), quad_bc<k>(jcol[1]), quad_bc<k>(jcol[2])};
      jrow[k] = pick3(v, c);
    });
  }
  const double rx = L.pf[0], ry = L.pf[1], rz = L.pf[2];
  const double k3[3] = {0.0, -rz, ry}, k4[3] = {rz, 0.0, -rx}, k5[3] = {-ry, rx, 0.0};
  const double Jb[6] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, pick3(k3, c), pick3(k4, c), pick3(k5, c)};
  double E[6];
#pragma unroll
  for (int b = 0; b < 6; b++) {
    const double e = Jb[b] - (jrow[0] * quad_bc<0>(G[b]) + jrow[1] * quad_bc<1>(G[b]) + jrow[2] * quad_bc<2>(G[b]));
    E[b] = row_on ? e : 0.0;
  }
  // right-hand side of my row: -(gamma + Js nu'_0)
  double cv;
  {
    double acc = pick3(gam, c);
#pragma unroll
    for (int b = 0; b < 6; b++) acc += Jb[b] * xb[b];
    acc += jrow[0] * quad_bc<0>(xj) + jrow[1] * quad_bc<1>(xj) + jrow[2] * quad_bc<2>(xj);
    cv = row_on ? -acc : 0.0;
  }
  // ---- my row of Js M^-1 Js'
  double Wv[6];
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) acc += S[a][b] * E[b];
    Wv[a] = acc;
  }
  double H[12];
#pragma unroll
  for (int j = 0; j < 12; j++) H[j] = 0.0;
  static_for<12>([&](auto J) {
    constexpr int j = J;
    static_for<6>([&](auto Bq) { constexpr int b = Bq; fmac_bc<lane_of(j), j == 0>(H[j], E[b], Wv[b]); });
  });
  {
    // the leg's own block J_leg A^-1 J_leg'; an unflagged foot's rows are the identity's (f = 0 exactly, control flow uniform)
    double kk[3], D[3];
    kk[0] = jrow[0] * Ai[0] + jrow[1] * Ai[1] + jrow[2] * Ai[2];
    kk[1] = jrow[0] * Ai[1] + jrow[1] * Ai[3] + jrow[2] * Ai[4];
    kk[2] = jrow[0] * Ai[2] + jrow[1] * Ai[4] + jrow[2] * Ai[5];
    static_for<3>([&](auto K) {
      constexpr int k = K;
      const double dk = kk[0] * quad_bc<k>(jrow[0]) + kk[1] * quad_bc<k>(jrow[1]) + kk[2] * quad_bc<k>(jrow[2]);
      D[k] = row_on ? dk : ((comp && c == k) ? 1.0 : 0.0);
    });
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int k = 0; k < 3; k++) H[3 * l + k] += sel(leg == l, D[k], 0.0);
  }
  double H0[12];
#pragma unroll
  for (int j = 0; j < 12; j++) H0[j] = H[j];
  const bool okH = plant_inverse12(H, comp, myidx);
  // ---- f, with one residual pass on the matrix itself
  double f = plant_row_dot(H, cv);
  {
    const double res = cv - plant_row_dot(H0, f);
    f += plant_row_dot(H, res);
  }
  f = row_on ? f : 0.0;
  // ---- nu' = nu'_0 + M^-1 Js' f
  double sb[6];
#pragma unroll
  for (int b = 0; b < 6; b++) sb[b] = row_sum(Wv[b] * f);
  const double jt = jcol[0] * quad_bc<0>(f) + jcol[1] * quad_bc<1>(f) + jcol[2] * quad_bc<2>(f);
  double nuj = xj + (arow[0] * quad_bc<0>(jt) + arow[1] * quad_bc<1>(jt) + arow[2] * quad_bc<2>(jt));
#pragma unroll
  for (int b = 0; b < 6; b++) nuj -= G[b] * sb[b];
  bool finite = (f - f == 0.0) && (!comp || (nuj - nuj == 0.0));
#pragma unroll
  for (int b = 0; b < 6; b++) { out.nub[b] = xb[b] + sb[b]; finite = finite && (out.nub[b] - out.nub[b] == 0.0); }
  out.nuj = nuj;
  out.f = f;
  out.ok = !row_any(!(okA && okS && okH && finite));
}

// quat (x) exp(phi), normalised: the exact exponential map of the rotation vector phi (base coordinates), (w, x, y, z)
__device__ __forceinline__ void plant_quat_step(const double q[4], const double phi[3], double o[4]) {
  const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  double cw, k; // exp(phi) = (cos(t / 2), sin(t / 2) / t * phi)
  if (t2 < 1e-16) {
    cw = 1.0 - t2 * 0.125;
    k = 0.5 - t2 * (1.0 / 48.0);
  } else {
    const double t = sqrt(t2);
    double sh;
    sincos_reduced(0.5 * t, sh, cw);
    k = sh / t;
  }
  const double bx = k * phi[0], by = k * phi[1], bz = k * phi[2];
  const double w = q[0] * cw - q[1] * bx - q[2] * by - q[3] * bz;
  const double x = q[0] * bx + q[1] * cw + q[2] * bz - q[3] * by;
  const double y = q[0] * by - q[1] * bz + q[2] * cw + q[3] * bx;
  const double z = q[0] * bz + q[1] * by - q[2] * bx + q[3] * cw;
  const double n = sqrt((w * w + x * x) + (y * y + z * z));
  o[0] = w / n; o[1] = x / n; o[2] = y / n; o[3] = z / n;
}

} // namespace coop
} // namespace qlamd

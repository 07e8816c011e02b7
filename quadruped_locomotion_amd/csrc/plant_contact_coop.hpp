// The plant step with touchdown impacts and contact stabilisation (qlamd_wholebody_plant_step_batch): plant_coop.hpp's KKT
// system split into FACTOR ONCE, APPLY TWICE.  Lane layout as there: 16 lanes per robot, lane 4*leg + c.  Device-only.
//
// Everything that depends on q alone is a factor:
//     A_l^-1 (my column), G = F A^-1 (my column), S^-1 (replicated), E (my row), W = S^-1 E (my row),
//     H0 = Js M^-1 Js' (my row) and H = H0^-1 (my row, plant_inverse12)
// and the KKT system  M x - Js' y = [b ; j],  Js x = r  is then, for any right-hand side,
//     x_0 = M^-1 [b ; j],     y = H (r - Js x_0) with one residual pass through H0,     x = x_0 + M^-1 Js' y.
// The impact  M (nu+ - nu) = Js' p, Js nu+ = 0  is the apply with b = j = 0 and r = -Js nu (x = nu+ - nu, y = p); the step is the
// apply with the bias forces at nu+ and r = -gamma(q, nu+) - k_v Js nu+ (x = nu', y = f).
#pragma once

#include "plant_coop.hpp"

namespace qlamd {
namespace coop {

struct PlantFactors {
  double arow[3]; // column (= row) c of A^-1 of my leg; 0 on the foot lane
  double Fi[6];   // my joint's column of the base rows of M, interface order [force ; moment]; 0 on the foot lane
  double G[6];    // my column of F A^-1
  double Si[21];  // S^-1, upper triangle by rows, replicated
  double Wv[6];   // my row of S^-1 E'
  double H[12];   // my row of (Js M^-1 Js')^-1
  double H0[12];  // my row of Js M^-1 Js'
  bool ok;        // every pivot positive (my lane's view: plant_apply's caller folds it over the row)
};

// index of entry (a, b) of a symmetric 6 x 6 matrix in its upper triangle stored by rows
constexpr int plant_tri(int a, int b) { return a <= b ? a * 6 - a * (a - 1) / 2 + (b - a) : b * 6 - b * (b - 1) / 2 + (a - b); }

// o = S^-1 v from the stored triangle
__device__ __forceinline__ void plant_sinv_mul(const double Si[21], const double v[6], double o[6]) {
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) acc += Si[plant_tri(a, b)] * v[b];
    o[a] = acc;
  }
}

// The cheap parts of my row of Js, from L again wherever they are needed (they are not kept across the dynamics pass):
// jcol = column c of J_leg (my joint's; lanes c < 3 of a flagged leg, else 0), jrow = row c of J_leg, Jb = [e_c , -[r]x row c]
__device__ __forceinline__ void plant_js_row(const WbLink &L, int c, bool row_on, double jcol[3], double jrow[3], double Jb[6]) {
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
  const double rx = L.pf[0], ry = L.pf[1], rz = L.pf[2];
  const double k3[3] = {0.0, -rz, ry}, k4[3] = {rz, 0.0, -rx}, k5[3] = {-ry, rx, 0.0};
  Jb[0] = c == 0 ? 1.0 : 0.0; Jb[1] = c == 1 ? 1.0 : 0.0; Jb[2] = c == 2 ? 1.0 : 0.0;
  Jb[3] = pick3(k3, c); Jb[4] = pick3(k4, c); Jb[5] = pick3(k5, c);
}

// my row of Js nu: component c of my foot point's velocity in base coordinates, v + w x r + J_leg qd (nub = [v ; w], qd: my joint's
// rate); 0 off the flagged rows
__device__ __forceinline__ double plant_js_dot(const double Jb[6], const double jrow[3], bool row_on, const double nub[6], double qd) {
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < 6; b++) acc += Jb[b] * nub[b];
  acc += jrow[0] * quad_bc<0>(qd) + jrow[1] * quad_bc<1>(qd) + jrow[2] * quad_bc<2>(qd);
  return row_on ? acc : 0.0;
}

// The factors.  T, Fcol, Mleg: wb_crba's; on: my leg is flagged.  The arithmetic is plant_solve's, in its order.
__device__ __forceinline__ void plant_factor(const WbLink &L, int leg, int c, const WbInertia &T, const double Fcol[6],
                                             const double Mleg[3], bool on, PlantFactors &F) {
  const bool comp = c < 3, row_on = comp && on;
  const int myidx = 3 * leg + c;
  double A[6], Ai[6];
  A[0] = quad_bc<0>(Mleg[0]); A[1] = quad_bc<0>(Mleg[1]); A[2] = quad_bc<0>(Mleg[2]);
  A[3] = quad_bc<1>(Mleg[1]); A[4] = quad_bc<1>(Mleg[2]); A[5] = quad_bc<2>(Mleg[2]);
  const bool okA = plant_inverse3(A, Ai);
  const double r0[3] = {Ai[0], Ai[1], Ai[2]}, r1[3] = {Ai[1], Ai[3], Ai[4]}, r2[3] = {Ai[2], Ai[4], Ai[5]};
  F.arow[0] = pick3(r0, c); F.arow[1] = pick3(r1, c); F.arow[2] = pick3(r2, c);
  F.Fi[0] = Fcol[3]; F.Fi[1] = Fcol[4]; F.Fi[2] = Fcol[5]; F.Fi[3] = Fcol[0]; F.Fi[4] = Fcol[1]; F.Fi[5] = Fcol[2];
#pragma unroll
  for (int b = 0; b < 6; b++)
    F.G[b] = F.arow[0] * quad_bc<0>(F.Fi[b]) + F.arow[1] * quad_bc<1>(F.Fi[b]) + F.arow[2] * quad_bc<2>(F.Fi[b]);
  // base Schur complement and its inverse.  M_bb = [[m 1, -[h]x], [[h]x, I]]
  double S[6][6];
  {
    const double m = T.m, hx = T.h[0], hy = T.h[1], hz = T.h[2];
    const double Mb[6][6] = {{m, 0.0, 0.0, 0.0, hz, -hy},      {0.0, m, 0.0, -hz, 0.0, hx},       {0.0, 0.0, m, hy, -hx, 0.0},
                             {0.0, -hz, hy, T.I[0], T.I[1], T.I[2]}, {hz, 0.0, -hx, T.I[1], T.I[3], T.I[4]}, {-hy, hx, 0.0, T.I[2], T.I[4], T.I[5]}};
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++) {
        S[a][b] = Mb[a][b] - row_sum(F.Fi[a] * F.G[b]); // (the foot lanes hold F = 0)
        S[b][a] = S[a][b];
      }
  }
  const bool okS = plant_inverse6(S);
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) F.Si[plant_tri(a, b)] = S[a][b];
  // my row of Js after the joint elimination, and of S^-1 E'
  double jcol[3], jrow[3], Jb[6], E[6];
  plant_js_row(L, c, row_on, jcol, jrow, Jb);
#pragma unroll
  for (int b = 0; b < 6; b++) {
    const double e = Jb[b] - (jrow[0] * quad_bc<0>(F.G[b]) + jrow[1] * quad_bc<1>(F.G[b]) + jrow[2] * quad_bc<2>(F.G[b]));
    E[b] = row_on ? e : 0.0;
  }
  plant_sinv_mul(F.Si, E, F.Wv);
  // my row of Js M^-1 Js'
  double H[12];
#pragma unroll
  for (int j = 0; j < 12; j++) H[j] = 0.0;
  static_for<12>([&](auto J) {
    constexpr int j = J;
    static_for<6>([&](auto Bq) { constexpr int b = Bq; fmac_bc<lane_of(j), j == 0>(H[j], E[b], F.Wv[b]); });
  });
  {
    // the leg's own block J_leg A^-1 J_leg'; an unflagged foot's rows are the identity's (y = 0 exactly, control flow uniform)
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
#pragma unroll
  for (int j = 0; j < 12; j++) { F.H0[j] = H[j]; F.H[j] = H[j]; }
  const bool okH = plant_inverse12(F.H, comp, myidx);
  F.ok = okA && okS && okH;
}

struct PlantApplied {
  double xb[6]; // base rows of x, interface order [v ; w], replicated
  double xj;    // my joint's row of x (lanes c < 3)
  double y;     // my row of the multiplier (lanes c < 3 of a flagged leg; 0 elsewhere)
};

// The apply.  kForce: the right-hand side has a force part, b [6] (base rows) and j (my joint's row; anything on the foot lane);
// without it (the impact) x_0 = 0 and its arithmetic is not emitted.  r: my row of the constraint right-hand side (read on the
// flagged rows only).  jcol, jrow, Jb: plant_js_row's.
template <bool kForce>
__device__ __forceinline__ void plant_apply(const PlantFactors &F, int c, bool on, const double jcol[3], const double jrow[3],
                                            const double Jb[6], const double b[6], double j, double r, PlantApplied &out) {
  const bool comp = c < 3, row_on = comp && on;
  double xb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xj = 0.0, cv = row_on ? r : 0.0;
  if constexpr (kForce) {
    const double bj = comp ? j : 0.0;
    const double yj = F.arow[0] * quad_bc<0>(bj) + F.arow[1] * quad_bc<1>(bj) + F.arow[2] * quad_bc<2>(bj);
    double bb[6];
#pragma unroll
    for (int a = 0; a < 6; a++) bb[a] = b[a] - row_sum(F.Fi[a] * yj);
    plant_sinv_mul(F.Si, bb, xb);
    xj = yj;
#pragma unroll
    for (int a = 0; a < 6; a++) xj -= F.G[a] * xb[a];
    cv = row_on ? r - plant_js_dot(Jb, jrow, true, xb, xj) : 0.0;
  }
  // the multiplier, with one residual pass on the matrix itself
  double y = plant_row_dot(F.H, cv);
  {
    const double res = cv - plant_row_dot(F.H0, y);
    y += plant_row_dot(F.H, res);
  }
  y = row_on ? y : 0.0;
  // x = x_0 + M^-1 Js' y
  double sb[6];
#pragma unroll
  for (int a = 0; a < 6; a++) sb[a] = row_sum(F.Wv[a] * y);
  const double jt = jcol[0] * quad_bc<0>(y) + jcol[1] * quad_bc<1>(y) + jcol[2] * quad_bc<2>(y);
  xj += F.arow[0] * quad_bc<0>(jt) + F.arow[1] * quad_bc<1>(jt) + F.arow[2] * quad_bc<2>(jt);
#pragma unroll
  for (int a = 0; a < 6; a++) { xj -= F.G[a] * sb[a]; out.xb[a] = xb[a] + sb[a]; }
  out.xj = xj;
  out.y = y;
}

// whether my lane's part of an apply is finite
__device__ __forceinline__ bool plant_applied_finite(const PlantApplied &x, bool comp) {
  bool finite = (x.y - x.y == 0.0) && (!comp || (x.xj - x.xj == 0.0));
#pragma unroll
  for (int a = 0; a < 6; a++) finite = finite && (x.xb[a] - x.xb[a] == 0.0);
  return finite;
}

// QLAMD_CONTACT_PULLS | QLAMD_CONTACT_OUTSIDE_CONE of my leg from its force (fx, fy, fz replicated in the quad) and the unit
// normal n, both in base coordinates
__device__ __forceinline__ unsigned plant_contact_bits(const double f[3], const double n[3], double mu) {
  const double fn = f[0] * n[0] + f[1] * n[1] + f[2] * n[2];
  const double t[3] = {f[0] - fn * n[0], f[1] - fn * n[1], f[2] - fn * n[2]};
  const double ft = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  return (fn < 0.0 ? 1u : 0u) | (ft > mu * (fn > 0.0 ? fn : 0.0) ? 2u : 0u);
}

} // namespace coop
} // namespace qlamd

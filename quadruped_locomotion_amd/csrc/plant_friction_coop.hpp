// The plant step with friction (qlamd_wholebody_plant_step_friction_batch): plant_contact_coop.hpp's FACTOR ONCE, APPLY TWICE with
// the multiplier step  y = H (r - Js x_0)  replaced by the minimiser of the same quadratic over the friction pyramid,
//     y = argmin_{y in K}  1/2 y'H0 y - y'(r - Js x_0),
// which is force_qp_coop.hpp's QP with Gm = my row of H0, g0 = -(r - Js x_0), the leg's n, t1, t2, mu, f_min = 0, cold, without
// kTorque, and with H = H0^-1 handed in (plant_factor has it: one elimination for the impulse QP and the force QP together).
// An apply is therefore in two halves here, around the QP: plant_free (x_0 and the QP's linear term) and plant_lift
// (x = x_0 + M^-1 Js' y); their arithmetic is plant_apply's, in its order.  Lane layout as there.  Device-only.
#pragma once

#include "plant_contact_coop.hpp"
#include "force_qp_coop.hpp"

namespace qlamd {
namespace coop {

struct PlantFree {
  double xb[6]; // base rows of x_0, interface order [v ; w], replicated
  double xj;    // my joint's row of x_0 (lanes c < 3)
  double cv;    // my row of r - Js x_0 (lanes c < 3 of a flagged leg; 0 elsewhere)
};

// kForce, b, j, r, jrow, Jb: plant_apply's
template <bool kForce>
__device__ __forceinline__ void plant_free(const PlantFactors &F, int c, bool on, const double jrow[3], const double Jb[6],
                                           const double b[6], double j, double r, PlantFree &out) {
  const bool comp = c < 3, row_on = comp && on;
#pragma unroll
  for (int a = 0; a < 6; a++) out.xb[a] = 0.0;
  out.xj = 0.0;
  out.cv = row_on ? r : 0.0;
  if constexpr (kForce) {
    const double bj = comp ? j : 0.0;
    const double yj = F.arow[0] * quad_bc<0>(bj) + F.arow[1] * quad_bc<1>(bj) + F.arow[2] * quad_bc<2>(bj);
    double bb[6];
#pragma unroll
    for (int a = 0; a < 6; a++) bb[a] = b[a] - row_sum(F.Fi[a] * yj);
    plant_sinv_mul(F.Si, bb, out.xb);
    double xj = yj;
#pragma unroll
    for (int a = 0; a < 6; a++) xj -= F.G[a] * out.xb[a];
    out.xj = xj;
    out.cv = row_on ? r - plant_js_dot(Jb, jrow, true, out.xb, xj) : 0.0;
  }
}

// x = x_0 + M^-1 Js' y.  y: my row of the multiplier (0 off the flagged rows); jcol: plant_js_row's
__device__ __forceinline__ void plant_lift(const PlantFactors &F, const double jcol[3], double y, const PlantFree &x0,
                                           PlantApplied &out) {
  double sb[6];
#pragma unroll
  for (int a = 0; a < 6; a++) sb[a] = row_sum(F.Wv[a] * y);
  const double jt = jcol[0] * quad_bc<0>(y) + jcol[1] * quad_bc<1>(y) + jcol[2] * quad_bc<2>(y);
  double xj = x0.xj + (F.arow[0] * quad_bc<0>(jt) + F.arow[1] * quad_bc<1>(jt) + F.arow[2] * quad_bc<2>(jt));
#pragma unroll
  for (int a = 0; a < 6; a++) { xj -= F.G[a] * sb[a]; out.xb[a] = x0.xb[a] + sb[a]; }
  out.xj = xj;
  out.y = y;
}

// The pyramid of my leg in base coordinates, by the control step's rule (wholebody_kernel.hip): t1 = normalise(n x y_B),
// t2 = normalise(n x t1), y_B = R' e_y.  nB: the unit normal.  Returns whether the tangents are finite (a normal parallel to y_B has none).
__device__ __forceinline__ bool plant_pyramid(const double Rm[9], const double nB[3], int c, double mu, ForceQp &Q) {
  const double ey[3] = {0.0, 1.0, 0.0};
  double yB[3];
  irot(Rm, ey, yB);
#pragma unroll
  for (int a = 0; a < 3; a++) Q.nb[a] = nB[a];
  cross3(Q.nb, yB, Q.t1);
  double nn = rsqrt_nr(dot3(Q.t1, Q.t1));
  Q.t1[0] *= nn; Q.t1[1] *= nn; Q.t1[2] *= nn;
  cross3(Q.nb, Q.t1, Q.t2);
  nn = rsqrt_nr(dot3(Q.t2, Q.t2));
  Q.t2[0] *= nn; Q.t2[1] *= nn; Q.t2[2] *= nn;
  Q.myn = pick3(Q.nb, c); Q.myt1 = pick3(Q.t1, c); Q.myt2 = pick3(Q.t2, c);
  Q.mu = mu; Q.f_min = 0.0;
  // (not `x - x == 0`: the tangents are products, and under the build's contraction of a * b - a * b into fma(a, b, -(a * b)) that
  // difference is the product's rounding error)
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; a++) finite = finite && __builtin_isfinite(Q.t1[a]) && __builtin_isfinite(Q.t2[a]) && __builtin_isfinite(nB[a]);
  return finite;
}

// One QP over the pyramid.  Q: plant_pyramid's, with on, comp, nS set; Gm = F.H0's row, g0 = my entry of the linear term.
// y: my component of the minimiser; set: the final working set (bit 5 leg + kind; kinds as in force_qp_coop.hpp).
__device__ __forceinline__ int plant_cone_qp(ForceQp &Q, const PlantFactors &F, bool bad, double g0, double *lds_row, double *lds_nrm,
                                             double &y, int &iters, unsigned &set) {
#pragma unroll
  for (int j = 0; j < 12; j++) Q.Gm[j] = F.H0[j];
  Q.g0 = g0;
  unsigned long long ws = 0ull;
  const int st = force_qp_coop<false, false, 4, true, true>(Q, lds_row, lds_nrm, y, iters, &ws, F.H, bad);
  set = (unsigned)ws;
  return st;
}

// QLAMD_CONTACT_SEPARATING | QLAMD_CONTACT_SLIDING of leg `leg` from the final working set of the force QP.  The row n.f >= 0
// holds with equality when it is in the set, and also when two opposite faces are (mu n.f + t.f = mu n.f - t.f = 0 gives n.f = 0):
// at the apex five rows of rank three are active, and which three the method ends with is the path's choice.
__device__ __forceinline__ unsigned plant_friction_bits(unsigned set, int leg) {
  const unsigned rows = (set >> (5 * leg)) & 31u;
  const bool apex = (rows & 1u) != 0u || (rows & 6u) == 6u || (rows & 24u) == 24u;
  return apex ? 8u : ((rows & 30u) != 0u ? 16u : 0u);
}

} // namespace coop
} // namespace qlamd

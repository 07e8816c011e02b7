// TEST INFRASTRUCTURE ONLY -- never part of the product library.
//
// Compiles the per-leg arithmetic of the swing-foot task (csrc/swing_task_core.hpp) for the HOST with g++, as mirror.cpp does
// for the other cores, so that tests/test_swing_task_cpu.py can check it against tests/swing_task_reference.py without a GPU.
// The robot's failure rule around the four legs is the one of swing_task_kernel.hip, restated.
#include <cstdint>

#include "params_build.hpp"
#include "swing_task_core.hpp"

using namespace qlamd;

// scalars [10]: the doubles of qlamd_swing_task in the struct's order.  ades, stance, normal, support, events, ref: or NULL.
extern "C" void mirror_swing_task_batch_model(const qlamd_robot_model *model, int64_t B, const double *q, const double *qd,
                                              const double *quat, const double *linvel, const double *angvel, const double *pos,
                                              const double *ades, const uint8_t *stance, const uint8_t *want,
                                              const double *foothold, const double *normal, const double *scalars, int keep,
                                              double *state, double *qdd, uint8_t *support, uint8_t *events, double *ref,
                                              int32_t *status) {
  qlamd_balance_params prm;
  default_balance_params(&prm);
  DeviceParams P;
  build_device_params(prm, *model, &P);
  const SwingRule rule = swing_rule(scalars[0], scalars[1], scalars[2], scalars[3], scalars[4], scalars[5], scalars[6], scalars[7],
                                    scalars[8], scalars[9]);
  for (int64_t i = 0; i < B; i++) {
    double Rm[9], a6[6] = {0, 0, 0, 0, 0, 0}, lq[4][3], lref[4][9], lnext[4][4];
    bool lsup[4], ok = true;
    unsigned lev[4];
    quat_to_matrix(quat + 4 * i, Rm);
    for (int a = 0; a < 6 && ades; a++) a6[a] = ades[6 * i + a];
    for (int a = 0; a < 4; a++) ok = ok && cu_finite(quat[4 * i + a]);
    for (int l = 0; l < 4; l++) {
      const int64_t t = 4 * i + l;
      const double ez[3] = {0.0, 0.0, 1.0};
      ok = swing_task_leg(P.legtab + kTabPerLeg * l, rule, q + 3 * t, qd + 3 * t, Rm, pos + 3 * i, linvel + 3 * i, angvel + 3 * i, a6,
                          want[t] != 0, stance && stance[t] != 0, state + 4 * t, foothold + 3 * t, normal ? normal + 3 * t : ez, lq[l],
                          lref[l], lnext[l], lsup[l], lev[l]) && ok;
    }
    status[i] = ok ? kStatusOk : kStatusNotPd;
    if (!ok && keep) continue;
    for (int l = 0; l < 4; l++) {
      const int64_t t = 4 * i + l;
      if (support) support[t] = ok ? (lsup[l] ? 1 : 0) : (stance ? stance[t] : 0);
      if (events) events[t] = ok ? (uint8_t)lev[l] : 0;
      for (int a = 0; a < 3; a++) qdd[3 * t + a] = ok ? lq[l][a] : 0.0;
      for (int a = 0; a < 9 && ref; a++) ref[9 * t + a] = ok ? lref[l][a] : 0.0;
      for (int a = 0; a < 4 && ok; a++) state[4 * t + a] = lnext[l][a];
    }
  }
}

// A thin caller of host/qlamd/robot_params.hpp: a friction sweep over a batch, from C++.  Fills the records on the host (no
// device needed), prints what the fold made of them, and -- with "--solve" and a GPU -- solves a standing batch in which every
// robot has its own friction coefficient, payload and torque limit through qlamd_balance_solve_robot_params_batch.
//   robot_params_demo [robots] [--solve]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qlamd/robot_params.hpp"

int main(int argc, char **argv) {
  int64_t B = 8;
  bool solve = false;
  for (int a = 1; a < argc; a++) {
    if (!std::strcmp(argv[a], "--solve")) solve = true;
    else B = std::atoll(argv[a]);
  }
  if (B < 1) return 2;
  qlamd_balance_params def;
  qlamd_balance_default_params(&def);
  qlamd::host::RobotParamsBatch rp(B, def);
  for (int64_t i = 0; i < B; i++) {
    qlamd_balance_params p = def;
    const double t = B > 1 ? (double)i / (double)(B - 1) : 0.0;
    p.friction = 0.3 + 0.6 * t;       // the sweep
    p.torso_mass = 27.0 + 10.0 * t;   // a payload
    p.torque_limit = 300.0 - 200.0 * t;
    rp.set(i, p);
  }
  std::printf("records %lld bytes %zu\n", (long long)rp.size(), rp.bytes());
  std::printf("first friction %.17g gravity_force_scale %.17g torque_limit %.17g\n", rp[0].friction, rp[0].gravity_force_scale, rp[0].torque_limit);
  std::printf("last friction %.17g gravity_force_scale %.17g torque_limit %.17g\n", rp[B - 1].friction, rp[B - 1].gravity_force_scale,
              rp[B - 1].torque_limit);
  if (!solve) return 0;

  qlamd_context *ctx = nullptr;
  int rc = qlamd_context_create(&def, nullptr, 0, &ctx);
  if (rc != QLAMD_OK) { std::printf("context: %s\n", qlamd_strerror(rc)); return 1; }
  // every robot standing in the nominal pose, on its desired pose
  std::vector<double> q(12 * B), pos(3 * B, 0.0), quat(4 * B, 0.0), zero3(3 * B, 0.0), tau(12 * B), grf(12 * B);
  std::vector<uint8_t> support(4 * B, 1);
  std::vector<int32_t> status(B, -1);
  for (int64_t i = 0; i < B; i++) {
    for (int l = 0; l < 4; l++) { q[12 * i + 3 * l] = 0.0; q[12 * i + 3 * l + 1] = 0.75; q[12 * i + 3 * l + 2] = -1.5; }
    pos[3 * i + 2] = 0.46;
    quat[4 * i] = 1.0;
  }
  qlamd_state_batch in;
  std::memset(&in, 0, sizeof(in));
  in.joint_position = q.data(); in.base_position = pos.data(); in.base_orientation = quat.data();
  in.base_linear_velocity = zero3.data(); in.base_angular_velocity = zero3.data();
  in.desired_position = pos.data(); in.desired_orientation = quat.data();
  in.desired_linear_velocity = zero3.data(); in.desired_angular_velocity = zero3.data();
  in.support_leg = support.data();
  rc = qlamd_balance_solve_robot_params_batch(ctx, &in, rp.data(), B, nullptr, tau.data(), grf.data(), status.data(), QLAMD_MEM_HOST,
                                              nullptr);
  if (rc != QLAMD_OK) { std::printf("solve: %s\n", qlamd_strerror(rc)); qlamd_context_destroy(ctx); return 1; }
  double fz_first = 0.0, fz_last = 0.0;
  for (int l = 0; l < 4; l++) { fz_first += grf[3 * l + 2]; fz_last += grf[12 * (B - 1) + 3 * l + 2]; }
  std::printf("status %d %d  sum of vertical contact forces: first %.6f last %.6f\n", status[0], status[B - 1], fz_first, fz_last);
  qlamd_context_destroy(ctx);
  return 0;
}

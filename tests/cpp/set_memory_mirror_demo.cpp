// RosBalanceController::setSetMemory -- the whole tick's working set per support set in the one-robot mirror -- on a gait:
// argv[1] holds the serialised /desired_robot_state messages of consecutive ticks, argv[2] bytes each (one publisher's layout);
// argv[3] one hex digit per tick: the contact sensors (bit l = leg l).  Three controllers tick through them side by side: a
// cold one, one with setWarmStart (the one-word set) and one with setSetMemory (the table).  Prints every tick's 12 efforts of
// each; the test compares.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "balance_controller/RosBalanceController.hpp"

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  std::vector<uint8_t> blob;
  if (FILE *fp = std::fopen(argv[1], "rb")) {
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), fp)) > 0) blob.insert(blob.end(), buf, buf + n);
    std::fclose(fp);
  }
  const size_t len = (size_t)std::atol(argv[2]), ticks = std::strlen(argv[3]);
  if (len == 0 || blob.size() != len * ticks) return 2;
  qlamd_balance_params params;
  qlamd_balance_default_params(&params);
  double q[12], qd[12];
  for (int l = 0; l < 4; ++l) { q[3 * l] = 0.05 * (l - 1.5); q[3 * l + 1] = 0.75; q[3 * l + 2] = -1.5; }
  for (int i = 0; i < 12; ++i) qd[i] = 0.1 * std::sin(1.0 + i);
  const double yaw = 0.5;
  const double orientation[4] = {std::cos(yaw / 2), 0.0, 0.0, std::sin(yaw / 2)};
  const double position[3] = {0.0, 0.0, 0.2}, linvel[3] = {0.01, -0.02, 0.0}, angvel[3] = {0.0, 0.01, 0.02};
  bool contact[4] = {true, true, true, true};
  double effort[3][12] = {{0}};
  balance_controller::RobotStateHandleData hw[3];
  balance_controller::RosBalanceController c[3];
  for (int k = 0; k < 3; ++k) {
    hw[k].orientation = orientation; hw[k].position = position; hw[k].linear_velocity = linvel; hw[k].angular_velocity = angvel;
    hw[k].joint_position_read = q; hw[k].joint_velocity_read = qd; hw[k].joint_effort_write = effort[k]; hw[k].foot_contact = contact;
    if (!c[k].init(hw[k], params, 0)) { std::printf("init_failed 1\n"); return 3; }
  }
  c[1].setWarmStart(true);
  c[2].setSetMemory(true);
  const char *name[3] = {"cold", "word", "table"};
  for (size_t t = 0; t < ticks; ++t) {
    const char d = argv[3][t];
    const unsigned mask = (unsigned)(d >= 'a' ? d - 'a' + 10 : d - '0');
    bool touching[4];
    for (int l = 0; l < 4; ++l) touching[l] = (mask >> l) & 1u;
    for (int k = 0; k < 3; ++k) {
      c[k].footContactsCallback(touching);
      if (!c[k].tick(blob.data() + t * len, len, 0.0025)) return 10 + k;
      std::printf("%s_%zu", name[k], t);
      for (int i = 0; i < 12; ++i) std::printf(" %.17g", effort[k][i]);
      std::printf("\n");
    }
  }
  return 0;
}

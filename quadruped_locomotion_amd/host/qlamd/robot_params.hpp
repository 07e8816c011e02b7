// Controller parameters that differ per robot, from C++: an owning array of the folded records that
// qlamd_balance_solve_robot_params_batch takes (one qlamd_robot_params of 32 doubles per robot), filled from
// qlamd_balance_params by the library's own fold (qlamd_robot_params_fill -- the arithmetic qlamd_context_create applies to a
// context's parameters, so a record filled from them holds the context's values bit for bit).  Needs qlamd.h only; the fill
// is a host function and needs no device.  tests/cpp/robot_params_demo.cpp is a thin caller; INTEGRATION.md shows the loop.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "qlamd.h"

namespace qlamd {
namespace host {

static_assert(sizeof(qlamd_robot_params) == QLAMD_ROBOT_PARAMS_DOUBLES * sizeof(double), "a record is 32 doubles");

// count parameter structs -> count records; the return code of qlamd_robot_params_fill
inline int fill(const qlamd_balance_params *params, int64_t count, qlamd_robot_params *out) {
  return qlamd_robot_params_fill(params, count, out);
}

// The records of a batch, on the host: every robot starts with `all` (e.g. the context's parameters), set(i, p) gives robot i
// its own.  data() is what a QLAMD_MEM_HOST call takes as robot_params, and what a caller copies to the device for a
// QLAMD_MEM_DEVICE call (bytes() bytes, 16-byte aligned there).  params[i].gravity is not part of a record: gravity is the
// context's.
class RobotParamsBatch {
 public:
  RobotParamsBatch(int64_t batch, const qlamd_balance_params &all) : rec_((size_t)batch) {
    qlamd_robot_params r;
    if (fill(&all, 1, &r) != QLAMD_OK) throw std::invalid_argument("qlamd_robot_params_fill");
    for (auto &x : rec_) x = r;
  }
  void set(int64_t robot, const qlamd_balance_params &p) {
    if (fill(&p, 1, &rec_.at((size_t)robot)) != QLAMD_OK) throw std::invalid_argument("qlamd_robot_params_fill");
  }
  qlamd_robot_params &operator[](int64_t robot) { return rec_.at((size_t)robot); }
  const qlamd_robot_params &operator[](int64_t robot) const { return rec_.at((size_t)robot); }
  const qlamd_robot_params *data() const { return rec_.data(); }
  int64_t size() const { return (int64_t)rec_.size(); }
  size_t bytes() const { return rec_.size() * sizeof(qlamd_robot_params); }

 private:
  std::vector<qlamd_robot_params> rec_;
};

} // namespace host
} // namespace qlamd

// Which form of the lane-cooperative balance kernel a launch takes, decided ONCE and as data: balance_launch (balance_kernel.hip)
// asks here, and uses the answer for the next order's writer, for the shadow wavefronts and for the kernel it picks.  Needs
// nothing but the public header, so that a host program can check the decision against a table (tests/cpp/launch_form_check.cpp).
#pragma once

#include <stdint.h>

#include "qlamd.h"

#ifndef QLAMD_THROUGHPUT_BATCH
#define QLAMD_THROUGHPUT_BATCH 16384 // robots from which the three-wavefront form of the balance kernel runs
#endif
#ifndef QLAMD_THREE_WAVE_WARM_BATCH
// ... of the warm-started kernel: later, because its two-wavefront form installs by rounds and lets robots without a set build
// one by rounds, which the 168 registers of the other form have no room for (trot, placed + warm loop, us per step, two- against
// three-wavefront form: 16 384 robots 30.0 / 32.6, 20 480: 33.6 / 34.3, 24 576: 37.9 / 37.1, 32 768: 45.6 / 42.8, 65 536:
// 76.7 / 70.5 -- profiles/r6/ab_three_wave_threshold.txt)
#define QLAMD_THREE_WAVE_WARM_BATCH 22528
#endif

namespace qlamd {
namespace rt {

struct LaunchForm {
  bool per_leg; // per-leg surface normals from the caller: always two wavefronts
  int waves;    // wavefronts per SIMD the kernel is built for: 2 (at most 256 registers) or 3 (168; large batches)
  bool placed;  // the kernel reads a robot order and carries the 6-variable form and the shadow wavefronts
  bool warm;    // ... and starts every QP from a working set (then placed)
  bool table;   // ... taken from the table of four (then warm): balance_table_kernel
};
// warm: the call hands in or asks for working sets; table: it has a table; placed: it has any other member of a placement
inline LaunchForm balance_launch_form(bool per_leg_normals, int64_t batch, bool warm, bool table, bool placed) {
  const bool w = warm || table;
  const int waves = (!per_leg_normals && batch >= (w ? QLAMD_THREE_WAVE_WARM_BATCH : QLAMD_THROUGHPUT_BATCH)) ? 3 : 2;
  return LaunchForm{per_leg_normals, waves, placed || w, w, table};
}

} // namespace rt
} // namespace qlamd

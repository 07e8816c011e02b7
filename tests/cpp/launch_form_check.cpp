// The launch form of the balance step (quadruped_locomotion_amd/csrc/launch_form.hpp) against a table written out by hand from
// the selection balance_launch made before the form was a function: which kernel family (plain, placed, warm, table), two or
// three wavefronts per SIMD.  Includes nothing but that header; no GPU.  Exit status 0: every row agrees.
#include "launch_form.hpp"

#include <stdio.h>

using qlamd::rt::LaunchForm;
using qlamd::rt::balance_launch_form;

namespace {
enum Kind { kPlain, kPlaced, kWarm, kTable };
const char *const kKindName[] = {"plain", "placed", "warm", "table"};
struct Row { long long batch; Kind kind; bool normals; int waves; };
// Without per-leg normals: three wavefronts from 16 384 robots (QLAMD_THROUGHPUT_BATCH), with a warm start -- a working set or
// the table -- from 22 528 (QLAMD_THREE_WAVE_WARM_BATCH).  With per-leg normals: always two.
const Row kRows[] = {
    {4, kPlain, false, 2},     {4, kPlaced, false, 2},     {4, kWarm, false, 2},     {4, kTable, false, 2},
    {16383, kPlain, false, 2}, {16383, kPlaced, false, 2}, {16383, kWarm, false, 2}, {16383, kTable, false, 2},
    {16384, kPlain, false, 3}, {16384, kPlaced, false, 3}, {16384, kWarm, false, 2}, {16384, kTable, false, 2},
    {22527, kPlain, false, 3}, {22527, kPlaced, false, 3}, {22527, kWarm, false, 2}, {22527, kTable, false, 2},
    {22528, kPlain, false, 3}, {22528, kPlaced, false, 3}, {22528, kWarm, false, 3}, {22528, kTable, false, 3},
    {4, kPlain, true, 2},      {4, kPlaced, true, 2},      {4, kWarm, true, 2},      {4, kTable, true, 2},
    {16383, kPlain, true, 2},  {16383, kPlaced, true, 2},  {16383, kWarm, true, 2},  {16383, kTable, true, 2},
    {16384, kPlain, true, 2},  {16384, kPlaced, true, 2},  {16384, kWarm, true, 2},  {16384, kTable, true, 2},
    {22527, kPlain, true, 2},  {22527, kPlaced, true, 2},  {22527, kWarm, true, 2},  {22527, kTable, true, 2},
    {22528, kPlain, true, 2},  {22528, kPlaced, true, 2},  {22528, kWarm, true, 2},  {22528, kTable, true, 2},
};
} // namespace

int main() {
  static_assert(QLAMD_THROUGHPUT_BATCH == 16384 && QLAMD_THREE_WAVE_WARM_BATCH == 22528, "the table below is written for these");
  int bad = 0;
  for (const Row &r : kRows) {
    // the call as balance_launch sees it: a placed call has a robot order; a warm call working sets (and no order of its own:
    // the form has to make it placed); a table call only the table (the form has to make it warm and placed)
    const LaunchForm f = balance_launch_form(r.normals, r.batch, r.kind == kWarm, r.kind == kTable, r.kind == kPlaced);
    const bool ok = f.per_leg == r.normals && f.waves == r.waves && f.placed == (r.kind != kPlain) && f.warm == (r.kind >= kWarm) &&
                    f.table == (r.kind == kTable);
    if (!ok) {
      bad++;
      printf("batch %lld %s normals %d: want waves %d, got per_leg %d waves %d placed %d warm %d table %d\n", r.batch, kKindName[r.kind],
             (int)r.normals, r.waves, (int)f.per_leg, f.waves, (int)f.placed, (int)f.warm, (int)f.table);
    }
  }
  printf("rows %d bad %d\n", (int)(sizeof(kRows) / sizeof(kRows[0])), bad);
  return bad ? 1 : 0;
}

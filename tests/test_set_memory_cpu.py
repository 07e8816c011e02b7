"""qlamd_placement::set_memory without a GPU: the slot table, the structure's layout against the C header, and the premise --
a robot that remembers, per support set, the set it ended with the last time it stood on these legs finds a set that is worth
starting from (tools/experiments/set_recall_model.py, the oracle alone)."""
import ctypes as C
import importlib.util
import os
import subprocess

from conftest import ROOT
from quadruped_locomotion_amd import capi


def test_the_slot_of_every_support_mask():
    # LF = bit 0, RF = 1, RH = 2, LH = 3: the trot's two diagonals, all four legs, one shared slot for everything else
    want = {0b0101: 0, 0b1010: 1, 0b1111: 2}
    for mask in range(16):
        assert capi.set_memory_slot(mask) == want.get(mask, 3), mask
    assert capi.set_memory_slot(0x10 | 0b0101) == 0     # (bits above the four legs are ignored)


def test_the_placement_structure_is_the_headers(tmp_path):
    assert capi.Placement._fields_[-1][0] == "set_memory"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qlamd.h"\n'
                   "int main(void) {\n"
                   "  const qlamd_placement old_style = {NULL, NULL, NULL, NULL, QLAMD_PLACEMENT_AUTO, NULL, NULL};\n"
                   '  printf("%zu %zu %d", sizeof(qlamd_placement), offsetof(qlamd_placement, set_memory), old_style.set_memory == NULL);\n'
                   "  for (unsigned m = 0; m < 16; m++) printf(\" %u\", QLAMD_SET_MEMORY_SLOT(m));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert int(out[0]) == C.sizeof(capi.Placement)
    assert int(out[1]) == capi.Placement.set_memory.offset == C.sizeof(capi.Placement) - C.sizeof(C.c_void_p)
    assert out[2] == "1"                                 # an initialiser written before the member existed leaves it NULL
    assert [int(x) for x in out[3:]] == [capi.set_memory_slot(m) for m in range(16)]   # the header's macro is the library's table


def test_the_remembered_set_is_worth_starting_from(oracle):
    """The premise of the table, on the size the issue was argued with (384 robots, 760 ticks of a trot, default seed; the
    oracle alone gives 0.669 exact and 0.61 of 5.18 rows): over the robot-ticks with a support switch from tick 400 on, the set
    remembered under the new support set is exactly the final set for more than half of them, and differs from it by less than
    half the rows such a robot would otherwise have to install.  Guards the premise and the trajectory generator, not the kernel."""
    spec = importlib.util.spec_from_file_location("set_recall_model", os.path.join(ROOT, "tools", "experiments", "set_recall_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    r = model.run(robots=384, ticks=760, from_tick=400, threads=8)
    print(r)
    assert r["switches"] > 1000
    assert r["exact"] > 0.5, r
    assert r["mean_diff"] < 0.5 * r["mean_size"], r

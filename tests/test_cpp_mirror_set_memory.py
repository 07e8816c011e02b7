"""RosBalanceController::setSetMemory (the whole tick's working set per support set in the one-robot C++ mirror, a host-memory tick
of batch 1 through the pinned staging slab) on a gait: a trot's support sets in turn, each one visited again, against the cold
mirror and the one-word mirror on the same messages."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from quadruped_locomotion_amd import synth

BIN = os.path.join(ROOT, "tests", "cpp", "set_memory_mirror_demo")
MASKS = "ff55ffaaff55ffaaff55"      # contact sensors = support flags per tick: all four, {LF, RH}, all four, {RF, LH}, ... twice over


def build_demo():
    from quadruped_locomotion_amd import build
    build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "quadruped_locomotion_amd", "host"), "-o", BIN,
                           os.path.join(ROOT, "tests", "cpp", "set_memory_mirror_demo.cpp"),
                           "-L" + os.path.join(ROOT, "quadruped_locomotion_amd"), "-lqlamd",
                           "-Wl,-rpath," + os.path.join(ROOT, "quadruped_locomotion_amd")])


def test_the_demo_builds():
    build_demo()


@pytest.mark.gpu
def test_the_table_mirror_ticks_a_gait_like_the_cold_mirror(tmp_path):
    build_demo()
    T = len(MASKS)
    masks = np.array([int(c, 16) for c in MASKS])
    support = ((masks[:, None] >> np.arange(4)) & 1).astype(np.uint8)
    rng = np.random.default_rng(4)
    mt = synth.MessageTemplate(["footstep"] * 4)
    f = {k: np.tile(rng.normal(size=(1, n)), (T, 1)) for k, n in mt.DOUBLES}
    yaw = 0.5
    f["des_pos"] = np.tile([[0.0, 0.0, 0.3]], (T, 1)) + 0.002 * np.arange(T)[:, None]
    f["des_quat"] = np.tile([[np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]], (T, 1))
    f["des_linvel"] = np.tile([[0.3, -0.2, 0.0]], (T, 1))       # a horizontal demand: friction rows in the working set
    f["des_angvel"] = np.zeros((T, 3))
    f["phase"] = np.full((T, 4), 0.3)
    blob, off = mt.pack(dict(f, support_leg=support))
    path = tmp_path / "gait.bin"
    path.write_bytes(blob.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    p = subprocess.run([BIN, str(path), str(int(off[1])), MASKS], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-400:])
    out = {}
    for line in p.stdout.splitlines():
        k, *v = line.split()
        out[k] = np.array([float(x) for x in v])
    worst = 0.0
    for t in range(T):
        for other in ("word", "table"):
            worst = max(worst, float(np.abs(out["%s_%d" % (other, t)] - out["cold_%d" % t]).max()))
    print("mirror, %d ticks of a gait: worst |dtau| against the cold mirror %.2e" % (T, worst))
    assert worst < 1e-7                                         # include/qlamd.h: any warm start against the cold start
    assert np.abs(out["cold_%d" % (T - 1)]).max() > 1.0

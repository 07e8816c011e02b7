#!/usr/bin/env python3
"""Does the trajectory of tests/test_tick_set_memory_gpu.py make the tick's own `support` output switch often enough?  The
oracle chain alone (oracle.full_tick, per-robot state carried along, no GPU) over the test's inputs: counts the robot-ticks from
--from-tick on whose support mask differs from the previous tick's and under whose mask the robot ended an earlier tick with
status OK -- the robot-ticks the test's assertions (a) and (b) run over; the test needs 1000 of them at 1024 robots -- and on how
many robot-ticks `support` is what the message's flags say.

usage: tick_support_switches.py [--robots 128] [--ticks 760] [--from-tick 400]"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(robots=128, ticks=760, from_tick=400):
    from oracle import oracle as O
    spec = importlib.util.spec_from_file_location("tick_test", os.path.join(ROOT, "tests", "test_tick_set_memory_gpu.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)                      # (the inputs are the test's own generator: nothing to keep in step)
    B = robots
    states = [O.new_tick_state() for _ in range(B)]
    ended_ok, prev = np.zeros((B, 16), bool), None
    n = follows = failed = 0
    for k, (s, tin) in enumerate(tt.tick_inputs(B, "trot", ticks)):
        off, st, sup = tin["offsets"], np.zeros(B, int), np.zeros((B, 4), np.uint8)
        for b in range(B):
            st[b], _, _ = O.full_tick(states[b], bytes(tin["messages"][off[b]:off[b + 1]]), tin["joint_position"][b], tin["joint_velocity"][b],
                                      tin["joint_velocity_oldest"][b], tin["base_position"][b], tin["base_orientation"][b],
                                      tin["base_linear_velocity"][b], tin["base_angular_velocity"][b], tin["contact"][b], tt.PERIOD)
            sup[b] = states[b].support[:]
        mask = tt.support_mask(sup)
        failed += int((st != 0).sum())
        follows += int((mask == tt.support_mask(s["stance"])).sum())
        if prev is not None and k >= from_tick:
            n += int(((mask != prev) & ended_ok[np.arange(B), mask]).sum())
        ended_ok[np.arange(B)[st == 0], mask[st == 0]] = True
        prev = mask
    return dict(robots=B, ticks=ticks, recalled_switches=n, per_robot=n / B, follows=follows, robot_ticks=B * ticks, failed=failed)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=128)
    ap.add_argument("--ticks", type=int, default=760)
    ap.add_argument("--from-tick", type=int, default=400)
    a = ap.parse_args()
    print(run(a.robots, a.ticks, a.from_tick))

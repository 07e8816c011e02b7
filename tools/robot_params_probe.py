#!/usr/bin/env python3
"""What controller parameters per robot cost in time: qlamd_balance_solve_robot_params_batch, every record filled from the
context's own parameters (so both entries compute the same thing, bit for bit), against qlamd_balance_solve_placed_batch -- same
process, same context, same resident inputs, the two entries' regions interleaved (A B A B ...), so that drift of the device's
clocks hits both alike.

Workloads (4096 robots by default):
  static warm  the loop over a static trajectory ("survey" errors), warm-started from the one-word array updated in place
  trot table   the loop over a trot trajectory, warm-started from the table (set_memory)
  cold plain   one state solved cold, no placement
A region is --ticks steps between two events with nothing but launches inside (the states of all ticks are resident); the first
region of each entry is its warm-up and is not reported.  Per workload and entry: every sample in us per step, the median and
the spread, and the ratio of the medians.

usage: robot_params_probe.py [--batch 4096] [--ticks 128] [--repeats 5] [--out file]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from quadruped_locomotion_amd import capi, synth
    B, T = a.batch, a.ticks
    ctx = capi.Context(device=0)
    stream = torch.cuda.current_stream().cuda_stream
    dev = dict(device="cuda:0")
    records = torch.from_numpy(np.ascontiguousarray(np.repeat(capi.robot_params_fill(ctx.params), B, axis=0))).to("cuda:0")
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    def fresh():
        return dict(ws=torch.zeros(B, dtype=torch.int32, **dev), mem=torch.zeros(B, 4, dtype=torch.int32, **dev),
                    tau=torch.zeros(B, 12, dtype=torch.float64, **dev), st=torch.zeros(B, dtype=torch.int32, **dev))

    def step(per_robot, d, z, warm):
        kw = dict(stream=stream)
        if warm == "one word":
            kw.update(prev_working_set=z["ws"], working_set=z["ws"])
        elif warm == "table":
            kw.update(set_memory=z["mem"])
        if per_robot:
            ctx.balance_solve_robot_params_device(d, records, z["tau"], None, z["st"], **kw)
        else:
            ctx.balance_solve_placed_device(d, z["tau"], None, z["st"], **kw)

    def region(per_robot, dstates, z, warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(T):
            step(per_robot, dstates[k % len(dstates)], z, warm)
        e1.record()
        torch.cuda.synchronize()
        assert (z["st"] == 0).all()
        return e0.elapsed_time(e1) * 1e3 / T

    def workload(name, dstates, warm):
        z = {False: fresh(), True: fresh()}
        samples = {False: [], True: []}
        for rep in range(a.repeats + 1):          # (repeat 0: the warm-up of both; a loop's state carries over from region to region)
            for per_robot in (False, True):
                t = region(per_robot, dstates, z[per_robot], warm)
                if rep:
                    samples[per_robot].append(t)
        same = torch.equal(z[False]["tau"], z[True]["tau"])
        med = {k: float(np.median(v)) for k, v in samples.items()}
        for per_robot in (False, True):
            v = samples[per_robot]
            say("%-11s %5d robots, %3d steps a region, %-13s: us/step %s median %.2f spread %.2f"
                % (name, B, T, "per robot" if per_robot else "context-wide", " ".join("%.2f" % x for x in v), med[per_robot], max(v) - min(v)))
        say("%-11s per robot / context-wide = %.3f; last efforts %s" % (name, med[True] / med[False], "equal bit for bit" if same else "DIFFER"))

    say("library %s, %d robots" % (capi.LIB_PATH, B))
    workload("static warm", [capi.to_device(s) for s in synth.trajectory(B, "static", T, errors="survey")], "one word")
    workload("trot table", [capi.to_device(s) for s in synth.trajectory(B, "trot", T)], "table")
    workload("cold plain", [capi.to_device(synth.make_states(B, "trot"))], None)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What qlamd_placement::set_memory -- a working set per support set -- is worth on the GPU: the caller's loop of include/qlamd.h
over a trot trajectory of two gait cycles (720 ticks), once with the one-word array updated in place and once with the table.

Per batch size and loop:
  iterations  mean `iterations` of the robots whose support set differs from the previous tick's, and of all robots, over the
              second gait cycle (the first one fills the table) -- a pass of its own with a synchronisation per tick
  us/step     the second gait cycle as ONE timed region: the first cycle is the warm-up region, a synchronisation, then 360
              steps between two events and a synchronisation; the states of all ticks are resident before the loop starts.
              Repeated --repeats times from a fresh start; every sample and the median are printed
and, for the cost of the longer argument block and first loads on a launch WITHOUT the table, the one-word loop on the static
4096 batch ("survey" errors), timed the same way.  --lib runs another build of the library (an earlier revision: its loops with
the table are skipped) through the same code, for an A/B on one machine in one session.

usage: set_memory_probe.py [--batches 4096,8192] [--ticks 720] [--repeats 3] [--lib path/to/libqlamd.so] [--out file]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,8192")
    ap.add_argument("--ticks", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from quadruped_locomotion_amd import capi, synth
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    has_table = hasattr(capi.lib(), "qlamd_set_memory_slot")
    ctx = capi.Context(device=0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    say("library %s (version %d), set_memory %s" % (capi.LIB_PATH, capi.lib().qlamd_version(), "available" if has_table else "absent"))

    def loop(dstates, B, table, lo, hi, state, collect=None):
        order, iters, ws, mem = state[:4]
        for k in range(lo, hi):
            ctx.balance_solve_placed_device(dstates[k], state[4], None, state[5], order=order[k & 1], iterations=iters[k & 1],
                                            prev_iterations=iters[(k - 1) & 1], next_order=order[(k + 1) & 1], policy=capi.PLACEMENT_AUTO,
                                            stream=stream, **(dict(set_memory=mem, working_set=None) if table else
                                                              dict(prev_working_set=ws, working_set=ws)))
            if collect is not None:
                torch.cuda.synchronize()
                collect(k, iters[k & 1].cpu().numpy())

    def fresh(B):
        dev = dict(device="cuda:0")
        return ([torch.arange(B, dtype=torch.int32, **dev) for _ in range(2)], [torch.zeros(B, dtype=torch.int32, **dev) for _ in range(2)],
                torch.zeros(B, dtype=torch.int32, **dev), torch.zeros(B, 4, dtype=torch.int32, **dev),
                torch.zeros(B, 12, dtype=torch.float64, **dev), torch.zeros(B, dtype=torch.int32, **dev))

    def timed(dstates, B, table, T):
        half, samples = T // 2, []
        for _ in range(a.repeats):
            state = fresh(B)
            loop(dstates, B, table, 0, half, state)          # the warm-up region: the first gait cycle
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loop(dstates, B, table, half, T, state)
            e1.record()
            torch.cuda.synchronize()
            assert (state[5] == 0).all()
            samples.append(e0.elapsed_time(e1) * 1e3 / (T - half))
        return samples

    for B in [int(x) for x in a.batches.split(",") if x]:
        T = a.ticks
        states = synth.trajectory(B, "trot", T)
        masks = [((s["stance"] != 0) * np.array([1, 2, 4, 8])).sum(1) for s in states]
        dstates = [capi.to_device(s) for s in states]
        del states
        for table in ((False, True) if has_table else (False,)):
            sw, al = [], []

            def collect(k, it):
                if k >= T // 2:
                    sw.append(it[masks[k] != masks[k - 1]])
                    al.append(it.mean())
            loop(dstates, B, table, 0, T, fresh(B), collect)
            samples = timed(dstates, B, table, T)
            say("trot %5d robots, %d ticks, %-9s: mean iterations of switching robots %.3f (%d robot-ticks), of all robots %.3f; us/step %s median %.2f"
                % (B, T, "table" if table else "one word", np.concatenate(sw).mean(), sum(len(x) for x in sw), np.mean(al),
                   " ".join("%.2f" % x for x in samples), np.median(samples)))
        del dstates
    B, T = 4096, 128
    dstates = [capi.to_device(s) for s in synth.trajectory(B, "static", T, errors="survey")]
    samples = timed(dstates, B, False, T)
    say("static %d robots, %d ticks, one word : us/step %s median %.2f spread %.2f" % (B, T, " ".join("%.2f" % x for x in samples),
                                                                                      np.median(samples), max(samples) - min(samples)))
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

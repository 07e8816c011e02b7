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

--workload full_tick | wholebody runs the same two measurements on qlamd_full_tick_batch (qlamd_tick_batch::set_memory against
::working_set, and cold; the messages of every tick resident, one controller state per loop) and on the whole-body step
(qlamd_wholebody_solve_placed_batch's [B][4] table of 64-bit words against the [B][2] set updated in place, and cold).  A
library without the entry / the members (an earlier revision) runs the one-word and cold loops only.
These two workloads time the second gait cycle as one captured hipGraph (replayed --repeats times, each replay one more cycle):
nothing is enqueued by the host inside the timed region.

usage: set_memory_probe.py [--workload balance|full_tick|wholebody] [--batches 4096,8192] [--ticks 720] [--repeats 3]
                           [--lib path/to/libqlamd.so] [--out file]"""
import argparse
import ctypes as C
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
    ap.add_argument("--workload", default="balance", choices=("balance", "full_tick", "wholebody"))
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

    def timed_calls(call, fresh_state, T):
        """call(k, state, stream): the ticks of the first gait cycle eagerly (the warm-up region; a captured tick needs an eager
        one before it), then the second cycle captured as ONE hipGraph and replayed: the host enqueues nothing inside the timed
        region.  The gait is periodic, so every replay is one more cycle on the same inputs from the state the last one left;
        one untimed replay, then a.repeats timed ones, each between two events."""
        half = T // 2
        state = fresh_state()
        for k in range(half):
            call(k, state, stream)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                cap = torch.cuda.current_stream().cuda_stream
                for k in range(half, T):
                    call(k, state, cap)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        samples = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / (T - half))
        assert ((state["st"] == 0) | (state["st"] == 4)).all()
        return samples

    def report(name, B, T, what, sw, al, samples):
        say("%s trot %5d robots, %d ticks, %-9s: mean iterations of switching robots %s, of all robots %s; us/step %s median %.2f spread %.2f"
            % (name, B, T, what, "%.3f (%d robot-ticks)" % (np.concatenate(sw).mean(), sum(len(x) for x in sw)) if sw else "-",
               "%.3f" % np.mean(al) if al else "-", " ".join("%.2f" % x for x in samples), np.median(samples), max(samples) - min(samples)))

    def wholebody(B, T):
        has_entry = hasattr(capi.lib(), "qlamd_wholebody_solve_placed_batch")
        states = synth.wholebody_trajectory(B, "trot", T)
        masks = [((s["stance"] != 0) * np.array([1, 2, 4, 8])).sum(1) for s in states]
        dstates = [capi.to_device(s) for s in states]
        del states
        dev = dict(device="cuda:0")

        def fresh_state():
            return dict(order=[torch.arange(B, dtype=torch.int32, **dev) for _ in range(2)], iters=[torch.zeros(B, dtype=torch.int32, **dev) for _ in range(2)],
                        ws=torch.zeros(B, 2, dtype=torch.int32, **dev), mem=torch.zeros(B, 4, dtype=torch.int64, **dev),
                        tau=torch.zeros(B, 12, dtype=torch.float64, **dev), st=torch.zeros(B, dtype=torch.int32, **dev))

        def caller(what):
            def call(k, z, st_=stream):
                pl = dict(order=z["order"][k & 1], iterations=z["iters"][k & 1], prev_iterations=z["iters"][(k - 1) & 1],
                          next_order=z["order"][(k + 1) & 1], policy=capi.PLACEMENT_AUTO)
                if what == "table":
                    capi.wholebody_solve_placed_device(ctx, dstates[k], z["tau"], None, z["st"], stream=st_, set_memory=z["mem"], **pl)
                    return
                warm = dict(prev_working_set=z["ws"], working_set=z["ws"]) if what == "one word" else {}
                if has_entry:
                    capi.wholebody_solve_placed_device(ctx, dstates[k], z["tau"], None, z["st"], stream=st_, **pl, **warm)
                else:   # an earlier revision: the same call through qlamd_place_next_call
                    p = capi.Placement(*[capi._ptr(x) for x in (pl["order"], pl["iterations"], pl["prev_iterations"], pl["next_order"])], pl["policy"],
                                       capi._ptr(warm.get("prev_working_set")), capi._ptr(warm.get("working_set")))
                    assert capi.lib().qlamd_place_next_call(ctx._h, C.byref(p)) == 0
                    capi.wholebody_solve_device(ctx, dstates[k], z["tau"], None, z["st"], stream=st_)
            return call

        for what in (("cold", "one word", "table") if has_entry else ("cold", "one word")):
            sw, al, call, z = [], [], caller(what), fresh_state()
            for k in range(T):
                call(k, z)
                torch.cuda.synchronize()
                if k >= T // 2:
                    it = z["iters"][k & 1].cpu().numpy()
                    sw.append(it[masks[k] != masks[k - 1]]); al.append(it.mean())
            report("whole-body", B, T, what, sw, al, timed_calls(call, fresh_state, T))

    def full_tick(B, T):
        from quadruped_locomotion_amd import wire  # noqa: F401
        has_members = capi.lib().qlamd_version() >= 8
        rng = np.random.default_rng(11)
        mt = synth.MessageTemplate(["footstep"] * 4)   # with the contacts below: the state machine follows the message's flags
        fixed = {k: rng.normal(size=(B, n)) for k, n in mt.DOUBLES}
        fixed["phase"] = rng.random((B, 4))
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")  # noqa: E731
        s = synth.make_states(B, "trot")
        phase = synth.trot_phase(B)
        shared = dict(joint_position=up(s["q"]), joint_velocity=up(rng.normal(scale=0.3, size=(B, 12))),
                      joint_velocity_oldest=up(rng.normal(scale=0.3, size=(B, 12))), base_linear_velocity=up(s["base_linvel"]),
                      base_angular_velocity=up(s["base_angvel"]))
        per_tick, masks = [], []
        for t in range(T):
            if t:
                s = synth.next_tick_states(s, synth.CONTROL_PERIOD)
                s["stance"] = synth.trot_stance(phase + t * synth.CONTROL_PERIOD / (synth.T_SWING + synth.T_STANCE))
            blob, off = mt.pack(dict(fixed, des_pos=s["des_pos"], des_quat=s["des_quat"], des_linvel=s["des_linvel"], des_angvel=s["des_angvel"],
                                     support_leg=s["stance"]))
            per_tick.append(dict(shared, messages=up(blob), offsets=up(off), base_position=up(s["base_pos"]), base_orientation=up(s["base_quat"]),
                                 contact=up(s["stance"].astype(np.uint8))))
            masks.append(((s["stance"] != 0) * np.array([1, 2, 4, 8])).sum(1))
        tctx = capi.Context(device=0)
        tctx.reserve(B)

        def fresh_state(what="cold", count=False):
            keep = dict(limb_state=np.zeros((B, 4), np.int8), store_flag=np.zeros((B, 4), np.uint8), stored_joint_position=np.zeros((B, 12)),
                        leg_mode=np.zeros((B, 4), np.uint8), support=np.ones((B, 4), np.uint8), pid_error_last=np.zeros((B, 12)),
                        pid_error_integral=np.zeros((B, 12)), joint_effort=np.zeros((B, 12)), st=np.full(B, -1, np.int32),
                        message_status=np.full(B, -1, np.int32), command=np.zeros(capi.tick_command_bytes(B), np.uint8))
            if what == "one word":
                keep["working_set"] = np.zeros(B, np.int32)
            if what == "table":
                keep["set_memory"] = np.zeros((B, 4), np.int32)
            if count:
                keep["iterations"] = np.zeros(B, np.int32)
            return {k: up(v) for k, v in keep.items()}   # ("st": qlamd_tick_batch::status)

        for what in (("cold", "one word", "table") if has_members else ("cold", "one word")):
            call = lambda k, z, st_=stream: capi.full_tick(tctx, dict(per_tick[k], status=z["st"], **{n: v for n, v in z.items() if n != "st"}),  # noqa: E731
                                                           synth.CONTROL_PERIOD, memory=capi.MEM_DEVICE, stream=st_)
            sw, al = [], []
            if has_members:   # (a tick reports its counts through qlamd_tick_batch::iterations only)
                z = fresh_state(what, count=True)
                for k in range(T):
                    call(k, z)
                    torch.cuda.synchronize()
                    if k >= T // 2:
                        it = z["iterations"].cpu().numpy()
                        sw.append(it[masks[k] != masks[k - 1]]); al.append(it.mean())
                assert ((z["st"] == 0) | (z["st"] == 4)).all()
            report("full tick", B, T, what, sw, al, timed_calls(call, lambda: fresh_state(what), T))
        tctx.close()

    if a.workload != "balance":
        for B in [int(x) for x in a.batches.split(",") if x]:
            (wholebody if a.workload == "wholebody" else full_tick)(B, a.ticks)
        ctx.close()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

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

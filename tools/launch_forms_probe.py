#!/usr/bin/env python3
"""Which kernel each kind of call runs.  The results cannot show a wrongly selected form of the balance kernel -- the two- and
three-wavefront forms and the 6- and 12-variable forms agree bit for bit -- so this makes one call per row of the selection,
through the public wrapper only, for a kernel trace to name the kernels:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_forms_probe.py run
    python tools/launch_forms_probe.py names OUT        # the library's kernels of that trace, in the order they started

Every call runs under a time limit of its own (an alarm that ends the process) and the first failure ends the script.  The
ordered list is compared with the one the same script gives on the commit before (profiles/r11/launch_forms.txt)."""
import csv
import glob
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALL_SECONDS = 60


def run():
    import numpy as np
    import torch
    from quadruped_locomotion_amd import capi, synth

    def timed(what, fn):
        def late(*_):
            print("TIMEOUT in", what, flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.alarm(CALL_SECONDS)
        fn()
        torch.cuda.synchronize()
        signal.alarm(0)
        print("ok", what, flush=True)

    def i32(*shape):
        return torch.zeros(*shape, dtype=torch.int32, device="cuda:0")

    def outputs(B):
        return (torch.zeros(B, 12, dtype=torch.float64, device="cuda:0"), torch.zeros(B, 12, dtype=torch.float64, device="cuda:0"), i32(B))

    ctx = capi.Context(device=0)
    ctx.reserve(22528)

    def balance(what, B, normals=False, **kw):
        s = synth.make_states(B, "trot")          # a trot mix: some wavefronts of 8 robots stand on two legs
        if normals:
            s["normals"] = np.tile(np.array([0.0, 0.0, 1.0]), (B, 4))
        d = capi.to_device(s)
        tau, grf, status = outputs(B)
        if kw:
            timed(what, lambda: ctx.balance_solve_placed_device(d, tau, grf, status, **kw))
        else:
            timed(what, lambda: ctx.balance_solve_device(d, tau, grf, status))
        assert (status.cpu().numpy() >= 0).all(), what

    # ---- the balance step: plain, placed, warm, table at 8 robots; the thresholds of the three-wavefront form
    balance("balance plain 8", 8)
    balance("balance placed 8", 8, order=torch.arange(8, dtype=torch.int32, device="cuda:0"))
    balance("balance warm 8", 8, prev_working_set=i32(8), working_set=i32(8))
    balance("balance table 8", 8, set_memory=i32(8, 4))
    balance("balance cold 16384", 16384)
    balance("balance warm 16384", 16384, prev_working_set=i32(16384), working_set=i32(16384))
    balance("balance warm 22528", 22528, prev_working_set=i32(22528), working_set=i32(22528))
    balance("balance normals 22528", 22528, normals=True)

    # ---- controller parameters per robot: cold, warm, table
    B = 8
    rp = synth.make_robot_params(B)
    rec = torch.from_numpy(capi.robot_params_fill([synth.robot_params_struct(rp, i, capi.BalanceParams) for i in range(B)])).to("cuda:0")
    d = capi.to_device(synth.make_states(B, "trot"))
    for what, kw in (("cold", {}), ("warm", dict(prev_working_set=i32(B), working_set=i32(B))), ("table", dict(set_memory=i32(B, 4)))):
        tau, grf, status = outputs(B)
        timed("robot params " + what, lambda: ctx.balance_solve_robot_params_device(d, rec, tau, grf, status, **kw))

    # ---- the whole-body step: cold, warm, table
    dw = capi.to_device(synth.make_wholebody_states(B, "trot"))
    ws = torch.zeros(B, dtype=torch.int64, device="cuda:0")
    mem = torch.zeros(B, 4, dtype=torch.int64, device="cuda:0")
    assert mem.data_ptr() % 32 == 0
    for what, kw in (("cold", {}), ("warm", dict(prev_working_set=ws, working_set=ws)), ("table", dict(set_memory=mem))):
        tau, grf, status = outputs(B)
        timed("whole body " + what, lambda: capi.wholebody_solve_placed_device(ctx, dw, tau, grf, status, **kw))

    # ---- the fused tick: cold, warm (one word), table; device memory
    rng = np.random.default_rng(11)
    mt = synth.MessageTemplate(["footstep"] * 4)
    s = synth.make_states(B, "trot")
    f = {k: rng.normal(size=(B, n)) for k, n in mt.DOUBLES}
    f["phase"] = rng.random((B, 4))
    blob, off = mt.pack(dict(f, des_pos=s["des_pos"], des_quat=s["des_quat"], des_linvel=s["des_linvel"], des_angvel=s["des_angvel"],
                             support_leg=s["stance"]))
    tin = dict(messages=blob, offsets=off, joint_position=s["q"], joint_velocity=np.ascontiguousarray(rng.normal(scale=0.3, size=(B, 12))),
               joint_velocity_oldest=np.ascontiguousarray(rng.normal(scale=0.3, size=(B, 12))),
               base_linear_velocity=np.ascontiguousarray(s["base_linvel"]), base_angular_velocity=np.ascontiguousarray(s["base_angvel"]),
               base_position=np.ascontiguousarray(s["base_pos"]), base_orientation=np.ascontiguousarray(s["base_quat"]),
               contact=np.ascontiguousarray(s["stance"], dtype=np.uint8))
    for what in ("cold", "warm", "table"):
        keep = dict(limb_state=np.zeros((B, 4), np.int8), store_flag=np.zeros((B, 4), np.uint8), stored_joint_position=np.zeros((B, 12)),
                    leg_mode=np.zeros((B, 4), np.uint8), support=np.ones((B, 4), np.uint8), pid_error_last=np.zeros((B, 12)),
                    pid_error_integral=np.zeros((B, 12)), joint_effort=np.zeros((B, 12)), leg_state_code=np.zeros((B, 4), np.int8),
                    status=np.full(B, -1, np.int32), message_status=np.full(B, -1, np.int32),
                    command=np.zeros(capi.tick_command_bytes(B), np.uint8), iterations=np.zeros(B, np.int32))
        if what == "warm":
            keep["working_set"] = np.zeros(B, np.int32)
        if what == "table":
            keep["set_memory"] = np.zeros((B, 4), np.int32)
        io = {k: torch.from_numpy(v).to("cuda:0") for k, v in dict(tin, **keep).items()}
        tctx = capi.Context(device=0)             # (a context of its own: the tick keeps a layout template between calls)
        tctx.reserve(B)
        timed("tick " + what, lambda: capi.full_tick(tctx, io, synth.CONTROL_PERIOD, memory=capi.MEM_DEVICE))
        tctx.close()
    ctx.close()
    print("done", flush=True)


def names(out_dir):
    """The library's kernels in a rocprofv3 kernel trace (csv), ordered by start time, without their parameter lists."""
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    for _, name in sorted(rows):
        if "(anonymous namespace)::" in name and "at::" not in name:
            print(name.split("(anonymous namespace)::", 1)[1].split("(")[0])
        elif name.startswith("_ZN12_GLOBAL__N_1"):  # (a trace that kept the mangled names)
            print(name)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "names":
        names(sys.argv[2])
    else:
        sys.exit(__doc__)

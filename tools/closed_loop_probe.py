#!/usr/bin/env python3
"""The plant step in time, and the whole-body step under a closed loop (measurements, not gates).

1. us per plant step (qlamd_wholebody_forward_dynamics_batch: nu', f and the next state, out of place so that every step does
   the same work) at each of --batches, next to today's only alternative for a caller who wants accelerations:
   qlamd_wholebody_dynamics_batch with all three outputs (M, h, Jc -- 4464 B per robot written, and an 18 + 3 nS linear system
   still to be solved on the host).  A region is --steps launches between two events; the first region is the warm-up; median
   and spread of --repeats regions.
2. The closed loop on --batch trot robots started from synth.make_wholebody_states: every tick ONE
   qlamd_wholebody_solve_placed_batch (warm-started from the table, set_memory) and ONE plant step IN PLACE with its efforts.
   The support flags follow the trot's phase as in synth.trajectory (contact switches included); the desired base acceleration
   stays as drawn.  Reported: us per tick, status counts of both entries per tick range, and the fraction of robots whose final
   working set is the previous tick's (`working_set_unchanged`; 0.975 on the open-loop trajectory of bench.py).

   Also per tick range: the largest and the median world speed of the held feet after the tick (Jc nu of the state the tick left).
3. --contacts: the plant step of both parts is qlamd_wholebody_plant_step_batch.  Part 1 adds its launch with contacts == NULL
   (the old entry's kernel), with contacts and no touchdown, and with every robot projecting; part 2 gives every tick the flags
   of the tick before as previous_support_leg (zeros at the first tick) and --velocity-gain as k_v (1/s; default 0).

4. --detect [--terrain plane|heightfield] (implies --contacts): part 1 times qlamd_wholebody_contact_update_batch alone, every
   output given, with its bytes per robot and GB/s next to those of qlamd_wholebody_dynamics_batch; part 2 runs THREE launches per
   tick -- whole-body step, plant step with its report, contact update in place -- and the support flags and surface normals come
   from the update, not from the trot's phase (which gives the first tick's flags only).  Every robot is lifted so that the feet
   the trot flags at the start stand at z = 0 on average; the terrain is that plane, or a 65 x 65 height field of +-5 mm around it.
   A foot is flagged at gap <= 0 while it does not move away, and released 10 mm above the ground or when the report says it pulls.
   Also reported: the share of (tick, leg) pairs on which detection and the trot schedule disagree.
5. --friction (implies --contacts; with or without --detect): the plant step of part 2 is qlamd_wholebody_plant_step_friction_batch
   with mu = 0.6 -- impulses and forces inside the friction pyramid -- and with --detect the update releases a foot on
   QLAMD_CONTACT_SEPARATING instead of QLAMD_CONTACT_PULLS.  Part 1 adds the new kernel alone, next to the contacts entry's, in two
   settings: the drawn states with the controller's own torques (qlamd_wholebody_solve_batch: the working sets are mostly empty)
   and with the random torques of the other rows, each without a touchdown and with every robot projecting, with the distribution
   of `iterations`.  Part 2 also reports the separating and sliding legs per tick and robot.

6. --anchor [--position-gain KP] [--max-error E] (implies --detect; with or without --friction): the update and the plant step of
   part 2 are qlamd_wholebody_contact_update_anchored_batch and qlamd_wholebody_plant_step_anchored_batch: the update keeps an
   anchor per leg (with --friction a sliding foot is re-anchored), the plant step pulls each held foot to its anchor with
   k_p = KP (1/s^2; default 0.1 / dt^2) on an error clamped to E metres (default 0.01).  The first anchors are the feet (an update
   without flags under a rule that takes no foot).  Part 1
   adds the three anchored kernels alone next to their parents (anchors 2 mm from the feet).  Part 2 also reports, per quarter of
   the run: |gap| of the held feet (largest and median), their distance |p - anchor| from the anchor the tick ran with, and the
   events per robot and tick, re-anchorings included.

7. --swing (implies --detect; with or without --friction and --anchor): FOUR launches per tick.  In front of the whole-body step
   qlamd_wholebody_swing_task_batch turns the trot's schedule (a leg the phase does not flag is to swing) and a foothold per swing
   -- the foot where the swing begins plus the desired base velocity x T / 2, on the ground z = 0 -- into desired joint
   accelerations and the flags the SOLVE runs with; the plant and the update keep the detected flags.  T is the trot's swing time,
   the profile 0.08 m high; --swing-gains KP,KD (default 400,40), the error clamped to 0.05 m, lambda 0.05, |qdd| <= 500, a landing
   counted from half the swing on, touchdown speed 0.1 m/s.  Part 1 times the new launch alone, every output given, next to the
   contact update's (a device copy of the records goes in front of every timed launch, so that each begins the same swings, and is
   timed alone beside it).  Part 2 also reports the task's events per tick and robot and, with or without --swing, the apex clearance:
   per (robot, leg) the largest gap seen on the ticks the schedule wants the leg in the air.

usage: closed_loop_probe.py [--batch 4096] [--ticks 64] [--batches 4096,65536,1048576] [--steps 64] [--repeats 5] [--out file]
                            [--contacts] [--velocity-gain K] [--detect] [--terrain plane|heightfield] [--friction]
                            [--anchor] [--position-gain KP] [--max-error E] [--swing] [--swing-gains KP,KD]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DT = 0.0025


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--batches", default="4096,65536,1048576")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--contacts", action="store_true")
    ap.add_argument("--velocity-gain", type=float, default=0.0)
    ap.add_argument("--detect", action="store_true")
    ap.add_argument("--terrain", choices=("plane", "heightfield"), default="plane")
    ap.add_argument("--friction", action="store_true")
    ap.add_argument("--anchor", action="store_true")
    ap.add_argument("--position-gain", type=float, default=0.1 / DT ** 2)
    ap.add_argument("--max-error", type=float, default=0.01)
    ap.add_argument("--swing", action="store_true")
    ap.add_argument("--swing-gains", default="400,40")
    a = ap.parse_args()
    a.detect = a.detect or a.anchor or a.swing
    a.contacts = a.contacts or a.detect or a.friction
    import torch
    from quadruped_locomotion_amd import capi, plant_contacts, synth
    if a.detect:
        from quadruped_locomotion_amd import contact_detection
    if a.friction:
        from quadruped_locomotion_amd import plant_friction
    if a.anchor:
        from quadruped_locomotion_amd import contact_anchor
    if a.swing:
        from quadruped_locomotion_amd import swing_task
    MU = 0.6
    SWING = dict(swing_duration=synth.T_SWING, profile_height=0.08, touchdown_speed=0.1, touchdown_phase=0.5, max_error=0.05, damping=0.05,
                 max_joint_acceleration=500.0, dt=DT, position_gain=float(a.swing_gains.split(",")[0]),
                 velocity_gain=float(a.swing_gains.split(",")[1]))
    ctx = capi.Context(device=0)
    stream = torch.cuda.current_stream().cuda_stream
    dev = dict(device="cuda:0")
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    def f64(*shape):
        return torch.zeros(*shape, dtype=torch.float64, **dev)

    def region(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def sample(fn, n):
        v = [region(fn, n) for _ in range(a.repeats + 1)][1:]
        return float(np.median(v)), max(v) - min(v)

    def terrain(B):
        """-> the terrain arguments of the contact update on the device (and what keeps them alive)"""
        if a.terrain == "plane":
            plane = f64(B, 4)
            plane[:, 2] = 1.0
            return dict(plane=plane)
        n, res = 65, 0.05
        x = (np.arange(n) - n // 2) * res
        X, Y = np.meshgrid(x, x)
        heights = torch.from_numpy(np.ascontiguousarray(0.005 * np.sin(2.0 * np.pi * X / 0.8) * np.cos(2.0 * np.pi * Y / 1.1))).to("cuda:0")
        return dict(hf=contact_detection.heightfield((x[0], x[0]), res, heights))

    def update_outputs(B):
        u8 = lambda: torch.zeros(B, 4, dtype=torch.uint8, **dev)  # noqa: E731
        return dict(support_next=u8(), sensor=u8(), events=u8(), gap=f64(B, 4), normals=f64(B, 12), foot_pos=f64(B, 12), foot_vel=f64(B, 12))

    RULE = dict(liftoff_distance=0.01, sensor_distance=0.005)
    if a.friction and a.detect:
        RULE["release_mask"] = plant_friction.CONTACT_SEPARATING
    UPDATE_BYTES = (96 + 96 + 32 + 24 + 24 + 24 + 4 + 4, 4 + 4 + 4 + 4 + 32 + 96 + 96 + 96)   # read (without the terrain), written

    say("plant step: %d launches a region, median (spread) of %d regions, us per launch" % (a.steps, a.repeats))
    for B in [int(x) for x in a.batches.split(",")]:
        n = a.steps if B <= 65536 else max(4, a.steps // 8)
        s = synth.make_wholebody_states(B, "trot")
        d = capi.to_device(s)
        tau = torch.from_numpy(np.random.default_rng(3).uniform(-30.0, 30.0, (B, 12))).to("cuda:0")
        st, acc, f = torch.zeros(B, dtype=torch.int32, **dev), f64(B, 18), f64(B, 12)
        nxt = dict(q=f64(B, 12), qd=f64(B, 12), base_pos=f64(B, 3), base_quat=f64(B, 4), base_linvel=f64(B, 3), base_angvel=f64(B, 3))
        t_acc = sample(lambda: capi.wholebody_forward_dynamics_device(ctx, d, tau, st, acc=acc, f=f, stream=stream), n)
        t_step = sample(lambda: capi.wholebody_forward_dynamics_device(ctx, d, tau, st, acc=acc, f=f, dt=DT, next=nxt, stream=stream), n)
        ok = int((st == 0).sum())
        if a.contacts:
            zeros = torch.zeros(B, 4, dtype=torch.uint8, **dev)
            kw = dict(acc=acc, f=f, dt=DT, next=nxt, stream=stream)
            t_null = sample(lambda: plant_contacts.wholebody_plant_step_device(ctx, d, tau, st, contacts=False, **kw), n)
            t_quiet = sample(lambda: plant_contacts.wholebody_plant_step_device(ctx, d, tau, st, velocity_gain=a.velocity_gain, **kw), n)
            t_proj = sample(lambda: plant_contacts.wholebody_plant_step_device(ctx, d, tau, st, prev_stance=zeros, velocity_gain=a.velocity_gain, **kw), n)
            say("%8d robots: qlamd_wholebody_plant_step_batch, nu', f and next state: contacts NULL %8.2f (%.2f)   contacts, no touchdown "
                "%8.2f (%.2f)   every robot projecting %8.2f (%.2f)   status OK %d / %d"
                % (B, t_null[0], t_null[1], t_quiet[0], t_quiet[1], t_proj[0], t_proj[1], int((st == 0).sum()), B))
        if a.friction:
            it = torch.zeros(B, 2, dtype=torch.int32, **dev)
            tau_c = f64(B, 12)
            capi.wholebody_solve_device(ctx, d, tau_c, None, st, stream=stream)
            now = torch.from_numpy(np.ascontiguousarray(s["stance"], dtype=np.uint8)).to("cuda:0")
            for name, tq in (("the controller's torques", tau_c), ("random torques", tau)):
                res = []
                for prev in (now, zeros):
                    res.append(sample(lambda: plant_friction.wholebody_plant_step_friction_device(
                        ctx, d, tq, st, MU, prev_stance=prev, velocity_gain=a.velocity_gain, iterations=it, **kw), n))
                    hist = [torch.bincount(it[:, j].clamp(0, 31).long(), minlength=32).tolist() for j in range(2)]
                    res.append((int((st == 0).sum()), [" ".join("%d:%d" % (k, c) for k, c in enumerate(h_) if c) for h_ in hist]))
                say("%8d robots: qlamd_wholebody_plant_step_friction_batch, mu %.1f, %s: no touchdown %8.2f (%.2f) status OK %d / %d   every "
                    "robot projecting %8.2f (%.2f) status OK %d / %d" % (B, MU, name, res[0][0], res[0][1], res[1][0], B, res[2][0], res[2][1], res[3][0], B))
                say("           iterations (count:robots) no touchdown: force QP %s | projecting: impulse QP %s ; force QP %s"
                    % (res[1][1][1], res[3][1][0], res[3][1][1]))
            del it, tau_c
        del nxt
        M, h, Jc = f64(B, 18, 18), f64(B, 18), f64(B, 12, 18)
        t_dyn = sample(lambda: capi.wholebody_dynamics_device(ctx, d, M, h, Jc, stream=stream), n)
        del M, h, Jc
        if a.detect:
            dd = dict(d, stance=torch.from_numpy(np.ascontiguousarray(s["stance"], dtype=np.uint8)).to("cuda:0"))
            ter, o, report = terrain(B), update_outputs(B), torch.zeros(B, 4, dtype=torch.uint8, **dev)
            call = contact_detection.ContactUpdateCall(ctx, dd, st, report=report, stream=stream, **ter, **o, **RULE)   # checked once
            t_upd = sample(call, n)
            del call
            per = sum(UPDATE_BYTES) + (32 if a.terrain == "plane" else 128)   # the plane, or four cells per foot
            say("%8d robots: qlamd_wholebody_contact_update_batch (%s, every output) %8.2f (%.2f) = %.0f GB/s of its %d B per robot (%d read, "
                "%d written)   status OK %d / %d   | qlamd_wholebody_dynamics_batch %.0f GB/s of its 4464 B written + 304 B read per robot"
                % (B, a.terrain, t_upd[0], t_upd[1], B * per / t_upd[0] * 1e-3, per, per - UPDATE_BYTES[1], UPDATE_BYTES[1],
                   int((st == 0).sum()), B, B * 4768 / t_dyn[0] * 1e-3))
            if a.swing:
                u8 = lambda: torch.zeros(B, 4, dtype=torch.uint8, **dev)  # noqa: E731
                dd["a_des"] = d["a_des"]
                want1 = 1 - dd["stance"]
                hold = o["foot_pos"].clone()    # (the update above left the feet there) every scheduled leg begins: 5 cm ahead, on the ground
                hold.reshape(B, 4, 3)[:, :, 0] += 0.05
                hold.reshape(B, 4, 3)[:, :, 2] = 0.0
                records, rec0 = f64(B, 16), f64(B, 16)
                rec0.reshape(B, 4, 4)[:, :, 3] = torch.from_numpy(np.random.default_rng(5).choice([0.0, 0.1, 0.3], size=(B, 4))).to("cuda:0")
                rec0.reshape(B, 4, 4)[:, :, :3] = o["foot_pos"].reshape(B, 4, 3)
                call = swing_task.SwingTaskCall(ctx, dd, st, want1, hold, records, f64(B, 12), normals=o["normals"], support_solve=u8(),
                                                foot_reference=f64(B, 36), events=u8(), stream=stream, **SWING)   # checked once

                def one_tick():      # (the records are put back every launch, so that each does the same work: one more copy of 128 B)
                    records.copy_(rec0)
                    call()
                t_copy = sample(lambda: records.copy_(rec0), n)
                t_sw = sample(one_tick, n)
                per_sw = (296 + 4 + 48 + 4 + 96 + 96 + 128, 96 + 4 + 4 + 288 + 128 + 4)   # read: state, flags, a_des, schedule, footholds, normals, records
                say("%8d robots: qlamd_wholebody_swing_task_batch (every input and output) %8.2f (%.2f) with a %.2f copy of the records in front "
                    "= %.0f GB/s of its %d B per robot (%d read, %d written)   status OK %d / %d   | the contact update %8.2f"
                    % (B, t_sw[0], t_sw[1], t_copy[0], B * sum(per_sw) / max(t_sw[0] - t_copy[0], 1e-3) * 1e-3, sum(per_sw), per_sw[0], per_sw[1],
                       int((st == 0).sum()), B, t_upd[0]))
                del call, records, rec0, hold, want1
            if a.anchor:
                anchor = f64(B, 12)
                call = contact_anchor.AnchoredContactUpdateCall(ctx, dd, st, anchor, reanchor_mask=16, report=report, stream=stream,
                                                                **ter, **o, **RULE)   # checked once
                t_anc = sample(call, n)
                del call
                say("%8d robots: qlamd_wholebody_contact_update_anchored_batch (%s, every output) %8.2f (%.2f) = %.0f GB/s of its %d B per "
                    "robot (up to 96 more written)   status OK %d / %d" % (B, a.terrain, t_anc[0], t_anc[1], B * (per + 96) / t_anc[0] * 1e-3,
                                                                           per + 96, int((st == 0).sum()), B))
                # anchors 2 mm from the feet, the plant kernels alone: hard contacts and (--friction) the cone, random torques
                anchor.copy_(o["foot_pos"])
                anchor += 0.002 / 3 ** 0.5
                perr = f64(B, 12)
                nxt2 = dict(q=f64(B, 12), qd=f64(B, 12), base_pos=f64(B, 3), base_quat=f64(B, 4), base_linvel=f64(B, 3), base_angvel=f64(B, 3))
                kw2 = dict(acc=acc, f=f, dt=DT, next=nxt2, stream=stream, velocity_gain=a.velocity_gain, position_error=perr)
                for cone_on in ((False, True) if a.friction else (False,)):
                    res = []
                    for prev in (dd["stance"], zeros):
                        res.append(sample(contact_anchor.AnchoredPlantStepCall(ctx, d, tau, st, anchor, a.position_gain, a.max_error, friction=MU,
                                                                               cone=cone_on, prev_stance=prev, **kw2), n))
                        res.append(int((st == 0).sum()))
                    say("%8d robots: qlamd_wholebody_plant_step_anchored_batch (%s), k_p %g, e_max %g, random torques: no touchdown %8.2f (%.2f) "
                        "status OK %d / %d   every robot projecting %8.2f (%.2f) status OK %d / %d"
                        % (B, "friction, mu %.1f" % MU if cone_on else "hard contacts", a.position_gain, a.max_error, res[0][0], res[0][1], res[1], B,
                           res[2][0], res[2][1], res[3], B))
                del anchor, perr, nxt2
            del dd, ter, o
        bytes_step = B * (272 + 96 + 4 + 24 + 144 + 96 + 296 + 4)
        say("%8d robots: nu' and f %8.2f (%.2f)   nu', f and next state %8.2f (%.2f) = %.0f GB/s of its %d B per robot   status OK %d / %d"
            "   | qlamd_wholebody_dynamics_batch (M, h, Jc) %8.2f (%.2f)"
            % (B, t_acc[0], t_acc[1], t_step[0], t_step[1], bytes_step / t_step[0] * 1e-3, bytes_step // B, ok, B, t_dyn[0], t_dyn[1]))

    # ---- the closed loop
    B, K = a.batch, a.ticks
    s = synth.make_wholebody_states(B, "trot")
    phase = synth.trot_phase(B, synth.SEED, 0)
    stance = torch.from_numpy(np.stack([synth.trot_stance(phase + k * DT / (synth.T_SWING + synth.T_STANCE)) for k in range(K)]).astype(np.uint8)).to("cuda:0")
    switched = float((stance[1:] != stance[:-1]).any(dim=2).float().mean())

    def held_foot_speeds(d, flags):
        """world speeds of the feet flagged in `flags` [B, 4]: |Jc nu| by foot (a rotation away from the world's)"""
        Jc = f64(B, 12, 18)
        capi.wholebody_dynamics_device(ctx, d, None, None, Jc, stream=stream)
        w, x, y, z = d["base_quat"].unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(B, 3, 3)
        nu = torch.cat([torch.einsum("bji,bj->bi", R, d["base_linvel"]), d["base_angvel"], d["qd"]], dim=1)
        speed = torch.einsum("brk,bk->br", Jc, nu).reshape(B, 4, 3).norm(dim=2)
        return speed[flags != 0]

    zero_flags = torch.zeros(B, 4, dtype=torch.uint8, **dev)

    if a.detect:
        # lift every robot so that the feet the trot flags at the start stand at z = 0 on average
        d0 = capi.to_device(s)
        o0, st0 = update_outputs(B), torch.zeros(B, dtype=torch.int32, **dev)
        contact_detection.wholebody_contact_update_device(ctx, d0, st0, stream=stream, **o0)
        on = stance[0].double()
        lift = (o0["foot_pos"].reshape(B, 4, 3)[:, :, 2] * on).sum(dim=1) / on.sum(dim=1).clamp(min=1.0)
        s = dict(s, base_pos=(d0["base_pos"] - torch.stack([torch.zeros_like(lift), torch.zeros_like(lift), lift], dim=1)).cpu().numpy())
        ter = terrain(B)
        disagree = []
        want_all = (1 - stance).contiguous()            # the schedule: a leg the trot's phase does not flag is to swing
        step = torch.from_numpy(np.ascontiguousarray(s["des_linvel"] * (0.5 * synth.T_SWING))).to("cuda:0")
        step[:, 2] = 0.0
        footholds, swing_events, apex = [], [], torch.full((B, 4), -float("inf"), dtype=torch.float64, **dev)

    def loop(timed):
        d = capi.to_device(s)
        if a.detect:
            d["stance"] = stance[0].clone()
            d["normals"] = f64(B, 12)
            d["normals"].reshape(B, 4, 3)[:, :, 2] = 1.0
            prev, report, st_up, o = zero_flags.clone(), zero_flags.clone(), torch.zeros(B, dtype=torch.int32, **dev), update_outputs(B)
            if a.anchor:
                anchor = f64(B, 12)   # the first anchors: every foot where it is (an update without flags, under a rule that takes no foot)
                contact_anchor.wholebody_contact_update_anchored_device(ctx, {k: v for k, v in d.items() if k != "stance"}, st_up, anchor,
                                                                        stream=stream, approach_speed=-1e300, **ter)
                update = contact_anchor.AnchoredContactUpdateCall(ctx, d, st_up, anchor, reanchor_mask=16 if a.friction else 0, report=report,
                                                                  stream=stream, support_next=d["stance"], sensor=o["sensor"],
                                                                  events=o["events"], gap=o["gap"], normals=d["normals"],
                                                                  foot_pos=o["foot_pos"], **ter, **RULE)
            else:
                update = contact_detection.ContactUpdateCall(ctx, d, st_up, report=report, stream=stream, support_next=d["stance"],
                                                             sensor=o["sensor"], events=o["events"], gap=o["gap"], normals=d["normals"],
                                                             **ter, **RULE)   # checked once; the tick launches it
            if a.swing:
                records, qdd, sup, sw_ev = f64(B, 16), f64(B, 12), zero_flags.clone(), zero_flags.clone()
                st_sw = torch.zeros(B, dtype=torch.int32, **dev)
                d_solve = dict(d, stance=sup, qdd_des=qdd)     # the solve's flags and accelerations; the plant keeps d["stance"]
                fh_now, fp_now = f64(B, 12), f64(B, 12)

                def swing_call(k):
                    return swing_task.SwingTaskCall(ctx, d, st_sw, want_all[k], footholds[k], records, qdd, normals=d["normals"], support_solve=sup,
                                                    events=sw_ev, stream=stream, **SWING)
                swing_calls = [swing_call(k) for k in range(len(footholds))]   # (a timed loop: the footholds of the loop that went before)
        tau, st_qp, st_pl = f64(B, 12), torch.zeros(B, dtype=torch.int32, **dev), torch.zeros(B, dtype=torch.int32, **dev)
        mem, ws = torch.zeros(B, 4, dtype=torch.int64, **dev), torch.zeros(B, dtype=torch.int64, **dev)
        prev_ws = torch.zeros_like(ws)
        report_f = report if a.detect else zero_flags.clone()   # (--friction without --detect: the report is only counted)
        stats = []

        def tick(k):
            if a.swing:
                swing_calls[k]()
            if a.detect:
                capi.wholebody_solve_placed_device(ctx, d_solve if a.swing else d, tau, None, st_qp, stream=stream, working_set=ws, set_memory=mem)
                if a.anchor:
                    contact_anchor.wholebody_plant_step_anchored_device(ctx, d, tau, st_pl, anchor, a.position_gain, max_error=a.max_error,
                                                                        friction=MU, cone=a.friction, dt=DT, next=d, stream=stream,
                                                                        velocity_gain=a.velocity_gain, prev_stance=prev, report=report)
                elif a.friction:
                    plant_friction.wholebody_plant_step_friction_device(ctx, d, tau, st_pl, MU, dt=DT, next=d, stream=stream,
                                                                        velocity_gain=a.velocity_gain, prev_stance=prev, report=report)
                else:
                    plant_contacts.wholebody_plant_step_device(ctx, d, tau, st_pl, dt=DT, next=d, stream=stream, velocity_gain=a.velocity_gain,
                                                               prev_stance=prev, friction=MU, report=report)
                prev.copy_(d["stance"])
                update()
                return
            d["stance"] = stance[k]
            capi.wholebody_solve_placed_device(ctx, d, tau, None, st_qp, stream=stream, working_set=ws, set_memory=mem)
            if a.friction:
                plant_friction.wholebody_plant_step_friction_device(ctx, d, tau, st_pl, MU, dt=DT, next=d, stream=stream,
                                                                    velocity_gain=a.velocity_gain, prev_stance=stance[k - 1] if k else zero_flags,
                                                                    report=report_f)
            elif a.contacts:
                plant_contacts.wholebody_plant_step_device(ctx, d, tau, st_pl, dt=DT, next=d, stream=stream, velocity_gain=a.velocity_gain,
                                                 prev_stance=stance[k - 1] if k else zero_flags)
            else:
                capi.wholebody_forward_dynamics_device(ctx, d, tau, st_pl, dt=DT, next=d, stream=stream)

        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for k in range(K):
                tick(k)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / K
        for k in range(K):
            ran_with = d["stance"].clone() if a.detect else stance[k]
            held_at = anchor.clone() if a.anchor else None
            if a.swing:
                # the foothold of a swing that begins now: the foot where it is (one more update, outside the tick) plus the step
                contact_detection.wholebody_contact_update_device(ctx, d, st_sw, stream=stream, foot_pos=fp_now, **ter)
                begins = (want_all[k] != 0) & ((want_all[k - 1] == 0) if k else torch.ones_like(want_all[0], dtype=torch.bool))
                target = fp_now.reshape(B, 4, 3) + step[:, None, :]
                target[:, :, 2] = 0.0
                fh_now.copy_(torch.where(begins[:, :, None], target, fh_now.reshape(B, 4, 3)).reshape(B, 12))
                footholds.append(fh_now.clone())
                swing_calls.append(swing_call(k))
            tick(k)
            torch.cuda.synchronize()
            if a.swing:
                swing_events.append(tuple(int((sw_ev & b).ne(0).sum()) for b in (1, 2, 4, 8)) + (int((st_sw == 0).sum()),))
            if a.detect:
                apex.copy_(torch.maximum(apex, torch.where(want_all[k] != 0, o["gap"], torch.full_like(apex, -float("inf")))))
            if a.anchor:
                on_ = ran_with != 0
                gap_ = o["gap"][on_].abs()
                off_ = (o["foot_pos"] - held_at).reshape(B, 4, 3).norm(dim=2)[on_]
                gap_, off_ = gap_[torch.isfinite(gap_)], off_[torch.isfinite(off_)]
                anchors.append((float(gap_.max()), float(gap_.median()), float(off_.max()), float(off_.median()),
                                int((o["events"] & 8).ne(0).sum())))
            same = float((ws == prev_ws).float().mean()) if k else float("nan")
            prev_ws.copy_(ws)
            if a.detect:
                disagree.append((float((ran_with != stance[k]).float().mean()), int((o["events"] & 1).ne(0).sum()),
                                 int((o["events"] & 2).ne(0).sum()), int((o["events"] & 4).ne(0).sum()), int((st_up == 0).sum())))
            speed = held_foot_speeds(d, ran_with)
            speed = speed[torch.isfinite(speed)]
            stats.append((int((st_qp == 0).sum()), int((st_pl == 0).sum()), same, bool(torch.isfinite(d["q"]).all()),
                          float(speed.max()), float(speed.median())))
            if a.friction:
                cone.append((int((report_f & 8).ne(0).sum()), int((report_f & 16).ne(0).sum())))
        return stats

    cone, anchors = [], []
    stats = loop(False)
    t = [loop(True) for _ in range(a.repeats + 1)][1:]
    say("closed loop: %d trot robots, %d ticks of qlamd_wholebody_solve_placed_batch (table) -> plant step in place (%s), dt %.4f s; "
        "support set switched per tick %.4f"
        % (B, K, "with contacts, k_v = %g / s" % a.velocity_gain if a.contacts else "qlamd_wholebody_forward_dynamics_batch", DT, switched))
    if a.friction:
        q4 = max(1, K // 4)
        say("  the plant step is qlamd_wholebody_plant_step_friction_batch, mu %.1f; per tick and robot: separating legs %.4f, sliding legs %.4f "
            "(first quarter %.4f / %.4f, last quarter %.4f / %.4f)"
            % (MU, np.mean([c[0] for c in cone]) / B, np.mean([c[1] for c in cone]) / B, np.mean([c[0] for c in cone[:q4]]) / B,
               np.mean([c[1] for c in cone[:q4]]) / B, np.mean([c[0] for c in cone[-q4:]]) / B, np.mean([c[1] for c in cone[-q4:]]) / B))
    if a.detect:
        say("  three launches per tick: the flags and normals come from qlamd_wholebody_contact_update_batch (%s; released at 10 mm or by a "
            "%s report), the trot's phase gives the first tick's flags only" % (a.terrain, "separating" if a.friction else "pulling"))
        say("  detection against the trot schedule: share of (tick, leg) pairs that disagree %.4f (first quarter %.4f, last quarter %.4f); "
            "per tick and robot: touchdowns %.4f, released by the report %.4f, by the gap %.4f; contact update OK %.4f"
            % (np.mean([x[0] for x in disagree]), np.mean([x[0] for x in disagree[:max(1, K // 4)]]), np.mean([x[0] for x in disagree[-max(1, K // 4):]]),
               np.mean([x[1] for x in disagree]) / B, np.mean([x[2] for x in disagree]) / B, np.mean([x[3] for x in disagree]) / B,
               np.mean([x[4] for x in disagree]) / B))
    if a.detect:
        top = apex[torch.isfinite(apex)]
        say("  apex clearance: over the %d (robot, leg) pairs the schedule wants in the air at some tick, the largest gap on those ticks: "
            "median %.4f m, largest %.4g m, share above 0.02 m %.4f, share never above 0.001 m %.4f"
            % (top.numel(), float(top.median()), float(top.max()), float((top > 0.02).float().mean()), float((top <= 0.001).float().mean())))
    if a.swing:
        say("  four launches per tick: qlamd_wholebody_swing_task_batch in front (T %.2f s, h %.2f m, k_p %g, k_d %g, e_max %g, lambda %g, "
            "|qdd| <= %g); the solve runs with its flags and accelerations" % (SWING["swing_duration"], SWING["profile_height"], SWING["position_gain"],
                                                                               SWING["velocity_gain"], SWING["max_error"], SWING["damping"], SWING["max_joint_acceleration"]))
        q4 = max(1, K // 4)
        for lo in range(0, K, q4):
            part = swing_events[lo:lo + q4]
            say("  ticks %3d-%3d: swing task OK %.4f; per tick and robot: began %.4f, landed %.4f, late lift-off %.4f, overtime %.4f"
                % (lo, lo + len(part) - 1, np.mean([x[4] for x in part]) / B, *[np.mean([x[j] for x in part]) / B for j in range(4)]))
    if a.anchor:
        say("  the update and the plant step are the anchored entries: k_p %g / s^2, e_max %g m, %s; per quarter of the run, over the feet "
            "each tick's plant step held:" % (a.position_gain, a.max_error, "a sliding foot is re-anchored" if a.friction else "no re-anchoring"))
        q4 = max(1, K // 4)
        for lo in range(0, K, q4):
            part, ev = anchors[lo:lo + q4], disagree[lo:lo + q4]
            say("  ticks %3d-%3d: held-foot |gap| m largest %.4g, median of the ticks' medians %.4g; |p - anchor| m largest %.4g, median %.4g; per "
                "tick and robot: touchdowns %.4f, released by the report %.4f, by the gap %.4f, re-anchored %.4f"
                % (lo, lo + len(part) - 1, max(x[0] for x in part), float(np.median([x[1] for x in part])), max(x[2] for x in part),
                   float(np.median([x[3] for x in part])), np.mean([x[1] for x in ev]) / B, np.mean([x[2] for x in ev]) / B,
                   np.mean([x[3] for x in ev]) / B, np.mean([x[4] for x in part]) / B))
    say("  us per tick (%s launches): %s median %.2f spread %.2f" % ("four" if a.swing else "three" if a.detect else "two", " ".join("%.2f" % x for x in t), float(np.median(t)), max(t) - min(t)))
    q = max(1, K // 4)
    for lo in range(0, K, q):
        part = stats[lo:lo + q]
        same = [p[2] for p in part if p[2] == p[2]]
        say("  ticks %3d-%3d: whole-body step OK %.4f, plant step OK %.4f, working_set_unchanged %.4f, state finite %s, "
            "held-foot speed m/s: largest %.4g, median of the ticks' medians %.4g"
            % (lo, lo + len(part) - 1, np.mean([p[0] for p in part]) / B, np.mean([p[1] for p in part]) / B, float(np.mean(same)),
               all(p[3] for p in part), max(p[4] for p in part), float(np.median([p[5] for p in part]))))
    say("  held-foot speed per tick, largest: " + " ".join("%.3g" % p[4] for p in stats))
    say("  held-foot speed per tick, median:  " + " ".join("%.3g" % p[5] for p in stats))
    same = [p[2] for p in stats if p[2] == p[2]]
    say("  all ticks: working_set_unchanged %.4f under the closed loop (open loop, bench.py's trajectory: 0.975); warm retries %d"
        % (float(np.mean(same)), ctx.counter(capi.COUNTER_WARM_RETRIES)))
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

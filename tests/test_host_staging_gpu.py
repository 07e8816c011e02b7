"""Every C-ABI entry that stages host buffers (csrc/context.hpp, Staged): the call on host buffers gives what the same call
on device arrays gives, bit for bit -- the same kernel runs on the same numbers, so anything else is a pointer that went to the
wrong array.  Two batch sizes per entry: one whose arrays total under the 256 KB up to which a host call goes through one
pinned slab (one copy each way), one over (a copy per array).  Optional arrays are passed as NULL where an entry has some:
NULL must stay NULL on the device side.  (The pose entries and the dense QP: tests/test_pose_sqp_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

from quadruped_locomotion_amd import synth

pytestmark = pytest.mark.gpu
SIZES = [16, 2000]   # per-robot footprints here are 250 B ... 8 KB: 16 robots stay under 256 KB, 2000 go over


@pytest.fixture(scope="module")
def gpu():
    import torch
    from quadruped_locomotion_amd import capi
    assert torch.cuda.is_available()
    ctx = capi.Context(device=0)
    yield capi, ctx, torch
    ctx.close()


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same(host, device, torch):
    torch.cuda.synchronize()
    assert np.array_equal(np.asarray(host), device.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("forces", [True, False])   # contact_force NULL
def test_balance_and_force_distribution(gpu, B, forces):
    capi, ctx, torch = gpu
    s = synth.make_states(B, "trot")
    tau, grf, st = ctx.balance_solve_host(s, want_forces=forces)
    d = capi.to_device(s)
    dt, dg, ds = dev(torch, np.zeros((B, 12))), dev(torch, np.zeros((B, 12))), dev(torch, np.zeros(B, np.int32))
    sb, _, _ = capi._state_batch(d, None, capi.MEM_DEVICE)
    assert capi.lib().qlamd_balance_solve_batch(ctx._h, C.byref(sb), B, dt.data_ptr(), dg.data_ptr() if forces else None,
                                                ds.data_ptr(), capi.MEM_DEVICE, None) == capi.OK
    same(tau, dt, torch); same(st, ds, torch)
    if forces:
        same(grf, dg, torch)
    assert (st == 0).sum() > B // 2 and np.abs(tau).max() > 1.0
    # the force-distribution entry (an external wrench; the pose fields alias joint_position inside the entry)
    w = capi.virtual_wrench(ctx, s)
    ht, hg, hs = capi.force_distribution(ctx, s["q"], s["base_quat"], s["stance"], w)
    dw = dev(torch, w)
    assert capi.lib().qlamd_force_distribution_batch(ctx._h, d["q"].data_ptr(), d["base_quat"].data_ptr(), d["stance"].data_ptr(), None,
                                                     dw.data_ptr(), B, dt.data_ptr(), dg.data_ptr(), ds.data_ptr(),
                                                     capi.MEM_DEVICE, None) == capi.OK
    same(ht, dt, torch); same(hg, dg, torch); same(hs, ds, torch)


@pytest.mark.parametrize("B", [16, 2000, 40000])   # (8 bytes a robot: 40 000 robots are over the pinned slab)
def test_placement_from_iterations(gpu, B):
    capi, ctx, torch = gpu
    it = np.random.default_rng(B).integers(0, 24, B).astype(np.int32)
    for policy in (capi.PLACEMENT_LATENCY, capi.PLACEMENT_THROUGHPUT):
        order = dev(torch, np.full(B, -1, np.int32))
        ctx.placement_from_iterations(dev(torch, it), order, policy=policy)
        same(ctx.placement_from_iterations(it, policy=policy), order, torch)


@pytest.mark.parametrize("B", SIZES)
def test_virtual_wrench_and_leg_kinematics(gpu, B):
    capi, ctx, torch = gpu
    s = synth.make_states(B, "trot")
    d = capi.to_device(s)
    w, foot, jac, grav = (dev(torch, np.zeros(sh)) for sh in ((B, 6), (B, 4, 3), (B, 4, 9), (B, 4, 3)))
    ctx.virtual_wrench_device(d, w)
    ctx.leg_kinematics_device(d["q"], d["base_quat"], foot, jac, grav)
    same(capi.virtual_wrench(ctx, s), w, torch)
    for h, t in zip(capi.leg_kinematics(ctx, s["q"], s["base_quat"]), (foot, jac, grav)):
        same(h, t, torch)
    assert np.abs(w.cpu().numpy()).max() > 0


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("with_id", [True, False])   # id_joint_position NULL
def test_swing_leg_torque_and_swing_branch(gpu, B, with_id):
    capi, ctx, torch = gpu
    si = synth.make_swing_inputs(B)
    s = synth.make_states(B, "trot")
    foot, _, _ = capi.leg_kinematics(ctx, si["q"], s["base_quat"])
    tpos = np.ascontiguousarray(foot.reshape(B, 12) + si["dpos"])
    q_id = np.ascontiguousarray(si["q"] + 0.01) if with_id else None
    ins = [si["q"], si["qd"], si["qd_old"], tpos, si["tvel"], si["support"]]
    host = capi.swing_leg_torque(ctx, *ins, q_id=q_id)
    out = dev(torch, np.zeros((B, 12)))
    capi.swing_leg_torque(ctx, *[dev(torch, a) for a in ins], q_id=dev(torch, q_id), memory=capi.MEM_DEVICE, out=out)
    same(host, out, torch)
    assert np.abs(host).max() > 0
    rng = np.random.default_rng(B)
    cmd, mode = rng.uniform(-1, 1, (B, 12)), rng.integers(0, 4, (B, 4)).astype(np.uint8)
    state = [np.full((B, 12), 7.0), rng.normal(size=(B, 12)), rng.normal(size=(B, 12))]   # effort, pid_error_last, pid_error_integral
    h = [a.copy() for a in state]
    t = [dev(torch, a) for a in state]
    capi.swing_branch(ctx, h[0], *ins, s["base_quat"], cmd, mode, h[1], h[2], 0.0025, q_id=q_id)
    capi.swing_branch(ctx, t[0], *[dev(torch, a) for a in ins], dev(torch, s["base_quat"]), dev(torch, cmd), dev(torch, mode), t[1], t[2],
                      0.0025, q_id=dev(torch, q_id), memory=capi.MEM_DEVICE)
    for a, b in zip(h, t):
        same(a, b, torch)
    assert (h[0] != 7.0).any() and (h[0] == 7.0).any()    # swing legs written, support legs kept


@pytest.mark.parametrize("B", SIZES)
def test_leg_state_machine(gpu, B):
    capi, ctx, torch = gpu
    rng = np.random.default_rng(B)
    flag = lambda: rng.integers(0, 2, (B, 4)).astype(np.uint8)  # noqa: E731
    io = dict(support_leg=flag(), phase=rng.choice([0.0, 0.1, 0.3, 0.6, 1.0], (B, 4)), is_footstep=flag(), contact=flag(),
              joint_position=rng.uniform(-1, 1, (B, 12)), limb_state=rng.integers(0, 9, (B, 4)).astype(np.int8), store_flag=flag(),
              stored_joint_position=rng.uniform(-1, 1, (B, 12)), joint_command=rng.uniform(-1, 1, (B, 12)),
              foot_target=rng.uniform(-0.5, 0.5, (B, 12)), support=flag(), leg_state_code=np.full((B, 4), 99, np.int8))
    d = {k: dev(torch, v) for k, v in io.items()}
    capi.leg_state_machine(ctx, io)
    capi.leg_state_machine(ctx, d, memory=capi.MEM_DEVICE)
    for k in io:
        same(io[k], d[k], torch)
    assert (io["leg_state_code"] != 99).all()


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("with_last", [True, False])   # joint_position_last NULL
def test_leg_inverse_kinematics(gpu, B, with_last):
    capi, ctx, torch = gpu
    s = synth.make_states(B, "trot")
    foot, _, _ = capi.leg_kinematics(ctx, s["q"], s["base_quat"])
    foot = foot.reshape(B, 12).copy()
    foot[::5, 1] = np.nan   # the only way to the failure branch, which reads joint_position_last
    last = s["q"] if with_last else None
    q, ok = capi.leg_inverse_kinematics(ctx, foot, last)
    dq, dok, prm = dev(torch, np.zeros((B, 12))), dev(torch, np.zeros((B, 4), np.uint8)), capi.default_ik_params()
    dl, df = dev(torch, last), dev(torch, foot)
    assert capi.lib().qlamd_leg_inverse_kinematics_batch(ctx._h, C.byref(prm), df.data_ptr(), dl.data_ptr() if with_last else None,
                                                         B, dq.data_ptr(), dok.data_ptr(), capi.MEM_DEVICE, None) == capi.OK
    same(q, dq, torch); same(ok, dok, torch)
    assert 0 < ok.sum() < ok.size


@pytest.mark.parametrize("B", SIZES)
def test_robot_state_unpack(gpu, B):
    capi, ctx, torch = gpu
    blob, off, _ = synth.make_messages(B, ragged=True)
    # a blob that does not start at offset 0: the kernel indexes with the caller's offsets
    lead = 37
    blob2 = np.concatenate([np.zeros(lead, np.uint8), np.frombuffer(bytes(blob), np.uint8)])
    off2 = np.asarray(off, np.int64) + lead
    out, st = capi.robot_state_unpack(ctx, blob2, off2)
    dout, dst = capi.robot_state_unpack_device(ctx, dev(torch, blob2), dev(torch, off2))
    same(st, dst, torch)
    for k in out:
        same(out[k], dout[k], torch)
    assert (st == 0).sum() > B // 2
    # optional outputs passed as NULL
    part, st2 = capi.robot_state_unpack(ctx, blob2, off2, want=("des_quat", "support_leg"))
    assert np.array_equal(st2, st) and np.array_equal(part["des_quat"], out["des_quat"]) and np.array_equal(part["support_leg"], out["support_leg"])


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("command", [True, False])   # io->command NULL
def test_full_tick(gpu, B, command):
    capi, ctx, torch = gpu
    blob, off, _ = synth.make_messages(B, ragged=True)
    s = synth.make_states(B, "trot")
    rng = np.random.default_rng(B)
    io = dict(messages=np.frombuffer(bytes(blob), np.uint8).copy(), offsets=np.asarray(off, np.int64), joint_position=s["q"],
              joint_velocity=rng.normal(scale=0.3, size=(B, 12)), joint_velocity_oldest=rng.normal(scale=0.3, size=(B, 12)),
              base_position=s["base_pos"], base_orientation=s["base_quat"], base_linear_velocity=np.ascontiguousarray(s["base_linvel"]),
              base_angular_velocity=np.ascontiguousarray(s["base_angvel"]), contact=rng.integers(0, 2, (B, 4)).astype(np.uint8),
              limb_state=np.zeros((B, 4), np.int8), store_flag=np.zeros((B, 4), np.uint8), stored_joint_position=np.zeros((B, 12)),
              leg_mode=np.zeros((B, 4), np.uint8), support=np.ones((B, 4), np.uint8), pid_error_last=np.zeros((B, 12)),
              pid_error_integral=np.zeros((B, 12)), joint_effort=np.full((B, 12), 7.0), leg_state_code=np.zeros((B, 4), np.int8),
              status=np.full(B, -1, np.int32), message_status=np.full(B, -1, np.int32), working_set=np.zeros(B, np.uint32))
    if command:
        io["command"] = np.zeros(capi.tick_command_bytes(B), np.uint8)
    d = {k: dev(torch, v) for k, v in io.items()}
    for _ in range(2):   # the second tick runs on the state and the working sets the first one left
        capi.full_tick(ctx, io, 0.0025)
        capi.full_tick(ctx, d, 0.0025, memory=capi.MEM_DEVICE)
        for k in io:
            same(io[k].view(np.int32) if k == "working_set" else io[k], d[k].view(torch.int32) if k == "working_set" else d[k], torch)
    assert (io["status"] == 0).sum() > B // 2 and (io["joint_effort"] != 7.0).any()


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("constrained", [True, False])   # C, c, D, d, f NULL
def test_weighted_lsq_qp(gpu, B, constrained):
    capi, ctx, torch = gpu
    rng = np.random.default_rng(B)
    n, k, p, m = 6, 8, 1, 4
    A, S, b, W = rng.normal(size=(B, k, n)), rng.uniform(0.5, 2, (B, k)), rng.normal(size=(B, k)), rng.uniform(0.01, 0.1, (B, n))
    opt = [rng.normal(size=(B, p, n)), rng.normal(size=(B, p)), rng.normal(size=(B, m, n)), -np.ones((B, m)), np.ones((B, m))] if constrained else [None] * 5
    x, st = capi.weighted_lsq_qp(ctx, A, S, b, W, *opt)
    out = (dev(torch, np.zeros((B, n))), dev(torch, np.zeros(B, np.int32)))
    capi.weighted_lsq_qp(ctx, *[dev(torch, a) for a in [A, S, b, W] + opt], memory=capi.MEM_DEVICE, out=out)
    same(x, out[0], torch); same(st, out[1], torch)
    assert (st == 0).sum() > B // 2


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("forces", [True, False])   # contact_force NULL
def test_wholebody_dynamics_and_solve(gpu, B, forces):
    capi, ctx, torch = gpu
    wb = synth.make_wholebody_states(B, "trot")
    d = capi.to_device(wb)
    h = capi.wholebody_dynamics(ctx, wb, want=("M", "h", "Jc") if forces else ("h",))   # (mass_matrix, contact_jacobian NULL)
    M, hh, Jc = dev(torch, np.zeros((B, 18, 18))), dev(torch, np.zeros((B, 18))), dev(torch, np.zeros((B, 12, 18)))
    capi.wholebody_dynamics_device(ctx, d, M if forces else None, hh, Jc if forces else None)
    same(h["h"], hh, torch)
    if forces:
        same(h["M"], M, torch); same(h["Jc"], Jc, torch)
    prm = capi.default_wholebody_params()
    keep = []
    hb = capi._wholebody_batch(wb, keep)
    tau, grf, st = np.zeros((B, 12)), np.zeros((B, 12)), np.full(B, -1, np.int32)
    assert capi.lib().qlamd_wholebody_solve_batch(ctx._h, C.byref(prm), C.byref(hb), B, tau.ctypes.data, grf.ctypes.data if forces else None,
                                                  st.ctypes.data, capi.MEM_HOST, None) == capi.OK
    dt, dg, ds = dev(torch, np.zeros((B, 12))), dev(torch, np.zeros((B, 12))), dev(torch, np.full(B, -1, np.int32))
    capi.wholebody_solve_device(ctx, d, dt, dg if forces else None, ds)
    same(tau, dt, torch); same(st, ds, torch)
    if forces:
        same(grf, dg, torch)
    assert (st == 0).sum() > B // 2 and np.abs(tau).max() > 1.0

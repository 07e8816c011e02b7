"""Every entry that reads the robot model, on the GPU, on the models of tests/robot_models.py, against the oracle compiled
on the same model (`with O.model(name):`) -- and on the default model through the same code, so that the figures stand
side by side.  One context per model.  Shapes are small (B in 1, 5, 37, 64, 67: a lone robot, a ragged wavefront, nine
full 16-lane groups plus a ragged one, all 16 support masks); the bar of every comparison is the bar of the default-model
GPU test of the same entry, taken from that test's own helper where it has one.  tests/test_model_variants_cpu.py
asserts that the oracle solves every robot of these states on every model and that the problems are conditioned like
the default's, which is what lets the bars carry over.

Each test prints `worst <entry> <model> <figure>` lines (pytest -s) for profiles/r19/model_variants.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_anchor_reference as CAR  # noqa: E402
import contact_update_reference as CUR  # noqa: E402
import plant_contacts_reference as PCR  # noqa: E402
import plant_friction_reference as PFR  # noqa: E402
import plant_reference as PR  # noqa: E402
import robot_models as RM  # noqa: E402
from oracle import oracle as O  # noqa: E402
from quadruped_locomotion_amd import synth  # noqa: E402
from test_contact_anchor_gpu import check_anchors  # noqa: E402
from test_contact_update_gpu import TOL as GEOMETRY_TOL  # noqa: E402
from test_contact_update_gpu import check as check_update  # noqa: E402
from test_contact_update_gpu import shifted, smooth_field  # noqa: E402
from test_full_tick_gpu import compare as compare_tick  # noqa: E402
from test_full_tick_gpu import fresh_state, make_tick_inputs, run_oracle_tick  # noqa: E402
from test_plant_contacts_gpu import check_four, flags_of, mask_cases  # noqa: E402
from test_plant_gpu import check_against  # noqa: E402
from test_swing_branch import branch_inputs, oracle_branch  # noqa: E402
from test_swing_leg import foot_targets  # noqa: E402

pytestmark = pytest.mark.gpu
TAU_TOL = 1e-6          # BASELINE.json north_star
DT, MU = 0.0025, 0.6
MODELS = pytest.mark.parametrize("name", RM.ALL)


@pytest.fixture(scope="module")
def contexts():
    import torch
    from quadruped_locomotion_amd import capi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ctxs = {name: capi.Context(model=None if name == "default" else RM.fill(name), device=0) for name in RM.ALL}
    yield capi, ctxs, torch
    for c in ctxs.values():
        c.close()


def worst(entry, name, value):
    print("worst %-34s %-19s %.3e" % (entry, name, value))


def all_masks(s):
    """the state dict with robot i on support mask i % 16"""
    B = s["q"].shape[0]
    return dict(s, stance=flags_of(np.arange(B) % 16))


# ---- whole-body dynamics and solve -----------------------------------------------------------------------------------------

@MODELS
def test_wholebody_dynamics(contexts, name):
    capi, _, _ = contexts
    err = dict(M=0.0, h=0.0, Jc=0.0)
    for form in (capi.DYNAMICS_ROW, capi.DYNAMICS_LEG, capi.DYNAMICS_AUTO):
        ctx = capi.Context(model=None if name == "default" else RM.fill(name), device=0)
        ctx.set_option(capi.OPT_DYNAMICS_FORM, form)
        for B in (1, 5, 37):
            s = synth.make_wholebody_states(B, "trot")
            out = capi.wholebody_dynamics(ctx, s)
            with O.model(name):
                for i in range(B):
                    q, quat = s["q"][i], s["base_quat"][i]
                    nu = np.concatenate([O.quat_to_matrix(quat).T @ s["base_linvel"][i], s["base_angvel"][i], s["qd"][i]])
                    M0, h0, J0 = O.wb_mass_matrix(q), O.wb_nonlinear_effects(q, quat, nu, 9.81), O.wb_contact_jacobian(q)
                    e = (np.abs(out["M"][i] - M0).max() / np.abs(M0).max(), np.abs(out["h"][i] - h0).max() / max(1.0, np.abs(h0).max()),
                         np.abs(out["Jc"][i] - J0).max())
                    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-12, (form, B, i, e)
                    err = dict(M=max(err["M"], e[0]), h=max(err["h"], e[1]), Jc=max(err["Jc"], e[2]))
        ctx.close()
    for k, v in err.items():
        worst("wholebody_dynamics %s" % k, name, v)


@MODELS
def test_wholebody_solve(contexts, name):
    capi, ctxs, _ = contexts
    ctx = ctxs[name]
    e_tau = 0.0
    for gait in ("trot", "static"):
        for B in (1, 5, 37):
            s = synth.make_wholebody_states(B, gait)
            tau, grf, st = capi.wholebody_solve(ctx, s)
            with O.model(name):
                t0, g0, s0 = O.wb_step_batch(s)
            assert np.array_equal(st, s0) and (st == 0).all()
            assert np.abs(tau - t0).max() < TAU_TOL and np.abs(grf - g0).max() < 1e-6
            e_tau = max(e_tau, np.abs(tau - t0).max())
    worst("wholebody_solve tau", name, e_tau)
    # every stance subset, per-leg normals, desired joint accelerations, torque limits that bind
    B = 64
    rng = np.random.default_rng(8)
    s = all_masks(synth.make_wholebody_states(B, "trot"))
    nw = np.tile(np.array([0, 0, 1.0]), (B, 4, 1)) + 0.15 * rng.normal(size=(B, 4, 3))
    s["normals"] = (nw / np.linalg.norm(nw, axis=2, keepdims=True)).reshape(B, 12)
    s["qdd_des"] = rng.normal(scale=2.0, size=(B, 12))
    prm, oprm = capi.default_wholebody_params(), O.default_wb_params()
    prm.torque_limit = oprm.torque_limit = 45.0
    tau, grf, st = capi.wholebody_solve(ctx, s, prm)
    with O.model(name):
        t0, g0, s0 = O.wb_step_batch(s, oprm)
    assert np.array_equal(st, s0)
    ok = st == 0
    assert ok.sum() > B // 2 and np.abs(tau[ok] - t0[ok]).max() < TAU_TOL
    stance_joints = np.repeat(s["stance"].astype(bool), 3, axis=1)
    assert (np.isclose(np.abs(tau), 45.0, atol=1e-6) & stance_joints & ok[:, None]).any()
    assert np.abs(tau[ok][stance_joints[ok]]).max() <= 45.0 + 1e-6
    assert np.all(tau[~ok] == 0) and np.all(grf[~ok] == 0)
    worst("wholebody_solve tau (limits bind)", name, np.abs(tau[ok] - t0[ok]).max())


# ---- the balance step --------------------------------------------------------------------------------------------------------

def balance_device(capi, torch, ctx, s, rpw):
    ctx.set_robots_per_wave(rpw)
    B = s["q"].shape[0]
    tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
    grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    ctx.balance_solve_device(capi.to_device(s), tau, grf, status, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.set_robots_per_wave(0)
    return tau.cpu().numpy(), grf.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("rpw", [0, 4, 16, 64])     # the lane-cooperative per-leg forms, and one lane per robot
@MODELS
def test_balance_step_every_kernel_form(contexts, name, rpw):
    capi, ctxs, torch = contexts
    e = 0.0
    for gait in ("trot", "static"):
        s = synth.make_states(67, gait)
        tau, grf, status = balance_device(capi, torch, ctxs[name], s, rpw)
        with O.model(name):
            t0, g0, s0 = O.balance_batch(s)
        assert (status == s0).all() and (status == 0).all()
        err = np.abs(tau - t0).max(axis=1)
        assert err.max() < TAU_TOL and np.median(err) < 1e-9 and np.abs(grf - g0).max() < 1e-6
        e = max(e, err.max())
    base = synth.make_states(16, "trot")
    for mask in range(16):
        s = {k: v.copy() for k, v in base.items()}
        s["stance"][:] = [(mask >> l) & 1 for l in range(4)]
        tau, grf, status = balance_device(capi, torch, ctxs[name], s, rpw)
        with O.model(name):
            t0, _, s0 = O.balance_batch(s)
        assert (status == s0).all()
        ok = status == 0
        assert np.abs(tau[ok] - t0[ok]).max(initial=0.0) < TAU_TOL
        e = max(e, np.abs(tau[ok] - t0[ok]).max(initial=0.0))
        if mask == 0:
            assert np.all(tau == 0) and np.all(grf == 0)
    worst("balance step rpw=%d tau" % rpw, name, e)


@MODELS
def test_balance_placed_warm_loop_and_robot_params(contexts, name):
    """The caller's loop of include/qlamd.h on a 6-tick trajectory (placement from tick k - 2, warm start from tick k - 1), and
    per-robot parameter records filled from the context's parameters: bit for bit the context-wide result."""
    capi, ctxs, torch = contexts
    ctx, B = ctxs[name], 64
    traj = synth.trajectory(B, "trot", 6)
    i32 = lambda: torch.zeros(B, dtype=torch.int32, device="cuda:0")  # noqa: E731
    orders = [torch.arange(B, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    its, ws = [i32(), i32()], i32()
    tau = torch.zeros(B, 12, dtype=torch.float64, device="cuda:0")
    grf, status = torch.zeros_like(tau), torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    e = 0.0
    for k, s_k in enumerate(traj):
        tau.zero_()
        ctx.balance_solve_placed_device(capi.to_device(s_k), tau, grf, status, order=orders[k & 1], iterations=its[k & 1],
                                        prev_iterations=its[(k - 1) & 1], next_order=orders[(k + 1) & 1], prev_working_set=ws,
                                        working_set=ws, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        with O.model(name):
            t_k, _, s_ref = O.balance_batch(s_k)
        assert (status.cpu().numpy() == s_ref).all() and (s_ref == 0).all(), k
        err = float(np.abs(tau.cpu().numpy() - t_k).max())
        assert err < TAU_TOL, (k, err)
        e = max(e, err)
        assert sorted(orders[(k + 1) & 1].cpu().numpy().tolist()) == list(range(B))
    assert int((ws != 0).sum()) > 0
    worst("balance placed + warm loop tau", name, e)
    d = capi.to_device(traj[-1])
    rec = torch.from_numpy(np.repeat(capi.robot_params_fill(ctx.params), B, axis=0)).to("cuda:0")
    tau_r, status_r = torch.zeros_like(tau), torch.full_like(status, -1)
    ctx.balance_solve_robot_params_device(d, rec, tau_r, None, status_r, stream=torch.cuda.current_stream().cuda_stream)
    ctx.balance_solve_placed_device(d, tau, None, status, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(tau_r, tau) and torch.equal(status_r, status)
    assert float(np.abs(tau.cpu().numpy() - t_k).max()) < TAU_TOL


# ---- the per-leg entries -----------------------------------------------------------------------------------------------------

@MODELS
def test_leg_kinematics_and_virtual_wrench(contexts, name):
    capi, ctxs, _ = contexts
    s = synth.make_states(37, "trot")
    w = capi.virtual_wrench(ctxs[name], s)
    foot, jac, grav = capi.leg_kinematics(ctxs[name], s["q"], s["base_quat"])
    e = dict(foot=0.0, jac=0.0, grav=0.0)
    with O.model(name):
        for i in range(37):
            assert np.allclose(w[i], O.virtual_wrench(s, i), rtol=1e-12, atol=1e-9)
            gB = O.quat_to_matrix(s["base_quat"][i]).T @ np.array([0, 0, -9.8])
            for l in range(4):
                q = s["q"][i][3 * l:3 * l + 3]
                d = (np.abs(foot[i, l] - O.leg_fk(l, q)[0]).max(), np.abs(jac[i, l].reshape(3, 3) - O.leg_jacobian(l, q)).max(),
                     np.abs(grav[i, l] - O.leg_gravity(l, q, gB)).max())
                assert d[0] <= 1e-13 and d[1] <= 1e-13 and d[2] <= 1e-12, (i, l, d)
                e = dict(foot=max(e["foot"], d[0]), jac=max(e["jac"], d[1]), grav=max(e["grav"], d[2]))
    for k, v in e.items():
        worst("leg_kinematics %s" % k, name, v)


@MODELS
def test_leg_ik(contexts, name):
    """Parity only: the analytic formula is tied to the reference's leg structure."""
    capi, ctxs, _ = contexts
    rng = np.random.default_rng(2)
    B = 37
    foot = RM.table(name)["joint_xyz"][None, :, 0] + rng.uniform(-0.45, 0.45, (B, 4, 3))
    foot[::10, :, 1] = np.nan
    last = rng.uniform(-1, 1, (B, 12))
    e = 0.0
    for geom, config in ((None, None), ((0.23, 0.308, 0.308), (2, 2, 0, 0))):
        prm = capi.default_ik_params()
        if geom:
            prm.d, prm.l1, prm.l2 = geom
            for l in range(4):
                prm.limb_config[l] = config[l]
        q, ok = capi.leg_inverse_kinematics(ctxs[name], foot.reshape(B, 12), last, prm)
        with O.model(name):
            for i in range(B):
                for l in range(4):
                    qo, oko = O.leg_ik(l, foot[i, l], prm.limb_config[l], (prm.d, prm.l1, prm.l2))
                    assert ok[i, l] == oko
                    d = np.abs(q[i, 3 * l:3 * l + 3] - (qo if oko else last[i, 3 * l:3 * l + 3])).max()
                    assert d < 1e-12
                    e = max(e, d)
    worst("leg_ik q", name, e)


@MODELS
def test_swing_leg_torque_and_swing_branch(contexts, name):
    capi, ctxs, _ = contexts
    ctx, B = ctxs[name], 37
    d = branch_inputs(B)
    with O.model(name):
        tpos = foot_targets(O, d)
        q_id = np.tile(d["q"][:, 9:12], (1, 4))
        for qid in (None, q_id):
            tau = capi.swing_leg_torque(ctx, d["q"], d["qd"], d["qd_old"], tpos, d["tvel"], d["support"], q_id=qid)
            ref = O.swing_batch(d["q"], d["qd"], d["qd_old"], tpos, d["tvel"], d["support"], q_id=qid)
            assert np.isfinite(tau).all() and np.abs(tau - ref).max() < 1e-9
            assert np.all(tau.reshape(B, 4, 3)[d["support"].astype(bool)] == 0)
        worst("swing_leg_torque tau", name, np.abs(tau - ref).max())
        eff = np.full((B, 12), 123.0)
        e_last, e_int = d["e_last"].copy(), d["e_int"].copy()
        for _ in range(2):
            capi.swing_branch(ctx, eff, d["q"], d["qd"], d["qd_old"], tpos, d["tvel"], d["support"], d["quat"], d["cmd"], d["mode"],
                              e_last, e_int, 0.0025)
        ref, rl, ri = oracle_branch(O, d, tpos, 0.0025, ticks=2)
    assert np.abs(eff - ref).max() < 1e-8
    assert np.abs(e_last - rl).max() < 1e-15 and np.abs(e_int - ri).max() < 1e-15
    worst("swing_branch effort", name, np.abs(eff - ref).max())


# ---- the plant steps ----------------------------------------------------------------------------------------------------------

def masks_case():
    s, tau = PR.case_states("trot", 64, seed_tau=11)
    masks, prev = mask_cases()
    return dict(s, stance=flags_of(masks)), tau, masks, prev


def rel(got, want):
    """worst err / (1e-6 x max(1, the robot's largest value)): the bar is 1"""
    return float((np.abs(got - want).max(axis=1) / PCR.tol(want)).max())


@MODELS
def test_forward_dynamics(contexts, name):
    capi, ctxs, _ = contexts
    s, tau, masks, _ = masks_case()
    with O.model(name):
        ref = PR.solve_batch(s, tau)
        out = capi.wholebody_forward_dynamics(ctxs[name], s, tau)
        assert (out["status"] == capi.STATUS_OK).all()
        check_against(ref, tau, out["acc"], out["f"], what="%s masks" % name)
        for B in (1, 5, 37):
            sb, tb = PR.case_states("static", B)
            ob = capi.wholebody_forward_dynamics(ctxs[name], sb, tb)
            assert (ob["status"] == capi.STATUS_OK).all()
            check_against(PR.solve_batch(sb, tb), tb, ob["acc"], ob["f"], what="%s static B=%d" % (name, B))
    off = np.repeat(s["stance"] == 0, 3, axis=1)
    assert (out["f"][off] == 0.0).all()
    worst("forward_dynamics nu' / bar", name, rel(out["acc"], ref["acc"]))
    worst("forward_dynamics f / bar", name, rel(out["f"], ref["f"]))


@pytest.mark.parametrize("kv", [0.0, 1.0 / DT])
@MODELS
def test_plant_step_with_contacts(contexts, name, kv):
    from quadruped_locomotion_amd import plant_contacts as PC
    capi, ctxs, _ = contexts
    s, tau, masks, prev = masks_case()
    with O.model(name):
        ref = PCR.solve_batch(s, tau, prev_masks=prev, kv=kv)
    out = PC.wholebody_plant_step(ctxs[name], s, tau, prev_stance=flags_of(prev), velocity_gain=kv, friction=MU)
    assert (out["status"] == capi.STATUS_OK).all()
    check_four(ref, out, "%s kv=%g" % (name, kv))
    assert np.array_equal((out["report"] & PC.CONTACT_TOUCHDOWN) != 0, flags_of(masks & ~prev) != 0)
    assert (out["report"][s["stance"] == 0] == 0).all()
    with O.model(name):
        bits, compare = PCR.report_batch(s, ref, MU)
    assert np.array_equal(out["report"][compare], bits[compare])
    for key, got in (("nu_plus", out["nu_plus"]), ("p", out["impulse"]), ("acc", out["acc"]), ("f", out["f"])):
        worst("plant contacts kv=%g %s / bar" % (kv, key), name, rel(got, ref[key]))


@pytest.mark.parametrize("kv", [0.0, 1.0 / DT])
@MODELS
def test_plant_step_with_friction(contexts, name, kv):
    from quadruped_locomotion_amd import plant_friction as PF
    capi, ctxs, _ = contexts
    s, tau, masks, prev = masks_case()
    with O.model(name):
        ref = PFR.solve_batch(s, tau, MU, prev_masks=prev, kv=kv)
        bits, compare, _ = PFR.report_batch(s, ref, MU)
    out = PF.wholebody_plant_step_friction(ctxs[name], s, tau, MU, prev_stance=flags_of(prev), velocity_gain=kv)
    assert (out["status"] == capi.STATUS_OK).all(), out["status"]
    check_four(ref, out, "%s kv=%g" % (name, kv))
    assert (~compare).sum() <= 0.01 * 256
    assert np.array_equal(out["report"][compare], bits[compare])
    assert np.array_equal((out["report"] & PFR.TOUCHDOWN) != 0, flags_of(masks & ~prev) != 0)
    for key, got in (("nu_plus", out["nu_plus"]), ("p", out["impulse"]), ("acc", out["acc"]), ("f", out["f"])):
        worst("plant friction kv=%g %s / bar" % (kv, key), name, rel(got, ref[key]))


@pytest.mark.parametrize("kv", [0.0, 1.0 / DT])
@pytest.mark.parametrize("cone", [False, True], ids=["hard", "cone"])
@MODELS
def test_plant_step_anchored(contexts, name, cone, kv):
    from quadruped_locomotion_amd import contact_anchor as CA
    capi, ctxs, _ = contexts
    s, tau, masks, prev = masks_case()
    kp, emax = 0.1 / DT ** 2, 0.002
    rng = np.random.default_rng(31)
    d = rng.normal(size=(64, 4, 3))
    d *= (rng.uniform(0.0, 0.005, (64, 4)) / np.linalg.norm(d, axis=2))[:, :, None]
    with O.model(name):
        anchors = np.ascontiguousarray((CAR.feet_world(s) + d).reshape(64, 12))
        ref = CAR.solve_batch(s, tau, anchors, kp, emax, prev_masks=prev, kv=kv, mu=MU if cone else None)
        bits, compare = CAR.report_batch(s, ref, MU, cone)
    out = CA.wholebody_plant_step_anchored(ctxs[name], s, tau, anchors, kp, emax, friction=MU, cone=cone, prev_stance=flags_of(prev),
                                           velocity_gain=kv)
    assert (out["status"] == capi.STATUS_OK).all(), out["status"]
    check_four(ref, out, "%s %s kv=%g" % (name, "cone" if cone else "hard", kv))
    err, tol = np.abs(out["position_error"] - ref["perr"]).max(axis=1), PCR.tol(ref["perr"])
    assert (err <= tol).all()
    flagged = s["stance"] != 0
    assert (flagged & ~compare).sum() <= 0.01 * 256
    assert np.array_equal(out["report"][compare], bits[compare])
    assert np.array_equal((out["report"] & 4) != 0, flags_of(masks & ~prev) != 0)
    what = "plant anchored %s kv=%g" % ("cone" if cone else "hard", kv)
    for key, got in (("nu_plus", out["nu_plus"]), ("p", out["impulse"]), ("acc", out["acc"]), ("f", out["f"])):
        worst("%s %s / bar" % (what, key), name, rel(got, ref[key]))


# ---- the contact update, plain and anchored --------------------------------------------------------------------------------------

def update_case(name, B=37):
    """Flags over all 16 masks, a report over all 32 patterns, per-robot planes through the median of the model's own feet, a fill
    of distinct finite anchors (the recipe of CAR.update_case, on the active model, not cached)."""
    s = all_masks({k: np.array(v, copy=True) for k, v in PR.case_states("trot", B)[0].items()})
    rng = np.random.default_rng(100 + B)
    abc = np.concatenate([rng.uniform(-0.3, 0.3, (B, 2)), np.ones((B, 1))], axis=1) * rng.uniform(0.5, 2.0, (B, 1))
    length = np.linalg.norm(abc, axis=1)
    d = np.array([np.median(CUR.feet(s, i)[0] @ (abc[i] / length[i])) for i in range(B)]) * length
    plane = np.ascontiguousarray(np.concatenate([abc, d[:, None]], axis=1))
    return s, rng.integers(0, 32, (B, 4)).astype(np.uint8), plane, np.ascontiguousarray(rng.uniform(100.0, 200.0, (B, 12)))


@MODELS
def test_contact_update_and_anchored_update(contexts, name):
    from quadruped_locomotion_amd import contact_anchor as CA
    from quadruped_locomotion_amd import contact_detection as CD
    _, ctxs, _ = contexts
    ctx, B = ctxs[name], 37
    field = smooth_field()
    hf = CD.heightfield(field["origin"], field["resolution"], field["heights"])
    e = {}
    with O.model(name):
        s, report, plane, sentinel = update_case(name, B)
        modes = (("plane", s, dict(plane=plane), dict(plane=plane)), ("height field", shifted(s, B), dict(hf=field), dict(hf=hf)))
        for mode, st, ref_kw, kw in modes:
            ref = CUR.update_batch(st, report=report & 7, **ref_kw, **CAR.UPDATE_RULE)
            out = CD.wholebody_contact_update(ctx, st, report=report & 7, **kw, **CAR.UPDATE_RULE)
            check_update(out, ref, "%s %s" % (name, mode))
            refa = CAR.update_batch(st, sentinel, CAR.SLIDING, report=report, **ref_kw, **CAR.UPDATE_RULE)
            anchor = sentinel.copy()
            outa = CA.wholebody_contact_update_anchored(ctx, st, anchor, reanchor_mask=CAR.SLIDING, report=report, **kw, **CAR.UPDATE_RULE)
            check_update(outa, refa, "%s anchored %s" % (name, mode))
            check_anchors(anchor, refa, sentinel, "%s anchored %s" % (name, mode), every_branch=False)
            re = (outa["events"] & CA.CONTACT_EVENT_REANCHORED) != 0
            assert np.array_equal(re[refa["compare"]], (refa["branch"] == 1)[refa["compare"]])
            smooth = ~ref["near_line"]
            for key in ("gap", "normals", "foot_pos", "foot_vel"):
                err = np.abs(out[key].reshape(ref[key].shape) - ref[key])
                e[key] = max(e.get(key, 0.0), float((err[smooth] if key in ("gap", "normals") else err).max()))
            stored = refa["compare"] & (refa["branch"] != 2)
            e["anchor"] = max(e.get("anchor", 0.0), float(np.abs(anchor.reshape(B, 4, 3) - refa["anchor"])[stored].max()))
    assert max(e.values()) <= GEOMETRY_TOL
    for k, v in e.items():
        worst("contact update %s" % k, name, v)


# ---- one whole tick ---------------------------------------------------------------------------------------------------------------

@MODELS
def test_whole_tick(contexts, name):
    """Two ticks of 64 trot robots through qlamd_tick_batch (message -> leg state machine -> balance solve for the stance legs,
    swing branch for the others) against the oracle's tick on the same model."""
    capi, ctxs, _ = contexts
    B, period = 64, 0.0025
    keep = fresh_state(B, capi)
    with O.model(name):
        states = [O.new_tick_state() for _ in range(B)]
        for b in range(B):
            for k in range(12):
                states[b].joint_effort[k] = 7.0
        e = 0.0
        for tick in range(2):
            msgs, tin = make_tick_inputs(B, tick)
            io = dict(tin, **keep)
            capi.full_tick(ctxs[name], io, period)
            st, mst, code = run_oracle_tick(O, states, msgs, tin, period)
            compare_tick(io, states, st, mst, code, tick)
            e = max(e, max(np.abs(io["joint_effort"][b] - np.array(states[b].joint_effort[:])).max() for b in range(B)))
    assert (st == 0).sum() > B // 2 and np.abs(io["joint_effort"]).max() > 1.0
    worst("whole tick joint effort", name, e)

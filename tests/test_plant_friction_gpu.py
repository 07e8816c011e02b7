"""qlamd_wholebody_plant_step_friction_batch on the GPU against tests/plant_friction_reference.py (numpy and the oracle's
solve_quadprog): parity of nu+, p, nu', f and the report, feasibility and complementarity from the device's own outputs, the hard
entry inside the cone, every support mask with four previous patterns, a rollout in place, the NULL form, the calling forms,
failures and refusals.  tests/test_plant_friction_cpu.py guards the reference itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plant_contacts_reference as PCR  # noqa: E402
import plant_friction_reference as PFR  # noqa: E402
import plant_reference as PR  # noqa: E402
from test_plant_contacts_gpu import (check_four, device_outputs, flags_of, mask_cases, step_tolerance,  # noqa: E402
                                     tilted_normals)

pytestmark = pytest.mark.gpu
DT = 0.0025
MU = 0.6
B = 64


@pytest.fixture(scope="module")
def gpu():
    import torch
    from quadruped_locomotion_amd import capi, plant_contacts, plant_friction
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plant_contacts.lib()
    plant_friction.lib()
    ctx = capi.Context(device=0)
    yield capi, plant_friction, ctx, torch
    ctx.close()


_REF, _OUT = {}, {}


def reference(gait, kv, normals):
    """States, torques, normals and the reference's solve with every robot projecting: computed once, shared, never modified."""
    key = (gait, kv, normals)
    if key not in _REF:
        s, tau = PR.case_states(gait, B)
        nw = tilted_normals(B) if normals else None
        st = dict(s, normals=nw) if normals else {k: v for k, v in s.items() if k != "normals"}
        ref = PFR.solve_batch(s, tau, MU, prev_masks=np.zeros(B, int), kv=kv, normals_world=None if nw is None else nw.reshape(B, 4, 3),
                              keep=True)
        _REF[key] = (st, tau, nw, ref)
    return _REF[key]


def device(gpu, gait, kv, normals):
    """the device's answer to reference()'s case: one call, shared by the parity and the feasibility test"""
    capi, PF, ctx, _ = gpu
    key = (gait, kv, normals)
    if key not in _OUT:
        st, tau, _, _ = reference(gait, kv, normals)
        _OUT[key] = PF.wholebody_plant_step_friction(ctx, st, tau, MU, prev_stance=np.zeros((B, 4), np.uint8), velocity_gain=kv)
    return _OUT[key]


CASES = [(g, kv, n) for g in ("trot", "static") for kv in (0.0, 1.0 / DT) for n in (False, True)]


@pytest.mark.parametrize("gait,kv,normals", CASES)
def test_parity_with_the_reference(gpu, gait, kv, normals):
    capi = gpu[0]
    st, tau, nw, ref = reference(gait, kv, normals)
    out = device(gpu, gait, kv, normals)
    print("iterations: device max %s, reference max %s" % (out["iterations"].max(axis=0), ref["iters"].max(axis=0)))
    assert (out["status"] == capi.STATUS_OK).all(), out["status"]
    check_four(ref, out, "%s kv=%g normals=%s" % (gait, kv, normals))
    nw4 = None if nw is None else nw.reshape(B, 4, 3)
    bits, compare, kind = PFR.report_batch(st, ref, MU, nw4)
    _, _, kind_p = PFR.report_batch(st, ref, MU, nw4, key="p")
    flagged = st["stance"] != 0
    left_out = int((flagged & ~compare).sum())
    counts = [int(((kind == k) & compare).sum()) for k in (1, PFR.SEPARATING, PFR.SLIDING)]
    print("report: %d flagged legs, %d left out; sticking %d, separating %d, sliding %d; the impulse slides on %d" % (
        flagged.sum(), left_out, counts[0], counts[1], counts[2], (kind_p == PFR.SLIDING).sum()))
    assert left_out <= 0.01 * flagged.sum()
    assert min(counts) >= 10, counts
    assert np.array_equal(out["report"][compare], bits[compare]), np.argwhere((out["report"] != bits) & compare)[:5]
    assert (out["report"][~flagged] == 0).all() and ((out["report"] & 3) == 0).all()
    assert (out["iterations"] >= 1).all()


@pytest.mark.parametrize("gait,kv,normals", CASES)
def test_feasibility_and_complementarity_of_the_devices_own_outputs(gpu, gait, kv, normals):
    """Nothing here but the bounds comes from the reference: the slacks of f and p, a = Js nu' - r at the device's nu+ from the
    oracle's matrices, and the kinetic energy over the impact."""
    st, tau, nw, ref = reference(gait, kv, normals)
    out = device(gpu, gait, kv, normals)
    tol_f, tol_p, tol_acc, tol_nu = (PCR.tol(ref[k]) for k in ("f", "p", "acc", "nu_plus"))
    worst = dict(slack=0.0, normal=0.0, stick=0.0, energy=0.0)
    sticking = 0
    for i in range(B):
        mask = int(ref["mask"][i])
        fr = PFR.frames(st["base_quat"][i], None if nw is None else nw.reshape(B, 4, 3)[i])
        for y, t in ((out["f"][i], tol_f[i]), (out["impulse"][i], tol_p[i])):
            sl = PFR.slacks(y, mask, fr, MU)
            assert (sl >= -(1.0 + MU) * t).all(), (i, sl.min(), t)
            worst["slack"] = max(worst["slack"], float((-sl / ((1.0 + MU) * t)).max()))
        R = ref["robots"][i]
        M, Js, H0, rows, legs = R["M"], R["Js"], R["H0"], R["rows"], R["legs"]
        nup = out["nu_plus"][i]
        r = -PR.gamma(st["q"][i], nup)[rows] - kv * (Js @ nup)
        a = Js @ out["acc"][i] - r
        bound = np.abs(H0).sum(axis=1).max() * tol_f[i] + np.abs(Js).sum(axis=1).max() * tol_acc[i]
        for k, l in enumerate(legs):
            al = a[3 * k:3 * k + 3]
            assert al @ fr[l][0] >= -bound, (i, l, al @ fr[l][0], bound)
            worst["normal"] = max(worst["normal"], float(-(al @ fr[l][0]) / bound))
            if out["report"][i, l] & (PFR.SEPARATING | PFR.SLIDING) == 0:
                sticking += 1
                assert np.abs(al).max() <= bound, (i, l, np.abs(al).max(), bound)
                worst["stick"] = max(worst["stick"], float(np.abs(al).max() / bound))
        nu = ref["nu"][i]
        e0, e1 = 0.5 * nu @ M @ nu, 0.5 * nup @ M @ nup
        e_bound = np.abs(M @ nup).sum() * tol_nu[i] + 1e-12 * max(1.0, e0)
        assert e1 <= e0 + e_bound, (i, e0, e1)
        worst["energy"] = max(worst["energy"], float((e1 - e0) / e_bound))
    print("worst / bound: %s; sticking legs %d" % (", ".join("%s %.3e" % kv_ for kv_ in worst.items()), sticking))
    assert sticking >= 10


@pytest.mark.parametrize("gait", ["trot", "static"])
def test_inside_the_cone_it_is_the_hard_entry(gpu, gait):
    """The controller's own torques, mu = 1, k_v = 0, no touchdown: the working set is empty on every robot."""
    capi, PF, ctx, _ = gpu
    from oracle import oracle as O
    from quadruped_locomotion_amd import plant_contacts as PC
    s, _ = PR.case_states(gait, B)
    tau, _, stt = O.wb_step_batch(s)
    assert (stt == 0).all()
    st = {k: v for k, v in s.items() if k != "normals"}
    prev = np.ascontiguousarray(s["stance"], dtype=np.uint8)
    hard = PC.wholebody_plant_step(ctx, st, tau, prev_stance=prev)
    out = PF.wholebody_plant_step_friction(ctx, st, tau, 1.0, prev_stance=prev)
    assert (out["status"] == capi.STATUS_OK).all() and (hard["status"] == capi.STATUS_OK).all()
    for k in ("f", "acc"):
        err, tol = np.abs(out[k] - hard[k]).max(axis=1), PCR.tol(hard[k])
        print("%s %s against the hard entry: max err %.3e, worst err / tol %.3e" % (gait, k, err.max(), (err / tol).max()))
        assert (err <= tol).all(), k
    assert (out["report"] == 0).all()
    assert np.array_equal(out["nu_plus"], hard["nu_plus"]) and (out["impulse"] == 0.0).all() and (out["iterations"][:, 0] == 0).all()
    assert (out["iterations"][:, 1] == 1).all()      # one selection, which finds no violated row


def test_all_16_masks_and_four_previous_patterns(gpu):
    """Projecting and non-projecting robots share wavefronts: the previous flags are shuffled over the batch; mask 0 is among them."""
    capi, PF, ctx, _ = gpu
    from quadruped_locomotion_amd import plant_contacts as PC
    s, tau = PR.case_states("trot", B, seed_tau=11)
    masks, prev = mask_cases()
    s = dict(s, stance=flags_of(masks))
    kv = 1.0 / DT
    ref = PFR.solve_batch(s, tau, MU, prev_masks=prev, kv=kv)
    out = PF.wholebody_plant_step_friction(ctx, s, tau, MU, prev_stance=flags_of(prev), velocity_gain=kv)
    assert (out["status"] == capi.STATUS_OK).all(), out["status"]
    check_four(ref, out, "masks")
    bits, compare, _ = PFR.report_batch(s, ref, MU)
    assert (~compare).sum() <= 2
    assert np.array_equal(out["report"][compare], bits[compare])
    quiet = (masks & ~prev) == 0
    assert quiet.sum() == 34
    nu_in = PC.wholebody_plant_step(ctx, s, tau, want=("nu_plus",))["nu_plus"]       # the hard entry without a touchdown: nu
    assert np.array_equal(out["nu_plus"][quiet], nu_in[quiet]) and (out["impulse"][quiet] == 0.0).all()
    assert (out["iterations"][quiet, 0] == 0).all() and (out["iterations"][~quiet, 0] >= 1).all()
    # (a projecting robot all of whose feet come moving away from the ground gets p = 0 and keeps nu: unlike the hard entry's, a
    # touchdown here need not change the velocity.  Where the reference's impulse is above its tolerance the velocity moves.)
    struck = ~quiet & (np.abs(ref["p"]).max(axis=1) > PCR.tol(ref["p"]))
    assert struck.sum() >= 20 and (out["nu_plus"][struck] != nu_in[struck]).any(axis=1).all()
    off = np.repeat(s["stance"] == 0, 3, axis=1)
    assert (out["f"][off] == 0.0).all() and (out["impulse"][off] == 0.0).all()
    assert (out["report"][s["stance"] == 0] == 0).all()
    assert np.array_equal((out["report"] & PFR.TOUCHDOWN) != 0, flags_of(masks & ~prev) != 0)


def test_rollout_in_place(gpu):
    """16 steps on 8 trot robots, in place on the device; the diagonal pairs swap at steps 5 and 11 and the previous flags are the
    step before's.  At every step the reference restarts from the device's previous state."""
    capi, PF, ctx, torch = gpu
    n = 8
    s, tau_np = PR.case_states("trot", n)
    kv = 1.0 / DT
    masks = np.where(np.arange(n) % 2 == 0, 0b0101, 0b1010)
    s = dict(s, stance=flags_of(masks))
    d = capi.to_device(s)
    tau = torch.from_numpy(tau_np).to("cuda:0")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    prev_t = torch.zeros(n, 4, dtype=torch.uint8, device="cuda:0")
    nu_plus = torch.zeros(n, 18, dtype=torch.float64, device="cuda:0")
    prev_masks = np.zeros(n, int)
    worst, touchdowns = 0.0, 0
    for k in range(16):
        if k in (5, 11):
            masks = masks ^ 0xF
            d["stance"] = torch.from_numpy(flags_of(masks)).to("cuda:0")
        before = {key: d[key].cpu().numpy().copy() for key in d}
        PF.wholebody_plant_step_friction_device(ctx, d, tau, st, MU, dt=DT, next=d, prev_stance=prev_t, velocity_gain=kv, nu_plus=nu_plus)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == capi.STATUS_OK).all(), k
        ref = PFR.solve_batch(before, tau_np, MU, prev_masks=prev_masks, kv=kv)
        touchdowns += int((ref["touch"] != 0).sum())
        want = PCR.step_batch(before, ref, DT)
        tol_nu = PCR.tol(ref["nu_plus"])
        assert (np.abs(nu_plus.cpu().numpy() - ref["nu_plus"]).max(axis=1) <= tol_nu).all(), k
        for key in PR.NEXT_KEYS:
            got = d[key].cpu().numpy()
            err, tol = np.abs(got - want[key]), tol_nu[:, None] + step_tolerance(ref["acc"], want[key])
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (k, key, err.max())
            assert not np.array_equal(got, before[key]), (k, key)
        assert np.abs(np.linalg.norm(d["base_quat"].cpu().numpy(), axis=1) - 1.0).max() <= 1e-15
        prev_masks = masks.copy()
        prev_t.copy_(d["stance"])
    assert touchdowns == 3 * n
    print("rollout: worst error / tolerance over 16 steps %.3e" % worst)


def test_friction_null_is_the_contacts_entry(gpu):
    capi, PF, ctx, _ = gpu
    from quadruped_locomotion_amd import plant_contacts as PC
    s, tau = PR.case_states("trot", 5)
    prev = flags_of(np.arange(5) % 3 * 5)
    kw = dict(dt=DT, prev_stance=prev, velocity_gain=1.0 / DT)
    hard = PC.wholebody_plant_step(ctx, s, tau, friction=MU, **kw)
    null = PF.wholebody_plant_step_friction(ctx, s, tau, MU, with_friction=False, **kw)
    assert "iterations" not in null
    for k in ("acc", "f", "status", "nu_plus", "impulse", "report"):
        assert np.array_equal(null[k], hard[k]), k
    for k in PR.NEXT_KEYS:
        assert np.array_equal(null["next"][k], hard["next"][k]), k
    assert (hard["report"] & 3).any()                   # the hard entry's own bits: this IS that entry


def device_call(PF, ctx, d, dtau, o, prev, kv, stream=None):
    n = d["q"].shape[0]
    PF.wholebody_plant_step_friction_device(ctx, d, dtau, o["st"][:n], MU, acc=o["acc"][:n], f=o["f"][:n], dt=DT,
                                            next={k: v[:n] for k, v in o["next"].items()}, prev_stance=prev, velocity_gain=kv,
                                            nu_plus=o["nu_plus"][:n], impulse=o["impulse"][:n], report=o["report"][:n],
                                            iterations=o["iterations"][:n], stream=stream)


def outputs(torch, n, fill=0.0):
    o = device_outputs(torch, n, fill)
    o["iterations"] = torch.full((n, 2), int(fill), dtype=torch.int32, device="cuda:0")
    return o


KEYS = (("acc", "acc"), ("f", "f"), ("nu_plus", "nu_plus"), ("impulse", "impulse"), ("report", "report"), ("iterations", "iterations"),
        ("st", "status"))


@pytest.mark.parametrize("n", [13, 64])      # a ragged batch, and 16 full wavefronts
def test_host_call_device_call_and_graph_replay_agree(gpu, n):
    capi, PF, ctx, torch = gpu
    s, tau = PR.case_states("trot", n)
    prev = flags_of(np.arange(n) % 3 * 5)
    kv = 1.0 / DT
    host = PF.wholebody_plant_step_friction(ctx, s, tau, MU, dt=DT, prev_stance=prev, velocity_gain=kv)
    assert (host["status"] == capi.STATUS_OK).all()
    # one row more than the batch in every output: the last, partly filled wavefront writes nothing past it
    d, dtau, dprev = capi.to_device(s), torch.from_numpy(tau).to("cuda:0"), torch.from_numpy(prev).to("cuda:0")
    eager, rep = outputs(torch, n + 1, fill=249.0), outputs(torch, n + 1, fill=249.0)
    eager["st"].fill_(-7); rep["st"].fill_(-7)
    device_call(PF, ctx, d, dtau, eager, dprev, kv)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            device_call(PF, ctx, d, dtau, rep, dprev, kv, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(rep["st"][0]) == -7  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for o in (eager, rep):
        for k, hk in KEYS:
            assert np.array_equal(o[k][:n].cpu().numpy(), host[hk]), k
            assert (o[k][n] == (-7 if k == "st" else 249)).all(), k
        for k in PR.NEXT_KEYS:
            assert np.array_equal(o["next"][k][:n].cpu().numpy(), host["next"][k]), k
            assert (o["next"][k][n] == 249.0).all(), k
    ref = PFR.solve_batch(s, tau, MU, prev_masks=np.arange(n) % 3 * 5, kv=kv)
    check_four(ref, host, "ragged B=%d" % n)


def test_a_failed_robot_fails_alone(gpu):
    """A NaN joint angle: NOT_PD for that robot alone; nu as it came, zeros and its state as it came -- or, with
    QLAMD_ON_FAILURE_KEEP, nothing of it touched."""
    capi, PF, _, torch = gpu
    from quadruped_locomotion_amd import plant_contacts as PC
    n = 7
    s, tau = PR.case_states("trot", n)
    prev = np.zeros((n, 4), np.uint8)
    ctx = capi.Context(device=0)
    kw = dict(dt=DT, prev_stance=prev, velocity_gain=1.0 / DT)
    clean = PF.wholebody_plant_step_friction(ctx, s, tau, MU, **kw)
    assert (clean["status"] == capi.STATUS_OK).all()
    bad = {k: np.array(v, copy=True) for k, v in s.items()}
    bad["q"][2, 4] = np.nan
    others = np.arange(n) != 2
    out = PF.wholebody_plant_step_friction(ctx, bad, tau, MU, **kw)
    assert out["status"][2] == capi.STATUS_NOT_PD and (out["status"][others] == capi.STATUS_OK).all()
    assert (out["acc"][2] == 0.0).all() and (out["f"][2] == 0.0).all() and (out["impulse"][2] == 0.0).all() and (out["report"][2] == 0).all()
    nu_in = PC.wholebody_plant_step(ctx, s, tau)["nu_plus"]          # no touchdown: nu+ = nu, as the device forms R' v
    assert np.array_equal(out["nu_plus"][2], nu_in[2])
    for k in PR.NEXT_KEYS:
        assert np.array_equal(out["next"][k][others], clean["next"][k][others]), k
        assert np.array_equal(out["next"][k][2], bad[k][2], equal_nan=True), k
    for k in ("acc", "f", "nu_plus", "impulse", "report", "iterations"):
        assert np.array_equal(out[k][others], clean[k][others]), k
    # KEEP, on the device, in place: sentinels and the state stay
    ctx.set_option(capi.OPT_ON_FAILURE, capi.ON_FAILURE_KEEP)
    d = capi.to_device(bad)
    o = outputs(torch, n, fill=249.0)
    PF.wholebody_plant_step_friction_device(ctx, d, torch.from_numpy(tau).to("cuda:0"), o["st"], MU, acc=o["acc"], f=o["f"], dt=DT,
                                            next=d, prev_stance=torch.from_numpy(prev).to("cuda:0"), velocity_gain=1.0 / DT,
                                            nu_plus=o["nu_plus"], impulse=o["impulse"], report=o["report"], iterations=o["iterations"])
    torch.cuda.synchronize()
    assert o["st"].cpu().numpy().tolist() == [0, 0, capi.STATUS_NOT_PD, 0, 0, 0, 0]
    for k in ("acc", "f", "nu_plus", "impulse", "report", "iterations"):
        assert (o[k][2] == 249).all() and np.array_equal(o[k][others].cpu().numpy(), clean[k][others]), k
    for k in PR.NEXT_KEYS:
        assert np.array_equal(d[k][2].cpu().numpy(), bad[k][2], equal_nan=True), k
        assert np.array_equal(d[k].cpu().numpy()[others], clean["next"][k][others]), k
    ctx.close()


def test_refusals_write_nothing(gpu):
    capi, PF, ctx, _ = gpu
    from quadruped_locomotion_amd import plant_contacts as PC
    n = 5
    s, tau = PR.case_states("trot", n)
    keep = []
    wb = capi._wholebody_batch(s, keep)
    pos = np.ascontiguousarray(s["base_pos"])
    outs = dict(acc=np.full((n, 18), -7.0), f=np.full((n, 12), -7.0), status=np.full(n, -7, np.int32), nu_plus=np.full((n, 18), -7.0),
                impulse=np.full((n, 12), -7.0), report=np.full((n, 4), 249, np.uint8), iterations=np.full((n, 2), -7, np.int32))
    nxt_arrays = {k: np.full((n, m), -7.0) for _, k, m in capi.PLANT_NEXT_FIELDS}
    nxt = capi.PlantNext(*[nxt_arrays[k].ctypes.data for _, k, _ in capi.PLANT_NEXT_FIELDS])
    fn = PF.lib().qlamd_wholebody_plant_step_friction_batch
    pf = PF.PlantFriction(outs["iterations"].ctypes.data)

    def call(tau_p=tau.ctypes.data, pos_p=pos.ctypes.data, dt=DT, batch=n, status_p=outs["status"].ctypes.data, kv=0.0, mu=MU,
             contacts=True):
        pc = PC.PlantContacts(None, kv, mu, outs["nu_plus"].ctypes.data, outs["impulse"].ctypes.data, outs["report"].ctypes.data)
        return fn(ctx._h, C.addressof(wb), tau_p, None, pos_p, 9.81, dt, batch, outs["acc"].ctypes.data, outs["f"].ctypes.data,
                  C.addressof(nxt), C.addressof(pc) if contacts else None, C.addressof(pf), status_p, capi.MEM_HOST, None)

    refused = [call(tau_p=None), call(status_p=None), call(pos_p=None), call(batch=-1), call(contacts=False)]
    refused += [call(dt=v) for v in (0.0, -DT, float("nan"), float("inf"))]
    refused += [call(kv=v) for v in (-1.0, float("nan"), float("inf"))]
    refused += [call(mu=v) for v in (0.0, -0.1, float("nan"), float("inf"))]
    assert refused == [capi.ERR_INVALID_ARGUMENT] * 16
    for a in list(outs.values()) + list(nxt_arrays.values()):
        assert ((a == -7) | (a == 249)).all()
    assert call() == capi.OK
    assert (outs["status"] == capi.STATUS_OK).all() and not (outs["report"] == 249).any() and not (outs["iterations"] == -7).any()
    assert not (nxt_arrays["q"] == -7.0).any()

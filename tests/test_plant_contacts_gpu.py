"""qlamd_wholebody_plant_step_batch on the GPU against tests/plant_contacts_reference.py (numpy, from the oracle's M, h, Jc):
the impact, the stabilised dynamics, every support mask with four previous patterns, the contact report, the state update and a
rollout in place, the NULL form, the calling forms, failures and refusals.  tests/test_plant_contacts_cpu.py guards the
reference itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plant_contacts_reference as PCR  # noqa: E402
import plant_reference as PR  # noqa: E402
from quadruped_locomotion_amd import plant_contacts as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DT = 0.0025
MU = 0.6


@pytest.fixture(scope="module")
def gpu():
    import torch
    from quadruped_locomotion_amd import capi, plant_contacts
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plant_contacts.lib()
    ctx = capi.Context(device=0)
    yield capi, ctx, torch
    ctx.close()


def step_tolerance(ref_acc, value):
    """tests/test_plant_gpu.py's: dt x (the acceleration tolerance of the robot) + 1e-12 x max(1, |value|)"""
    tol_a = 1e-6 * np.maximum(1.0, np.abs(ref_acc).max(axis=1))
    return DT * tol_a[:, None] + 1e-12 * np.maximum(1.0, np.abs(value))


def flags_of(masks):
    return np.ascontiguousarray(((np.asarray(masks)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8))


def check_four(ref, out, what):
    """nu+, p, nu', f: each within 1e-6 x max(1, largest value of that robot) of the reference"""
    for key, got in (("nu_plus", out["nu_plus"]), ("p", out["impulse"]), ("acc", out["acc"]), ("f", out["f"])):
        err, tol = np.abs(got - ref[key]).max(axis=1), PCR.tol(ref[key])
        print("%s %-7s max err %.3e, worst err / tol %.3e" % (what, key, err.max(), (err / tol).max()))
        assert (err <= tol).all(), (what, key, err.max(), int(np.argmax(err / tol)))


_REF = {}


def reference(gait, kv):
    """States, torques and the reference's solve with every robot projecting: computed once, shared, never modified."""
    if (gait, kv) not in _REF:
        s, tau = PR.case_states(gait, 64)
        _REF[(gait, kv)] = (s, tau, PCR.solve_batch(s, tau, prev_masks=np.zeros(64, int), kv=kv))
    return _REF[(gait, kv)]


@pytest.mark.parametrize("gait", ["trot", "static"])
@pytest.mark.parametrize("kv", [0.0, 1.0 / DT])
def test_impact_and_dynamics_match_the_reference(gpu, gait, kv):
    capi, ctx, _ = gpu
    s, tau, ref = reference(gait, kv)
    out = PC.wholebody_plant_step(ctx, s, tau, prev_stance=np.zeros((64, 4), np.uint8), velocity_gain=kv)
    assert (out["status"] == capi.STATUS_OK).all()
    check_four(ref, out, "%s kv=%g" % (gait, kv))
    # the projected feet stand still.  The reference's nu+ has Js nu+ = 0 to 1e-12 x max(1, |Js nu|) (test_plant_contacts_cpu.py) and
    # the device's nu+ lies within tol of it, so every row of Js nu+ is at most (that row's 1-norm) x tol + 1e-12 x max(1, |Js nu|)
    before, after, worst = 0.0, 0.0, 0.0
    tol_nu = PCR.tol(ref["nu_plus"])
    for i in range(64):
        Js = PR.O.wb_contact_jacobian(s["q"][i])[PR.rows_of(int(ref["mask"][i]))]
        came, left = np.abs(Js @ ref["nu"][i]), np.abs(Js @ out["nu_plus"][i])
        bound = np.abs(Js).sum(axis=1) * tol_nu[i] + 1e-12 * max(1.0, came.max())
        assert (left <= bound).all(), (i, left.max(), bound.min())
        before, after, worst = max(before, came.max()), max(after, left.max()), max(worst, (left / bound).max())
    print("held feet, |Js nu|: %.3e m/s before the impact, %.3e after (worst / bound %.3e)" % (before, after, worst))
    assert before > 0.1


def mask_cases():
    """mask i % 16; previous flags by one of four patterns -- 0, the mask, the mask without its lowest leg, 0xF -- picked by
    i // 16 and then shuffled among the four robots of each mask, so that all 64 combinations stay and every wavefront mixes them"""
    masks = np.arange(64) % 16
    pattern = np.arange(64) // 16
    rng = np.random.default_rng(3)
    for m in range(16):
        pattern[m::16] = rng.permutation(4)
    lowest = masks & -masks
    prev = np.select([pattern == 0, pattern == 1, pattern == 2], [np.zeros(64, int), masks, masks & ~lowest], 0xF)
    return masks, prev


def test_all_16_masks_and_four_previous_patterns(gpu):
    """Projecting and non-projecting robots share wavefronts: the previous flags are shuffled over the batch."""
    capi, ctx, _ = gpu
    s, tau = PR.case_states("trot", 64, seed_tau=11)
    masks, prev = mask_cases()
    s = dict(s, stance=flags_of(masks))
    kv = 1.0 / DT
    ref = PCR.solve_batch(s, tau, prev_masks=prev, kv=kv)
    out = PC.wholebody_plant_step(ctx, s, tau, prev_stance=flags_of(prev), velocity_gain=kv, friction=MU)
    assert (out["status"] == capi.STATUS_OK).all()
    check_four(ref, out, "masks")
    quiet = (masks & ~prev) == 0
    assert quiet.sum() == 34 and sum(0 < quiet[w:w + 4].sum() < 4 for w in range(0, 64, 4)) >= 12    # wavefronts that hold both kinds
    # nu as the device forms it (v = R' v_W in its own arithmetic; w and qd are the inputs' bits): a call without a touchdown
    nu_in = PC.wholebody_plant_step(ctx, s, tau, want=("nu_plus",))["nu_plus"]
    assert np.array_equal(nu_in[:, 3:6], s["base_angvel"]) and np.array_equal(nu_in[:, 6:], s["qd"])
    assert np.abs(nu_in - ref["nu"]).max() <= 1e-15
    assert np.array_equal(out["nu_plus"][quiet], nu_in[quiet]) and (out["impulse"][quiet] == 0.0).all()
    assert not (out["nu_plus"][~quiet] == nu_in[~quiet]).all(axis=1).any()
    assert np.abs(out["impulse"][~quiet]).max(axis=1).min() > 0.0
    off = np.repeat(s["stance"] == 0, 3, axis=1)
    assert (out["f"][off] == 0.0).all() and (out["impulse"][off] == 0.0).all()
    assert np.array_equal((out["report"] & PC.CONTACT_TOUCHDOWN) != 0, flags_of(masks & ~prev) != 0)
    assert (out["report"][s["stance"] == 0] == 0).all()


def tilted_normals(B, seed=9, most=0.3):
    """unit world normals [B, 12]: z turned by up to `most` rad about a random horizontal axis"""
    rng = np.random.default_rng(seed)
    ang, az = rng.uniform(0.0, most, (B, 4)), rng.uniform(0.0, 2.0 * np.pi, (B, 4))
    n = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=2)
    return np.ascontiguousarray(n.reshape(B, 12))


@pytest.mark.parametrize("gait", ["trot", "static"])
@pytest.mark.parametrize("normals", [False, True])
def test_contact_report(gpu, gait, normals):
    capi, ctx, _ = gpu
    s, tau, ref = reference(gait, 0.0)
    nw = tilted_normals(64) if normals else None
    st = dict(s, normals=nw) if normals else {k: v for k, v in s.items() if k != "normals"}
    out = PC.wholebody_plant_step(ctx, st, tau, prev_stance=np.zeros((64, 4), np.uint8), friction=MU)
    assert (out["status"] == capi.STATUS_OK).all()
    bits, compare = PCR.report_batch(s, ref, MU, None if nw is None else nw.reshape(64, 4, 3))
    flagged = s["stance"] != 0
    left_out = int((flagged & ~compare).sum())
    print("report %s normals=%s: %d of %d flagged legs left out; pulls %d, outside %d" % (
        gait, normals, left_out, flagged.sum(), ((bits & 1) != 0).sum(), ((bits & 2) != 0).sum()))
    assert left_out <= 0.01 * flagged.sum()
    assert np.array_equal(out["report"][compare], bits[compare])
    assert (out["report"][~flagged] == 0).all()
    assert np.array_equal((out["report"] & 4) != 0, flagged)          # previous flags of zero: every flagged leg touches down


def test_state_update_and_rollout_in_place(gpu):
    """16 steps on 8 trot robots, in place on the device; the diagonal pairs swap at steps 5 and 11 and the previous flags are the
    step before's.  At every step the reference restarts from the device's previous state."""
    capi, ctx, torch = gpu
    s, tau_np = PR.case_states("trot", 8)
    B, kv = 8, 1.0 / DT
    masks = np.where(np.arange(B) % 2 == 0, 0b0101, 0b1010)
    s = dict(s, stance=flags_of(masks))
    d = capi.to_device(s)
    tau = torch.from_numpy(tau_np).to("cuda:0")
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    prev_t = torch.zeros(B, 4, dtype=torch.uint8, device="cuda:0")
    nu_plus = torch.zeros(B, 18, dtype=torch.float64, device="cuda:0")
    prev_masks = np.zeros(B, int)
    worst, touchdowns = 0.0, 0
    for k in range(16):
        if k in (5, 11):
            masks = masks ^ 0xF
            d["stance"] = torch.from_numpy(flags_of(masks)).to("cuda:0")
        before = {key: d[key].cpu().numpy().copy() for key in d}
        PC.wholebody_plant_step_device(ctx, d, tau, st, dt=DT, next=d, prev_stance=prev_t, velocity_gain=kv, nu_plus=nu_plus)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == capi.STATUS_OK).all(), k
        ref = PCR.solve_batch(before, tau_np, prev_masks=prev_masks, kv=kv)
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
    assert touchdowns == 3 * B
    speed = PCR.held_foot_speeds({key: d[key].cpu().numpy() for key in d}, masks).max()
    print("rollout: worst error / tolerance over 16 steps %.3e; largest held-foot speed at the end %.3e m/s" % (worst, speed))


def test_contacts_null_is_the_old_entry_and_all_off_agrees(gpu):
    capi, ctx, _ = gpu
    s, tau = PR.case_states("trot", 5)
    old = capi.wholebody_forward_dynamics(ctx, s, tau, dt=DT)
    null = PC.wholebody_plant_step(ctx, s, tau, dt=DT, contacts=False)
    for k in ("acc", "f", "status"):
        assert np.array_equal(null[k], old[k]), k
    for k in PR.NEXT_KEYS:
        assert np.array_equal(null["next"][k], old["next"][k]), k
    off = PC.wholebody_plant_step(ctx, s, tau, dt=DT, want=())
    assert (off["status"] == capi.STATUS_OK).all() and "nu_plus" not in off and "report" not in off
    tol_a, tol_f = PR.tolerances(old["acc"], old["f"])
    ea, ef = np.abs(off["acc"] - old["acc"]).max(axis=1), np.abs(off["f"] - old["f"]).max(axis=1)
    print("everything off against the old entry: nu' %.3e f %.3e, bit-identical: %s" % (
        ea.max(), ef.max(), np.array_equal(off["acc"], old["acc"]) and np.array_equal(off["f"], old["f"])))
    assert (ea <= tol_a).all() and (ef <= tol_f).all()
    for k in PR.NEXT_KEYS:
        assert (np.abs(off["next"][k] - old["next"][k]) <= step_tolerance(old["acc"], old["next"][k])).all(), k


def device_outputs(torch, B, fill=0.0):
    mk = lambda n, dtype=torch.float64: torch.full((B, n), fill, dtype=dtype, device="cuda:0")  # noqa: E731
    return dict(acc=mk(18), f=mk(12), nu_plus=mk(18), impulse=mk(12), report=mk(4, torch.uint8),
                st=torch.full((B,), -7, dtype=torch.int32, device="cuda:0"),
                next=dict(q=mk(12), qd=mk(12), base_pos=mk(3), base_quat=mk(4), base_linvel=mk(3), base_angvel=mk(3)))


def device_call(capi, ctx, d, dtau, o, prev, kv, stream=None):
    """every output given; `o` may hold more rows than the batch (the wrapper wants exactly B: the first B rows are passed)"""
    B = d["q"].shape[0]
    PC.wholebody_plant_step_device(ctx, d, dtau, o["st"][:B], acc=o["acc"][:B], f=o["f"][:B], dt=DT,
                                     next={k: v[:B] for k, v in o["next"].items()}, prev_stance=prev, velocity_gain=kv, friction=MU,
                                     nu_plus=o["nu_plus"][:B], impulse=o["impulse"][:B], report=o["report"][:B], stream=stream)


@pytest.mark.parametrize("B", [5, 7, 64])      # two ragged batches, and 16 full wavefronts
def test_host_and_device_calls_agree_and_ragged_batches(gpu, B):
    capi, ctx, torch = gpu
    s, tau = PR.case_states("trot", B)
    prev = flags_of(np.arange(B) % 3 * 5)
    kv = 1.0 / DT
    host = PC.wholebody_plant_step(ctx, s, tau, dt=DT, prev_stance=prev, velocity_gain=kv, friction=MU)
    assert (host["status"] == capi.STATUS_OK).all()
    # one row more than the batch in every output: the last, partly filled wavefront writes nothing past it
    o = device_outputs(torch, B + 1, fill=249.0)
    device_call(capi, ctx, capi.to_device(s), torch.from_numpy(tau).to("cuda:0"), o, torch.from_numpy(prev).to("cuda:0"), kv)
    torch.cuda.synchronize()
    for k, hk in (("acc", "acc"), ("f", "f"), ("nu_plus", "nu_plus"), ("impulse", "impulse"), ("report", "report"), ("st", "status")):
        assert np.array_equal(o[k][:B].cpu().numpy(), host[hk]), k
        assert (o[k][B] == (-7 if k == "st" else 249)).all(), k
    for k in PR.NEXT_KEYS:
        assert np.array_equal(o["next"][k][:B].cpu().numpy(), host["next"][k]), k
        assert (o["next"][k][B] == 249.0).all(), k
    ref = PCR.solve_batch(s, tau, prev_masks=np.arange(B) % 3 * 5, kv=kv)
    check_four(ref, host, "ragged B=%d" % B)


def test_captured_call_replays_to_the_eager_result(gpu):
    capi, _, torch = gpu
    B = 7
    s, tau = PR.case_states("trot", B)
    ctx = capi.Context(device=0)          # (no qlamd_reserve: a device call of this entry uses no scratch of the context's)
    d, dtau = capi.to_device(s), torch.from_numpy(tau).to("cuda:0")
    prev = torch.zeros(B, 4, dtype=torch.uint8, device="cuda:0")
    eager, rep = device_outputs(torch, B), device_outputs(torch, B)
    device_call(capi, ctx, d, dtau, eager, prev, 1.0 / DT)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            device_call(capi, ctx, d, dtau, rep, prev, 1.0 / DT, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(rep["st"][0]) == -7  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert (eager["st"] == 0).all()
    for k in ("st", "acc", "f", "nu_plus", "impulse", "report"):
        assert torch.equal(rep[k], eager[k]), k
    for k in PR.NEXT_KEYS:
        assert torch.equal(rep["next"][k], eager["next"][k]), k
    ctx.close()


def test_a_failed_robot(gpu):
    """A NaN joint angle: NOT_PD for that robot alone; nu as it came, zeros and its state as it came -- or, with
    QLAMD_ON_FAILURE_KEEP, nothing of it touched."""
    capi, _, torch = gpu
    B = 7
    s, tau = PR.case_states("trot", B)
    prev = np.zeros((B, 4), np.uint8)
    ctx = capi.Context(device=0)
    kw = dict(dt=DT, prev_stance=prev, velocity_gain=1.0 / DT, friction=MU)
    clean = PC.wholebody_plant_step(ctx, s, tau, **kw)
    bad = {k: np.array(v, copy=True) for k, v in s.items()}
    bad["q"][2, 4] = np.nan
    others = np.arange(B) != 2
    out = PC.wholebody_plant_step(ctx, bad, tau, **kw)
    assert out["status"][2] == capi.STATUS_NOT_PD and (out["status"][others] == capi.STATUS_OK).all()
    assert (out["acc"][2] == 0.0).all() and (out["f"][2] == 0.0).all() and (out["impulse"][2] == 0.0).all() and (out["report"][2] == 0).all()
    nu_in = PC.wholebody_plant_step(ctx, s, tau)["nu_plus"]          # no touchdown: nu+ = nu, as the device forms R' v
    assert np.abs(nu_in[2] - PR.nu_of(s, 2)).max() <= 1e-15 and np.array_equal(out["nu_plus"][2], nu_in[2])
    for k in PR.NEXT_KEYS:
        assert np.array_equal(out["next"][k][others], clean["next"][k][others]), k
        assert np.array_equal(out["next"][k][2], bad[k][2], equal_nan=True), k
    for k in ("acc", "f", "nu_plus", "impulse", "report"):
        assert np.array_equal(out[k][others], clean[k][others]), k
    # KEEP, on the device, in place: sentinels and the state stay
    ctx.set_option(capi.OPT_ON_FAILURE, capi.ON_FAILURE_KEEP)
    d = capi.to_device(bad)
    o = device_outputs(torch, B, fill=249.0)
    PC.wholebody_plant_step_device(ctx, d, torch.from_numpy(tau).to("cuda:0"), o["st"], acc=o["acc"], f=o["f"], dt=DT, next=d,
                                     prev_stance=torch.from_numpy(prev).to("cuda:0"), velocity_gain=1.0 / DT, friction=MU,
                                     nu_plus=o["nu_plus"], impulse=o["impulse"], report=o["report"])
    torch.cuda.synchronize()
    assert o["st"].cpu().numpy().tolist() == [0, 0, capi.STATUS_NOT_PD, 0, 0, 0, 0]
    for k in ("acc", "f", "nu_plus", "impulse", "report"):
        assert (o[k][2] == 249).all() and np.array_equal(o[k][others].cpu().numpy(), clean[k][others]), k
    for k in PR.NEXT_KEYS:
        assert np.array_equal(d[k][2].cpu().numpy(), bad[k][2], equal_nan=True), k
        assert np.array_equal(d[k].cpu().numpy()[others], clean["next"][k][others]), k
    ctx.close()


def test_refusals_write_nothing(gpu):
    capi, ctx, _ = gpu
    B = 5
    s, tau = PR.case_states("trot", B)
    keep = []
    wb = capi._wholebody_batch(s, keep)
    pos = np.ascontiguousarray(s["base_pos"])
    outs = dict(acc=np.full((B, 18), -7.0), f=np.full((B, 12), -7.0), status=np.full(B, -7, np.int32), nu_plus=np.full((B, 18), -7.0),
                impulse=np.full((B, 12), -7.0), report=np.full((B, 4), 249, np.uint8))
    nxt_arrays = {k: np.full((B, n), -7.0) for _, k, n in capi.PLANT_NEXT_FIELDS}
    nxt = capi.PlantNext(*[nxt_arrays[k].ctypes.data for _, k, _ in capi.PLANT_NEXT_FIELDS])
    fn = PC.lib().qlamd_wholebody_plant_step_batch

    def call(tau_p=tau.ctypes.data, pos_p=pos.ctypes.data, dt=DT, batch=B, nxt_p=C.addressof(nxt), status_p=outs["status"].ctypes.data,
             kv=0.0, mu=MU, report=True):
        pc = PC.PlantContacts(None, kv, mu, outs["nu_plus"].ctypes.data, outs["impulse"].ctypes.data,
                                outs["report"].ctypes.data if report else None)
        return fn(ctx._h, C.addressof(wb), tau_p, None, pos_p, 9.81, dt, batch, outs["acc"].ctypes.data, outs["f"].ctypes.data, nxt_p,
                  C.addressof(pc), status_p, capi.MEM_HOST, None)

    refused = [call(tau_p=None), call(status_p=None), call(pos_p=None), call(batch=-1)]
    refused += [call(dt=v) for v in (0.0, -DT, float("nan"), float("inf"))]
    refused += [call(kv=v) for v in (-1.0, float("nan"), float("inf"))]
    refused += [call(mu=v) for v in (-0.1, float("nan"), float("inf"))]
    assert refused == [capi.ERR_INVALID_ARGUMENT] * 14
    for a in list(outs.values()) + list(nxt_arrays.values()):
        assert ((a == -7) | (a == 249)).all()
    # ... and accepted where the header says so: the friction coefficient is read only with a report
    assert call(mu=float("nan"), report=False) == capi.OK
    assert (outs["status"] == capi.STATUS_OK).all() and (outs["report"] == 249).all() and not (nxt_arrays["q"] == -7.0).any()
    assert call() == capi.OK and not (outs["report"] == 249).any()

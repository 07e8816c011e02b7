"""The contact anchors (include/qlamd_contact_anchor.h), everything that needs no GPU: the numpy reference the GPU tests compare
against (tests/contact_anchor_reference.py) checked on its own and on what tests/test_contact_anchor_gpu.py assumes of its cases,
the exports, the binding against its header and the compiler, the header's feature-test macro and structs, the C++ wrapper, the
marshalling of the Python wrappers, and the new kernels' resources against DESIGN.md section 4.6g."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contact_anchor_reference as CAR  # noqa: E402
import contact_update_reference as CUR  # noqa: E402
import plant_contacts_reference as PCR  # noqa: E402
import plant_friction_reference as PFR  # noqa: E402
import plant_reference as PR  # noqa: E402
import binding_checks as BC  # noqa: E402
from binding_checks import GCC, GXX, NEXT, WB, Recorder, f64, p  # noqa: E402

HEADER = os.path.join(ROOT, "include", "qlamd_contact_anchor.h")
ENTRIES = ("qlamd_wholebody_contact_update_anchored_batch", "qlamd_wholebody_plant_step_anchored_batch")
DT, MU = CAR.PLANT_DT, CAR.PLANT_MU


# ---- the reference on its own: the plant step ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cone", [False, True])
def test_without_gain_it_is_the_reference_without_anchors(oracle, cone):
    s, tau, anchors = CAR.plant_inputs()
    prev = np.zeros(CAR.PLANT_B, int)
    got = CAR.solve_batch(s, tau, anchors, 0.0, 0.002, prev_masks=prev, kv=1.0 / DT, mu=MU if cone else None)
    want = PFR.solve_batch(s, tau, MU, prev_masks=prev, kv=1.0 / DT) if cone else PCR.solve_batch(s, tau, prev_masks=prev, kv=1.0 / DT)
    for k in ("nu_plus", "p", "acc", "f"):
        assert np.array_equal(got[k], want[k]), k
    assert np.abs(got["perr"]).max() > 1e-3                    # the error is there; the gain is not


def test_the_constraint_holds_with_the_position_term(oracle):
    """Hard contacts: Js nu' = -gamma(q, nu+) - k_v Js nu+ - k_p e^ on the reference's own answer, from the oracle's matrices."""
    s, tau, anchors = CAR.plant_inputs()
    kv, kp, emax = 1.0 / DT, 0.1 / DT ** 2, 0.002
    ref = CAR.solve_batch(s, tau, anchors, kp, emax, prev_masks=np.zeros(CAR.PLANT_B, int), kv=kv)
    worst = 0.0
    for i in range(CAR.PLANT_B):
        rows = PR.rows_of(int(ref["mask"][i]))
        r = PCR.solve(s["q"][i], s["base_quat"][i], ref["nu"][i], tau[i], int(ref["mask"][i]), 0, kv)
        Js = r["Jc"][rows]
        want = -r["gamma"][rows] - kv * (Js @ ref["nu_plus"][i]) - kp * ref["perr"][i][rows]
        worst = max(worst, float(np.abs(Js @ ref["acc"][i] - want).max() / max(1.0, np.abs(want).max())))
        off = [j for j in range(12) if j not in rows]
        assert (ref["perr"][i][off] == 0.0).all() and (ref["f"][i][off] == 0.0).all()
    print("Js nu' against -gamma - k_v Js nu+ - k_p e^: %.2e relative" % worst)
    assert worst < 1e-9


def test_anchors_at_the_feet_give_no_error_and_the_clamp_acts_both_ways(oracle):
    s, _, anchors = CAR.plant_inputs()
    feet = CAR.feet_world(s)
    clamped = free = 0
    for i in range(CAR.PLANT_B):
        mask = PR.mask_of(s["stance"][i])
        eh, e, _ = CAR.error(s["q"][i], s["base_quat"][i], s["base_pos"][i], feet[i], mask)
        assert np.abs(eh).max() <= 1e-15 and np.abs(e).max() <= 1e-15
        eh, e, cl = CAR.error(s["q"][i], s["base_quat"][i], s["base_pos"][i], anchors[i], mask, 0.002)
        # e is the displacement, turned into the base's frame, with the other sign: the foot minus the anchor
        R = CAR.O.quat_to_matrix(s["base_quat"][i])
        want = (R.T @ (feet[i] - anchors[i].reshape(4, 3)).T).T
        for l in range(4):
            el, ehl = e[3 * l:3 * l + 3], eh[3 * l:3 * l + 3]
            if not (mask >> l) & 1:
                assert (el == 0.0).all() and (ehl == 0.0).all() and not cl[l]
                continue
            assert np.abs(el - want[l]).max() <= 1e-15
            length = np.linalg.norm(el)
            if cl[l]:
                clamped += 1
                assert length > 0.002 and abs(np.linalg.norm(ehl) - 0.002) <= 1e-15 and np.abs(np.cross(ehl, el)).max() <= 1e-18
            else:
                free += 1
                assert length <= 0.002 and np.array_equal(ehl, el)
        # an unflagged leg's anchor is not looked at
        poisoned = anchors[i].reshape(4, 3).copy()
        poisoned[[l for l in range(4) if not (mask >> l) & 1]] = np.nan
        assert np.array_equal(CAR.error(s["q"][i], s["base_quat"][i], s["base_pos"][i], poisoned, mask, 0.002)[0], eh)
    print("clamped %d, not clamped %d flagged legs" % (clamped, free))
    assert clamped >= 10 and free >= 10


def test_the_cases_of_the_gpu_parity_test(oracle):
    """What tests/test_contact_anchor_gpu.py asserts about its plant cases from the reference alone: at most 1 % of the flagged legs
    left out of the report's comparison, and with the clamp at least 10 flagged legs clamped and 10 not."""
    for case in CAR.PLANT_CASES:
        st, _, _, _, _, ref, _, compare = CAR.plant_case(*case)
        flagged = st["stance"] != 0
        clamped = ref["clamped"] & flagged
        assert (flagged & ~compare).sum() <= 0.01 * flagged.sum(), case
        if np.isfinite(case[2]):
            assert clamped.sum() >= 10 and (flagged & ~clamped).sum() >= 10, case
        else:
            assert not clamped.any()
        assert ((ref["touch"] != 0) == case[4]).all()


# ---- the reference on its own: the rollout and the loop ---------------------------------------------------------------------------

def test_the_rollout_with_the_gain_holds_the_feet(oracle):
    """8 trot robots, 64 steps of 2.5 ms, constant flags, hard contacts, k_v = 1 / dt: k_p = 1 / dt^2 leaves at most a tenth of the
    k_p = 0 drift at the last step (measured: 0.38 against 13.8 mm on the maximum, 0.13 against 2.3 mm on the median)."""
    s, tau = PR.case_states("trot", CAR.ROLLOUT_ROBOTS)
    dt = CAR.ROLLOUT_DT
    loose = CAR.rollout(s, tau, CAR.ROLLOUT_STEPS, dt, 1.0 / dt, 0.0)[2]
    held = CAR.rollout(s, tau, CAR.ROLLOUT_STEPS, dt, 1.0 / dt, 1.0 / dt ** 2)[2]
    print("drift at step %d: k_p = 0 max %.3e median %.3e m; k_p = 1 / dt^2 max %.3e median %.3e m" % (
        CAR.ROLLOUT_STEPS, loose.max(), np.median(loose), held.max(), np.median(held)))
    assert len(held) == len(loose) >= 16
    assert held.max() <= 0.1 * loose.max() and np.median(held) <= 0.1 * np.median(loose)


@pytest.mark.parametrize("cone", [False, True])
def test_the_loop_with_anchors_brings_the_feet_back_to_the_ground(oracle, cone):
    """CUR.loop_case() under CAR.loop_rule (with the cone the liftoff at 3 mm: that docstring says why), k_p = 0.1 / dt^2, e_max =
    10 mm: the largest |gap| of a held foot at the last tick is under half of the k_p = 0 loop's (measured: 2.1 against 10.2 mm
    hard, 3.2 against 10.2 mm with the cone).  At most 2 of the 16 robots may have left the comparison at the end.  With
    loop_case()'s own liftoff of 10 mm the cone's loop ends at 7.7 mm: the penetration goes (1.2 mm), and what is left are sliding
    feet that float inside the liftoff distance, which a cone without pulling forces does not bring down at any gain."""
    s, tau, plane, _ = CUR.loop_case()
    kw, re_mask = CAR.loop_rule(cone)
    worst = {}
    for kp in (0.0, CAR.LOOP_KP):
        _, ticks = CAR.loop(s, tau, CUR.LOOP_TICKS, CUR.LOOP_DT, 1.0 / CUR.LOOP_DT, CUR.LOOP_MU, plane, kp, CAR.LOOP_EMAX, cone=cone,
                            reanchor_mask=re_mask, **kw)
        last = ticks[-1]
        assert (~last["valid"]).sum() <= 2
        gap = last["gap"][(last["flags"] != 0) & last["valid"][:, None]]
        events = np.stack([k["events"] for k in ticks])[np.stack([k["valid"] for k in ticks])]
        worst[kp] = (np.abs(gap).max(), np.maximum(-gap, 0.0).max())
        print("%s k_p = %g: |gap| %.3e m, penetration %.3e m; %d touchdowns, %d releases, %d re-anchorings" % (
            "cone" if cone else "hard", kp, *worst[kp], ((events & 1) != 0).sum(), ((events & 6) != 0).sum(), ((events & 8) != 0).sum()))
        assert not ticks[0]["flags"].any()
    assert worst[CAR.LOOP_KP][0] < 0.5 * worst[0.0][0]


def test_the_anchor_rule_and_the_update_cases_of_the_gpu_test(oracle):
    """The rule's four branches on a hand-made update, and from the reference alone what tests/test_contact_anchor_gpu.py asserts of
    its 259-robot case: at least 10 comparable legs in each branch."""
    upd = dict(status=np.array([0, CUR.STATUS_NOT_PD]), events=np.zeros((2, 4), np.uint8),
               support_next=np.array([[1, 1, 1, 0], [1, 1, 1, 0]], np.uint8), gap=np.full((2, 4), 0.5),
               foot_pos=np.arange(24.0).reshape(2, 4, 3), normals=np.tile(np.array([0.0, 0.0, 1.0]), (2, 4, 1)))
    cur = np.array([[0, 1, 1, 1], [0, 1, 1, 1]], np.uint8)
    report = np.array([[16, 16, 0, 16], [16, 16, 0, 16]], np.uint8)
    fill = np.full((2, 4, 3), -7.0)
    got, events, branch = CAR.anchor_rule(upd, cur, fill, report, 16)
    assert branch.tolist() == [[0, 1, 2, 3], [-1] * 4] and events.tolist() == [[0, 8, 0, 0], [0] * 4]
    assert np.array_equal(got[0, 0], [0.0, 1.0, 1.5]) and np.array_equal(got[0, 1], [3.0, 4.0, 4.5])
    assert np.array_equal(got[0, 2], [-7.0] * 3) and np.array_equal(got[0, 3], [9.0, 10.0, 11.0]) and (got[1] == -7.0).all()
    assert CAR.anchor_rule(upd, cur, fill, None, 0xFF)[2].tolist()[0] == [0, 2, 2, 3]           # no report: no leg is re-anchored
    s, rep, plane, sentinel = CAR.update_case(259)
    ref = CAR.update_batch(s, sentinel, CAR.SLIDING, plane=plane, report=rep, **CAR.UPDATE_RULE)
    # an update without flags is not "every foot where it is": a foot the rule takes is a touchdown; under NO_TOUCHDOWN none is
    free = {k: v for k, v in s.items() if k != "stance"}
    taken = CAR.update_batch(free, sentinel, plane=plane, **CAR.UPDATE_RULE)
    none = CAR.update_batch(free, sentinel, plane=plane, **dict(CAR.UPDATE_RULE, **CAR.NO_TOUCHDOWN))
    assert (taken["branch"] == 0).sum() >= 10 and np.abs(taken["anchor"] - taken["foot_pos"]).max() > 1e-3
    assert (none["branch"] == 3).all() and np.array_equal(none["anchor"], none["foot_pos"])
    counts = [int((ref["compare"] & (ref["branch"] == b)).sum()) for b in range(4)]
    print("B = 259, plane: touchdown %d, re-anchored %d, kept %d, free %d comparable legs" % tuple(counts))
    assert min(counts) >= 10


# ---- the export, the header, the binding ------------------------------------------------------------------------------------------

def test_the_library_exports_the_entries():
    from quadruped_locomotion_amd import build, contact_anchor
    lib = build.build()
    names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, names, re.M), name
    assert contact_anchor.EXPORTS == ENTRIES
    assert "contact_anchor_kernel.hip" in build.SOURCE_NAMES and HEADER in build.headers()


def test_the_binding_matches_the_header_and_the_compiler(tmp_path):
    from quadruped_locomotion_amd import build, contact_anchor as CA, contact_detection as CD, plant_friction as PF
    names = BC.signatures_match(CA, HEADER)
    assert list(names) == list(ENTRIES) and all(CA.SIGNATURES[name][0] is C.c_int for name in names)
    # the siblings' parameters with the new struct behind theirs
    upd = CD.SIGNATURES["qlamd_wholebody_contact_update_batch"][1]
    got = CA.SIGNATURES[ENTRIES[0]][1]
    assert got[:4] == upd[:4] and got[4] is C.c_void_p and got[5:] == upd[4:] and names[ENTRIES[0]][3:5] == ["update", "anchors"]
    fr = PF.SIGNATURES["qlamd_wholebody_plant_step_friction_batch"][1]
    got = CA.SIGNATURES[ENTRIES[1]][1]
    assert got[:13] == fr[:13] and got[13] is C.c_void_p and got[14:] == fr[13:]
    assert names[ENTRIES[1]][11:14] == ["contacts", "friction", "anchor"]
    structs = {"qlamd_contact_anchors": CA.ContactAnchors, "qlamd_plant_anchor": CA.PlantAnchor}
    assert BC.header_structs(HEADER) == set(structs)
    got = BC.layout(HEADER, structs, ["CONTACT_EVENT_REANCHORED"], tmp_path)
    BC.mirrors_match(structs, got)
    assert got["sizeof qlamd_contact_anchors"] == C.sizeof(CA.ContactAnchors) == 16
    assert got["sizeof qlamd_plant_anchor"] == C.sizeof(CA.PlantAnchor) == 32
    assert got["value CONTACT_EVENT_REANCHORED"] == CA.CONTACT_EVENT_REANCHORED == CAR.REANCHORED == 8
    assert CA.CONTACT_EVENT_REANCHORED & (CD.CONTACT_EVENT_TOUCHDOWN | CD.CONTACT_EVENT_RELEASED_PULL | CD.CONTACT_EVENT_RELEASED_GAP) == 0
    build.build()
    for name in ENTRIES:
        fn = getattr(CA.lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == CA.SIGNATURES[name][1]


def test_the_header_compiles_alone_and_qlamd_h_brings_it(tmp_path):
    """As C and as C++, included first or behind any of its siblings; qlamd.h's own text is what it was."""
    body = ("#if !defined(QLAMD_HAS_CONTACT_ANCHORS) || QLAMD_HAS_CONTACT_ANCHORS != 1\n#error no contact anchors\n#endif\n"
            "#if QLAMD_CONTACT_EVENT_REANCHORED != 8\n#error bits\n#endif\n"
            "typedef int (*update_fn)(qlamd_context *, const qlamd_wholebody_batch *, const double *, const qlamd_contact_update *,\n"
            "                         const qlamd_contact_anchors *, int64_t, int32_t *, int, void *);\n"
            "typedef int (*step_fn)(qlamd_context *, const qlamd_wholebody_batch *, const double *, const double *, const double *,\n"
            "                       double, double, int64_t, double *, double *, const qlamd_plant_next *,\n"
            "                       const qlamd_plant_contacts *, const qlamd_plant_friction *, const qlamd_plant_anchor *, int32_t *, int, void *);\n"
            "update_fn update_entry = qlamd_wholebody_contact_update_anchored_batch;\n"
            "step_fn step_entry = qlamd_wholebody_plant_step_anchored_batch;\n")
    firsts = ("qlamd_contact_anchor.h", "qlamd.h", "qlamd_plant_contacts.h", "qlamd_contact_detection.h", "qlamd_plant_friction.h")
    for k, first in enumerate(firsts):
        for cmd, ext in ((GCC, "c"), (GXX, "cpp")):
            src = tmp_path / ("anchor%d.%s" % (k, ext))
            src.write_text('#include <stddef.h>\n#include "%s"\n' % first + body)
            subprocess.check_call(cmd + ["-c", str(src), "-o", str(tmp_path / ("anchor%d_%s.o" % (k, ext)))])
    text = open(os.path.join(ROOT, "include", "qlamd.h")).read()
    assert "qlamd_contact_anchor" not in text          # it comes in at the end of the last header qlamd.h includes
    incs = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(ROOT, "include", "qlamd_plant_friction.h")).read(), flags=re.M)
    assert incs == ["qlamd.h", "qlamd_contact_anchor.h"]


def test_the_cpp_wrapper_compiles_against_the_header(tmp_path):
    src = tmp_path / "anchor.cpp"
    src.write_text('#include "qlamd/contact_anchor.hpp"\n'
                   "int run(qlamd_context *ctx) {\n"
                   "  qlamd::host::PlantState s(3);\n  qlamd::host::ContactDetector d;\n  qlamd::host::ContactAnchors a(3);\n"
                   "  std::vector<double> tau(36), f(36), e(36);\n  std::vector<int32_t> st(3), it(6);\n  std::vector<uint8_t> report(12);\n"
                   "  a.position_gain = 16000.0; a.max_error = 0.01; a.reanchor_mask = QLAMD_CONTACT_SLIDING;\n"
                   "  int rc = qlamd::host::init_anchors(ctx, s, d, a, st.data());\n"
                   "  if (rc != QLAMD_OK) return rc;\n"
                   "  rc = qlamd::host::step_anchored(ctx, s, a, tau.data(), 9.81, 0.0025, 400.0, 0.6, false, st.data());\n"
                   "  if (rc != QLAMD_OK) return rc;\n"
                   "  rc = qlamd::host::step_anchored(ctx, s, a, tau.data(), 9.81, 0.0025, 400.0, 0.6, true, st.data(), f.data(), report.data(),\n"
                   "                                  e.data(), it.data());\n"
                   "  if (rc != QLAMD_OK) return rc;\n"
                   "  return qlamd::host::detect_contacts_anchored(ctx, s, d, a, report.data(), st.data());\n}\n")
    subprocess.check_call(GXX + ["-I" + os.path.join(ROOT, "quadruped_locomotion_amd", "host"), "-c", str(src), "-o", str(tmp_path / "anchor.o")])


def test_the_wrappers_marshal_every_struct(monkeypatch):
    import torch
    from quadruped_locomotion_amd import capi, contact_anchor as CA
    rec = Recorder()
    monkeypatch.setattr(capi, "_lib", rec)
    ctx = capi.Context()
    ctx._h = C.c_void_p(0xC0FFEE)
    B = 5
    s = dict(q=f64(B, 12), qd=f64(B, 12), base_quat=f64(B, 4), base_linvel=f64(B, 3), base_angvel=f64(B, 3), base_pos=f64(B, 3),
             stance=np.ones((B, 4), np.uint8), normals=f64(B, 12))
    tau, g_ext, prev, anchor = f64(B, 12), f64(B, 18), np.ones((B, 4), np.uint8), f64(B, 12)

    def last(entry, n):
        name, args = rec.calls[-1]
        assert name == entry and len(args) == n
        return args

    # the plant step, host: base_pos goes over with or without dt
    out = CA.wholebody_plant_step_anchored(ctx, s, tau, anchor, 1600.0, 0.01, friction=0.6, cone=True, g_ext=g_ext, gravity=3.5, dt=0.002,
                                           prev_stance=prev, velocity_gain=400.0)
    a = last(ENTRIES[1], 17)
    assert a[0] == 0xC0FFEE and a[2] == p(tau) and a[3] == p(g_ext) and a[4] == p(s["base_pos"]) and a[5:8] == [3.5, 0.002, B]
    assert a[8] == p(out["acc"]) and a[9] == p(out["f"]) and a[14] == p(out["status"]) and a[15] == capi.MEM_HOST and a[16] is None
    for key, member in WB.items():
        assert a[1][member] == p(s[key]), member
    assert a[10] == {m: p(out["next"][k]) for m, k in NEXT}
    assert a[11] == dict(previous_support_leg=p(prev), velocity_gain=400.0, friction_coefficient=0.6, post_impact_velocity=p(out["nu_plus"]),
                         impulse=p(out["impulse"]), contact_report=p(out["report"]))
    assert a[12] == dict(iterations=p(out["iterations"]))
    assert a[13] == dict(anchor=p(anchor), position_gain=1600.0, max_error=0.01, position_error=p(out["position_error"]))
    assert out["position_error"].shape == (B, 12) and out["iterations"].dtype == np.int32
    out = CA.wholebody_plant_step_anchored(ctx, s, tau, anchor, 2.0, want=("position_error",))
    a = last(ENTRIES[1], 17)
    assert a[4] == p(s["base_pos"]) and a[6] == 0.0 and a[10] is None and a[12] is None and "next" not in out and "report" not in out
    assert a[13] == dict(anchor=p(anchor), position_gain=2.0, max_error=float("inf"), position_error=p(out["position_error"]))
    out = CA.wholebody_plant_step_anchored(ctx, s, tau, None, 2.0, with_anchor=False)
    assert last(ENTRIES[1], 17)[13] is None and "position_error" not in out
    n = len(rec.calls)
    with pytest.raises(ValueError, match="anchor"):
        CA.wholebody_plant_step_anchored(ctx, s, tau, f64(B, 11), 2.0)
    assert len(rec.calls) == n
    # the plant step, device
    d = {k: torch.from_numpy(v) for k, v in s.items()}
    dtau, st, danchor, perr = torch.from_numpy(tau), torch.zeros(B, dtype=torch.int32), torch.from_numpy(anchor), torch.from_numpy(f64(B, 12))
    report, iters = torch.zeros(B, 4, dtype=torch.uint8), torch.zeros(B, 2, dtype=torch.int32)
    CA.wholebody_plant_step_anchored_device(ctx, d, dtau, st, danchor, 3.0, max_error=0.02, friction=0.7, cone=True, dt=0.001, next=d,
                                            stream=0x5151, report=report, iterations=iters, position_error=perr)
    a = last(ENTRIES[1], 17)
    assert a[2] == p(dtau) and a[4] == p(d["base_pos"]) and a[5:8] == [9.81, 0.001, B] and a[14] == p(st) and a[15] == capi.MEM_DEVICE
    assert a[16] == 0x5151 and a[10] == {m: p(d[k]) for m, k in NEXT} and a[12] == dict(iterations=p(iters))
    assert a[13] == dict(anchor=p(danchor), position_gain=3.0, max_error=0.02, position_error=p(perr))
    CA.wholebody_plant_step_anchored_device(ctx, d, dtau, st, danchor, 3.0)
    a = last(ENTRIES[1], 17)
    assert a[4] == p(d["base_pos"]) and a[10] is None and a[12] is None and a[13]["position_error"] is None
    call = CA.AnchoredPlantStepCall(ctx, d, dtau, st, None, 0.0)
    n = len(rec.calls)
    call(); call()
    assert len(rec.calls) == n + 2 and last(ENTRIES[1], 17)[13] is None
    for bad in (dict(position_error=torch.zeros(B, 11, dtype=torch.float64)), dict(iterations=torch.zeros(B, 2, dtype=torch.int64))):
        with pytest.raises(ValueError, match=list(bad)[0]):
            CA.wholebody_plant_step_anchored_device(ctx, d, dtau, st, danchor, 3.0, **bad)
    # the update
    rep = np.ones((B, 4), np.uint8)
    out = CA.wholebody_contact_update_anchored(ctx, s, anchor, reanchor_mask=16, report=rep, liftoff_distance=0.02)
    a = last(ENTRIES[0], 9)
    assert a[0] == 0xC0FFEE and a[2] == p(s["base_pos"]) and a[4] == dict(anchor=p(anchor), reanchor_mask=16) and a[5] == B
    assert a[6] == p(out["status"]) and a[7] == capi.MEM_HOST and a[8] is None
    assert a[3]["liftoff_distance"] == 0.02 and a[3]["contact_report"] == p(rep) and a[3]["support_next"] == p(out["support_next"])
    assert a[1]["support_leg"] == p(s["stance"])
    CA.wholebody_contact_update_anchored(ctx, s, anchor, with_anchors=False)
    assert last(ENTRIES[0], 9)[4] is None
    nxt = torch.zeros(B, 4, dtype=torch.uint8)
    call = CA.AnchoredContactUpdateCall(ctx, d, st, danchor, reanchor_mask=8, support_next=nxt, stream=0x77)
    n = len(rec.calls)
    call(); call()
    a = last(ENTRIES[0], 9)
    assert len(rec.calls) == n + 2 and a[4] == dict(anchor=p(danchor), reanchor_mask=8) and a[3]["support_next"] == p(nxt)
    assert a[1]["support_leg"] == p(d["stance"]) and a[7] == capi.MEM_DEVICE and a[8] == 0x77
    with pytest.raises(ValueError, match="anchor"):
        CA.wholebody_contact_update_anchored_device(ctx, d, st, torch.zeros(B, 11, dtype=torch.float64))
    ctx._h = C.c_void_p()


# ---- the kernels' resources -------------------------------------------------------------------------------------------------------

def test_resources_are_what_design_states(tmp_path):
    """DESIGN.md 4.6g names the three kernels' registers, private segment and LDS; the figures are the code-object metadata of the
    unit compiled with the build's flags.  No private segment in any of them; the update keeps four wavefronts per SIMD."""
    seen = BC.resources("contact_anchor_kernel.hip", ("anchored_contact_update_kernel", "anchored_plant_contact_kernel",
                                                      "anchored_plant_friction_kernel"), 3, tmp_path)
    assert all(got[2] == 0 for got, _ in seen.values())
    assert seen["anchored_contact_update_kernel"][0][0] <= 128         # 512 / 128: four wavefronts per SIMD

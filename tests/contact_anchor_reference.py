"""Reference of the contact anchors (include/qlamd_contact_anchor.h) in numpy, on tests/contact_update_reference.py,
tests/plant_contacts_reference.py and tests/plant_friction_reference.py: the anchor rule on update_batch's outputs, the plant step
with the position term -k_p e^ in its constraint right-hand side (hard contacts on the oracle's M, h, Jc; the cone through
plant_friction_reference), the rollout with constant flags and the closed loop.  Test infrastructure."""
import numpy as np

import contact_update_reference as CUR
import plant_contacts_reference as PCR
import plant_friction_reference as PFR
import plant_reference as PR
from oracle import oracle as O

REANCHORED = 8


# ---------------------------------------------------------------------------------------------------------------- the update

def anchor_rule(upd, cur, anchors, report=None, reanchor_mask=0):
    """upd: CUR.update_batch's result for the current flags `cur` [B,4]; anchors [B,4,3].
    -> (anchors after the update, events with REANCHORED, branch [B,4]: 0 touchdown, 1 re-anchored, 2 kept, 3 free; -1 on a failed
    robot, whose anchors stay)"""
    B = cur.shape[0]
    out, events, branch = np.array(anchors, dtype=float).reshape(B, 4, 3).copy(), upd["events"].copy(), np.full((B, 4), -1)
    for i in range(B):
        if upd["status"][i] != CUR.STATUS_OK:
            continue
        for l in range(4):
            p, n, gap = upd["foot_pos"][i, l], upd["normals"][i, l], upd["gap"][i, l]
            nxt, was = upd["support_next"][i, l] != 0, cur[i, l] != 0
            moved = nxt and was and report is not None and (int(report[i, l]) & int(reanchor_mask)) != 0
            if nxt and not was:
                out[i, l], branch[i, l] = p - gap * n, 0
            elif moved:
                out[i, l], branch[i, l] = p - gap * n, 1
                events[i, l] |= REANCHORED
            elif nxt:
                branch[i, l] = 2
            else:
                out[i, l], branch[i, l] = p, 3
    return out, events, branch


def update_batch(s, anchors, reanchor_mask=0, plane=None, hf=None, report=None, **rule):
    """CUR.update_batch with the anchors kept: its dict, with events carrying REANCHORED, and anchor [B,4,3], branch [B,4]."""
    B = s["q"].shape[0]
    upd = CUR.update_batch(s, plane=plane, hf=hf, report=report, **rule)
    cur = np.zeros((B, 4), np.uint8) if s.get("stance") is None else np.asarray(s["stance"], np.uint8)
    upd["anchor"], upd["events"], upd["branch"] = anchor_rule(upd, cur, anchors, report, reanchor_mask)
    return upd


UPDATE_BATCHES = (1, 17, 65, 259)
UPDATE_RULE = dict(touchdown_distance=0.01, approach_speed=0.05, liftoff_distance=0.03, sensor_distance=0.02)
SLIDING = 16
NO_TOUCHDOWN = dict(approach_speed=-1e300)      # a rule that takes no foot: an update without flags then leaves anchor = p on every leg
_UPD = {}


def update_case(B):
    """The case of the update tests, computed once, shared, never modified (the recipe of tests/test_contact_update_gpu.py's
    case("trot", B): flags over all 16 masks, per-robot planes through the median of the feet) with a report drawn over all 32
    patterns of the five report bits and a fill of the anchors with distinct finite values, so that a kept entry is recognised
    bit for bit.  -> (s, report uint8 [B,4], plane [B,4], fill [B,12])"""
    if B not in _UPD:
        s = {k: np.array(v, copy=True) for k, v in PR.case_states("trot", B)[0].items()}
        rng = np.random.default_rng(100 + B)
        s["stance"] = np.ascontiguousarray(((rng.integers(0, 16, B)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8))
        rng.integers(0, 8, (B, 4))              # (that file draws its own report here: the planes keep its stream)
        abc = np.concatenate([rng.uniform(-0.3, 0.3, (B, 2)), np.ones((B, 1))], axis=1) * rng.uniform(0.5, 2.0, (B, 1))
        length = np.linalg.norm(abc, axis=1)
        d = np.array([np.median(CUR.feet(s, i)[0] @ (abc[i] / length[i])) for i in range(B)]) * length
        plane = np.ascontiguousarray(np.concatenate([abc, d[:, None]], axis=1))
        rng = np.random.default_rng(500 + B)
        _UPD[B] = (s, rng.integers(0, 32, (B, 4)).astype(np.uint8), plane, np.ascontiguousarray(rng.uniform(100.0, 200.0, (B, 12))))
    return _UPD[B]


def feet_world(s):
    """[B,4,3]"""
    return np.stack([CUR.foot_world_position(s["q"][i], s["base_quat"][i], s["base_pos"][i]) for i in range(s["q"].shape[0])])


# ------------------------------------------------------------------------------------------------------------ the plant step

def error(q, quat, pos, anchor, mask, emax=np.inf):
    """-> (e^ [12], e [12], clamped [4] bool): per flagged leg e = r - R'(a - pos) in base coordinates and e^ = e min(1, emax / |e|);
    zeros on an unflagged leg, whose anchor is not looked at."""
    R = O.quat_to_matrix(quat)
    a = np.asarray(anchor, dtype=float).reshape(4, 3)
    eh, e, clamped = np.zeros(12), np.zeros(12), np.zeros(4, bool)
    for l in range(4):
        if not (mask >> l) & 1:
            continue
        el = O.leg_fk(l, q[3 * l:3 * l + 3])[0] - R.T @ (a[l] - pos)
        length = np.linalg.norm(el)
        clamped[l] = length > emax
        e[3 * l:3 * l + 3] = el
        eh[3 * l:3 * l + 3] = el * (emax / length) if clamped[l] else el
    return eh, e, clamped


def solve(q, quat, pos, nu, tau, mask, anchor, kp, emax=np.inf, prev_mask=None, kv=0.0, mu=None, g_ext=None, gravity=9.81,
          normals_world=None):
    """The anchored plant step of one robot.  mu None: hard contacts (PCR.solve with r = -gamma - kv Js nu+ - kp e^); mu: the cone
    (PFR.solve with the same r in c = r - Js x0).  -> dict(nu_plus, p, acc, f, touch, perr [12], clamped [4], and iters with mu).
    Both are the non-anchored reference's result corrected through its own matrices, so kp = 0 IS that reference."""
    eh, _, clamped = error(q, quat, pos, anchor, mask, emax)
    rows = PR.rows_of(mask)
    if mu is None:
        base = PCR.solve(q, quat, nu, tau, mask, prev_mask, kv, g_ext, gravity)
        out = dict(nu_plus=base["nu_plus"], p=base["p"], acc=base["acc"], f=base["f"], touch=base["touch"])
        if rows and kp != 0.0:
            Js, n = base["Jc"][rows], len(rows)
            K = np.zeros((18 + n, 18 + n))
            K[:18, :18] = base["M"]
            K[:18, 18:] = -Js.T
            K[18:, :18] = Js
            dx = np.linalg.solve(K, np.concatenate([np.zeros(18), -kp * eh[rows]]))
            f = base["f"].copy()
            f[rows] += dx[18:]
            out.update(acc=base["acc"] + dx[:18], f=f)
    else:
        base = PFR.solve(q, quat, nu, tau, mask, mu, prev_mask, kv, g_ext, gravity, normals_world)
        out = dict(nu_plus=base["nu_plus"], p=base["p"], acc=base["acc"], f=base["f"], touch=base["touch"], iters=base["iters"])
        if rows and kp != 0.0:
            Mi, Js = np.linalg.inv(base["M"]), base["Js"]
            x0 = base["acc"] - Mi @ (Js.T @ base["f"][rows])
            y, it_f = PFR.cone_qp(base["H0"], base["c_f"] - kp * eh[rows], base["CI"])
            f = np.zeros(12)
            f[rows] = y
            out.update(acc=x0 + Mi @ (Js.T @ y), f=f, iters=(base["iters"][0], it_f))
    out.update(perr=eh, clamped=clamped)
    return out


def solve_batch(s, tau, anchors, kp, emax=np.inf, masks=None, prev_masks=None, kv=0.0, mu=None, g_ext=None, gravity=9.81,
                normals_world=None):
    """Per robot -> the dict PCR.solve_batch / PFR.solve_batch give (nu_plus, p, acc, f, nu, mask, touch) with perr [B,12] and
    clamped [B,4]: what PCR.report_batch, PFR.report_batch and PCR.step_batch take."""
    B = s["q"].shape[0]
    anchors = np.asarray(anchors, dtype=float).reshape(B, 4, 3)
    out = dict(nu_plus=np.zeros((B, 18)), p=np.zeros((B, 12)), acc=np.zeros((B, 18)), f=np.zeros((B, 12)), nu=np.zeros((B, 18)),
               mask=np.zeros(B, int), touch=np.zeros(B, int), perr=np.zeros((B, 12)), clamped=np.zeros((B, 4), bool))
    for i in range(B):
        m = PR.mask_of(s["stance"][i]) if masks is None else int(masks[i])
        nu = PR.nu_of(s, i)
        r = solve(s["q"][i], s["base_quat"][i], s["base_pos"][i], nu, tau[i], m, anchors[i], kp, emax,
                  None if prev_masks is None else int(prev_masks[i]), kv, mu, None if g_ext is None else g_ext[i], gravity,
                  None if normals_world is None else normals_world[i])
        for k in ("nu_plus", "p", "acc", "f", "perr", "clamped"):
            out[k][i] = r[k]
        out["nu"][i], out["mask"][i], out["touch"][i] = nu, m, r["touch"]
    return out


def report_batch(s, ref, mu, cone, normals_world=None):
    """-> (bits [B,4], compare [B,4]) by the hard entry's rule or the cone's"""
    if cone:
        bits, compare, _ = PFR.report_batch(s, ref, mu, normals_world)
        return bits, compare
    return PCR.report_batch(s, ref, mu, normals_world)


# ------------------------------------------------------------------------------------------------------------------- rollouts

ROLLOUT_ROBOTS, ROLLOUT_STEPS, ROLLOUT_DT = 8, 64, 0.0025


def rollout(s, tau, steps, dt, kv, kp, emax=np.inf, mu=None):
    """Constant flags and torques.  Step 0 has the plastic impact (previous flags of zero) and runs with the anchors at the feet;
    the anchors are then set to where the feet stand after it (all of them: on the device an update without flags under
    NO_TOUCHDOWN) and held with kp for the other steps.
    -> (final state, anchors [B,4,3], drift: |p - anchor| of the flagged feet at the end, one flat array)"""
    s = {k: np.array(v, copy=True) for k, v in s.items()}
    B = s["q"].shape[0]
    anchors = feet_world(s)
    for k in range(steps):
        ref = solve_batch(s, tau, anchors, kp, emax, prev_masks=np.zeros(B, int) if k == 0 else None, kv=kv, mu=mu)
        s.update(PCR.step_batch(s, ref, dt))
        if k == 0:
            anchors = feet_world(s)
    return s, anchors, drift(s, anchors)


def drift(s, anchors):
    d = np.linalg.norm(feet_world(s) - np.asarray(anchors).reshape(-1, 4, 3), axis=2)
    return d[np.asarray(s["stance"]) != 0]


LOOP_KP, LOOP_EMAX = 0.1 / CUR.LOOP_DT ** 2, 0.010


def loop_rule(cone):
    """-> (the rule's keywords for CUR.loop_case()'s loop, reanchor_mask).  Hard contacts: loop_case()'s own distances, a pulling
    foot released, no re-anchoring.  The cone: a separating foot released, a sliding one re-anchored, and the liftoff and sensor
    distances at 3 mm instead of 10 and 5.  The reason: a cone has no pulling force, so a held foot that slides and floats above
    the ground is not brought down by any gain; the largest |gap| of a held foot is then the liftoff distance plus one tick's rise,
    and the tests ask for under half of the 10.2 mm of the k_p = 0 loop."""
    kw = CUR.loop_case()[3]
    if cone:
        return dict(kw, release_mask=PFR.SEPARATING, liftoff_distance=0.003, sensor_distance=0.003), SLIDING
    return kw, 0


def loop(s, tau, ticks, dt, kv, mu, plane, kp, emax=np.inf, cone=False, reanchor_mask=0, **rule):
    """CUR.loop with anchors: the first anchors are the feet (the device: an update without flags, in which no foot of
    loop_case() is taken, the ground lying under all of them), then plant step (hard, or
    with the cone) -> anchored update, `ticks` times, from no foot flagged.  -> (state, list per tick of CUR.loop's dict with anchor
    [B,4,3] after the update).  A robot is valid as there: until a leg of it is borderline in the update or in the plant's report."""
    s = {k: np.array(v, copy=True) for k, v in s.items()}
    B = s["q"].shape[0]
    s["stance"] = np.zeros((B, 4), np.uint8)
    prev = np.zeros(B, int)
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (B, 4, 1))
    anchors = feet_world(s)
    valid = np.ones(B, bool)
    ticks_out = []
    for _ in range(ticks):
        masks = np.array([PR.mask_of(r) for r in s["stance"]])
        ref = solve_batch(s, tau, anchors, kp, emax, masks=masks, prev_masks=prev, kv=kv, mu=mu if cone else None, normals_world=normals)
        bits, cmp_report = report_batch(s, ref, mu, cone, normals)
        s.update(PCR.step_batch(s, ref, dt))
        upd = update_batch(s, anchors, reanchor_mask, plane=plane, report=bits, **rule)
        valid = valid & upd["compare"].all(axis=1) & cmp_report.all(axis=1)
        ticks_out.append(dict(flags=s["stance"].copy(), report=bits, support_next=upd["support_next"], events=upd["events"],
                              gap=upd["gap"], nu=upd["nu"], valid=valid.copy(), anchor=upd["anchor"].copy(),
                              acc_max=np.abs(ref["acc"]).max(axis=1)))
        prev = masks
        s["stance"] = upd["support_next"].copy()
        normals = upd["normals"]
        anchors = upd["anchor"]
    return s, ticks_out


def held_gap(tick):
    """|gap| of the feet the tick's plant step held, one flat array"""
    return np.abs(tick["gap"][tick["flags"] != 0])


# ------------------------------------------------------------------------------------------- the cases of the plant parity tests

PLANT_B, PLANT_DT, PLANT_MU = 64, 0.0025, 0.6
PLANT_GAINS = (0.1 / PLANT_DT ** 2, 1.0 / PLANT_DT ** 2)
PLANT_CLAMPS = (np.inf, 0.002)
PLANT_CASES = [(cone, kp, emax, normals, touchdown) for cone in (False, True) for kp in PLANT_GAINS for emax in PLANT_CLAMPS
               for normals in (False, True) for touchdown in (False, True)]
_PLANT = {}


def tilted_normals(B, seed=9, most=0.3):
    """unit world normals [B, 12]: z turned by up to `most` rad about a random horizontal axis (tests/test_plant_contacts_gpu.py's)"""
    rng = np.random.default_rng(seed)
    ang, az = rng.uniform(0.0, most, (B, 4)), rng.uniform(0.0, 2.0 * np.pi, (B, 4))
    n = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=2)
    return np.ascontiguousarray(n.reshape(B, 12))


def plant_inputs(seed=31):
    """64 trot robots with the efforts as drawn, and anchors = the feet displaced by vectors of uniform direction and a length
    uniform in 0 ... 5 mm.  -> (s, tau, anchors [B,12])"""
    if "inputs" not in _PLANT:
        s, tau = PR.case_states("trot", PLANT_B)
        rng = np.random.default_rng(seed)
        d = rng.normal(size=(PLANT_B, 4, 3))
        d *= (rng.uniform(0.0, 0.005, (PLANT_B, 4)) / np.linalg.norm(d, axis=2))[:, :, None]
        _PLANT["inputs"] = (s, tau, np.ascontiguousarray((feet_world(s) + d).reshape(PLANT_B, 12)))
    return _PLANT["inputs"]


def plant_case(cone, kp, emax, normals, touchdown):
    """One case of the parity tests, computed once, shared, never modified -> (state for the call, tau, anchors, previous flags
    [B,4], world normals [B,12] or None, the reference's solve, its report bits, the legs to compare).  k_v = 1 / dt."""
    key = (cone, kp, emax, normals, touchdown)
    if key not in _PLANT:
        s, tau, anchors = plant_inputs()
        nw = tilted_normals(PLANT_B) if normals else None
        st = dict(s, normals=nw) if normals else {k: v for k, v in s.items() if k != "normals"}
        prev = np.zeros((PLANT_B, 4), np.uint8) if touchdown else np.ascontiguousarray(s["stance"], dtype=np.uint8)
        nw4 = None if nw is None else nw.reshape(PLANT_B, 4, 3)
        ref = solve_batch(s, tau, anchors, kp, emax, prev_masks=np.array([PR.mask_of(r) for r in prev]), kv=1.0 / PLANT_DT,
                          mu=PLANT_MU if cone else None, normals_world=nw4)
        bits, compare = report_batch(s, ref, PLANT_MU, cone, nw4)
        _PLANT[key] = (st, tau, anchors, prev, nw, ref, bits, compare)
    return _PLANT[key]

"""Reference of the contact update (qlamd_wholebody_contact_update_batch) in numpy, on the oracle's leg_fk, leg_jacobian and
quat_to_matrix and plant_reference.foot_world_velocity: the feet in the world, the terrain under them (plane, height field, z = 0),
the flag rule, the legs to leave out of a comparison, and the closed loop with tests/plant_contacts_reference.py.
Test infrastructure."""
import numpy as np

import plant_contacts_reference as PCR
import plant_reference as PR
from oracle import oracle as O

TOUCHDOWN, RELEASED_PULL, RELEASED_GAP = 1, 2, 4
STATUS_OK, STATUS_NOT_PD = 0, 2
NEAR = 1e-9          # a tested quantity this close to its threshold, or a foot this close (in cells) to a cell line: not compared
RULE = dict(release_mask=PCR.PULLS, touchdown_distance=0.0, approach_speed=0.0, liftoff_distance=0.0, sensor_distance=0.0)


def foot_world_position(q, quat, pos):
    """[4][3]: p = pos + R r"""
    R = O.quat_to_matrix(quat)
    return np.stack([pos + R @ O.leg_fk(l, q[3 * l:3 * l + 3])[0] for l in range(4)])


def feet(s, i):
    """(p [4][3], u [4][3]) of robot i: world position and velocity of its feet"""
    return (foot_world_position(s["q"][i], s["base_quat"][i], s["base_pos"][i]),
            PR.foot_world_velocity(s["q"][i], s["base_quat"][i], PR.nu_of(s, i)))


def plane_terrain(plane, p):
    """-> (n [3], gap, ok): n = (a, b, c) / |.|, gap = n . p - d / |.|; ok false for a normal of length 0"""
    length = np.linalg.norm(plane[:3])
    if not length > 0.0:
        return np.zeros(3), 0.0, False
    n = plane[:3] / length
    return n, n @ p - plane[3] / length, True


def cell_of(x, origin, resolution, n):
    """-> (cell, frac, near): s = clamp((x - origin) / resolution, 0, n - 1), cell = min(floor(s), n - 2), frac = s - cell;
    near: s lies within NEAR of a cell line (the borders included: there the clamp switches on)"""
    s = min(max((x - origin) / resolution, 0.0), n - 1.0)
    raw = (x - origin) / resolution
    cell = min(int(np.floor(s)), n - 2)
    return cell, s - cell, abs(raw - np.round(raw)) <= NEAR


def heightfield_terrain(hf, p):
    """hf: dict(origin (x, y), resolution, heights [ny, nx]) -> (n [3], gap, near_line, cells [4])"""
    H = hf["heights"]
    ny, nx = H.shape
    i, a, near_x = cell_of(p[0], hf["origin"][0], hf["resolution"], nx)
    j, b, near_y = cell_of(p[1], hf["origin"][1], hf["resolution"], ny)
    h00, h10, h01, h11 = H[j, i], H[j, i + 1], H[j + 1, i], H[j + 1, i + 1]
    h = (1 - a) * (1 - b) * h00 + a * (1 - b) * h10 + (1 - a) * b * h01 + a * b * h11
    hx = ((1 - b) * (h10 - h00) + b * (h11 - h01)) / hf["resolution"]
    hy = ((1 - a) * (h01 - h00) + a * (h11 - h10)) / hf["resolution"]
    n = np.array([-hx, -hy, 1.0]) / np.sqrt(hx * hx + hy * hy + 1.0)
    return n, n[2] * (p[2] - h), near_x or near_y, np.array([h00, h10, h01, h11])


def flag_rule(flagged, report, gap, nu, rule):
    """-> (next, events, sensor, borderline) for one leg"""
    pull = (int(report) & int(rule["release_mask"])) != 0
    far = gap > rule["liftoff_distance"]
    touch = gap <= rule["touchdown_distance"] and nu <= rule["approach_speed"]
    sensor = gap <= rule["sensor_distance"]
    border = abs(gap - rule["sensor_distance"]) <= NEAR
    if flagged:
        border = border or abs(gap - rule["liftoff_distance"]) <= NEAR
        return (not (pull or far)), (RELEASED_PULL if pull else 0) | (RELEASED_GAP if far else 0), sensor, border
    border = border or abs(gap - rule["touchdown_distance"]) <= NEAR or abs(nu - rule["approach_speed"]) <= NEAR
    return touch, TOUCHDOWN if touch else 0, sensor, border


def update_batch(s, plane=None, hf=None, report=None, **rule):
    """The whole entry.  s: q, qd, base_quat, base_linvel, base_angvel, base_pos and, optionally, stance (the current flags).
    -> dict(support_next, sensor, events uint8 [B,4]; gap [B,4]; normals, foot_pos, foot_vel [B,4,3]; status [B]; nu [B,4] = n . u;
    compare [B,4] bool: false where a tested quantity lies within NEAR of its threshold or, with a height field, the foot within
    NEAR cells of a cell line; near_line [B,4] bool: the second of the two alone)"""
    rule = dict(RULE, **rule)
    B = s["q"].shape[0]
    stance = s.get("stance")
    cur = np.zeros((B, 4), np.uint8) if stance is None else np.asarray(stance, np.uint8)
    out = dict(support_next=cur.copy(), sensor=np.zeros((B, 4), np.uint8), events=np.zeros((B, 4), np.uint8), gap=np.zeros((B, 4)),
               normals=np.zeros((B, 4, 3)), foot_pos=np.zeros((B, 4, 3)), foot_vel=np.zeros((B, 4, 3)), nu=np.zeros((B, 4)),
               status=np.zeros(B, np.int32), compare=np.ones((B, 4), bool), near_line=np.zeros((B, 4), bool))
    for i in range(B):
        read = [s[k][i] for k in ("q", "qd", "base_quat", "base_linvel", "base_angvel", "base_pos")]
        ok = all(np.isfinite(v).all() for v in read)
        rows = []
        if ok:
            p, u = feet(s, i)
            ok = bool(np.isfinite(p).all() and np.isfinite(u).all())
        for l in range(4) if ok else ():
            near = False
            if hf is not None:
                n, gap, near, cells = heightfield_terrain(hf, p[l])
                ok = ok and bool(np.isfinite(cells).all())
            elif plane is not None:
                n, gap, good = plane_terrain(plane[i], p[l])
                ok = ok and good and bool(np.isfinite(plane[i]).all())
            else:
                n, gap = np.array([0.0, 0.0, 1.0]), p[l][2]
            ok = ok and bool(np.isfinite(gap) and np.isfinite(n).all())
            rows.append((n, gap, near))
        if not ok:
            out["status"][i] = STATUS_NOT_PD
            continue
        for l, (n, gap, near) in enumerate(rows):
            nu = n @ u[l]
            nxt, ev, sensor, border = flag_rule(cur[i, l] != 0, 0 if report is None else report[i, l], gap, nu, rule)
            out["support_next"][i, l], out["events"][i, l], out["sensor"][i, l] = nxt, ev, sensor
            out["gap"][i, l], out["normals"][i, l], out["nu"][i, l] = gap, n, nu
            out["compare"][i, l], out["near_line"][i, l] = not (border or near), near
        out["foot_pos"][i], out["foot_vel"][i] = p, u
    return out


def loop(s, tau, ticks, dt, kv, mu, plane, **rule):
    """The closed loop on the CPU: plant step (plant_contacts_reference) -> contact update, `ticks` times, from no foot flagged.
    The plant's report takes the update's normals.  -> (state, list per tick of dict(flags = the flags the plant ran with, report,
    support_next, events, gap, nu, valid [B] bool)): a robot is valid until the tick at which one of its legs is borderline -- in
    the update, or in the plant's report (plant_contacts_reference.report) -- and never again after."""
    s = {k: np.array(v, copy=True) for k, v in s.items()}
    B = s["q"].shape[0]
    s["stance"] = np.zeros((B, 4), np.uint8)
    prev = np.zeros(B, int)
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (B, 4, 1))
    valid = np.ones(B, bool)
    ticks_out = []
    for _ in range(ticks):
        masks = np.array([PR.mask_of(r) for r in s["stance"]])
        ref = PCR.solve_batch(s, tau, masks=masks, prev_masks=prev, kv=kv)
        bits, cmp_report = PCR.report_batch(s, ref, mu, normals)
        s.update(PCR.step_batch(s, ref, dt))
        upd = update_batch(s, plane=plane, report=bits, **rule)
        valid = valid & upd["compare"].all(axis=1) & cmp_report.all(axis=1)
        ticks_out.append(dict(flags=s["stance"].copy(), report=bits, support_next=upd["support_next"], events=upd["events"],
                              gap=upd["gap"], nu=upd["nu"], valid=valid.copy()))
        prev = masks
        s["stance"] = upd["support_next"].copy()
        normals = upd["normals"]
    return s, ticks_out


LOOP_TICKS, LOOP_DT, LOOP_MU = 32, 0.0025, 0.6


def loop_case():
    """The case of the loop tests: 16 trot robots with the efforts as drawn, the ground 5 mm under each robot's lowest foot, a
    foot released 10 mm above it.  -> (states, tau, plane [16,4], the rule's distances)"""
    s, tau = PR.case_states("trot", 16)
    low = np.array([feet(s, i)[0][:, 2].min() for i in range(16)])
    plane = np.zeros((16, 4))
    plane[:, 2], plane[:, 3] = 1.0, low - 0.005
    return s, tau, plane, dict(liftoff_distance=0.01, sensor_distance=0.005)

"""Reference of the plant step with contacts (qlamd_wholebody_plant_step_batch) in numpy, on tests/plant_reference.py and the
oracle's M, h, Jc: the impact KKT, the stabilised KKT at nu+, the contact report with the entries to skip near a boundary, the
state update starting from nu+ and the tolerances.  Test infrastructure."""
import numpy as np

import plant_reference as PR
from oracle import oracle as O

PULLS, OUTSIDE_CONE, TOUCHDOWN = 1, 2, 4


def impact(M, Jc, nu, mask):
    """M (nu+ - nu) = Js' p, Js nu+ = 0 over the legs of `mask` -> (nu+ [18], p [12])."""
    rows = PR.rows_of(mask)
    if not rows:
        return nu.copy(), np.zeros(12)
    Js = Jc[rows]
    n = len(rows)
    K = np.zeros((18 + n, 18 + n))
    K[:18, :18] = M
    K[:18, 18:] = -Js.T
    K[18:, :18] = Js
    x = np.linalg.solve(K, np.concatenate([M @ nu, np.zeros(n)]))
    p = np.zeros(12)
    p[rows] = x[18:]
    return x[:18], p


def solve(q, quat, nu, tau, mask, prev_mask=None, kv=0.0, g_ext=None, gravity=9.81):
    """-> dict(nu_plus [18], p [12], acc [18], f [12], touch, M, h, Jc, gamma): the impact over all of `mask` when a leg of it is
    not in prev_mask (None: no touchdown), then M nu' - Js' f = [0; tau] + g_ext - h(q, nu+), Js nu' = -gamma(q, nu+) - kv Js nu+."""
    M = O.wb_mass_matrix(q)
    Jc = O.wb_contact_jacobian(q)
    touch = 0 if prev_mask is None else mask & ~prev_mask & 0xF
    if touch:
        nup, p = impact(M, Jc, nu, mask)
    else:
        nup, p = nu.copy(), np.zeros(12)
    h = O.wb_nonlinear_effects(q, quat, nup, gravity)
    gam = PR.gamma(q, nup)
    rows = PR.rows_of(mask)
    Js = Jc[rows]
    n = len(rows)
    rhs = np.concatenate([np.zeros(6), tau]) - h
    if g_ext is not None:
        rhs = rhs + g_ext
    K = np.zeros((18 + n, 18 + n))
    K[:18, :18] = M
    K[:18, 18:] = -Js.T
    K[18:, :18] = Js
    x = np.linalg.solve(K, np.concatenate([rhs, -gam[rows] - kv * (Js @ nup)]))
    f = np.zeros(12)
    f[rows] = x[18:]
    return dict(nu_plus=nup, p=p, acc=x[:18], f=f, touch=touch, M=M, h=h, Jc=Jc, gamma=gam)


def solve_batch(s, tau, masks=None, prev_masks=None, kv=0.0, g_ext=None, gravity=9.81):
    """Per robot; masks: [B] or None = from s["stance"]; prev_masks: [B] or None = no touchdown anywhere."""
    B = s["q"].shape[0]
    out = dict(nu_plus=np.zeros((B, 18)), p=np.zeros((B, 12)), acc=np.zeros((B, 18)), f=np.zeros((B, 12)), nu=np.zeros((B, 18)),
               mask=np.zeros(B, int), touch=np.zeros(B, int))
    for i in range(B):
        m = PR.mask_of(s["stance"][i]) if masks is None else int(masks[i])
        nu = PR.nu_of(s, i)
        r = solve(s["q"][i], s["base_quat"][i], nu, tau[i], m, None if prev_masks is None else int(prev_masks[i]), kv,
                  None if g_ext is None else g_ext[i], gravity)
        for k in ("nu_plus", "p", "acc", "f"):
            out[k][i] = r[k]
        out["nu"][i], out["mask"][i], out["touch"][i] = nu, m, r["touch"]
    return out


def tol(ref):
    """Per robot: 1e-6 x max(1, max |value| of that robot) -- plant_reference.tolerances, for one array."""
    return PR.tolerances(ref, ref)[0]


def normals_in_base(quat, normals_world=None):
    """[4][3]: the unit normals of the report in base coordinates: R' n_W, or the base's z axis."""
    if normals_world is None:
        return np.tile(np.array([0.0, 0.0, 1.0]), (4, 1))
    R = O.quat_to_matrix(quat)
    return np.asarray(normals_world).reshape(4, 3) @ R   # rows: (R' n)' = n' R


def report(f, mask, touch, n_base, mu, tol_f):
    """-> (bits [4], compare [4] bool).  A flagged leg is left out of the comparison when f.n lies within tol_f of 0, or
    |f_t| - mu max(f.n, 0) within (1 + mu) tol_f of 0: there the device's f, which may differ by tol_f, can fall on the other side.
    (TOUCHDOWN is exact and compared on every leg.)"""
    bits, compare = np.zeros(4, np.uint8), np.ones(4, bool)
    for l in range(4):
        if not (mask >> l) & 1:
            continue
        fl, n = f[3 * l:3 * l + 3], n_base[l]
        fn = fl @ n
        margin = np.linalg.norm(fl - fn * n) - mu * max(fn, 0.0)
        bits[l] = (PULLS if fn < 0.0 else 0) | (OUTSIDE_CONE if margin > 0.0 else 0) | (TOUCHDOWN if (touch >> l) & 1 else 0)
        compare[l] = abs(fn) > tol_f and abs(margin) > (1.0 + mu) * tol_f
    return bits, compare


def report_batch(s, ref, mu, normals_world=None):
    B = s["q"].shape[0]
    tol_f = tol(ref["f"])
    bits, compare = np.zeros((B, 4), np.uint8), np.ones((B, 4), bool)
    for i in range(B):
        nb = normals_in_base(s["base_quat"][i], None if normals_world is None else normals_world[i])
        bits[i], compare[i] = report(ref["f"][i], int(ref["mask"][i]), int(ref["touch"][i]), nb, mu, tol_f[i])
    return bits, compare


def update(q, pos, quat, nu_plus, acc, dt):
    """plant_reference.update starting from nu+ (its world linear velocity is R(quat) v+)."""
    R = O.quat_to_matrix(quat)
    return PR.update(q, nu_plus[6:], pos, quat, R @ nu_plus[0:3], nu_plus[3:6], acc, dt)


def step_batch(s, ref, dt):
    B = s["q"].shape[0]
    rows = [update(s["q"][i], s["base_pos"][i], s["base_quat"][i], ref["nu_plus"][i], ref["acc"][i], dt) for i in range(B)]
    return {k: np.stack([r[k] for r in rows]) for k in PR.NEXT_KEYS}


def held_foot_speeds(s, masks=None):
    """World speeds of the feet flagged in s["stance"] (or masks), all robots, one flat array."""
    out = []
    for i in range(s["q"].shape[0]):
        m = PR.mask_of(s["stance"][i]) if masks is None else int(masks[i])
        v = PR.foot_world_velocity(s["q"][i], s["base_quat"][i], PR.nu_of(s, i))
        out += [np.linalg.norm(v[l]) for l in range(4) if (m >> l) & 1]
    return np.array(out)


def rollout(s, tau, steps, dt, project, kv):
    """`steps` reference steps with constant flags and torques; project: the plastic impact at step 0 (previous flags of zero).
    -> the final state."""
    s = {k: np.array(v, copy=True) for k, v in s.items()}
    B = s["q"].shape[0]
    for k in range(steps):
        ref = solve_batch(s, tau, prev_masks=np.zeros(B, int) if (project and k == 0) else None, kv=kv)
        s.update(step_batch(s, ref, dt))
    return s

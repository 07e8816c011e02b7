"""Reference of the plant step with friction (qlamd_wholebody_plant_step_friction_batch) in numpy, on tests/plant_reference.py,
tests/plant_contacts_reference.py and the oracle's M, h, Jc: the pyramid, the impulse QP and the force QP through the oracle's own
solve_quadprog, the report from the slacks of f with the legs to leave out near a boundary.  Test infrastructure.
include/qlamd_plant_friction.h has the model."""
import numpy as np

import plant_contacts_reference as PCR
import plant_reference as PR
from oracle import oracle as O

TOUCHDOWN, SEPARATING, SLIDING = 4, 8, 16


def frames(quat, normals_world=None):
    """[(n, t1, t2)] per leg in base coordinates: n = R' n_W or the base's z axis, t1 = normalise(n x y_B), t2 = normalise(n x t1)."""
    R = O.quat_to_matrix(quat)
    yB = R.T @ np.array([0.0, 1.0, 0.0])
    nb = PCR.normals_in_base(quat, normals_world)
    out = []
    for l in range(4):
        n = nb[l]
        t1 = np.cross(n, yB)
        t1 = t1 / np.linalg.norm(t1)
        t2 = np.cross(n, t1)
        t2 = t2 / np.linalg.norm(t2)
        out.append((n, t1, t2))
    return out


def pyramid(legs, fr, mu):
    """CI [3 |S|, 5 |S|]: per flagged leg the columns n, mu n + t1, mu n - t1, mu n + t2, mu n - t2 on the leg's three variables."""
    CI = np.zeros((3 * len(legs), 5 * len(legs)))
    for k, l in enumerate(legs):
        n, t1, t2 = fr[l]
        for j, v in enumerate((n, mu * n + t1, mu * n - t1, mu * n + t2, mu * n - t2)):
            CI[3 * k:3 * k + 3, 5 * k + j] = v
    return CI


def cone_qp(H0, c, CI):
    """argmin_{CI'y >= 0} 1/2 y'H0 y - y'c -> (y, iterations)."""
    if H0.shape[0] == 0:
        return np.zeros(0), 0
    r = O.solve_quadprog(H0, -c, CI=CI, ci0=np.zeros(CI.shape[1]))
    assert r["status"] == 0, r["status"]
    return r["x"], int(r["iters"])


def solve(q, quat, nu, tau, mask, mu, prev_mask=None, kv=0.0, g_ext=None, gravity=9.81, normals_world=None):
    """-> dict(nu_plus [18], p [12], acc [18], f [12], touch, iters (2), H0, Js, CI, c_p, c_f, r, legs, rows, M)."""
    M = O.wb_mass_matrix(q)
    Jc = O.wb_contact_jacobian(q)
    Mi = np.linalg.inv(M)
    rows = PR.rows_of(mask)
    legs = [l for l in range(4) if (mask >> l) & 1]
    Js = Jc[rows]
    H0 = Js @ Mi @ Js.T
    CI = pyramid(legs, frames(quat, normals_world), mu)
    touch = 0 if prev_mask is None else mask & ~prev_mask & 0xF
    p, it_p, c_p = np.zeros(12), 0, -(Js @ nu)
    if touch:
        y, it_p = cone_qp(H0, c_p, CI)
        p[rows] = y
        nup = nu + Mi @ (Js.T @ y)
    else:
        nup = nu.copy()
    h = O.wb_nonlinear_effects(q, quat, nup, gravity)
    gam = PR.gamma(q, nup)
    rhs = np.concatenate([np.zeros(6), tau]) - h
    if g_ext is not None:
        rhs = rhs + g_ext
    x0 = Mi @ rhs
    r = -gam[rows] - kv * (Js @ nup)
    c_f = r - Js @ x0
    y, it_f = cone_qp(H0, c_f, CI)
    f = np.zeros(12)
    f[rows] = y
    return dict(nu_plus=nup, p=p, acc=x0 + Mi @ (Js.T @ y), f=f, touch=touch, iters=(it_p, it_f), H0=H0, Js=Js, CI=CI, c_p=c_p, c_f=c_f,
                r=r, legs=legs, rows=rows, M=M)


def solve_batch(s, tau, mu, masks=None, prev_masks=None, kv=0.0, g_ext=None, gravity=9.81, normals_world=None, keep=False):
    """Per robot; masks: [B] or None = from s["stance"]; prev_masks: [B] or None = no touchdown anywhere; normals_world [B,4,3] or
    None.  keep: the per-robot dicts as well, under "robots"."""
    B = s["q"].shape[0]
    out = dict(nu_plus=np.zeros((B, 18)), p=np.zeros((B, 12)), acc=np.zeros((B, 18)), f=np.zeros((B, 12)), nu=np.zeros((B, 18)),
               mask=np.zeros(B, int), touch=np.zeros(B, int), iters=np.zeros((B, 2), int), robots=[])
    for i in range(B):
        m = PR.mask_of(s["stance"][i]) if masks is None else int(masks[i])
        nu = PR.nu_of(s, i)
        r = solve(s["q"][i], s["base_quat"][i], nu, tau[i], m, mu, None if prev_masks is None else int(prev_masks[i]), kv,
                  None if g_ext is None else g_ext[i], gravity, None if normals_world is None else normals_world[i])
        for k in ("nu_plus", "p", "acc", "f"):
            out[k][i] = r[k]
        out["nu"][i], out["mask"][i], out["touch"][i], out["iters"][i] = nu, m, r["touch"], r["iters"]
        if keep:
            out["robots"].append(r)
    return out


def kinds(y, mask, fr, mu, tol_y):
    """Per leg from the slacks of y [12] (a force or an impulse): (kind [4], compare [4]); kind 0 unflagged, 1 sticking, SEPARATING
    or SLIDING.  A row is active if its slack <= (1 + mu) tol_y and inactive if its slack > 100 (1 + mu) tol_y; a leg with a slack
    in between is left out of comparisons."""
    kind, compare = np.zeros(4, int), np.ones(4, bool)
    lo, hi = (1.0 + mu) * tol_y, 100.0 * (1.0 + mu) * tol_y
    for l in range(4):
        if not (mask >> l) & 1:
            continue
        n, t1, t2 = fr[l]
        yl = y[3 * l:3 * l + 3]
        sl = np.array([n @ yl, (mu * n + t1) @ yl, (mu * n - t1) @ yl, (mu * n + t2) @ yl, (mu * n - t2) @ yl])
        compare[l] = not ((sl > lo) & (sl <= hi)).any()
        kind[l] = SEPARATING if sl[0] <= lo else (SLIDING if sl[1:].min() <= lo else 1)
    return kind, compare


def report_batch(s, ref, mu, normals_world=None, key="f"):
    """-> (bits [B,4] uint8, compare [B,4] bool, kind [B,4]) of the force (key "f": the report, with TOUCHDOWN) or the impulse."""
    B = s["q"].shape[0]
    tol_y = PCR.tol(ref[key])
    bits, compare, kind = np.zeros((B, 4), np.uint8), np.ones((B, 4), bool), np.zeros((B, 4), int)
    for i in range(B):
        fr = frames(s["base_quat"][i], None if normals_world is None else normals_world[i])
        kind[i], compare[i] = kinds(ref[key][i], int(ref["mask"][i]), fr, mu, tol_y[i])
        for l in range(4):
            if (int(ref["mask"][i]) >> l) & 1:
                bits[i, l] = (kind[i, l] if kind[i, l] > 1 else 0) | (TOUCHDOWN if (int(ref["touch"][i]) >> l) & 1 else 0)
    return bits, compare, kind


def slacks(y, mask, fr, mu):
    """[n flagged legs, 5] pyramid slacks of y [12]"""
    out = []
    for l in range(4):
        if (mask >> l) & 1:
            n, t1, t2 = fr[l]
            yl = y[3 * l:3 * l + 3]
            out.append([n @ yl, (mu * n + t1) @ yl, (mu * n - t1) @ yl, (mu * n + t2) @ yl, (mu * n - t2) @ yl])
    return np.array(out).reshape(-1, 5)

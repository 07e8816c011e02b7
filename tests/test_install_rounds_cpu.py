"""The arithmetic of a warm start's install round (force_qp_coop.hpp), restated in numpy: the block form -- Gram block of the
round's four rows, its LDL', corrected directions, four rank-one updates in one go -- against the sequential form it replaces
(direction, pivot, full step, rank-one update, row after row).  Block elimination of the same rows in the same order: the same
H, N*, x and u to rounding, and the same row left out."""
import numpy as np
import pytest

PIVOT_MIN = 1e-6   # a row whose pivot n'z~ is below this depends on the rows before it and is left out
NV, NLEGS = 12, 4


def _spd(rng, cond=3e5):
    q, _ = np.linalg.qr(rng.normal(size=(NV, NV)))
    ev = np.logspace(0.0, np.log10(cond), NV) * 1e-4     # H = G^-1 reaches 1e4, as with w_reg = 1e-4
    return (q * ev) @ q.T


def _leg_row(rng, leg):
    n = np.zeros(NV)
    n[3 * leg:3 * leg + 3] = rng.normal(size=3)
    return n


class State:
    """H, N* (a row per slot), x, u and the slots in use."""

    def __init__(self, G, g0):
        self.H = np.linalg.inv(G)
        self.H = 0.5 * (self.H + self.H.T)
        self.Ns = np.zeros((NV, NV))
        self.x = -self.H @ g0
        self.u = np.zeros(NV)
        self.used = []          # slot -> row id, in slot order
        self.left_out = []

    def copy(self):
        o = State.__new__(State)
        o.H, o.Ns, o.x, o.u = self.H.copy(), self.Ns.copy(), self.x.copy(), self.u.copy()
        o.used, o.left_out = list(self.used), list(self.left_out)
        return o


def install_sequential(S, rows, offsets, ids, have):
    for n, b, rid, hv in zip(rows, offsets, ids, have):
        z, r = S.H @ n, S.Ns @ n
        d = n @ z
        if not (hv and d > PIVOT_MIN):
            if hv:
                S.left_out.append(rid)
            continue
        tw = -(n @ S.x - b) / d
        S.x = S.x + tw * z
        S.u = S.u - tw * r
        slot = len(S.used)
        S.u[slot] = tw
        r = r.copy()
        r[slot] = -1.0
        S.H = S.H - np.outer(z, z) / d
        S.Ns = S.Ns - np.outer(r, z) / d
        S.used.append(rid)


def install_block(S, rows, offsets, ids, have):
    K = len(rows)
    N = np.stack(rows, axis=1)                     # 12 x K
    Z, R = S.H @ N, S.Ns @ N                       # one sweep for all rows
    D = N.T @ Z                                    # the Gram block: D[m][k] = n_m'z_k
    sl = N.T @ S.x - np.asarray(offsets)
    L, W = np.zeros((K, K)), np.zeros((K, K))      # W[m][k] = n_m'z~_k = L[m][k] d_k
    zi, tw, d = np.zeros(K), np.zeros(K), np.zeros(K)
    for k in range(K):
        d[k] = D[k, k] - sum(L[k, j] * W[k, j] for j in range(k))
        s = sl[k] + sum(tw[j] * W[k, j] for j in range(k))
        ok = have[k] and d[k] > PIVOT_MIN
        zi[k] = 1.0 / d[k] if ok else 0.0
        tw[k] = -s * zi[k]
        for m in range(k + 1, K):
            W[m, k] = D[k, m] - sum(L[k, j] * W[m, j] for j in range(k))
            L[m, k] = W[m, k] * zi[k]
        for j in range(k):
            Z[:, k] -= L[k, j] * Z[:, j]
            R[:, k] -= L[k, j] * R[:, j]
        if not ok:
            Z[:, k] = 0.0
            R[:, k] = 0.0
            if have[k]:
                S.left_out.append(ids[k])
            continue
        S.x = S.x + tw[k] * Z[:, k]
        S.u = S.u - tw[k] * R[:, k]
        slot = len(S.used)
        S.u[slot] = tw[k]
        R[slot, k] = -1.0
        S.used.append(ids[k])
    # the K rank-one updates in one go
    S.H = S.H - (Z * zi) @ Z.T
    S.Ns = S.Ns - (R * zi) @ Z.T


def _problem(seed, n_installed, dependent_leg):
    rng = np.random.default_rng(seed)
    G = _spd(rng)
    assert 1e5 < np.linalg.cond(G) < 1e6
    S = State(G, rng.normal(size=NV))
    per_leg = [[] for _ in range(NLEGS)]
    for i in range(n_installed):                   # at most two rows a leg, so that every leg has room for one more
        leg = i % NLEGS
        n = _leg_row(rng, leg)
        per_leg[leg].append(n)
        install_sequential(S, [n], [rng.normal()], [100 + i], [True])
    assert len(S.used) == n_installed and not S.left_out
    rows = [_leg_row(rng, leg) for leg in range(NLEGS)]
    have = [True] * NLEGS
    if dependent_leg is not None:
        if per_leg[dependent_leg]:                 # a combination of the rows of its leg that are in already
            rows[dependent_leg] = sum(rng.normal() * n for n in per_leg[dependent_leg])
        else:                                      # nothing to depend on: a leg without a row (zero normal, biased divisor)
            rows[dependent_leg] = np.zeros(NV)
            have[dependent_leg] = False
    return S, rows, list(rng.normal(size=NLEGS)), list(range(NLEGS)), have


def _rel(a, b, before):
    """Relative to the entries the round works on: with twelve independent rows in, H is exactly 0 and what either form leaves
    is the cancellation noise of entries the size of the H it started from."""
    return np.abs(a - b).max() / max(np.abs(b).max(), np.abs(before).max(), 1e-300)


@pytest.mark.parametrize("n_installed", [0, 1, 3, 5, 8])
@pytest.mark.parametrize("dependent_leg", [None, 0, 2, 3])
def test_the_block_form_is_the_sequential_form(n_installed, dependent_leg):
    S0, rows, offsets, ids, have = _problem(7 + n_installed, n_installed, dependent_leg)
    A, B = S0.copy(), S0.copy()
    install_sequential(A, rows, offsets, ids, have)
    install_block(B, rows, offsets, ids, have)
    assert A.used == B.used and A.left_out == B.left_out
    if dependent_leg is not None and have[dependent_leg]:
        assert A.left_out == [dependent_leg]       # the dependent row, and only that one
    else:
        assert A.left_out == []
    assert len(A.used) == n_installed + sum(have) - len(A.left_out)
    for name in ("H", "Ns", "x", "u"):
        rel = _rel(getattr(B, name), getattr(A, name), getattr(S0, name))
        assert rel < 1e-9, (name, rel)
    # and it is an install: the rows that went in hold with equality at the new x
    for k in A.used[n_installed:]:
        assert abs(rows[k] @ B.x - offsets[k]) < 1e-8 * max(1.0, np.abs(B.x).max())


def test_rows_of_one_round_that_share_a_leg_depend_through_the_block():
    """(The kernel never puts two rows of a leg into one round; the factorisation does not know that.)  Rows 0 and 2 on the same
    leg and parallel: the pivot of the later one vanishes inside the LDL', where the sequential form finds it in H."""
    S0, rows, offsets, ids, have = _problem(3, 4, None)
    rows[2] = 1.7 * rows[0]
    A, B = S0.copy(), S0.copy()
    install_sequential(A, rows, offsets, ids, have)
    install_block(B, rows, offsets, ids, have)
    assert A.left_out == B.left_out == [2] and A.used == B.used
    for name in ("H", "Ns", "x", "u"):
        assert _rel(getattr(B, name), getattr(A, name), getattr(S0, name)) < 1e-9, name

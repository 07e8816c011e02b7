"""The warm start's install rounds with a fixed slot map and the bookkeeping behind the loop (force_qp_coop.hpp, the block form
without a robot that builds its set), in numpy on top of the arithmetic of tests/test_install_rounds_cpu.py.

What the kernel does: the working set is known before the first round, so round r brings the (r + 1)-th row of every leg (lowest
kind first); the row of leg k in round r takes slot lane kLegs * r + k whatever went in before it; a round keeps a flag per slot
lane ("taken") and nothing else, asks the pivot alone whether a row goes in (a leg without a row has a zero normal, so its pivot
is an exact 0), and gives the new slot its multiplier through the -1 it holds in r~ (a free lane's row of N* and its u are exact
zeros).  used, q, the ids, the active mask and the update count are rebuilt from the flags behind the last round.  Against it: the
row-by-row form with its lowest-free-slot bookkeeping, the same rows in the same order."""
import numpy as np
import pytest

from test_install_rounds_cpu import NV, PIVOT_MIN, State, _spd, install_sequential

KINDS = 5          # rows of a leg: 0 minimum force, 1..4 friction; row id = KINDS * leg + kind


def decode(word, legs):
    """The rows round r brings: [r][k] = kind of leg k's (r + 1)-th row (lowest bit first), None without one."""
    per_leg = [[kd for kd in range(KINDS) if (word >> (KINDS * k + kd)) & 1] for k in range(legs)]
    return [[per_leg[k][r] if r < len(per_leg[k]) else None for k in range(legs)] for r in range(3)]


def slot_lane(r, k, legs):
    return legs * r + k


def slot_row_id(lane, word, legs):
    """What the kernel decodes on slot lane `lane` before the loop: the id of the row the fixed map would put there."""
    sr, sk = lane // legs, lane % legs
    rows = (word >> (KINDS * sk)) & 0x1F
    for _ in range(sr):
        rows &= rows - 1
    return KINDS * sk + (rows & -rows).bit_length() - 1 if rows else None


def normals_of(rng, legs, dependent=None):
    """A normal per (leg, kind), each on the three variables of its leg; `dependent` = (leg, kind, of): that row is a
    combination of the rows `of` of its leg."""
    n = np.zeros((legs, KINDS, NV))
    for k in range(legs):
        n[k, :, 3 * k:3 * k + 3] = rng.normal(size=(KINDS, 3))
    if dependent is not None:
        k, kd, of = dependent
        n[k, kd] = sum(rng.normal() * n[k, o] for o in of)
    return n


def rounds_row_by_row(S, word, legs, nrm, off):
    """The form being replaced, bookkeeping included: lowest free slot, one row after the other."""
    used, act, idk, q = 0, 0, {}, 0
    for r, kinds in enumerate(decode(word, legs)):
        for k, kd in enumerate(kinds):
            if kd is None:
                continue
            before = len(S.used)
            install_sequential(S, [nrm[k, kd]], [off[k, kd]], [KINDS * k + kd], [True])
            if len(S.used) == before:
                continue                            # left out
            slot = (~used & (used + 1)).bit_length() - 1
            assert slot == before                   # (no drops in between: the lowest free slot is the next one)
            used |= 1 << slot
            act |= 1 << (KINDS * k + kd)
            idk[slot] = KINDS * k + kd
            q += 1
    return dict(used=used, act_mask=act, idk=idk, q=q, warm_updates=q)


def rounds_fixed_map(S, word, legs, nrm, off):
    """The new form.  S.used is not touched: the slots are S.Ns' rows, at the lanes of the fixed map."""
    taken = [False] * 16
    for r, kinds in enumerate(decode(word, legs)):
        if all(kd is None for kd in kinds):
            break
        N = np.stack([nrm[k, kd] if kd is not None else np.zeros(NV) for k, kd in enumerate(kinds)], axis=1)
        b = np.array([off[k, kd] if kd is not None else 0.0 for k, kd in enumerate(kinds)])
        K = legs
        Z, R = S.H @ N, S.Ns @ N
        D = N.T @ Z
        sl = N.T @ S.x - b
        L, W = np.zeros((K, K)), np.zeros((K, K))
        zi, tw = np.zeros(K), np.zeros(K)
        for k in range(K):
            d = D[k, k] - sum(L[k, j] * W[k, j] for j in range(k))
            s = sl[k] + sum(tw[j] * W[k, j] for j in range(k))
            if kinds[k] is None:
                assert d == 0.0                     # exactly: the pivot alone says that there is no row
            ok = d > PIVOT_MIN
            zi[k] = 1.0 / d if ok else 0.0
            tw[k] = -s * zi[k]
            for m in range(k + 1, K):
                W[m, k] = D[k, m] - sum(L[k, j] * W[m, j] for j in range(k))
                L[m, k] = W[m, k] * zi[k]
            for j in range(k):
                Z[:, k] -= L[k, j] * Z[:, j]
                R[:, k] -= L[k, j] * R[:, j]
            okf = 1.0 if ok else 0.0
            Z[:, k] *= okf
            R[:, k] *= okf
            S.x = S.x + tw[k] * Z[:, k]
            lane = slot_lane(r, k, legs)
            if ok:
                assert not taken[lane] and S.u[lane] == 0.0 and R[lane, k] == 0.0 and not S.Ns[lane].any()
                R[lane, k] = -1.0
                taken[lane] = True
            S.u = S.u - tw[k] * R[:, k]             # no select: 0 + t_k on the new slot's lane
            if ok:
                assert S.u[lane] == tw[k]
        S.H = S.H - (Z * zi) @ Z.T
        S.Ns = S.Ns - (R * zi) @ Z.T
    # ---- behind the loop: everything from the flags and the decoded set
    used = sum(1 << lane for lane in range(16) if taken[lane])
    idk = {lane: slot_row_id(lane, word, legs) for lane in range(16) if taken[lane]}
    act = 0
    for rid in idk.values():
        act |= 1 << rid
    q = bin(used).count("1")
    return dict(used=used, act_mask=act, idk=idk, q=q, warm_updates=q)


def _word(per_leg_kinds):
    return sum(1 << (KINDS * k + kd) for k, kinds in enumerate(per_leg_kinds) for kd in kinds)


def _random_sets(rng, legs, n):
    out = []
    for _ in range(n):
        out.append(_word([sorted(rng.choice(KINDS, size=rng.integers(0, 4), replace=False).tolist()) for _ in range(legs)]))
    return out


HAND_MADE = {
    4: [_word([[0, 1, 3], [0, 2, 4], [1, 2, 3], [0, 3, 4]]),      # twelve rows: three full rounds
        _word([[0], [], [1, 4], [2, 3, 4]]),                     # gaps: legs without a row in round 0, 1 and 2
        _word([[], [], [], [0, 1, 2]]),                          # one leg alone: lanes 3, 7, 11
        _word([[], [2], [], []]),
        0],
    2: [_word([[0, 1, 3], [0, 2, 4]]),
        _word([[], [1, 2, 4]]),                                  # lanes 1, 3, 5
        _word([[0, 3], []]),
        0],
}


@pytest.mark.parametrize("legs", [4, 2])
def test_the_bookkeeping_rebuilt_behind_the_loop_is_the_row_by_row_bookkeeping(legs):
    rng = np.random.default_rng(31 + legs)
    for word in HAND_MADE[legs] + _random_sets(rng, legs, 40):
        S0 = State(_spd(rng), rng.normal(size=NV))
        nrm, off = normals_of(rng, legs), rng.normal(size=(legs, KINDS))
        A, B = S0.copy(), S0.copy()
        a = rounds_row_by_row(A, word, legs, nrm, off)
        b = rounds_fixed_map(B, word, legs, nrm, off)
        assert not A.left_out
        _same_bookkeeping(a, b, word, legs)
        _same_state(A, a, B, b, S0)


def _same_bookkeeping(a, b, word, legs):
    assert b["q"] == a["q"] == bin(b["used"]).count("1") == bin(a["used"]).count("1")
    assert b["warm_updates"] == a["warm_updates"]
    assert b["act_mask"] == a["act_mask"]
    assert sorted(b["idk"].values()) == sorted(a["idk"].values())             # the slots hold the same rows ...
    rows = decode(word, legs)
    for lane, rid in b["idk"].items():                                       # ... at the lanes of the fixed map
        r, k = lane // legs, lane % legs
        assert rid == KINDS * k + rows[r][k] and lane == slot_lane(r, k, legs)
    assert b["used"] >> (3 * legs) == 0


def _same_state(A, a, B, b, S0):
    """H, x to rounding; N* and u slot by slot, matched through the row ids."""
    scale = lambda name: max(np.abs(getattr(A, name)).max(), np.abs(getattr(S0, name)).max(), 1e-300)  # noqa: E731
    assert np.abs(B.H - A.H).max() / scale("H") < 1e-9
    assert np.abs(B.x - A.x).max() / scale("x") < 1e-9
    lane_of_row = {rid: lane for lane, rid in b["idk"].items()}
    ns_scale, u_scale = max(np.abs(A.Ns).max(), 1e-300), max(np.abs(A.u).max(), 1e-300)
    for slot, rid in a["idk"].items():
        lane = lane_of_row[rid]
        assert np.abs(B.Ns[lane] - A.Ns[slot]).max() / ns_scale < 1e-9
        assert abs(B.u[lane] - A.u[slot]) / u_scale < 1e-9
    for lane in range(NV):
        if lane not in b["idk"]:
            assert not B.Ns[lane].any() and B.u[lane] == 0.0                  # a free lane stays exactly free


@pytest.mark.parametrize("legs", [4, 2])
def test_a_dependent_row_is_left_out_and_leaves_its_lane_free(legs):
    """The third row of leg 1 is a combination of its first two: its pivot is rounding noise, the row stays out in both forms,
    and in the fixed map its lane -- kLegs * 2 + 1 -- stays free while the other legs' third rows take theirs."""
    rng = np.random.default_rng(5 + legs)
    per_leg = [[0, 1, 3], [0, 2, 4]] + [[1, 2, 3], [1, 3, 4]][:legs - 2]
    word = _word(per_leg)
    S0 = State(_spd(rng), rng.normal(size=NV))
    nrm, off = normals_of(rng, legs, dependent=(1, 4, (0, 2))), rng.normal(size=(legs, KINDS))
    A, B = S0.copy(), S0.copy()
    a = rounds_row_by_row(A, word, legs, nrm, off)
    b = rounds_fixed_map(B, word, legs, nrm, off)
    assert A.left_out == [KINDS * 1 + 4]
    assert a["q"] == 3 * legs - 1
    _same_bookkeeping(a, b, word, legs)
    _same_state(A, a, B, b, S0)
    assert not (b["used"] >> slot_lane(2, 1, legs)) & 1
    assert not (b["act_mask"] >> (KINDS * 1 + 4)) & 1
    assert b["used"] == ((1 << (3 * legs)) - 1) & ~(1 << slot_lane(2, 1, legs))


@pytest.mark.parametrize("legs,kv", [(4, 12), (2, 6)])
def test_the_slot_map_stays_below_the_variables(legs, kv):
    lanes = [slot_lane(r, k, legs) for r in range(3) for k in range(legs)]
    assert sorted(lanes) == list(range(kv))          # one lane per (round, leg), every one below kV, none twice
    # and the decode on a slot lane names the row the map puts there, for every set of at most three rows a leg
    for rows0 in range(32):
        if bin(rows0).count("1") > 3:
            continue
        word = sum(rows0 << (KINDS * k) for k in range(legs))
        dec = decode(word, legs)
        for r in range(3):
            for k in range(legs):
                want = None if dec[r][k] is None else KINDS * k + dec[r][k]
                assert slot_row_id(slot_lane(r, k, legs), word, legs) == want

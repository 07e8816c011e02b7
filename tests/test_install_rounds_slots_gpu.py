"""The warm start's install rounds with a fixed slot map and the bookkeeping behind the loop (force_qp_coop.hpp; the arithmetic
and the bookkeeping in numpy: tests/test_install_rounds_slots_cpu.py): the caller's loop on two wavefronts, hand-made first-tick
sets that fill every slot lane, leave gaps in the map or bring a row that is left out, the second attempt behind a first attempt
by rounds, the table kernel, and the working-set words that come out -- which name rows, never slot lanes, so they are what they
were.  Bounds: DESIGN.md 4.1c -- efforts within 1e-7 of the cold start's and 1e-6 of the oracle's, statuses equal."""
import numpy as np
import pytest

from quadruped_locomotion_amd import synth
from test_trajectory_gpu import TAU_TOL, gpu  # noqa: F401  (gpu: the module's fixture)

pytestmark = pytest.mark.gpu
COLD_TOL = 1e-7
B, T = 8, 12
CASES = {"static": "survey", "trot": None}
_cache = {}


def trajectory(oracle, gait):
    """States of the T ticks and the oracle's answers for them: computed once, shared, never written to."""
    if gait not in _cache:
        states = synth.trajectory(B, gait, T, errors=CASES[gait])
        ref = [oracle.balance_batch(s, nthreads=4) for s in states]
        for t0, g0, s0 in ref:
            for a in (t0, g0, s0):
                a.setflags(write=False)
        _cache[gait] = (states, ref)
    return _cache[gait]


def loop(gpu, states, warm, table=False, first_sets=None):
    """The caller's loop of include/qlamd.h through qlamd_balance_solve_placed_batch; per tick (tau, status, working_set)."""
    capi, ctx, torch = gpu
    order = [torch.arange(B, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    iters = [torch.zeros(B, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    ws = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    if first_sets is not None:
        ws = torch.from_numpy(np.asarray(first_sets, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    mem = torch.zeros(B, 4, dtype=torch.int32, device="cuda:0") if table else None
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for k, s in enumerate(states):
        tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        ctx.balance_solve_placed_device(capi.to_device(s), tau, None, status, order=order[k & 1], iterations=iters[k & 1],
                                        prev_iterations=iters[(k - 1) & 1], next_order=order[(k + 1) & 1],
                                        policy=capi.PLACEMENT_AUTO, prev_working_set=ws if warm and not table else None,
                                        working_set=ws if warm else None, set_memory=mem, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(np.sort(order[(k + 1) & 1].cpu().numpy()), np.arange(B)), k
        out.append((tau.cpu().numpy(), status.cpu().numpy(), ws.cpu().numpy().view(np.uint32).copy()))
    return out


def oracle_working_set(oracle, state, i):
    """The word of robot i from the oracle's own final working set: the force problem assembled as oracle_balance_step does
    (ContactForceDistribution's rows: minimum force per support leg, then four friction rows a leg) and solved by its QuadProg++.
    Bit 5 * leg + kind (kind 0 minimum force, 1..4 friction), the support legs in bits 20..23.  Also returns the slacks of all
    twenty rows at the solution (NaN for rows of swing legs)."""
    stance = np.asarray(state["stance"])[i]
    legs = [leg for leg in range(4) if stance[leg]]
    nS = len(legs)
    R = oracle.quat_to_matrix(state["base_quat"][i])
    yB = R.T @ np.array([0.0, 1.0, 0.0])
    nB = R.T @ (R @ np.array([0.0, 0.0, 1.0]))
    t1 = np.cross(nB, yB)
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(nB, t1)
    t2 /= np.linalg.norm(t2)
    r_feet = np.stack([oracle.leg_fk(leg, state["q"][i][3 * leg:3 * leg + 3])[0] for leg in legs])
    step = oracle.balance_step(state, i)
    G, g0, CI, ci0 = oracle.force_qp_assemble(r_feet, step["wrench"], np.tile(nB, nS), np.tile(t1, nS), np.tile(t2, nS))
    res = oracle.solve_quadprog(G, g0, CI=CI, ci0=ci0)
    assert res["status"] == 0 and np.abs(res["x"] - np.concatenate([step["grf"][3 * leg:3 * leg + 3] for leg in legs])).max() < 1e-9
    word = sum(1 << (20 + leg) for leg in legs)
    for a in res["active"]:
        leg, kind = (legs[a], 0) if a < nS else (legs[(a - nS) // 4], (a - nS) % 4 + 1)
        word |= 1 << (5 * leg + kind)
    slack = np.full(20, np.nan)
    sl = CI.T @ res["x"] + ci0
    for a in range(5 * nS):
        leg, kind = (legs[a], 0) if a < nS else (legs[(a - nS) // 4], (a - nS) % 4 + 1)
        slack[5 * leg + kind] = sl[a]
    return word, slack


def check_working_sets(oracle, state, words, what):
    """Every word is the oracle's working set at the solution; where the two differ the vertex is degenerate and named by another
    basis: then they have as many rows, and every row of either is tight at the oracle's solution (forces of order 100 N solved
    to 1e-9: 1e-6 N is tight)."""
    for i, w in enumerate(words):
        want, slack = oracle_working_set(oracle, state, i)
        w = int(w)
        assert w >> 20 == want >> 20, (what, i, hex(w), hex(want))
        if w != want:
            diff = (w ^ want) & 0xFFFFF
            assert bin(w).count("1") == bin(want).count("1"), (what, i, hex(w), hex(want))
            for bit in range(20):
                if (diff >> bit) & 1:
                    assert abs(slack[bit]) < 1e-6, (what, i, hex(w), hex(want), bit, slack[bit])


@pytest.mark.parametrize("gait", sorted(CASES))
def test_the_warm_loop_against_the_oracle_and_the_cold_loop(gpu, oracle, gait):
    """static: four support legs, sets of 6 to 12 rows, every tick but the first by three rounds of the fixed map (asserted below).
    trot: two support legs and sets of one to three rows, which mostly go in row by row, and a wavefront with a robot whose
    support has just changed takes the greedy copy -- this loop checks that the change leaves those paths' answers alone; the
    6-variable form of the fixed map is reached by the hand-made sets of test_hand_made_first_tick_sets (four rows and more on
    two legs)."""
    capi, ctx, torch = gpu
    states, ref = trajectory(oracle, gait)
    retries0 = ctx.counter(capi.COUNTER_WARM_RETRIES)
    cold = loop(gpu, states, warm=False)
    warm = loop(gpu, states, warm=True)
    for k in range(T):
        (tau, status, ws), (tc, sc, _), (t0, _, s0) = warm[k], cold[k], ref[k]
        e_or, e_cold = np.abs(tau - t0).max(), np.abs(tau - tc).max()
        print("%s tick %d: |dtau| oracle %.3e cold %.3e, rows handed on %s" % (gait, k, e_or, e_cold, [bin(int(w) & 0xFFFFF).count("1") for w in ws]))
        assert np.array_equal(status, s0) and np.array_equal(sc, s0) and (s0 == 0).all(), (k, status, sc, s0)
        assert e_or < TAU_TOL, (k, e_or)
        assert e_cold < COLD_TOL, (k, e_cold)
        check_working_sets(oracle, states[k], ws, "%s tick %d" % (gait, k))
    assert ctx.counter(capi.COUNTER_WARM_RETRIES) == retries0
    if gait == "static":   # the loop did go by rounds: sets of six rows and more were handed on
        assert max(bin(int(w) & 0xFFFFF).count("1") for _, _, ws in warm[:-1] for w in ws) >= 6


def _hand_made(gait, stance):
    """First-tick sets, one list of eight words each; rows only on support legs, bits 20..23 = the support legs."""
    rng = np.random.default_rng(17)
    support = [[leg for leg in range(4) if st[leg]] for st in stance]
    triples = [m for m in range(32) if bin(m).count("1") == 3]

    def words(rows_of):
        out = []
        for i, legs in enumerate(support):
            w = sum(1 << (20 + leg) for leg in legs)
            for j, leg in enumerate(legs):
                w |= int(rows_of(i, j)) << (5 * leg)
            out.append(w)
        return np.array(out, dtype=np.uint32)

    gaps = [(0b01011, 0b00010, 0b00000, 0b10100), (0b00000, 0b01101, 0b00001, 0b11000), (0b00100, 0b00000, 0b10011, 0b00110),
            (0b11001, 0b10001, 0b01000, 0b00000)]
    sets = {
        "full": words(lambda i, j: 0b01011),                              # f_min, +t1, +t2 of every leg: every slot lane
        "gaps": words(lambda i, j: gaps[i % 4][(j + i // 4) % 4] if gait == "static" else (0b01011, 0b00000, 0b10100, 0b00010)[(i + j) % 4]),
        # n, mu n + t1, mu n - t1: the third is a combination of the first two and is left out in the last round
        "dependent": words(lambda i, j: 0b00111),
        "junk": words(lambda i, j: rng.choice(triples)),
        "junk2": words(lambda i, j: 0b11100 if (i + j) & 1 else 0b10101),
    }
    return sets


@pytest.mark.parametrize("gait", sorted(CASES))
def test_hand_made_first_tick_sets(gpu, oracle, gait):
    capi, ctx, torch = gpu
    states, ref = trajectory(oracle, gait)
    t0, _, s0 = ref[0]
    ctx.set_option(capi.OPT_WARM_FALLBACK, 1)
    for name, words in _hand_made(gait, np.asarray(states[0]["stance"])).items():
        retries0 = ctx.counter(capi.COUNTER_WARM_RETRIES)
        (tau, status, ws), = loop(gpu, states[:1], warm=True, first_sets=words)
        err = np.abs(tau - t0).max()
        print("%s %s: sets in %s, max |dtau| %.3e, retried %d, sets out %s" % (
            gait, name, [hex(int(w)) for w in words], err, ctx.counter(capi.COUNTER_WARM_RETRIES) - retries0, [hex(int(w)) for w in ws]))
        assert np.array_equal(status, s0) and (status == 0).all(), (name, status)
        assert err < TAU_TOL, (name, err)
        if not name.startswith("junk"):
            assert ctx.counter(capi.COUNTER_WARM_RETRIES) == retries0, name
        retried = ws == 0                                                 # (a robot solved again hands on the empty set)
        check_working_sets(oracle, states[0], [w if not r else oracle_working_set(oracle, states[0], i)[0]
                                               for i, (w, r) in enumerate(zip(ws, retried))], "%s %s" % (gait, name))
        if name == "dependent":   # all three cannot be independent: at most two of them in a final set
            for w in ws:
                for leg in range(4):
                    assert bin((int(w) >> (5 * leg)) & 0b00111).count("1") <= 2, hex(int(w))


def test_the_second_attempt_behind_a_first_attempt_by_rounds(gpu, oracle):
    """QLAMD_OPT_WARM_FALLBACK 2: every robot that ends its warm-started solve with a set is solved again from the empty one by
    the same launch -- here behind three rounds of the block form."""
    capi, ctx, torch = gpu
    states, ref = trajectory(oracle, "static")
    sets = loop(gpu, states[:1], warm=True)[0][2]
    assert max(bin(int(w) & 0xFFFFF).count("1") for w in sets) >= 6
    t0, _, s0 = ref[1]
    before = ctx.counter(capi.COUNTER_WARM_RETRIES)
    ctx.set_option(capi.OPT_WARM_FALLBACK, 2)
    try:
        (tau, status, ws), = loop(gpu, states[1:2], warm=True, first_sets=sets)
    finally:
        ctx.set_option(capi.OPT_WARM_FALLBACK, 1)
    assert ctx.counter(capi.COUNTER_WARM_RETRIES) - before == B and (ws == 0).all()
    assert np.array_equal(status, s0) and np.abs(tau - t0).max() < TAU_TOL


def test_the_table_kernel(gpu, oracle):
    """qlamd_placement::set_memory: the same rounds inside balance_table_kernel."""
    capi, ctx, torch = gpu
    states, ref = trajectory(oracle, "static")
    retries0 = ctx.counter(capi.COUNTER_WARM_RETRIES)
    one_word = loop(gpu, states, warm=True)
    table = loop(gpu, states, warm=True, table=True)
    for k in range(T):
        (tau, status, ws), (t0, _, s0) = table[k], ref[k]
        assert np.array_equal(status, s0) and np.abs(tau - t0).max() < TAU_TOL, k
        check_working_sets(oracle, states[k], ws, "table tick %d" % k)
        # four support legs throughout: one slot of the table in use, the loop is the one-word loop's
        assert np.abs(tau - one_word[k][0]).max() < COLD_TOL and np.array_equal(ws, one_word[k][2]), k
    assert ctx.counter(capi.COUNTER_WARM_RETRIES) == retries0

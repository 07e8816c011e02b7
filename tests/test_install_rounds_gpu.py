"""The warm start's install rounds in their block form (force_qp_coop.hpp: Gram block of the round's rows, its LDL' on every
lane, corrected directions in place, one stream of rank-one updates): the caller's loop on small batches -- two wavefronts, so
that a round sees legs with and without a row and ghost legs -- in the 12-variable and the 6-variable form, and working sets whose
rows depend on one another or have nothing to do with the robot.  Efforts against the oracle within the north star's 1e-6."""
import numpy as np
import pytest

from quadruped_locomotion_amd import synth
from test_trajectory_gpu import TAU_TOL, gpu, run_loop  # noqa: F401  (gpu: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gait,errors", [("static", "survey"), ("trot", None)])
def test_the_warm_loop_on_two_wavefronts(gpu, oracle, gait, errors):
    """static: four support legs, the 12-variable form, sets of 6 to 12 rows installed by rounds; trot: two support legs, the
    6-variable form.  Every tick: every status OK, efforts within 1e-6 of the oracle's, no warm start rejected."""
    capi, ctx, torch = gpu
    B, T = 8, 6
    states = synth.trajectory(B, gait, T, errors=errors)
    retries0 = ctx.counter(capi.COUNTER_WARM_RETRIES)
    worst = [0.0]

    def check(k, tau, status):
        t0, _, s0 = oracle.balance_batch(states[k], nthreads=4)
        assert (s0 == 0).all() and (status == 0).all(), (k, status, s0)
        err = np.abs(tau - t0).max()
        worst[0] = max(worst[0], err)
        print("%s tick %d: max |dtau| %.3e" % (gait, k, err))
        assert err < TAU_TOL, (k, err)
        assert ctx.counter(capi.COUNTER_WARM_RETRIES) == retries0, k

    stats = run_loop(gpu, states, warm=True, check=check)
    # the loop did run warm: from the second tick on the sets handed in are the sets that come out, for most robots
    assert np.mean([st["unchanged"] for st in stats[2:]]) > 0.5
    print("%s B=%d T=%d: worst |dtau| %.3e" % (gait, B, T, worst[0]))


def _solve_with_sets(gpu, d, B, words):
    capi, ctx, torch = gpu
    tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    ws = torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    ctx.balance_solve_placed_device(d, tau, None, status, prev_working_set=ws, working_set=ws,
                                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tau.cpu().numpy(), status.cpu().numpy(), ws.cpu().numpy().view(np.uint32)


def test_a_row_that_depends_on_the_installed_ones_is_left_out(gpu, oracle):
    """A set that claims the rows f_min, +t1 and -t1 of every leg: their normals are n, mu n + t1 and mu n - t1, so the third is
    a combination of the first two.  Three rounds of four rows; the third round's pivots are rounding noise and its rows are left
    out.  Every status OK, efforts within 1e-6, nothing rejected."""
    capi, ctx, torch = gpu
    B = 4
    s = synth.make_states(B, "static", errors="survey")
    t0, _, s0 = oracle.balance_batch(s, nthreads=4)
    assert (s0 == 0).all()
    word = sum(0b00111 << (5 * leg) for leg in range(4))
    before = ctx.counter(capi.COUNTER_WARM_RETRIES)
    tau, status, ws = _solve_with_sets(gpu, capi.to_device(s), B, np.full(B, word, dtype=np.uint32))
    err = np.abs(tau - t0).max()
    print("dependent rows: max |dtau| %.3e, final sets %s" % (err, [bin(int(w) & 0xFFFFF) for w in ws]))
    assert (status == 0).all(), status
    assert err < TAU_TOL, err
    assert ctx.counter(capi.COUNTER_WARM_RETRIES) == before
    # a final set holds at most two of the three rows: all three cannot be independent
    for w in ws:
        for leg in range(4):
            assert bin((int(w) >> (5 * leg)) & 0b00111).count("1") <= 2, bin(int(w))


def test_junk_sets_of_three_rows_a_leg(gpu, oracle):
    """Sets that have nothing to do with the robots' states, three rows on every leg (twelve rows: three full rounds): with the
    second attempt on (the default) every status is OK and every effort within 1e-6 of the oracle's."""
    capi, ctx, torch = gpu
    B = 4
    s = synth.make_states(B, "static", errors="survey")
    d = capi.to_device(s)
    t0, _, s0 = oracle.balance_batch(s, nthreads=4)
    assert (s0 == 0).all()
    rng = np.random.default_rng(11)
    triples = [m for m in range(32) if bin(m).count("1") == 3]
    sets = [np.full(B, 0b01011_10101_01110_10011, dtype=np.uint32)]
    for _ in range(3):
        pick = rng.choice(triples, size=(B, 4))
        sets.append(sum(pick[:, leg].astype(np.uint32) << np.uint32(5 * leg) for leg in range(4)).astype(np.uint32))
    ctx.set_option(capi.OPT_WARM_FALLBACK, 1)
    for words in sets:
        tau, status, _ = _solve_with_sets(gpu, d, B, words)
        err = np.abs(tau - t0).max()
        print("junk sets %s: max |dtau| %.3e" % ([hex(int(w)) for w in words], err))
        assert (status == 0).all(), status
        assert err < TAU_TOL, err

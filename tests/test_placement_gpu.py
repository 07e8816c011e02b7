"""Placement of robots into wavefronts (qlamd_balance_solve_placed_batch, qlamd_force_distribution_placed_batch,
qlamd_placement_from_iterations): whatever the placement, every robot gets bit for bit the result of the plain entry --
what is checked against the oracle elsewhere (tests/test_balance_gpu.py) therefore holds for every placement -- and the
iteration counts are those of the reference's method (QuadProg++.cc:216-445, restated in oracle/oracle_quadprog.c)."""
import ctypes as C

import numpy as np
import pytest

from quadruped_locomotion_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from quadruped_locomotion_amd import capi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    ctx = capi.Context(device=0)
    yield capi, ctx, torch
    ctx.close()


def plain(gpu, d, B, normals=False):
    capi, ctx, torch = gpu
    tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
    grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    ctx.balance_solve_device(d, tau, grf, status, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tau.cpu().numpy(), grf.cpu().numpy(), status.cpu().numpy()


def placed(gpu, d, B, order, fill=np.nan):
    capi, ctx, torch = gpu
    tau = torch.full((B, 12), fill, dtype=torch.float64, device="cuda:0")
    grf = torch.full((B, 12), fill, dtype=torch.float64, device="cuda:0")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    iters = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    o = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to("cuda:0")
    ctx.balance_solve_placed_device(d, tau, grf, status, order=o, iterations=iters,
                                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tau.cpu().numpy(), grf.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()


def reference_placement(iters, throughput, support=None):
    """The documented placement (include/qlamd.h), restated: stable sort by iteration count (clipped to 23), hardest first;
    `support` ([B][4], sorted placement by launches of their own only): robots on more than two legs before the others."""
    B = len(iters)
    key = -np.clip(iters, 0, 23)
    if support is not None and throughput:
        key = key + 24 * (np.asarray(support).astype(bool).sum(1) <= 2)
    rank_to_robot = np.argsort(key, kind="stable")
    if throughput:
        return rank_to_robot.astype(np.int32)
    W = (B + 3) // 4
    order = np.full(B, -1, dtype=np.int32)
    for r, robot in enumerate(rank_to_robot):
        e = B - 1 - r
        order[4 * r if r < W else 4 * (e // 3) + 1 + e % 3] = robot
    return order


@pytest.mark.parametrize("gait,errors,B", [("static", "survey", 4096), ("trot", None, 4099), ("trot", None, 16385), ("static", "calm", 7)])
def test_results_are_bit_equal_under_any_placement(gpu, oracle, gait, errors, B):
    """Identity, a random permutation, the reversed order and both placements of the library, at batch sizes that leave
    the last wavefront ragged and on both forms of the kernel (two / three wavefronts per SIMD from 16 384 robots).
    (Also the test of the ghost rows, ADVICE r4: a robot that has finished rides along while the other rows of its wavefront
    run on -- for one pass next to easy companions, for twenty next to a hard one; if its operators were touched after it
    latched, its refinement, and so its result, would depend on who it sits with.)"""
    capi, ctx, torch = gpu
    s = synth.make_states(B, gait, errors=errors)
    d = capi.to_device(s)
    t0, g0, s0 = plain(gpu, d, B)
    assert (s0 == 0).all()
    rng = np.random.default_rng(5)
    t1, g1, s1, it1 = placed(gpu, d, B, None)
    assert np.array_equal(t1, t0) and np.array_equal(g1, g0) and np.array_equal(s1, s0)
    assert (it1 >= 0).all() and it1.max() <= 41
    # the reference's own count (the restated QuadProg++): equal wherever no tie in the pivot rule is broken differently
    n_check = min(B, 512)
    it_ref = np.array([oracle.balance_step(s, i)["iters"] for i in range(n_check)])
    has_qp = s["stance"][:n_check].any(axis=1)
    assert (it1[:n_check][~has_qp] == 0).all()
    # (rows whose slacks agree to 18 bits enter in lane order here: another path to the same minimiser, a few passes apart)
    assert (it1[:n_check][has_qp] == it_ref[has_qp]).mean() > 0.9
    assert np.abs(it1[:n_check] - it_ref).max() <= 6
    orders = [rng.permutation(B), np.arange(B)[::-1].copy()]
    for policy in (capi.PLACEMENT_LATENCY, capi.PLACEMENT_THROUGHPUT, capi.PLACEMENT_AUTO):
        orders.append(ctx.placement_from_iterations(it1, policy=policy))
    for order in orders:
        assert sorted(order.tolist()) == list(range(B))
        t, g, st, it = placed(gpu, d, B, order)
        assert np.array_equal(t, t0) and np.array_equal(g, g0) and np.array_equal(st, s0) and np.array_equal(it, it1)


def test_placement_kernel_matches_the_documented_rule(gpu):
    """Host and device memory, both policies, ragged sizes, counts beyond the 23 the sort distinguishes, negative counts."""
    capi, ctx, torch = gpu
    rng = np.random.default_rng(11)
    for B in (1, 2, 3, 5, 64, 255, 256, 257, 4096, 4099, 65536 + 3):
        it = rng.integers(-2, 45, size=B).astype(np.int32)
        for policy, thr in ((capi.PLACEMENT_LATENCY, False), (capi.PLACEMENT_THROUGHPUT, True)):
            want = reference_placement(np.maximum(it, 0), thr)
            got_h = ctx.placement_from_iterations(it, policy=policy)
            assert np.array_equal(got_h, want), (B, policy)
            d_it = torch.from_numpy(it).to("cuda:0")
            d_or = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            ctx.placement_from_iterations(d_it, order=d_or, policy=policy, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_or.cpu().numpy(), want), (B, policy)
        auto = ctx.placement_from_iterations(it, policy=capi.PLACEMENT_AUTO)
        assert np.array_equal(auto, reference_placement(np.maximum(it, 0), B >= 16384))


def test_latency_placement_puts_the_hardest_robots_next_to_the_easiest(gpu):
    """What the placement is for: the hardest quarter one per wavefront, the three easiest robots in wavefront 0."""
    capi, ctx, torch = gpu
    s = synth.make_states(4096, "static", errors="survey")
    d = capi.to_device(s)
    _, _, _, it = placed(gpu, d, 4096, None)
    order = ctx.placement_from_iterations(it, policy=capi.PLACEMENT_LATENCY)
    hard = it[order[0::4]]
    assert (np.diff(hard) <= 0).all() and hard[0] == it.max()
    assert it[order[1:4]].max() == np.sort(it)[2]
    assert hard.min() >= np.sort(it)[::-1][1023]


def test_host_memory_order_is_validated_and_device_order_cannot_corrupt(gpu):
    capi, ctx, torch = gpu
    B = 64
    s = synth.make_states(B, "trot")
    tau, grf, st, it = ctx.balance_solve_placed_host(s, order=np.arange(B)[::-1])
    t0, g0, s0 = ctx.balance_solve_host(s)
    assert np.array_equal(tau, t0) and np.array_equal(grf, g0) and np.array_equal(st, s0) and (it >= 0).all()
    for bad in (np.zeros(B), np.r_[np.arange(B - 1), B], np.r_[np.arange(B - 1), -1]):
        with pytest.raises(capi.QlamdError) as e:
            ctx.balance_solve_placed_host(s, order=bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    # device memory is not checked: an entry outside [0, B) leaves its slot empty and the robot it displaced untouched
    d = capi.to_device(s)
    order = np.arange(B, dtype=np.int32)
    order[5], order[17] = -3, B + 100
    t, g, stt, itt = placed(gpu, d, B, order, fill=7.0)
    for i in (5, 17):
        assert (t[i] == 7.0).all() and (g[i] == 7.0).all() and stt[i] == -1 and itt[i] == -1
    keep = np.setdiff1d(np.arange(B), [5, 17])
    assert np.array_equal(t[keep], t0[keep]) and np.array_equal(stt[keep], s0[keep])


def test_one_lane_kernels_refuse_a_placement(gpu):
    capi, ctx, torch = gpu
    s = synth.make_states(64, "trot")
    ctx.set_robots_per_wave(16)
    try:
        with pytest.raises(capi.QlamdError) as e:
            ctx.balance_solve_placed_host(s, order=np.arange(64))
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    finally:
        ctx.set_robots_per_wave(0)


def test_force_distribution_placed_equals_the_plain_entry(gpu):
    capi, ctx, torch = gpu
    B = 1027
    s = synth.make_states(B, "trot")
    d = capi.to_device(s)
    w = torch.zeros(B, 6, dtype=torch.float64, device="cuda:0")
    ctx.virtual_wrench_device(d, w, stream=torch.cuda.current_stream().cuda_stream)
    out = {}
    for name in ("plain", "placed"):
        tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        st = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        it = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        order = torch.from_numpy(np.random.default_rng(3).permutation(B).astype(np.int32)).to("cuda:0")
        args = [ctx._h, d["q"].data_ptr(), d["base_quat"].data_ptr(), d["stance"].data_ptr(), None, w.data_ptr(), B]
        if name == "plain":
            rc = capi.lib().qlamd_force_distribution_batch(*args, tau.data_ptr(), grf.data_ptr(), st.data_ptr(), capi.MEM_DEVICE, None)
        else:
            pl = capi.Placement(order.data_ptr(), it.data_ptr(), None, None, 0)
            rc = capi.lib().qlamd_force_distribution_placed_batch(*args, C.byref(pl), tau.data_ptr(), grf.data_ptr(),
                                                                  st.data_ptr(), capi.MEM_DEVICE, None)
        assert rc == 0
        torch.cuda.synchronize()
        out[name] = (tau.cpu().numpy(), grf.cpu().numpy(), st.cpu().numpy())
    for a, b in zip(out["plain"], out["placed"]):
        assert np.array_equal(a, b)
    assert (it.cpu().numpy() >= 0).all()


@pytest.mark.parametrize("B", [4096, 4099, 8192, 8704, 8705, 16383, 16385, 70, 65536, 262145, 1048577])
def test_next_placement_made_inside_the_solve_equals_the_placement_entry(gpu, B):
    """prev_iterations -> next_robot_order: by extra wavefronts of the solve's own launch (one per 1024 robots, per 4096 from 16 384 robots up, up to
    1 M robots: several of them meet at a barrier in global memory), by launches of their own beyond -- the documented placement
    either way, the same from launch to launch (the barrier resets itself), and the solve's results untouched."""
    capi, ctx, torch = gpu
    s = synth.make_states(B, "trot")
    d = capi.to_device(s)
    t0, g0, s0 = plain(gpu, d, B)
    rng = np.random.default_rng(B)
    prev = rng.integers(0, 30, size=B).astype(np.int32)
    d_prev = torch.from_numpy(prev).to("cuda:0")
    for policy in (capi.PLACEMENT_LATENCY, capi.PLACEMENT_THROUGHPUT, capi.PLACEMENT_AUTO):
        # the entry on its own knows the counts only; the placed solve also knows who stands on how many legs, and a sorted
        # placement made there sorts by class first (robots on at most two legs last)
        thr = policy == capi.PLACEMENT_THROUGHPUT or (policy == capi.PLACEMENT_AUTO and B >= 16384)
        assert np.array_equal(ctx.placement_from_iterations(prev, policy=policy), reference_placement(prev, thr))
        want = reference_placement(prev, thr, support=s["stance"])
        tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        iters = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        nxt = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to("cuda:0")
        ctx.balance_solve_placed_device(d, tau, grf, status, order=order, iterations=iters, prev_iterations=d_prev,
                                        next_order=nxt, policy=policy, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(nxt.cpu().numpy(), want), policy
        assert np.array_equal(tau.cpu().numpy(), t0) and np.array_equal(grf.cpu().numpy(), g0)
        assert np.array_equal(status.cpu().numpy(), s0) and (iters.cpu().numpy() >= 0).all()
    # host memory: the same through the staged path; one of the pair alone, or aliased buffers, are refused
    if B <= 4099:
        out = ctx.balance_solve_placed_host(s, prev_iterations=prev, policy=capi.PLACEMENT_LATENCY)
        assert np.array_equal(out[4], ctx.placement_from_iterations(prev, policy=capi.PLACEMENT_LATENCY))
        assert np.array_equal(out[0], t0)
        pl = capi.Placement(None, None, d_prev.data_ptr(), None, 0)
        sb, _, _ = capi._state_batch(d, None, capi.MEM_DEVICE)
        tau = torch.zeros(B, 12, dtype=torch.float64, device="cuda:0")
        status = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        rc = capi.lib().qlamd_balance_solve_placed_batch(ctx._h, C.byref(sb), B, C.byref(pl), tau.data_ptr(), None, status.data_ptr(),
                                                         capi.MEM_DEVICE, None)
        assert rc == capi.ERR_INVALID_ARGUMENT
        pl = capi.Placement(None, d_prev.data_ptr(), d_prev.data_ptr(), status.data_ptr(), 0)
        rc = capi.lib().qlamd_balance_solve_placed_batch(ctx._h, C.byref(sb), B, C.byref(pl), tau.data_ptr(), None, status.data_ptr(),
                                                         capi.MEM_DEVICE, None)
        assert rc == capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("B", [8192, 65536])
def test_shadow_wavefronts_that_give_up_leave_the_identity_order(gpu, B):
    """QLAMD_OPT_PLACEMENT_WAIT = 0: the wavefronts that make the next placement do not wait for each other at all, so all but
    the last to arrive give up -- the launch has ONE outcome (a compare-and-swap on the barrier's state): every wavefront
    writes the identity order, a valid placement; the solve's results are untouched, and the launches after it (waiting
    again) make the documented placement: the barrier is left in order."""
    capi, ctx2, torch = gpu
    ctx = capi.Context(device=0)
    try:
        s = synth.make_states(B, "trot")
        d = capi.to_device(s)
        t0, g0, s0 = plain((capi, ctx, torch), d, B)
        rng = np.random.default_rng(B + 1)
        prev = rng.integers(0, 30, size=B).astype(np.int32)
        d_prev = torch.from_numpy(prev).to("cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def launch():
            tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
            status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            iters = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            nxt = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            ctx.balance_solve_placed_device(d, tau, None, status, iterations=iters, prev_iterations=d_prev, next_order=nxt,
                                            policy=capi.PLACEMENT_LATENCY, stream=stream)
            torch.cuda.synchronize()
            assert np.array_equal(tau.cpu().numpy(), t0) and np.array_equal(status.cpu().numpy(), s0)
            return nxt.cpu().numpy()

        want = reference_placement(prev, False)
        assert np.array_equal(launch(), want)
        ctx.set_option(capi.OPT_PLACEMENT_WAIT, 0)
        for _ in range(3):
            got = launch()
            # (with luck every wavefront arrives before the first one polls twice: then the placement is simply made)
            assert np.array_equal(got, np.arange(B, dtype=np.int32)) or np.array_equal(got, want)
        ctx.set_option(capi.OPT_PLACEMENT_WAIT, 1 << 24)
        for _ in range(3):
            assert np.array_equal(launch(), want)
        with pytest.raises(capi.QlamdError):
            ctx.set_option(capi.OPT_PLACEMENT_WAIT, -1)
    finally:
        ctx.close()


def _force_qps(torch, B):
    """The golden force QPs (n = 12, m = 20) tiled to B problems, on the device, in both forms the library takes."""
    import os
    from conftest import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "qp_goldens.npz"))
    reps = B // 128
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))  # noqa: E731
    dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    qp = tuple(dev(tile(g["n12_" + k])) for k in ("G", "g0", "CI", "ci0"))
    lam, V = np.linalg.eigh(g["n12_G"] - 1e-4 * np.eye(12))
    A = np.sqrt(np.clip(lam, 0.0, None))[:, :, None] * np.transpose(V, (0, 2, 1))
    b = np.stack([-np.linalg.lstsq(A[i].T, g["n12_g0"][i], rcond=None)[0] for i in range(128)])
    D, d = np.transpose(g["n12_CI"], (0, 2, 1)), -g["n12_ci0"]
    lsq = tuple(dev(tile(a)) for a in (A, np.ones((128, 12)), b, np.full((128, 12), 1e-4), D, d, np.full(d.shape, 1.7976931348623157e308)))
    return qp, lsq


def test_place_next_call_on_the_other_qp_entries(gpu):
    """qlamd_place_next_call: the dense QP batch, the weighted least-squares entry and the whole-body step take a placement
    through the context -- same results bit for bit under any placement, iteration counts out, the placement for the next
    call made behind the solve, and a pending placement is used exactly once."""
    capi, ctx, torch = gpu
    B = 1024
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    (G, g0, CI, ci0), (A, S, b, W, D, d, f) = _force_qps(torch, B)
    wb = capi.to_device(synth.make_wholebody_states(B, "trot"))
    i32 = lambda fill: torch.full((B,), fill, dtype=torch.int32, device="cuda:0")  # noqa: E731

    def qp():
        x, obj, st = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.float64, device="cuda:0"), i32(-1)
        rc = L.qlamd_qp_solve_batch(ctx._h, 12, 0, 20, G.data_ptr(), g0.data_ptr(), None, None, CI.data_ptr(), ci0.data_ptr(), B,
                                    x.data_ptr(), obj.data_ptr(), st.data_ptr(), capi.MEM_DEVICE, C.c_void_p(stream))
        assert rc == 0
        return x, obj, st

    def lsq():
        x, st = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0"), i32(-1)
        capi.weighted_lsq_qp(ctx, A, S, b, W, None, None, D, d, f, memory=capi.MEM_DEVICE, out=(x, st), stream=stream)
        return x, st

    def whole():
        tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        st = i32(-1)
        capi.wholebody_solve_device(ctx, wb, tau, grf, st, stream=stream)
        return tau, grf, st

    rng = np.random.default_rng(2)
    for entry in (qp, lsq, whole):
        ref = [t.cpu().numpy() for t in (entry(), torch.cuda.synchronize())[0]]
        it = i32(-1)
        ctx.place_next_call(iterations=it)
        got = [t.cpu().numpy() for t in (entry(), torch.cuda.synchronize())[0]]
        for a, r in zip(got, ref):
            assert np.array_equal(a, r, equal_nan=True)
        itn = it.cpu().numpy()
        assert (itn >= 0).all() and itn.max() > 2
        # used once: the next call runs unplaced and writes no counts
        it.fill_(-7)
        _ = entry()
        torch.cuda.synchronize()
        assert (it.cpu().numpy() == -7).all()
        it.copy_(torch.from_numpy(itn))
        for order in (rng.permutation(B).astype(np.int32), ctx.placement_from_iterations(itn, policy=capi.PLACEMENT_LATENCY)):
            o = torch.from_numpy(order).to("cuda:0")
            it3, nxt = i32(-1), i32(-1)
            ctx.place_next_call(order=o, iterations=it3, prev_iterations=it, next_order=nxt, policy=capi.PLACEMENT_THROUGHPUT)
            got = [t.cpu().numpy() for t in (entry(), torch.cuda.synchronize())[0]]
            for a, r in zip(got, ref):
                assert np.array_equal(a, r, equal_nan=True)
            assert np.array_equal(it3.cpu().numpy(), itn)
            assert np.array_equal(nxt.cpu().numpy(), ctx.placement_from_iterations(itn, policy=capi.PLACEMENT_THROUGHPUT))
    # a host-memory call that finds a placement pending refuses and clears it; NULL withdraws one
    ctx.place_next_call(iterations=i32(-1))
    with pytest.raises(capi.QlamdError) as e:
        capi.wholebody_solve(ctx, synth.make_wholebody_states(8, "trot"))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    capi.wholebody_solve(ctx, synth.make_wholebody_states(8, "trot"))
    it4 = i32(-7)
    ctx.place_next_call(iterations=it4)
    ctx.place_next_call()
    _ = whole()
    torch.cuda.synchronize()
    assert (it4.cpu().numpy() == -7).all()


def test_records_instead_of_per_field_arrays(gpu):
    """QLAMD_OPT_STATE_LAYOUT = QLAMD_STATE_RECORDS: the nine double fields of a robot in one 48-double record (every field pointer
    of qlamd_state_batch into the same array of records): the same arithmetic on the same numbers -- efforts, forces, statuses,
    iteration counts and working sets bit for bit those of the per-field arrays, plain, placed and warm-started, in the latency
    and the throughput form; refused for the one-lane kernels and the force-distribution entries."""
    capi, ctx, torch = gpu
    stream = torch.cuda.current_stream().cuda_stream
    for B, gait in ((4099, "static"), (4096, "trot"), (24001, "trot")):
        s = synth.make_states(B, gait, errors="survey" if gait == "static" else None)
        df, dr = capi.to_device(s), capi.to_device_records(s)
        rng = np.random.default_rng(B)
        order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to("cuda:0")
        out = {}
        for layout, d in ((capi.STATE_FIELDS, df), (capi.STATE_RECORDS, dr)):
            ctx.set_option(capi.OPT_STATE_LAYOUT, layout)
            try:
                res = []
                tau, grf = torch.zeros(B, 12, dtype=torch.float64, device="cuda:0"), torch.zeros(B, 12, dtype=torch.float64, device="cuda:0")
                st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
                ctx.balance_solve_device(d, tau, grf, st, stream=stream)
                torch.cuda.synchronize()
                res += [tau.clone(), grf.clone(), st.clone()]
                it, ws = torch.zeros(B, dtype=torch.int32, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
                for _ in range(2):   # cold through the warm kernel, then from its own sets, in a random placement
                    ctx.balance_solve_placed_device(d, tau, grf, st, order=order, iterations=it, prev_working_set=ws, working_set=ws, stream=stream)
                torch.cuda.synchronize()
                res += [tau.clone(), grf.clone(), st.clone(), it.clone(), ws.clone()]
                out[layout] = res
            finally:
                ctx.set_option(capi.OPT_STATE_LAYOUT, capi.STATE_FIELDS)
        for a, b in zip(out[capi.STATE_FIELDS], out[capi.STATE_RECORDS]):
            assert torch.equal(a, b), (B, gait)
        assert (out[capi.STATE_RECORDS][2] == 0).all()
    ctx.set_option(capi.OPT_STATE_LAYOUT, capi.STATE_RECORDS)
    try:
        ctx.set_robots_per_wave(64)
        with pytest.raises(capi.QlamdError):
            ctx.balance_solve_device(dr, tau, grf, st, stream=stream)
        ctx.set_robots_per_wave(0)
        w = torch.zeros(B, 6, dtype=torch.float64, device="cuda:0")
        rc = capi.lib().qlamd_force_distribution_batch(ctx._h, dr["q"].data_ptr(), dr["base_quat"].data_ptr(), dr["stance"].data_ptr(), None,
                                                       w.data_ptr(), B, tau.data_ptr(), grf.data_ptr(), st.data_ptr(), capi.MEM_DEVICE, None)
        assert rc == capi.ERR_INVALID_ARGUMENT
    finally:
        ctx.set_robots_per_wave(0)
        ctx.set_option(capi.OPT_STATE_LAYOUT, capi.STATE_FIELDS)


def test_no_placement_and_what_auto_means_with_a_warm_start(gpu):
    """QLAMD_PLACEMENT_NONE leaves the identity in next_robot_order (written by the solving launch itself, or by
    qlamd_placement_from_iterations).  QLAMD_PLACEMENT_AUTO with a warm start: no placement up to 4096 robots, the throughput
    policy above (include/qlamd.h); without one: latency below 16 384 robots as before.  Results do not depend on any of it."""
    capi, ctx, torch = gpu
    dev = "cuda:0"
    for B in (4096, 6144, 20000):   # (20 000 without a warm start: the 168-register form, whose identity order is a launch of its own)
        s = synth.make_states(B, "trot")
        d = capi.to_device(s)
        ident = np.arange(B, dtype=np.int32)
        prev = torch.from_numpy(np.random.default_rng(B).integers(1, 20, B).astype(np.int32)).to(dev)
        out = {}
        for name, policy, warm in (("none", capi.PLACEMENT_NONE, False), ("auto cold", capi.PLACEMENT_AUTO, False),
                                   ("auto warm", capi.PLACEMENT_AUTO, True), ("throughput warm", capi.PLACEMENT_THROUGHPUT, True)):
            tau = torch.zeros(B, 12, dtype=torch.float64, device=dev)
            st = torch.full((B,), -1, dtype=torch.int32, device=dev)
            it = torch.zeros(B, dtype=torch.int32, device=dev)
            nxt = torch.full((B,), -7, dtype=torch.int32, device=dev)
            ws = torch.zeros(B, dtype=torch.int32, device=dev) if warm else None
            ctx.balance_solve_placed_device(d, tau, None, st, iterations=it, prev_iterations=prev, next_order=nxt, policy=policy,
                                            prev_working_set=ws, working_set=ws)
            torch.cuda.synchronize()
            assert (st.cpu().numpy() == 0).all()
            out[name] = (tau.cpu().numpy(), nxt.cpu().numpy())
            assert sorted(out[name][1].tolist()) == ident.tolist(), name               # always a permutation
        assert np.array_equal(out["none"][1], ident)
        assert not np.array_equal(out["auto cold"][1], ident)                         # the latency policy, from the counts
        if B <= 4096:
            assert np.array_equal(out["auto warm"][1], ident)
        else:
            assert np.array_equal(out["auto warm"][1], out["throughput warm"][1]) and not np.array_equal(out["auto warm"][1], ident)
        assert np.abs(out["none"][0] - out["auto cold"][0]).max() == 0.0              # the cold kernels: bit for bit
        assert np.abs(out["auto warm"][0] - out["none"][0]).max() < 1e-7
        # the placement entry on its own
        o = torch.full((B,), -7, dtype=torch.int32, device=dev)
        rc = capi.lib().qlamd_placement_from_iterations(ctx._h, prev.data_ptr(), B, capi.PLACEMENT_NONE, o.data_ptr(), capi.MEM_DEVICE, None)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(o.cpu().numpy(), ident)
        ho = np.full(B, -7, np.int32)
        hp = prev.cpu().numpy()
        rc = capi.lib().qlamd_placement_from_iterations(ctx._h, hp.ctypes.data, B, capi.PLACEMENT_NONE, ho.ctypes.data, capi.MEM_HOST, None)
        assert rc == 0 and np.array_equal(ho, ident)

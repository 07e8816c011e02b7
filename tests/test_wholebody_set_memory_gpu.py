"""qlamd_wholebody_solve_placed_batch: the whole-body step with its placement as an argument and with a working set per support
set -- [B][4] 64-bit words -- on synth.wholebody_trajectory.  The [B][2] one-set loop through qlamd_place_next_call, which this
entry leaves alone, is the yardstick for what the table buys; the oracle's whole-body step is the yardstick for every answer."""
import ctypes as C

import numpy as np
import pytest

from quadruped_locomotion_amd import synth

pytestmark = pytest.mark.gpu
TAU_TOL = 1e-6       # the north star: efforts within 1e-6 of the oracle
WARM_TOL = 1e-7      # include/qlamd.h: any warm start agrees with the same entry's cold start to 1e-7
ROWS = np.uint64((1 << 44) - 1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from quadruped_locomotion_amd import capi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    ctx = capi.Context(device=0)
    yield capi, ctx, torch
    ctx.close()


def support_mask(stance):
    return ((np.asarray(stance) != 0).astype(np.int64) * np.array([1, 2, 4, 8])).sum(1)


def slots_of(capi, stance):
    return np.array([capi.set_memory_slot(m) for m in range(16)])[support_mask(stance)]


def legs_of(words):
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(44)) & np.uint64(0xF)).astype(np.int64)


def aligned_table(torch, B, fill=None):
    """int64 [B, 4] on a 32-byte boundary (the allocator's blocks are aligned far beyond that; asserted)"""
    t = torch.zeros(B, 4, dtype=torch.int64, device="cuda:0")
    assert t.data_ptr() % 32 == 0
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.int64)))
    return t


class Outputs:
    def __init__(self, torch, B):
        self.tau = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        self.grf = torch.full((B, 12), np.nan, dtype=torch.float64, device="cuda:0")
        self.status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")

    def host(self):
        return self.tau.cpu().numpy(), self.grf.cpu().numpy(), self.status.cpu().numpy()


def run_loop(gpu, states, start, placed=False, check=None, ctx=None, normals=None):
    """The caller's loop over the ticks of `states`.  start: "table" (set_memory, working_set beside it as a plain output),
    "word" (the [B][2] set updated in place) or "cold"; placed: with robot_order / next_robot_order and QLAMD_PLACEMENT_AUTO.
    Per tick: iterations, efforts, statuses, the support masks and (table) the word each robot started from, read before the call."""
    capi, ctx0, torch = gpu
    ctx = ctx or ctx0
    stream = torch.cuda.current_stream().cuda_stream
    B = states[0]["q"].shape[0]
    order = [torch.arange(B, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    iters = [torch.zeros(B, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    ws = torch.zeros(B, 2, dtype=torch.int32, device="cuda:0")
    mem = aligned_table(torch, B)
    out = []
    for k, s in enumerate(states):
        if normals is not None:
            s = dict(s, normals=normals)
        o = Outputs(torch, B)
        started = None
        if start == "table":
            started = mem.cpu().numpy().view(np.uint64)[np.arange(B), slots_of(capi, s["stance"])]
        kw = dict(iterations=iters[k & 1])
        if placed:
            order[(k + 1) & 1].fill_(-1)                             # (this call must write every entry of the next order)
            kw.update(order=order[k & 1], prev_iterations=iters[(k - 1) & 1], next_order=order[(k + 1) & 1], policy=capi.PLACEMENT_AUTO)
        if start == "table":
            kw.update(working_set=ws, set_memory=mem)
        elif start == "word":
            kw.update(prev_working_set=ws, working_set=ws)
        capi.wholebody_solve_placed_device(ctx, capi.to_device(s), o.tau, o.grf, o.status, stream=stream, **kw)
        torch.cuda.synchronize()
        nxt = None
        if placed:
            nxt = order[(k + 1) & 1].cpu().numpy().copy()
            assert np.array_equal(np.sort(nxt), np.arange(B)), k    # a permutation every tick
        tau, _, status = o.host()
        out.append(dict(next_order=nxt, iters=iters[k & 1].cpu().numpy().copy(), tau=tau, status=status, mask=support_mask(s["stance"]), started=started,
                        ws=ws.cpu().numpy().view(np.uint32).reshape(B, 2).copy().view(np.uint64).reshape(B)))
        if check is not None:
            check(k, s, tau, status)
    return out, mem.cpu().numpy().view(np.uint64)


def test_without_a_table_it_is_place_next_call_and_the_plain_entry(gpu):
    """set_memory == NULL: cold (no placement; iterations only) and with the one-set warm start, bit for bit -- efforts, forces,
    statuses, counts, sets."""
    capi, ctx, torch = gpu
    B = 4096
    stream = torch.cuda.current_stream().cuda_stream
    s0, s1 = synth.wholebody_trajectory(B, "trot", 2)

    def old(d, it, prev, ws):
        o = Outputs(torch, B)
        pl = capi.Placement(None, it.data_ptr(), None, None, 0, None if prev is None else prev.data_ptr(), None if ws is None else ws.data_ptr())
        assert capi.lib().qlamd_place_next_call(ctx._h, C.byref(pl)) == 0
        capi.wholebody_solve_device(ctx, d, o.tau, o.grf, o.status, stream=stream)
        torch.cuda.synchronize()
        return o.host()

    def new(d, it, prev, ws):
        o = Outputs(torch, B)
        capi.wholebody_solve_placed_device(ctx, d, o.tau, o.grf, o.status, stream=stream, iterations=it, prev_working_set=prev, working_set=ws)
        torch.cuda.synchronize()
        return o.host()

    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda:0")  # noqa: E731
    for entry_a, entry_b in ((old, new),):
        res = []
        for entry in (entry_a, entry_b):
            it, ws = i32(B), i32(B, 2)
            r = [entry(capi.to_device(s0), it, None, None), it.cpu().numpy().copy()]          # cold
            r += [entry(capi.to_device(s0), it, None, ws), ws.cpu().numpy().copy()]           # cold, sets out
            r += [entry(capi.to_device(s1), it, ws, ws), it.cpu().numpy().copy(), ws.cpu().numpy().copy()]   # warm, in place
            res.append(r)
        for a, b in zip(*res):
            if isinstance(a, tuple):
                for x, y in zip(a, b):
                    assert np.array_equal(x, y, equal_nan=True)
            else:
                assert np.array_equal(a, b)
        assert (res[1][0][2] == 0).all() and (res[1][5] != 0).any()
    # bare: no placement at all is the plain entry
    o1, o2 = Outputs(torch, B), Outputs(torch, B)
    capi.wholebody_solve_device(ctx, capi.to_device(s0), o1.tau, o1.grf, o1.status, stream=stream)
    capi.wholebody_solve_placed_device(ctx, capi.to_device(s0), o2.tau, o2.grf, o2.status, stream=stream)
    torch.cuda.synchronize()
    for x, y in zip(o1.host(), o2.host()):
        assert np.array_equal(x, y)
    # a placement pending on the context is neither taken nor cleared by the placed entry
    it = i32(B)
    pl = capi.Placement(None, it.data_ptr(), None, None, 0, None, None)
    assert capi.lib().qlamd_place_next_call(ctx._h, C.byref(pl)) == 0
    capi.wholebody_solve_placed_device(ctx, capi.to_device(s0), o2.tau, o2.grf, o2.status, stream=stream)
    torch.cuda.synchronize()
    assert (it == 0).all()
    capi.wholebody_solve_device(ctx, capi.to_device(s0), o2.tau, o2.grf, o2.status, stream=stream)
    torch.cuda.synchronize()
    assert (it > 0).any()


def test_a_trot_recalls_its_sets_and_that_pays_in_work(gpu, oracle):
    """1024 robots x 760 ticks.  Every tick against the oracle's whole-body step (1e-6, statuses equal) and against the cold step
    (1e-7).  From tick 400 on, over the robot-ticks whose support mask differs from the previous tick's and under whose mask the
    robot ended an earlier tick with status OK: (a) every one started from a word recording exactly that mask; (b) their mean
    placement->iterations is strictly below the [B][2] one-set loop's over the same robot-ticks."""
    capi, ctx, torch = gpu
    B, T = 1024, 760
    states = synth.wholebody_trajectory(B, "trot", T)
    worst = [0.0]

    def check(k, s, tau, status):
        t0, _, s0 = oracle.wb_step_batch(s, nthreads=16)
        assert np.array_equal(status, s0), (k, int((status != s0).sum()))
        ok = s0 == 0
        err = float(np.abs(tau[ok] - t0[ok]).max())
        worst[0] = max(worst[0], err)
        assert err < TAU_TOL, (k, err)

    tab, mem = run_loop(gpu, states, "table", check=check)
    word, _ = run_loop(gpu, states, "word")
    cold, _ = run_loop(gpu, states, "cold")
    ended_ok = np.zeros((B, 16), bool)
    n = recalled = it_tab = it_word = 0
    worst_cold = 0.0
    for k in range(T):
        assert np.array_equal(tab[k]["status"], cold[k]["status"]), k
        ok = cold[k]["status"] == 0
        worst_cold = max(worst_cold, float(np.abs(tab[k]["tau"][ok] - cold[k]["tau"][ok]).max()))
        mask = tab[k]["mask"]
        if k >= 400:
            sel = (mask != tab[k - 1]["mask"]) & ended_ok[np.arange(B), mask]
            n += int(sel.sum())
            recalled += int((legs_of(tab[k]["started"])[sel] == mask[sel]).sum())
            it_tab += int(tab[k]["iters"][sel].sum())
            it_word += int(word[k]["iters"][sel].sum())
        ended_ok[np.arange(B)[tab[k]["status"] == 0], mask[tab[k]["status"] == 0]] = True
    print("whole-body, trot B=%d T=%d: worst |dtau| oracle %.2e, cold %.2e; from tick 400: %d switching robot-ticks, %d recalled, mean "
          "iterations table %.3f / one set %.3f" % (B, T, worst[0], worst_cold, n, recalled, it_tab / max(n, 1), it_word / max(n, 1)))
    assert worst_cold < WARM_TOL
    assert n >= 1000
    assert recalled == n                       # (a)
    assert it_tab < it_word                    # (b): the same robot-ticks on both sides
    # the table's words record their slot's own support set; working_set beside the table is this tick's word
    for slot, m in ((0, 0b0101), (1, 0b1010), (2, 0b1111)):
        assert np.isin(legs_of(mem[:, slot]), (0, m)).all()
    assert (mem[:, 3] == 0).all()
    assert np.array_equal(tab[-1]["ws"], mem[np.arange(B), slots_of(capi, states[-1]["stance"])])


def test_the_table_with_a_placement_at_8192_robots(gpu):
    capi, ctx, torch = gpu
    B, T = 8192, 24
    states = synth.wholebody_trajectory(B, "trot", T)
    placed, _ = run_loop(gpu, states, "table", placed=True)           # (asserts a permutation every tick)
    plain, _ = run_loop(gpu, states, "table")
    for k in range(T):
        assert np.array_equal(placed[k]["status"], plain[k]["status"]), k
        ok = plain[k]["status"] == 0
        assert np.abs(placed[k]["tau"][ok] - plain[k]["tau"][ok]).max() < WARM_TOL, k
    assert (plain[-1]["status"] == 0).sum() > B // 2


def test_a_small_placed_table_loop_writes_the_identity_order_itself(gpu):
    """QLAMD_PLACEMENT_AUTO counts the table as a warm start: up to 4096 robots that means no placement, and the solving launch
    writes the identity into next_robot_order itself (the buffer is filled with -1 before every call)."""
    capi, ctx, torch = gpu
    B, T = 4096, 6
    states = synth.wholebody_trajectory(B, "trot", T)
    placed, mem_p = run_loop(gpu, states, "table", placed=True)
    plain, mem_u = run_loop(gpu, states, "table")
    for k in range(T):
        assert np.array_equal(placed[k]["next_order"], np.arange(B)), k
        for key in ("status", "tau", "iters", "ws"):
            assert np.array_equal(placed[k][key], plain[k][key]), (k, key)     # the batch order: the unplaced launch bit for bit
    assert np.array_equal(mem_p, mem_u) and (mem_p != 0).any()


def test_per_leg_normals_and_the_second_attempt(gpu, oracle):
    capi, ctx, torch = gpu
    B, T = 1024, 8
    states = synth.wholebody_trajectory(B, "trot", T)
    rng = np.random.default_rng(21)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (B, 4)) + rng.normal(scale=0.08, size=(B, 12))
    nrm = np.ascontiguousarray((nrm.reshape(B, 4, 3) / np.linalg.norm(nrm.reshape(B, 4, 3), axis=2, keepdims=True)).reshape(B, 12))

    def check(k, s, tau, status):
        t0, _, s0 = oracle.wb_step_batch(s, nthreads=16)
        assert np.array_equal(status, s0), k
        assert np.abs(tau[s0 == 0] - t0[s0 == 0]).max() < TAU_TOL, k

    tab, mem = run_loop(gpu, states, "table", check=check, normals=nrm)
    cold, _ = run_loop(gpu, states, "cold", normals=nrm)
    for k in range(T):
        assert np.array_equal(tab[k]["status"], cold[k]["status"])
        assert np.abs(tab[k]["tau"] - cold[k]["tau"])[cold[k]["status"] == 0].max() < WARM_TOL, k
    assert (mem != 0).any()
    # QLAMD_OPT_WARM_FALLBACK 2: every robot that ends with a non-empty set is solved again cold; its slot in use holds 0 -- with
    # per-leg normals and without (the two instantiations of the table kernel and of its second attempt)
    ctx2 = capi.Context(device=0)
    ctx2.set_option(capi.OPT_WARM_FALLBACK, 2)
    for normals in (nrm, None):
        before = ctx2.counter(capi.COUNTER_WARM_RETRIES)
        retry, mem2 = run_loop(gpu, states, "table", ctx=ctx2, normals=normals)
        plain, mem1 = run_loop(gpu, states, "table", normals=normals)
        cold, _ = run_loop(gpu, states, "cold", normals=normals)
        for k in range(T):
            assert np.array_equal(retry[k]["status"], cold[k]["status"])
            assert np.abs(retry[k]["tau"] - cold[k]["tau"])[cold[k]["status"] == 0].max() < WARM_TOL, k
        slot = slots_of(capi, states[-1]["stance"])
        used, ref = mem2[np.arange(B), slot], mem1[np.arange(B), slot]
        retried = (ref & ROWS) != 0
        assert retried.any() and (used[retried] == 0).all() and (retry[-1]["ws"][retried] == 0).all()
        assert ctx2.counter(capi.COUNTER_WARM_RETRIES) - before >= int(retried.sum())
    ctx2.close()


def test_a_failed_robot_leaves_zero_in_its_slot_and_the_others_alone(gpu):
    capi, ctx, torch = gpu
    B = 1024
    s = synth.make_wholebody_states(B, "trot")
    slot = slots_of(capi, s["stance"])
    rng = np.random.default_rng(3)
    broken = rng.choice(B, size=19, replace=False)
    s["q"] = s["q"].copy()
    s["q"][broken] = np.nan
    marks = rng.integers(1, 1 << 63, size=(B, 4), dtype=np.uint64)
    marks[np.arange(B), slot] = 0
    mem = aligned_table(torch, B, marks)
    o = Outputs(torch, B)
    capi.wholebody_solve_placed_device(ctx, capi.to_device(s), o.tau, o.grf, o.status, set_memory=mem)
    torch.cuda.synchronize()
    st, got = o.host()[2], mem.cpu().numpy().view(np.uint64)
    assert (st[broken] != 0).all() and (np.delete(st, broken) == 0).all()
    assert (got[broken, slot[broken]] == 0).all()
    ok = np.setdiff1d(np.arange(B), broken)
    assert (legs_of(got[ok, slot[ok]]) == support_mask(s["stance"])[ok]).all()
    others = np.ones((B, 4), bool)
    others[np.arange(B), slot] = False
    assert np.array_equal(got[others], marks[others])
    # a failed robot that had a record loses it
    capi.wholebody_solve_placed_device(ctx, capi.to_device(synth.make_wholebody_states(B, "trot")), o.tau, o.grf, o.status, set_memory=mem)
    capi.wholebody_solve_placed_device(ctx, capi.to_device(s), o.tau, o.grf, o.status, set_memory=mem)
    torch.cuda.synchronize()
    got = mem.cpu().numpy().view(np.uint64)
    assert (got[broken, slot[broken]] == 0).all() and (got[ok, slot[ok]] != 0).all()


def test_refusals_write_nothing(gpu):
    capi, ctx, torch = gpu
    B = 256
    s = synth.make_wholebody_states(B, "trot")
    d = capi.to_device(s)
    o = Outputs(torch, B)
    mem = aligned_table(torch, B)
    off = torch.zeros(4 * B + 2, dtype=torch.int64, device="cuda:0")[1:4 * B + 1].view(B, 4)       # 8 bytes off
    assert off.data_ptr() % 32 == 8
    ws = torch.zeros(B, 2, dtype=torch.int32, device="cuda:0")
    small = torch.zeros(B, 4, dtype=torch.int32, device="cuda:0")

    def refused(call):
        with pytest.raises(capi.QlamdError) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        tau, grf, st = o.host()
        assert np.isnan(tau).all() and np.isnan(grf).all() and (st == -1).all()
        assert (mem == 0).all() and (off == 0).all() and (ws == 0).all() and (small == 0).all()

    refused(lambda: capi.wholebody_solve_placed_device(ctx, d, o.tau, o.grf, o.status, set_memory=off))
    refused(lambda: capi.wholebody_solve_placed_device(ctx, d, o.tau, o.grf, o.status, set_memory=mem, prev_working_set=ws))
    # placement->set_memory (the balance step's 32-bit table) and a host-memory call: through the C interface
    prm, keep = capi.default_wholebody_params(), []
    wb = capi._wholebody_batch(d, keep)
    fn = capi.lib().qlamd_wholebody_solve_placed_batch
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    pl = capi.Placement(None, None, None, None, 0, None, None, small.data_ptr())

    def raw(placement, table, memory):
        rc = fn(ctx._h, C.addressof(prm), C.addressof(wb), B, C.addressof(placement) if placement is not None else None, table,
                o.tau.data_ptr(), o.grf.data_ptr(), o.status.data_ptr(), memory, None)
        if rc != 0:
            raise capi.QlamdError(rc, "qlamd_wholebody_solve_placed_batch")

    refused(lambda: raw(pl, mem.data_ptr(), capi.MEM_DEVICE))
    refused(lambda: raw(pl, None, capi.MEM_DEVICE))
    hs = {k: np.ascontiguousarray(v) for k, v in s.items()}
    hwb = capi._wholebody_batch(hs, keep)
    htau, hgrf, hst = np.full((B, 12), np.nan), np.full((B, 12), np.nan), np.full(B, -1, np.int32)
    hmem = np.zeros((B, 4), np.uint64)
    for table in (hmem.ctypes.data, None):
        rc = fn(ctx._h, C.addressof(prm), C.addressof(hwb), B, None, table, htau.ctypes.data, hgrf.ctypes.data, hst.ctypes.data, capi.MEM_HOST, None)
        assert rc == capi.ERR_INVALID_ARGUMENT
        assert np.isnan(htau).all() and (hst == -1).all() and (hmem == 0).all()
    # ... and the call that is not refused runs
    capi.wholebody_solve_placed_device(ctx, d, o.tau, o.grf, o.status, set_memory=mem)
    torch.cuda.synchronize()
    assert (o.host()[2] == 0).all() and (mem != 0).any()

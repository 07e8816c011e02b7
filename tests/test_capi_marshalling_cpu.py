"""CPU-only: what every public wrapper of capi.py hands to the C entries.

capi._lib is replaced by a stand-in whose every qlamd_* attribute records its arguments and returns 0; each wrapper is then
called at B = 5 (no multiple of the 4 robots of a wavefront, so a length taken from the wrong array shows), the host form
with numpy arrays, the device form with CPU torch tensors (they have data_ptr(), dtype, numel() and is_contiguous(), and
nothing dereferences them), once with every optional argument given and once with none.  Checked per call: the entry's name,
every scalar, which pointers are NULL, and for struct arguments every pointer member read back from the recorded byref /
address -- it is the array that was passed, or NULL.  Inputs are contiguous and of the entry's dtype, so no wrapper copies
them and the pointers can be compared.  Nothing here knows how the binding is written: the test holds for any capi.py that
marshals the same way."""
import ctypes as C

import numpy as np
import pytest
import torch

from quadruped_locomotion_amd import capi

B = 5
H = 0xC0FFEE      # the context handle the wrappers pass on
STREAM = 0x5151
NN = object()     # "some pointer, not NULL": an array the wrapper made for itself and does not return

# struct arguments that may arrive as an address instead of a byref: entry -> {argument index: mirror}
BY_ADDRESS = {"qlamd_wholebody_solve_placed_batch": {1: "WholebodyParams", 2: "WholebodyBatch", 4: "Placement"},
              "qlamd_wholebody_forward_dynamics_batch": {1: "WholebodyBatch", 10: "PlantNext"}}
DEFAULTS = ("qlamd_balance_default_params", "qlamd_default_robot_model", "qlamd_pose_default_params", "qlamd_swing_default_params",
            "qlamd_ik_default_params", "qlamd_joint_pid_default_params", "qlamd_wholebody_default_params")


def snap(v, cls=None):
    """An argument as the entry would see it, taken while the call is in progress: scalars by value, structs as (mirror's name,
    address, {member: value} of the pointer and int members)."""
    if cls is not None and isinstance(v, int):
        v = getattr(capi, cls).from_address(v)
    elif hasattr(v, "_obj"):
        v = v._obj
    if isinstance(v, C.Structure):
        return (type(v).__name__, C.addressof(v), {n: getattr(v, n) for n, t in v._fields_ if t in (C.c_void_p, C.c_int)})
    if isinstance(v, C._SimpleCData):
        return v.value
    return v


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("qlamd_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, [snap(a, BY_ADDRESS.get(name, {}).get(i)) for i, a in enumerate(args)]))
            return 0
        fn.__name__ = name
        return fn

    def take(self):
        """The calls since the last take(), without the *_default_params fills (asserted on their own)."""
        calls, self.calls = [c for c in self.calls if c[0] not in DEFAULTS], []
        return calls


class S:
    """Expected struct argument: the mirror's name, the members that are not NULL / 0, optionally its address."""

    def __init__(self, name, _at=None, **members):
        self.name, self.at, self.members = name, _at, members


def p(a):
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def same(got, want, where):
    if isinstance(want, S):
        assert isinstance(got, tuple) and got[0] == want.name, where
        if want.at is not None:
            assert got[1] == want.at, where
        full = {n: (0 if t is C.c_int else None) for n, t in getattr(capi, want.name)._fields_ if t in (C.c_void_p, C.c_int)}
        assert set(want.members) <= set(full), where
        full.update(want.members)
        assert got[2].keys() == full.keys(), where
        for n in full:
            same(got[2][n], full[n], "%s.%s" % (where, n))
    elif want is NN:
        assert isinstance(got, int) and got != 0, where
    elif want is None:
        assert got is None or got == 0 and not isinstance(got, float), where
    elif isinstance(want, float):
        assert isinstance(got, float) and got == want, where
    else:
        assert got == want and not isinstance(got, float), where


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(capi, "_lib", r)
    return r


@pytest.fixture
def ctx(rec):
    c = capi.Context()
    c._h = C.c_void_p(H)
    rec.take()
    yield c
    c._h = C.c_void_p()


def one(rec, name, *want):
    calls = rec.take()
    assert [c[0] for c in calls] == [name], calls
    got = calls[0][1]
    assert len(got) == len(want), (name, len(got))
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, "%s arg %d" % (name, i))


def f64(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 1.0


def arr(dtype, *shape):
    return np.ones(shape, dtype=dtype)


def tt(a):
    return None if a is None else torch.from_numpy(a)


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


STATE_SHAPES = dict(q=12, base_pos=3, base_quat=4, base_linvel=3, base_angvel=3, des_pos=3, des_quat=4, des_linvel=3, des_angvel=3)
STATE_MEMBER = dict(q="joint_position", base_pos="base_position", base_quat="base_orientation", base_linvel="base_linear_velocity",
                    base_angvel="base_angular_velocity", des_pos="desired_position", des_quat="desired_orientation",
                    des_linvel="desired_linear_velocity", des_angvel="desired_angular_velocity", stance="support_leg",
                    normals="surface_normal")


def make_state():
    s = {k: f64(B, n) for k, n in STATE_SHAPES.items()}
    s["stance"] = arr(np.uint8, B, 4)
    return s


def state_struct(s, normals=None, skip=()):
    m = {STATE_MEMBER[k]: p(v) for k, v in s.items() if k in STATE_MEMBER and k not in skip and k != "normals"}
    if normals is not None:
        m["surface_normal"] = p(normals)
    return S("StateBatch", **m)


PLACEMENT_MEMBER = dict(order="robot_order", iterations="iterations", prev_iterations="prev_iterations", next_order="next_robot_order",
                        prev_working_set="prev_working_set", working_set="working_set", set_memory="set_memory")


def placement_struct(policy=0, **arrays):
    return S("Placement", policy=policy, **{PLACEMENT_MEMBER[k]: p(v) for k, v in arrays.items() if v is not None})


# ---- context, options, defaults ---------------------------------------------------------------------------------------------

def test_context_and_scalars(rec):
    c = capi.Context()
    calls = rec.calls
    assert [n for n, _ in calls] == ["qlamd_balance_default_params", "qlamd_context_create"]
    same(calls[0][1][0], S("BalanceParams", _at=C.addressof(c.params)), "default params")
    for g, w in zip(calls[1][1], (S("BalanceParams", _at=C.addressof(c.params)), None, 0, None)):
        same(g, w, "context_create")
    rec.calls = []
    prm, model = capi.BalanceParams(), capi.RobotModel()
    c2 = capi.Context(prm, model, device=3)
    one(rec, "qlamd_context_create", S("BalanceParams", _at=C.addressof(prm)), S("RobotModel", _at=C.addressof(model)), 3, None)
    assert c2.params is prm and c2.device == 3
    c._h = C.c_void_p(H)
    c.set_option(capi.OPT_STATE_LAYOUT, capi.STATE_RECORDS)
    one(rec, "qlamd_set_option", H, 8, 1)
    assert c.counter(capi.COUNTER_WARM_RETRIES) == 0
    one(rec, "qlamd_get_counter", H, 1, 0)
    c.reserve(4096)
    one(rec, "qlamd_reserve", H, 4096)
    c.set_robots_per_wave(16)
    one(rec, "qlamd_set_robots_per_wave", H, 16)
    c.close()
    one(rec, "qlamd_context_destroy", H)
    c.close()                                        # a closed context is not destroyed twice
    assert rec.take() == []


def test_defaults_and_host_functions(rec):
    for fn, entry, mirror in ((capi.default_params, "qlamd_balance_default_params", "BalanceParams"),
                              (capi.default_pose_params, "qlamd_pose_default_params", "PoseParams"),
                              (capi.default_robot_model, "qlamd_default_robot_model", "RobotModel"),
                              (capi.default_swing_params, "qlamd_swing_default_params", "SwingParams"),
                              (capi.default_joint_pid_params, "qlamd_joint_pid_default_params", "JointPidParams"),
                              (capi.default_ik_params, "qlamd_ik_default_params", "IkParams"),
                              (capi.default_wholebody_params, "qlamd_wholebody_default_params", "WholebodyParams")):
        out = fn()
        assert [n for n, _ in rec.calls] == [entry] and len(rec.calls[0][1]) == 1
        same(rec.calls[0][1][0], S(mirror, _at=C.addressof(out)), entry)
        rec.calls = []
    assert capi.set_memory_slot(5) == 0
    one(rec, "qlamd_set_memory_slot", 5)
    assert capi.tick_command_bytes(B) == 0
    one(rec, "qlamd_tick_command_bytes", B)
    params = (capi.BalanceParams * B)()
    out = capi.robot_params_fill(params)
    assert out.shape == (B, capi.ROBOT_PARAMS_DOUBLES) and out.dtype == np.float64
    one(rec, "qlamd_robot_params_fill", C.addressof(params), B, p(out))
    out = capi.robot_params_fill([capi.BalanceParams() for _ in range(B)])
    one(rec, "qlamd_robot_params_fill", NN, B, p(out))
    out = capi.robot_params_fill(capi.BalanceParams())
    one(rec, "qlamd_robot_params_fill", NN, 1, p(out))


def test_errors_carry_the_entry_and_the_code(rec, ctx, monkeypatch):
    def failing(name):
        def fn(*args):
            return b"refused" if name == "qlamd_strerror" else capi.ERR_BUSY
        fn.__name__ = name
        return fn
    monkeypatch.setattr(Recorder, "__getattr__", lambda self, name: failing(name))
    for call, entry in ((lambda: ctx.reserve(8), "qlamd_reserve"), (lambda: capi.virtual_wrench(ctx, make_state()), "qlamd_virtual_wrench_batch"),
                        (lambda: capi.wholebody_solve(ctx, make_wb()), "qlamd_wholebody_solve_batch"),
                        (lambda: ctx.place_next_call(), "qlamd_place_next_call")):
        with pytest.raises(capi.QlamdError) as e:
            call()
        assert e.value.code == capi.ERR_BUSY and str(e.value) == "%s failed: refused (-6)" % entry


# ---- the balance step -------------------------------------------------------------------------------------------------------

def test_balance_solve_host(rec, ctx):
    s, normals = make_state(), f64(B, 12)
    tau, grf, st = ctx.balance_solve_host(s)
    assert tau.shape == grf.shape == (B, 12) and st.shape == (B,) and st.dtype == np.int32 and (st == -1).all()
    one(rec, "qlamd_balance_solve_batch", H, state_struct(s), B, p(tau), p(grf), p(st), capi.MEM_HOST, None)
    mine_t, mine_g = np.zeros((B, 12)), np.zeros((B, 12))
    tau, grf, st = ctx.balance_solve_host(s, normals=normals, want_forces=True, tau=mine_t, grf=mine_g)
    assert tau is mine_t and grf is mine_g
    one(rec, "qlamd_balance_solve_batch", H, state_struct(s, normals), B, p(mine_t), p(mine_g), p(st), capi.MEM_HOST, None)
    tau, grf, st = ctx.balance_solve_host(s, want_forces=False)
    assert grf is None
    one(rec, "qlamd_balance_solve_batch", H, state_struct(s), B, p(tau), None, p(st), capi.MEM_HOST, None)
    flat = dict(s, q=s["q"].reshape(-1), base_pos=s["base_pos"].reshape(-1), stance=s["stance"].reshape(-1))   # B comes from q / 12
    tau, grf, st = ctx.balance_solve_host(flat)
    one(rec, "qlamd_balance_solve_batch", H, state_struct(s), B, p(tau), p(grf), p(st), capi.MEM_HOST, None)
    for bad in (np.zeros((B, 12), np.float32), np.zeros((B - 1, 12)), np.zeros((12, B)).T):
        with pytest.raises(ValueError):
            ctx.balance_solve_host(s, tau=bad)
        with pytest.raises(ValueError):
            ctx.balance_solve_host(s, grf=bad)
    assert rec.take() == []


def device_state(normals=False):
    s = make_state()
    d = {k: tt(v) for k, v in s.items()}
    if normals:
        d["normals"] = tt(f64(B, 12))
    return d


def test_balance_solve_device(rec, ctx):
    tau, grf, st = tt(f64(B, 12)), tt(f64(B, 12)), i32(B)
    d = device_state()
    ctx.balance_solve_device(d, tau, None, st)
    one(rec, "qlamd_balance_solve_batch", H, state_struct(d), B, p(tau), None, p(st), capi.MEM_DEVICE, None)
    d = device_state(normals=True)
    ctx.balance_solve_device(d, tau, grf, st, stream=STREAM)
    one(rec, "qlamd_balance_solve_batch", H, state_struct(d, d["normals"]), B, p(tau), p(grf), p(st), capi.MEM_DEVICE, STREAM)


def placement_arrays():
    return dict(order=i32(B), iterations=i32(B), prev_iterations=i32(B), next_order=i32(B), prev_working_set=i32(B), working_set=i32(B),
                set_memory=i32(B, 4))


def bad_tensors(good):
    """wrong dtype, wrong length, not contiguous -- each with the other two properties right"""
    n = good.numel()
    return (torch.zeros(good.shape, dtype=torch.int64 if good.dtype != torch.int64 else torch.int32),
            torch.zeros(n + 1, dtype=good.dtype), torch.zeros(2 * n, dtype=good.dtype)[::2])


def test_balance_solve_placed_device(rec, ctx):
    tau, grf, st = tt(f64(B, 12)), tt(f64(B, 12)), i32(B)
    d = device_state()
    ctx.balance_solve_placed_device(d, tau, None, st)
    one(rec, "qlamd_balance_solve_placed_batch", H, state_struct(d), B, placement_struct(), p(tau), None, p(st), capi.MEM_DEVICE, None)
    d, a = device_state(normals=True), placement_arrays()
    ctx.balance_solve_placed_device(d, tau, grf, st, policy=capi.PLACEMENT_THROUGHPUT, stream=STREAM, **a)
    one(rec, "qlamd_balance_solve_placed_batch", H, state_struct(d, d["normals"]), B, placement_struct(2, **a), p(tau), p(grf), p(st),
        capi.MEM_DEVICE, STREAM)
    for name, good in a.items():
        for bad in bad_tensors(good):
            with pytest.raises(ValueError, match=name):
                ctx.balance_solve_placed_device(d, tau, grf, st, **{name: bad})
    assert rec.take() == []


def test_force_distribution_placed_device(rec, ctx):
    q, quat, sup, wrench, normals = tt(f64(B, 12)), tt(f64(B, 4)), tt(arr(np.uint8, B, 4)), tt(f64(B, 6)), tt(f64(B, 12))
    tau, grf, st = tt(f64(B, 12)), tt(f64(B, 12)), i32(B)
    ctx.force_distribution_placed_device(q, quat, sup, wrench, tau, None, st)
    one(rec, "qlamd_force_distribution_placed_batch", H, p(q), p(quat), p(sup), None, p(wrench), B, placement_struct(), p(tau), None, p(st),
        capi.MEM_DEVICE, None)
    a = placement_arrays()
    ctx.force_distribution_placed_device(q, quat, sup, wrench, tau, grf, st, normals=normals, policy=1, stream=STREAM, **a)
    one(rec, "qlamd_force_distribution_placed_batch", H, p(q), p(quat), p(sup), p(normals), p(wrench), B, placement_struct(1, **a), p(tau),
        p(grf), p(st), capi.MEM_DEVICE, STREAM)
    for bad in bad_tensors(a["set_memory"]):
        with pytest.raises(ValueError, match="set_memory"):
            ctx.force_distribution_placed_device(q, quat, sup, wrench, tau, grf, st, set_memory=bad)
    assert rec.take() == []


def test_balance_solve_robot_params_device(rec, ctx):
    tau, grf, st = tt(f64(B, 12)), tt(f64(B, 12)), i32(B)
    rp = tt(f64(B, capi.ROBOT_PARAMS_DOUBLES))
    d = device_state()
    ctx.balance_solve_robot_params_device(d, rp, tau, None, st)
    one(rec, "qlamd_balance_solve_robot_params_batch", H, state_struct(d), p(rp), B, placement_struct(), p(tau), None, p(st),
        capi.MEM_DEVICE, None)
    ctx.balance_solve_robot_params_device(d, None, tau, None, st)                     # NULL records: the library's to refuse
    one(rec, "qlamd_balance_solve_robot_params_batch", H, state_struct(d), None, B, placement_struct(), p(tau), None, p(st),
        capi.MEM_DEVICE, None)
    d, a = device_state(normals=True), placement_arrays()
    ctx.balance_solve_robot_params_device(d, rp, tau, grf, st, policy=3, stream=STREAM, **a)
    one(rec, "qlamd_balance_solve_robot_params_batch", H, state_struct(d, d["normals"]), p(rp), B, placement_struct(3, **a), p(tau), p(grf),
        p(st), capi.MEM_DEVICE, STREAM)
    for name, good in a.items():
        for bad in bad_tensors(good):
            with pytest.raises(ValueError, match=name):
                ctx.balance_solve_robot_params_device(d, rp, tau, grf, st, **{name: bad})
    for bad in (torch.zeros(B, 32, dtype=torch.float32), torch.zeros(B, 31, dtype=torch.float64), torch.zeros(B, 64, dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="robot_params"):
            ctx.balance_solve_robot_params_device(d, bad, tau, grf, st)
    assert rec.take() == []


def test_balance_solve_placed_and_robot_params_host(rec, ctx):
    s, normals = make_state(), f64(B, 12)
    order, prev, rp = np.arange(B, dtype=np.int32)[::-1].copy(), arr(np.int32, B), f64(B, capi.ROBOT_PARAMS_DOUBLES)
    tau, grf, st, it = ctx.balance_solve_placed_host(s)
    assert (it == -1).all() and it.dtype == np.int32 and it.shape == (B,)
    one(rec, "qlamd_balance_solve_placed_batch", H, state_struct(s), B, placement_struct(iterations=it), p(tau), p(grf), p(st),
        capi.MEM_HOST, None)
    tau, grf, st, it, nxt = ctx.balance_solve_placed_host(s, order=order, normals=normals, want_forces=False, prev_iterations=prev, policy=2)
    assert grf is None and nxt.shape == (B,) and nxt.dtype == np.int32
    one(rec, "qlamd_balance_solve_placed_batch", H, state_struct(s, normals), B,
        placement_struct(2, order=order, iterations=it, prev_iterations=prev, next_order=nxt), p(tau), None, p(st), capi.MEM_HOST, None)
    tau, grf, st, it = ctx.balance_solve_robot_params_host(s, rp)
    one(rec, "qlamd_balance_solve_robot_params_batch", H, state_struct(s), p(rp), B, placement_struct(iterations=it), p(tau), p(grf), p(st),
        capi.MEM_HOST, None)
    tau, grf, st, it = ctx.balance_solve_robot_params_host(s, None, order=order, normals=normals, want_forces=False)
    one(rec, "qlamd_balance_solve_robot_params_batch", H, state_struct(s, normals), None, B, placement_struct(order=order, iterations=it),
        p(tau), None, p(st), capi.MEM_HOST, None)


def test_place_next_call_and_placement_from_iterations(rec, ctx):
    ctx.place_next_call()
    one(rec, "qlamd_place_next_call", H, None)
    ctx.place_next_call(prev_iterations=i32(B), policy=2)          # (withdrawn as well: prev_iterations alone is no placement)
    one(rec, "qlamd_place_next_call", H, None)
    a = {k: v for k, v in placement_arrays().items() if k in ("order", "iterations", "prev_iterations", "next_order")}
    ctx.place_next_call(policy=1, **a)
    one(rec, "qlamd_place_next_call", H, placement_struct(1, **a))
    ctx.place_next_call(iterations=a["iterations"])
    one(rec, "qlamd_place_next_call", H, placement_struct(iterations=a["iterations"]))
    it = arr(np.int32, B)
    order = ctx.placement_from_iterations(it)
    assert order.shape == (B,) and order.dtype == np.int32 and (order == -1).all()
    one(rec, "qlamd_placement_from_iterations", H, p(it), B, 0, p(order), capi.MEM_HOST, None)
    order = ctx.placement_from_iterations(it, policy=2)
    one(rec, "qlamd_placement_from_iterations", H, p(it), B, 2, p(order), capi.MEM_HOST, None)
    dit, dorder = i32(B), i32(B)
    assert ctx.placement_from_iterations(dit, dorder) is dorder
    one(rec, "qlamd_placement_from_iterations", H, p(dit), B, 0, p(dorder), capi.MEM_DEVICE, None)
    ctx.placement_from_iterations(dit, dorder, policy=1, stream=STREAM)
    one(rec, "qlamd_placement_from_iterations", H, p(dit), B, 1, p(dorder), capi.MEM_DEVICE, STREAM)
    for args in ((dit, None), (dit, i32(B + 1)), (dit, torch.zeros(B, dtype=torch.int64)), (torch.zeros(B, dtype=torch.int64), dorder)):
        with pytest.raises(ValueError):
            ctx.placement_from_iterations(*args)
    assert rec.take() == []


def test_virtual_wrench_and_leg_kinematics(rec, ctx):
    s = make_state()
    w = capi.virtual_wrench(ctx, s)
    assert w.shape == (B, 6)
    one(rec, "qlamd_virtual_wrench_batch", H, state_struct(s, skip=("q", "stance")), B, p(w), capi.MEM_HOST, None)
    d, dw = device_state(normals=True), tt(f64(B, 6))
    ctx.virtual_wrench_device(d, dw)
    one(rec, "qlamd_virtual_wrench_batch", H, state_struct(d), B, p(dw), capi.MEM_DEVICE, None)      # (the normals are not passed on)
    ctx.virtual_wrench_device(d, dw, stream=STREAM)
    one(rec, "qlamd_virtual_wrench_batch", H, state_struct(d), B, p(dw), capi.MEM_DEVICE, STREAM)
    foot, jac, grav = capi.leg_kinematics(ctx, s["q"], s["base_quat"])
    assert foot.shape == (B, 4, 3) and jac.shape == (B, 4, 9) and grav.shape == (B, 4, 3)
    one(rec, "qlamd_leg_kinematics_batch", H, p(s["q"]), p(s["base_quat"]), B, p(foot), p(jac), p(grav), capi.MEM_HOST, None)
    ctx.leg_kinematics_device(d["q"], d["base_quat"])
    one(rec, "qlamd_leg_kinematics_batch", H, p(d["q"]), p(d["base_quat"]), B, None, None, None, capi.MEM_DEVICE, None)
    foot, jac, grav = tt(f64(B, 4, 3)), tt(f64(B, 4, 9)), tt(f64(B, 4, 3))
    ctx.leg_kinematics_device(d["q"], d["base_quat"], foot, jac, grav, stream=STREAM)
    one(rec, "qlamd_leg_kinematics_batch", H, p(d["q"]), p(d["base_quat"]), B, p(foot), p(jac), p(grav), capi.MEM_DEVICE, STREAM)


def test_force_distribution(rec, ctx):
    q, quat, sup, wrench, normals = f64(B, 12), f64(B, 4), arr(np.uint8, B, 4), f64(B, 6), f64(B, 12)
    tau, grf, st = capi.force_distribution(ctx, q, quat, sup, wrench)
    assert tau.shape == grf.shape == (B, 12) and st.dtype == np.int32 and (st == -1).all()
    one(rec, "qlamd_force_distribution_batch", H, p(q), p(quat), p(sup), None, p(wrench), B, p(tau), p(grf), p(st), capi.MEM_HOST, None)
    mine_t, mine_g = np.zeros((B, 12)), np.zeros((B, 12))
    tau, grf, st = capi.force_distribution(ctx, q, quat, sup, wrench, normals=normals, tau=mine_t, grf=mine_g)
    assert tau is mine_t and grf is mine_g
    one(rec, "qlamd_force_distribution_batch", H, p(q), p(quat), p(sup), p(normals), p(wrench), B, p(tau), p(grf), p(st), capi.MEM_HOST, None)
    with pytest.raises(ValueError):
        capi.force_distribution(ctx, q, quat, sup, wrench, tau=np.zeros((B, 12), np.float32))
    with pytest.raises(ValueError):
        capi.force_distribution(ctx, q, quat, sup, wrench, memory=capi.MEM_DEVICE, tau=mine_t)
    assert rec.take() == []


# ---- swing leg, pose, state machine, messages ---------------------------------------------------------------------------------

SWING_MEMBERS = ("joint_position", "joint_velocity", "joint_velocity_oldest", "target_foot_position", "target_foot_velocity", "support_leg",
                 "id_joint_position")
EXTRA_MEMBERS = ("base_orientation", "joint_command", "leg_mode", "pid_error_last", "pid_error_integral")


def swing_inputs(device):
    a = [f64(B, 12), f64(B, 12), f64(B, 12), f64(B, 4, 3), f64(B, 4, 3), arr(np.uint8, B, 4), f64(B, 12)]
    return [tt(x) for x in a] if device else a


def struct_of(name, members, arrays):
    return S(name, **{m: p(a) for m, a in zip(members, arrays) if a is not None})


@pytest.mark.parametrize("device", [False, True])
def test_swing_leg_torque(rec, ctx, device):
    a = swing_inputs(device)
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    out = tt(f64(B, 12)) if device else None
    tau = capi.swing_leg_torque(ctx, *a[:6], memory=mem, out=out)
    assert tau is out if device else tau.shape == (B, 12)
    one(rec, "qlamd_swing_leg_torque_batch", H, S("SwingParams"), struct_of("SwingBatch", SWING_MEMBERS, a[:6]), B, p(tau), mem, None)
    prm = capi.SwingParams()
    tau = capi.swing_leg_torque(ctx, *a, params=prm, memory=mem, out=out, stream=STREAM)
    one(rec, "qlamd_swing_leg_torque_batch", H, S("SwingParams", _at=C.addressof(prm)), struct_of("SwingBatch", SWING_MEMBERS, a), B, p(tau),
        mem, STREAM)


@pytest.mark.parametrize("device", [False, True])
def test_swing_branch(rec, ctx, device):
    a = swing_inputs(device)
    ext = [f64(B, 4), f64(B, 12), arr(np.uint8, B, 4), f64(B, 12), f64(B, 12)]
    effort = f64(B, 12)
    if device:
        ext, effort = [tt(x) for x in ext], tt(effort)
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    got = capi.swing_branch(ctx, effort, *a[:6], ext[0], ext[1], None, ext[3], ext[4], 0.0025, memory=mem)
    assert got is effort
    one(rec, "qlamd_swing_branch_batch", H, S("SwingParams"), S("JointPidParams"), struct_of("SwingBatch", SWING_MEMBERS, a[:6]),
        struct_of("SwingBranchExtra", EXTRA_MEMBERS, [ext[0], ext[1], None, ext[3], ext[4]]), 0.0025, B, p(effort), mem, None)
    prm, pid = capi.SwingParams(), capi.JointPidParams()
    capi.swing_branch(ctx, effort, *a[:6], *ext, 0.005, q_id=a[6], params=prm, pid=pid, memory=mem, stream=STREAM)
    one(rec, "qlamd_swing_branch_batch", H, S("SwingParams", _at=C.addressof(prm)), S("JointPidParams", _at=C.addressof(pid)),
        struct_of("SwingBatch", SWING_MEMBERS, a), struct_of("SwingBranchExtra", EXTRA_MEMBERS, ext), 0.005, B, p(effort), mem, STREAM)


POSE_KEYS = (("stance", "stance"), ("stance_mask", "stance_mask"), ("nominal", "nominal_stance"), ("polygon", "support_polygon"),
             ("n_vertices", "n_vertices"), ("r_com", "center_of_mass"), ("max_len", "max_limb_length"), ("pose", "pose"))


def pose_problems(device, optional=True):
    pr = dict(stance=f64(B, 4, 3), nominal=f64(B, 4, 3), polygon=f64(B, 4, 2), max_len=f64(B, 4), pose=f64(B, 7))
    if optional:
        pr.update(stance_mask=arr(np.uint8, B, 4), n_vertices=arr(np.int32, B), r_com=f64(B, 3))
    return {k: tt(v) for k, v in pr.items()} if device else pr


def pose_struct(pr):
    return S("PoseBatch", **{m: p(pr[k]) for k, m in POSE_KEYS if k in pr})


@pytest.mark.parametrize("device", [False, True])
def test_pose_sqp_and_base_auto(rec, ctx, device):
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    out3 = (tt(f64(B, 7)), i32(B), i32(B)) if device else None
    out4 = (tt(f64(B, 7)), i32(B), i32(B), i32(B)) if device else None
    pr = pose_problems(device, optional=False)
    pose, it, st = capi.pose_sqp(ctx, pr, memory=mem, out=out3)
    assert pose.shape == (B, 7) and it.shape == st.shape == (B,)
    one(rec, "qlamd_pose_sqp_batch", H, S("PoseParams"), pose_struct(pr), B, p(pose), p(it), p(st), mem, None)
    pose, stage, it, st = capi.base_auto_optimize_pose(ctx, pr, memory=mem, out=out4)
    one(rec, "qlamd_base_auto_optimize_pose_batch", H, S("PoseParams"), pose_struct(pr), None, None, 0.0, B, p(pose), p(stage), p(it), p(st),
        mem, None)
    pr, prm = pose_problems(device), capi.PoseParams()
    pose, it, st = capi.pose_sqp(ctx, pr, params=prm, memory=mem, out=out3, stream=STREAM)
    one(rec, "qlamd_pose_sqp_batch", H, S("PoseParams", _at=C.addressof(prm)), pose_struct(pr), B, p(pose), p(it), p(st), mem, STREAM)
    sfo, mn = (tt(f64(B, 12)), tt(f64(B, 4))) if device else (f64(B, 12), f64(B, 4))
    pose, stage, it, st = capi.base_auto_optimize_pose(ctx, pr, stance_for_orientation=sfo, min_len=mn, leg_tol=0.25, params=prm, memory=mem,
                                                       out=out4, stream=STREAM)
    one(rec, "qlamd_base_auto_optimize_pose_batch", H, S("PoseParams", _at=C.addressof(prm)), pose_struct(pr), p(sfo), p(mn), 0.25, B, p(pose),
        p(stage), p(it), p(st), mem, STREAM)
    if not device:
        assert (st == -1).all() and st.dtype == it.dtype == stage.dtype == np.int32


def test_pose_qp_check_geometric(rec, ctx):
    prm = capi.PoseParams()
    for pr, params, want_prm in ((pose_problems(False, optional=False), None, S("PoseParams")),
                                 (pose_problems(False), prm, S("PoseParams", _at=C.addressof(prm)))):
        pose, st = capi.pose_qp(ctx, pr, params=params)
        assert pose.shape == (B, 7) and st.dtype == np.int32 and (st == -1).all()
        one(rec, "qlamd_pose_qp_batch", H, want_prm, pose_struct(pr), B, p(pose), p(st), capi.MEM_HOST, None)
        ok = capi.pose_check(ctx, pr, params=params)
        assert ok.shape == (B,) and ok.dtype == np.uint8
        one(rec, "qlamd_pose_check_batch", H, want_prm, pose_struct(pr), None, 0.0, B, p(ok), capi.MEM_HOST, None)
        pose = capi.pose_geometric(ctx, pr, params=params)
        one(rec, "qlamd_pose_geometric_batch", H, want_prm, pose_struct(pr), None, B, p(pose), capi.MEM_HOST, None)
    mn, sfo = f64(B, 4), f64(B, 12)
    ok = capi.pose_check(ctx, pr, min_len=mn, leg_tol=0.5, params=prm)
    one(rec, "qlamd_pose_check_batch", H, want_prm, pose_struct(pr), p(mn), 0.5, B, p(ok), capi.MEM_HOST, None)
    pose = capi.pose_geometric(ctx, pr, stance_for_orientation=sfo, params=prm)
    one(rec, "qlamd_pose_geometric_batch", H, want_prm, pose_struct(pr), p(sfo), B, p(pose), capi.MEM_HOST, None)


@pytest.mark.parametrize("device", [False, True])
def test_leg_state_machine(rec, ctx, device):
    io = {n: arr(dt, B, 12 if n in ("joint_position", "stored_joint_position", "joint_command", "foot_target") else 4)
          for n, dt in capi.LEG_STATE_DTYPES.items()}
    if device:
        io = {n: tt(a) for n, a in io.items()}
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    want = S("LegStateBatch", **{n: p(a) for n, a in io.items()})
    assert capi.leg_state_machine(ctx, io, memory=mem) is io
    one(rec, "qlamd_leg_state_machine_batch", H, want, 1, B, mem, None)
    capi.leg_state_machine(ctx, io, index_quirk=0, memory=mem, stream=STREAM)
    one(rec, "qlamd_leg_state_machine_batch", H, want, 0, B, mem, STREAM)


def test_robot_state_unpack(rec, ctx):
    blob, off = arr(np.uint8, 40), np.arange(B + 1, dtype=np.int64) * 8
    names = [n for n, _ in capi.ROBOT_STATE_FIELDS] + ["support_leg", "leg_mode"]
    out, st = capi.robot_state_unpack(ctx, blob, off)
    assert list(out) == names and (st == -1).all() and st.dtype == np.int32
    for n, w in capi.ROBOT_STATE_FIELDS:
        assert out[n].shape == (B, w) and out[n].dtype == np.float64
    assert out["support_leg"].shape == out["leg_mode"].shape == (B, 4) and out["leg_mode"].dtype == np.uint8
    one(rec, "qlamd_robot_state_unpack_batch", H, p(blob), p(off), B, S("RobotStateFields", **{n: p(out[n]) for n in names}), p(st),
        capi.MEM_HOST, None)
    out, st = capi.robot_state_unpack(ctx, blob, off, want=("des_quat", "leg_mode"))
    assert list(out) == ["des_quat", "leg_mode"]
    one(rec, "qlamd_robot_state_unpack_batch", H, p(blob), p(off), B, S("RobotStateFields", des_quat=p(out["des_quat"]), leg_mode=p(out["leg_mode"])),
        p(st), capi.MEM_HOST, None)
    out, st = capi.robot_state_unpack(ctx, b"", np.zeros(B + 1, np.int64), want=())          # no bytes at all: still a pointer
    one(rec, "qlamd_robot_state_unpack_batch", H, NN, NN, B, S("RobotStateFields"), p(st), capi.MEM_HOST, None)
    dblob, doff = tt(blob), tt(off)
    for stream in (None, STREAM):
        out, st = capi.robot_state_unpack_device(ctx, dblob, doff, stream=stream)
        assert list(out) == names and st.dtype == torch.int32 and (st == -1).all() and st.shape == (B,)
        for n, w in capi.ROBOT_STATE_FIELDS:
            assert out[n].shape == (B, w) and out[n].dtype == torch.float64
        assert out["support_leg"].shape == (B, 4) and out["support_leg"].dtype == torch.uint8
        one(rec, "qlamd_robot_state_unpack_batch", H, p(dblob), p(doff), B, S("RobotStateFields", **{n: p(out[n]) for n in names}), p(st),
            capi.MEM_DEVICE, stream)


def test_leg_inverse_kinematics_and_qps(rec, ctx):
    foot, last, prm = f64(B, 12), f64(B, 12), capi.IkParams()
    q, ok = capi.leg_inverse_kinematics(ctx, foot)
    assert q.shape == (B, 12) and ok.shape == (B, 4) and ok.dtype == np.uint8
    one(rec, "qlamd_leg_inverse_kinematics_batch", H, S("IkParams"), p(foot), None, B, p(q), p(ok), capi.MEM_HOST, None)
    q, ok = capi.leg_inverse_kinematics(ctx, foot, joint_position_last=last, params=prm)
    one(rec, "qlamd_leg_inverse_kinematics_batch", H, S("IkParams", _at=C.addressof(prm)), p(foot), p(last), B, p(q), p(ok), capi.MEM_HOST, None)

    n, pe, m = 7, 2, 11
    G, g0, CE, ce0, CI, ci0 = f64(B, n, n), f64(B, n), f64(B, n, pe), f64(B, pe), f64(B, n, m), f64(B, m)
    x, f, st = capi.qp_solve(ctx, G, g0, CE, ce0, CI, ci0)
    assert x.shape == (B, n) and f.shape == (B,) and (st == -1).all()
    one(rec, "qlamd_qp_solve_batch", H, n, pe, m, p(G), p(g0), p(CE), p(ce0), p(CI), p(ci0), B, p(x), p(f), p(st), capi.MEM_HOST, None)
    x, f, st = capi.qp_solve(ctx, G, g0, None, None, None, None)
    one(rec, "qlamd_qp_solve_batch", H, n, 0, 0, p(G), p(g0), None, None, None, None, B, p(x), p(f), p(st), capi.MEM_HOST, None)

    k = 6
    a = [f64(B, k, n), f64(B, k), f64(B, k), f64(B, n), f64(B, pe, n), f64(B, pe), f64(B, m, n), f64(B, m), f64(B, m)]
    x, st = capi.weighted_lsq_qp(ctx, *a)
    assert x.shape == (B, n) and (st == -1).all()
    one(rec, "qlamd_weighted_lsq_qp_batch", H, n, k, pe, m, *[p(v) for v in a], B, p(x), p(st), capi.MEM_HOST, None)
    x, st = capi.weighted_lsq_qp(ctx, *a[:4])
    one(rec, "qlamd_weighted_lsq_qp_batch", H, n, k, 0, 0, *[p(v) for v in a[:4]], None, None, None, None, None, B, p(x), p(st),
        capi.MEM_HOST, None)
    d, out = [tt(v) for v in a], (tt(f64(B, n)), i32(B))
    x, st = capi.weighted_lsq_qp(ctx, *d, memory=capi.MEM_DEVICE, out=out, stream=STREAM)
    assert x is out[0] and st is out[1]
    one(rec, "qlamd_weighted_lsq_qp_batch", H, n, k, pe, m, *[p(v) for v in d], B, p(out[0]), p(out[1]), capi.MEM_DEVICE, STREAM)
    capi.weighted_lsq_qp(ctx, *d[:4], memory=capi.MEM_DEVICE, out=out)
    one(rec, "qlamd_weighted_lsq_qp_batch", H, n, k, 0, 0, *[p(v) for v in d[:4]], None, None, None, None, None, B, p(out[0]), p(out[1]),
        capi.MEM_DEVICE, None)


# ---- whole body -------------------------------------------------------------------------------------------------------------

WB_MEMBER = dict(q="joint_position", qd="joint_velocity", base_quat="base_orientation", base_linvel="base_linear_velocity",
                 base_angvel="base_angular_velocity", a_des="desired_base_acceleration", qdd_des="desired_joint_acceleration",
                 stance="support_leg", normals="surface_normal")


def make_wb(optional=True, device=False):
    s = dict(q=f64(B, 12), qd=f64(B, 12), base_quat=f64(B, 4), base_linvel=f64(B, 3), base_angvel=f64(B, 3), a_des=f64(B, 6),
             stance=arr(np.uint8, B, 4), base_pos=f64(B, 3))
    if optional:
        s.update(qdd_des=f64(B, 12), normals=f64(B, 12))
    return {k: tt(v) for k, v in s.items()} if device else s


def wb_struct(s, free_flight=False):
    return S("WholebodyBatch", **{m: p(s[k]) for k, m in WB_MEMBER.items() if k in s and not (free_flight and k == "stance")})


def test_wholebody_dynamics_and_solve(rec, ctx):
    s = make_wb(optional=False)
    out = capi.wholebody_dynamics(ctx, s)
    assert out["M"].shape == (B, 18, 18) and out["h"].shape == (B, 18) and out["Jc"].shape == (B, 12, 18)
    one(rec, "qlamd_wholebody_dynamics_batch", H, wb_struct(s), 9.81, B, p(out["M"]), p(out["h"]), p(out["Jc"]), capi.MEM_HOST, None)
    s = make_wb()
    out = capi.wholebody_dynamics(ctx, s, gravity=1.5, want=("h",))
    assert out["M"] is None and out["Jc"] is None
    one(rec, "qlamd_wholebody_dynamics_batch", H, wb_struct(s), 1.5, B, None, p(out["h"]), None, capi.MEM_HOST, None)
    d, (M, h, Jc) = make_wb(device=True), (tt(f64(B, 18, 18)), tt(f64(B, 18)), tt(f64(B, 12, 18)))
    capi.wholebody_dynamics_device(ctx, d, None, None, None)
    one(rec, "qlamd_wholebody_dynamics_batch", H, wb_struct(d), 9.81, B, None, None, None, capi.MEM_DEVICE, None)
    capi.wholebody_dynamics_device(ctx, d, M, h, Jc, gravity=2.5, stream=STREAM)
    one(rec, "qlamd_wholebody_dynamics_batch", H, wb_struct(d), 2.5, B, p(M), p(h), p(Jc), capi.MEM_DEVICE, STREAM)

    prm = capi.WholebodyParams()
    s = make_wb(optional=False)
    tau, grf, st = capi.wholebody_solve(ctx, s)
    assert tau.shape == grf.shape == (B, 12) and (st == -1).all() and st.dtype == np.int32
    one(rec, "qlamd_wholebody_solve_batch", H, S("WholebodyParams"), wb_struct(s), B, p(tau), p(grf), p(st), capi.MEM_HOST, None)
    s, mine_t, mine_g = make_wb(), np.zeros((B, 12)), np.zeros((B, 12))
    tau, grf, st = capi.wholebody_solve(ctx, s, params=prm, tau=mine_t, grf=mine_g)
    assert tau is mine_t and grf is mine_g
    one(rec, "qlamd_wholebody_solve_batch", H, S("WholebodyParams", _at=C.addressof(prm)), wb_struct(s), B, p(tau), p(grf), p(st),
        capi.MEM_HOST, None)
    with pytest.raises(ValueError):
        capi.wholebody_solve(ctx, s, tau=np.zeros((B, 12), np.float32))
    tau, grf, st = tt(f64(B, 12)), tt(f64(B, 12)), i32(B)
    d = make_wb(optional=False, device=True)
    capi.wholebody_solve_device(ctx, d, tau, None, st)
    one(rec, "qlamd_wholebody_solve_batch", H, S("WholebodyParams"), wb_struct(d), B, p(tau), None, p(st), capi.MEM_DEVICE, None)
    d = make_wb(device=True)
    capi.wholebody_solve_device(ctx, d, tau, grf, st, params=prm, stream=STREAM)
    one(rec, "qlamd_wholebody_solve_batch", H, S("WholebodyParams", _at=C.addressof(prm)), wb_struct(d), B, p(tau), p(grf), p(st),
        capi.MEM_DEVICE, STREAM)


def test_wholebody_solve_placed_device(rec, ctx):
    tau, grf, st, prm = tt(f64(B, 12)), tt(f64(B, 12)), i32(B), capi.WholebodyParams()
    d = make_wb(optional=False, device=True)
    entry = "qlamd_wholebody_solve_placed_batch"
    capi.wholebody_solve_placed_device(ctx, d, tau, None, st, policy=2)               # no array of a placement: NULL, whatever the policy
    one(rec, entry, H, S("WholebodyParams"), wb_struct(d), B, None, None, p(tau), None, p(st), capi.MEM_DEVICE, None)
    mem = torch.zeros(B, 4, dtype=torch.int64)
    capi.wholebody_solve_placed_device(ctx, d, tau, None, st, set_memory=mem)         # the table is an argument of its own
    one(rec, entry, H, S("WholebodyParams"), wb_struct(d), B, None, p(mem), p(tau), None, p(st), capi.MEM_DEVICE, None)
    d = make_wb(device=True)
    a = dict(order=i32(B), iterations=i32(B), prev_iterations=i32(B), next_order=i32(B), prev_working_set=i32(B, 2),
             working_set=torch.zeros(B, dtype=torch.int64))
    capi.wholebody_solve_placed_device(ctx, d, tau, grf, st, params=prm, stream=STREAM, policy=1, set_memory=mem, **a)
    one(rec, entry, H, S("WholebodyParams", _at=C.addressof(prm)), wb_struct(d), B, placement_struct(1, **a), p(mem), p(tau), p(grf), p(st),
        capi.MEM_DEVICE, STREAM)
    capi.wholebody_solve_placed_device(ctx, d, tau, grf, st, working_set=a["prev_working_set"])
    one(rec, entry, H, S("WholebodyParams"), wb_struct(d), B, placement_struct(working_set=a["prev_working_set"]), None, p(tau), p(grf), p(st),
        capi.MEM_DEVICE, None)
    for bad in bad_tensors(mem):
        with pytest.raises(ValueError, match="set_memory"):
            capi.wholebody_solve_placed_device(ctx, d, tau, grf, st, set_memory=bad)
    for name in ("prev_working_set", "working_set"):
        for bad in (i32(B), i32(B, 3), torch.zeros(B, 2, dtype=torch.int64)[:, 0]):   # 4 and 12 bytes a robot; 8, but strided
            with pytest.raises(ValueError, match=name):
                capi.wholebody_solve_placed_device(ctx, d, tau, grf, st, **{name: bad})
    assert rec.take() == []


PLANT_KEYS = (("joint_position", "q"), ("joint_velocity", "qd"), ("base_position", "base_pos"), ("base_orientation", "base_quat"),
              ("base_linear_velocity", "base_linvel"), ("base_angular_velocity", "base_angvel"))


def plant_struct(nxt):
    return S("PlantNext", **{m: p(nxt[k]) for m, k in PLANT_KEYS})


def test_wholebody_forward_dynamics(rec, ctx):
    entry = "qlamd_wholebody_forward_dynamics_batch"
    s, tau, g_ext = make_wb(), f64(B, 12), f64(B, 18)
    out = capi.wholebody_forward_dynamics(ctx, s, tau)
    assert out["acc"].shape == (B, 18) and out["f"].shape == (B, 12) and (out["status"] == -1).all() and "next" not in out
    one(rec, entry, H, wb_struct(s), p(tau), None, None, 9.81, 0.0, B, p(out["acc"]), p(out["f"]), None, p(out["status"]), capi.MEM_HOST, None)
    out = capi.wholebody_forward_dynamics(ctx, s, tau, g_ext=g_ext, gravity=3.5, dt=0.002, free_flight=True)
    nxt = out["next"]
    assert [nxt[k].shape for _, k in PLANT_KEYS] == [(B, 12), (B, 12), (B, 3), (B, 4), (B, 3), (B, 3)] and nxt["q"] is not s["q"]
    one(rec, entry, H, wb_struct(s, free_flight=True), p(tau), p(g_ext), p(s["base_pos"]), 3.5, 0.002, B, p(out["acc"]), p(out["f"]),
        plant_struct(nxt), p(out["status"]), capi.MEM_HOST, None)
    out = capi.wholebody_forward_dynamics(ctx, s, tau, dt=0.004, in_place=True)
    assert all(out["next"][k] is s[k] for _, k in PLANT_KEYS)
    one(rec, entry, H, wb_struct(s), p(tau), None, p(s["base_pos"]), 9.81, 0.004, B, p(out["acc"]), p(out["f"]), plant_struct(s),
        p(out["status"]), capi.MEM_HOST, None)
    with pytest.raises(ValueError):
        capi.wholebody_forward_dynamics(ctx, dict(s, qd=s["qd"].astype(np.float32)), tau, dt=0.004, in_place=True)
    with pytest.raises(ValueError):
        capi.wholebody_forward_dynamics(ctx, s, f64(B + 1, 12))
    with pytest.raises(ValueError):
        capi.wholebody_forward_dynamics(ctx, s, tau, g_ext=f64(B, 12))
    assert rec.take() == []

    d, dtau, st = make_wb(device=True), tt(tau), i32(B)
    capi.wholebody_forward_dynamics_device(ctx, d, dtau, st)
    one(rec, entry, H, wb_struct(d), p(dtau), None, None, 9.81, 0.0, B, None, None, None, p(st), capi.MEM_DEVICE, None)
    acc, f, dg = tt(f64(B, 18)), tt(f64(B, 12)), tt(g_ext)
    nxt = {k: tt(f64(*d[k].shape)) for _, k in PLANT_KEYS}
    capi.wholebody_forward_dynamics_device(ctx, d, dtau, st, acc=acc, f=f, g_ext=dg, gravity=4.5, dt=0.001, next=nxt, free_flight=True,
                                           stream=STREAM)
    one(rec, entry, H, wb_struct(d, free_flight=True), p(dtau), p(dg), p(d["base_pos"]), 4.5, 0.001, B, p(acc), p(f), plant_struct(nxt), p(st),
        capi.MEM_DEVICE, STREAM)
    capi.wholebody_forward_dynamics_device(ctx, d, dtau, st, dt=0.001, next=d)                   # a rollout in place
    one(rec, entry, H, wb_struct(d), p(dtau), None, p(d["base_pos"]), 9.81, 0.001, B, None, None, plant_struct(d), p(st), capi.MEM_DEVICE, None)


# ---- the whole tick ---------------------------------------------------------------------------------------------------------

TICK_WIDTH = dict(messages=None, offsets=None, joint_position=12, joint_velocity=12, joint_velocity_oldest=12, base_position=3,
                  base_orientation=4, base_linear_velocity=3, base_angular_velocity=3, contact=4, limb_state=4, store_flag=4,
                  stored_joint_position=12, leg_mode=4, support=4, pid_error_last=12, pid_error_integral=12, joint_effort=12,
                  leg_state_code=4, status=0, message_status=0, command=None, working_set=0, placement_state=None, set_memory=4,
                  iterations=0)
TICK_OPTIONAL = ("leg_state_code", "command", "working_set", "placement_state", "set_memory", "iterations")


def make_tick(device, optional):
    io = {}
    for n, dt in capi.TICK_FIELDS:
        if n in TICK_OPTIONAL and not optional:
            continue
        if device and dt == np.uint32:
            dt = np.int32                           # (a torch tensor holds the 32-bit words as int32)
        w = TICK_WIDTH[n]
        io[n] = (np.arange(B + 1, dtype=np.int64) * 8 if n == "offsets" else arr(dt, 4 * B) if n == "placement_state" else
                 arr(dt, 64) if w is None else arr(dt, B) if w == 0 else arr(dt, B, w))
    return {n: tt(a) for n, a in io.items()} if device else io


@pytest.mark.parametrize("device", [False, True])
def test_full_tick(rec, ctx, device):
    assert set(TICK_WIDTH) == {n for n, _ in capi.TICK_FIELDS}
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    io = make_tick(device, optional=False)
    assert capi.full_tick(ctx, io, 0.0025, memory=mem) is io
    one(rec, "qlamd_full_tick_batch", H, S("SwingParams"), S("JointPidParams"), S("TickBatch", **{n: p(a) for n, a in io.items()}), 0.0025, 1, B,
        mem, None)
    io = dict(make_tick(device, optional=False), leg_state_code=None, command=None)                  # None as good as absent
    capi.full_tick(ctx, io, 0.0025, memory=mem)
    one(rec, "qlamd_full_tick_batch", H, S("SwingParams"), S("JointPidParams"),
        S("TickBatch", **{n: p(a) for n, a in io.items() if a is not None}), 0.0025, 1, B, mem, None)
    io, prm, pid = make_tick(device, optional=True), capi.SwingParams(), capi.JointPidParams()
    capi.full_tick(ctx, io, 0.005, index_quirk=0, params=prm, pid=pid, memory=mem, stream=STREAM)
    one(rec, "qlamd_full_tick_batch", H, S("SwingParams", _at=C.addressof(prm)), S("JointPidParams", _at=C.addressof(pid)),
        S("TickBatch", **{n: p(a) for n, a in io.items()}), 0.005, 0, B, mem, STREAM)
    bad = [arr(np.uint32, B, 3)]
    if device:
        bad = [i32(B, 3), torch.zeros(B, 4, dtype=torch.int64), i32(B, 8)[:, ::2]]
    for sm in bad:
        with pytest.raises(ValueError, match="set_memory"):
            capi.full_tick(ctx, dict(io, set_memory=sm), 0.005, memory=mem)
    assert rec.take() == []

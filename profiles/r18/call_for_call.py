"""The record of check 5 of profiles/r18/binding_fold.md: every public wrapper of the plant and contact bindings driven against a
recorder in the place of the library, over a grid of its options, and what reached the entry written to a JSON file.

    python call_for_call.py <tree> <out.json>       one process per tree (the parent's checkout, this one)
    python call_for_call.py --compare a.json b.json

Recorded per call: the entry reached, every scalar, every struct member, and for each pointer NULL or the name of the input or
result array it points to (raw addresses differ between processes).  A wrapper that raises is recorded by the exception's type."""
import ctypes as C
import itertools
import json
import sys

import numpy as np


def main(tree, out_path):
    sys.path.insert(0, tree)
    import torch
    from quadruped_locomotion_amd import capi, contact_anchor as CA, contact_detection as CD, plant_contacts as PC, plant_friction as PF

    names, calls, log = {}, [], []

    def reg(name, a):
        """name the memory of `a` (array, tensor, dict of them, ctypes struct); -> a"""
        if isinstance(a, dict):
            for k, v in a.items():
                reg("%s.%s" % (name, k), v)
        elif isinstance(a, C.Structure):
            names.setdefault(C.addressof(a), name)
        elif a is not None:
            names.setdefault(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data, name)
        return a

    def snap(v):
        if hasattr(v, "_obj"):
            v = v._obj
        if isinstance(v, C.Structure):
            return {n: getattr(v, n) for n, _ in v._fields_}
        return v.value if isinstance(v, C._SimpleCData) else v

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("qlamd_"):
                raise AttributeError(name)

            def fn(*args):
                calls.append((name, [snap(v) for v in args]))
                return 0
            fn.__name__ = name
            return fn

    def resolve(v):
        if isinstance(v, dict):
            return {k: resolve(x) for k, x in v.items()}
        if isinstance(v, int) and not isinstance(v, bool) and v in names:
            return names[v]
        if isinstance(v, int) and v > 1 << 20:
            return "ctx" if v == 0xC0FFEE else "UNNAMED POINTER"
        if isinstance(v, float) and v != v:
            return "nan"
        return v

    def drive(label, fn, *args, **kwargs):
        """one wrapper call: what it handed to the library, with the result's arrays named as well"""
        del calls[:]
        try:
            out = fn(*args, **kwargs)
            if callable(out):                                  # a kept call: launched twice
                out(); out()
                out = None
            reg("out", out if isinstance(out, dict) else None)
            log.append([label, [[name, [resolve(v) for v in a]] for name, a in calls], sorted(out) if isinstance(out, dict) else None])
        except (ValueError, TypeError) as e:
            log.append([label, "raises " + type(e).__name__, None])
        names.clear()

    capi._lib = Recorder()
    ctx = capi.Context()
    ctx._h = C.c_void_p(0xC0FFEE)
    f64 = lambda *shape: np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 1.0  # noqa: E731
    onoff = (False, True)

    for B in (1, 5):
        def state(device):
            s = dict(q=f64(B, 12), qd=f64(B, 12), base_quat=f64(B, 4), base_linvel=f64(B, 3), base_angvel=f64(B, 3), base_pos=f64(B, 3),
                     stance=np.ones((B, 4), np.uint8), normals=f64(B, 12))
            return reg("state", {k: torch.from_numpy(v) for k, v in s.items()} if device else s)

        def arr(name, device, *shape, dtype=np.float64):
            a = np.ones(shape, dtype)
            return reg(name, torch.from_numpy(a) if device else a)

        # ---- the plant step, host form
        for full, with_dt, in_place, free, flag, cone in itertools.product(onoff, repeat=6):
            def opt(contacts=True):                            # (fresh arrays for every call: the names are per call)
                o = dict(free_flight=free, in_place=in_place, **(dict(dt=0.002) if with_dt else {}))
                if full:
                    o.update(g_ext=arr("g_ext", False, B, 18), gravity=3.5)
                    if contacts:
                        o.update(prev_stance=arr("prev", False, B, 4, dtype=np.uint8), velocity_gain=400.0)
                return o
            label = "B%d full%d dt%d in_place%d free%d flag%d cone%d" % (B, full, with_dt, in_place, free, flag, cone)
            if not cone:
                if flag:
                    drive("forward_dynamics " + label, capi.wholebody_forward_dynamics, ctx, state(False), arr("tau", False, B, 12), **opt(False))
                drive("plant_step " + label, PC.wholebody_plant_step, ctx, state(False), arr("tau", False, B, 12), contacts=flag,
                      **opt(), **(dict(friction=0.6) if full else dict(want=("impulse",))))
                drive("plant_step_friction " + label, PF.wholebody_plant_step_friction, ctx, state(False), arr("tau", False, B, 12), 0.6,
                      with_friction=flag, **opt(), **({} if full else dict(want=("report",))))
            drive("plant_step_anchored " + label, CA.wholebody_plant_step_anchored, ctx, state(False), arr("tau", False, B, 12),
                  arr("anchor", False, B, 12), 1600.0, with_anchor=flag, cone=cone, **opt(),
                  **(dict(max_error=0.01, friction=0.6) if full else dict(want=("position_error",))))
        drive("plant_step_anchored B%d no anchor" % B, CA.wholebody_plant_step_anchored, ctx, state(False), arr("tau", False, B, 12), None, 2.0)
        drive("plant_step B%d bad prev" % B, PC.wholebody_plant_step, ctx, state(False), arr("tau", False, B, 12),
              prev_stance=np.ones((B + 1, 4), np.uint8))

        # ---- the plant step, device form: next = none / the state itself / apart
        for full, nxt, free, flag, cone in itertools.product(onoff, (None, "state", "apart"), onoff, onoff, onoff):
            label = "B%d full%d next-%s free%d flag%d cone%d" % (B, full, nxt, free, flag, cone)

            def args():
                d = state(True)
                o = dict(free_flight=free)
                if nxt:
                    o.update(dt=0.001, next=d if nxt == "state" else reg("next", {k: torch.from_numpy(f64(*v.shape)) for k, v in d.items()}))
                if full:
                    o.update(g_ext=arr("g_ext", True, B, 18), gravity=3.5, stream=0x5151, acc=arr("acc", True, B, 18), f=arr("f", True, B, 12))
                return (ctx, d, arr("tau", True, B, 12), arr("status", True, B, dtype=np.int32)), o

            def con(*keys):
                shapes = dict(prev_stance=(4, np.uint8), nu_plus=(18, np.float64), impulse=(12, np.float64), report=(4, np.uint8),
                              iterations=(2, np.int32), position_error=(12, np.float64))
                return dict({k: arr(k, True, B, shapes[k][0], dtype=shapes[k][1]) for k in keys}, velocity_gain=2.0) if full else {}
            if not cone:
                if flag:
                    a, o = args()
                    drive("forward_dynamics_device " + label, capi.wholebody_forward_dynamics_device, *a, **o)
                a, o = args()
                drive("plant_step_device " + label, PC.wholebody_plant_step_device, *a, contacts=flag, **o,
                      **con("prev_stance", "nu_plus", "impulse", "report"), **(dict(friction=0.5) if full else {}))
                a, o = args()
                drive("plant_step_friction_device " + label, PF.wholebody_plant_step_friction_device, *a, 0.7, with_friction=flag, **o,
                      **con("prev_stance", "nu_plus", "impulse", "report", "iterations"))
            for what, fn in (("anchored_device", CA.wholebody_plant_step_anchored_device), ("AnchoredPlantStepCall", CA.AnchoredPlantStepCall)):
                a, o = args()
                drive("plant_step_%s %s" % (what, label), fn, *a, arr("anchor", True, B, 12) if flag else None, 3.0, cone=cone, **o,
                      **con("prev_stance", "nu_plus", "impulse", "report", "iterations", "position_error"),
                      **(dict(max_error=0.02, friction=0.7) if full else {}))
        d = state(True)
        del d["base_pos"]
        drive("plant_step_anchored_device B%d no base_pos" % B, CA.wholebody_plant_step_anchored_device, ctx, d, arr("tau", True, B, 12),
              arr("status", True, B, dtype=np.int32), arr("anchor", True, B, 12), 3.0)
        drive("plant_step_friction_device B%d bad iterations" % B, PF.wholebody_plant_step_friction_device, ctx, state(True),
              arr("tau", True, B, 12), arr("status", True, B, dtype=np.int32), 0.7, iterations=torch.zeros(B, 2, dtype=torch.int64))

        # ---- the contact update: a plane / a height field / neither
        rule = dict(release_mask=3, touchdown_distance=0.01, approach_speed=0.2, liftoff_distance=0.03, sensor_distance=0.02)
        for full, terrain, in_place, flag in itertools.product(onoff, ("plane", "hf", None), onoff, onoff):
            label = "B%d full%d %s in_place%d flag%d" % (B, full, terrain, in_place, flag)

            def ground(device):
                if terrain == "plane":
                    return dict(plane=arr("plane", device, B, 4))
                return dict(hf=reg("hf", CD.heightfield((-1.0, 2.0), 0.05, arr("heights", device, 7, 9)))) if terrain else {}
            host = dict(report=arr("report", False, B, 4, dtype=np.uint8), **rule) if full else dict(want=("gap",))
            drive("contact_update " + label, CD.wholebody_contact_update, ctx, state(False), in_place=in_place, **ground(False), **host)
            host = dict(report=arr("report", False, B, 4, dtype=np.uint8), reanchor_mask=16, **rule) if full else dict(want=("gap",))
            drive("contact_update_anchored " + label, CA.wholebody_contact_update_anchored, ctx, state(False), arr("anchor", False, B, 12),
                  in_place=in_place, with_anchors=flag, **ground(False), **host)

            def dev(d):
                o = dict(support_next=d["stance"]) if in_place else {}
                if full:
                    o.update(report=arr("report", True, B, 4, dtype=np.uint8), stream=0x77, **rule)
                    for k, n, dtype in (("sensor", 4, np.uint8), ("events", 4, np.uint8), ("gap", 4, np.float64), ("normals", 12, np.float64),
                                        ("foot_pos", 12, np.float64), ("foot_vel", 12, np.float64)):
                        o[k] = arr(k, True, B, n, dtype=dtype)
                    if not in_place:
                        o["support_next"] = arr("support_next", True, B, 4, dtype=np.uint8)
                return o
            for what, fn in (("device", CD.wholebody_contact_update_device), ("ContactUpdateCall", CD.ContactUpdateCall)):
                d = state(True)
                drive("contact_update_%s %s" % (what, label), fn, ctx, d, arr("status", True, B, dtype=np.int32), **ground(True), **dev(d))
            for what, fn in (("anchored_device", CA.wholebody_contact_update_anchored_device), ("AnchoredContactUpdateCall", CA.AnchoredContactUpdateCall)):
                d = state(True)
                drive("contact_update_%s %s" % (what, label), fn, ctx, d, arr("status", True, B, dtype=np.int32),
                      arr("anchor", True, B, 12) if flag else None, **(dict(reanchor_mask=8) if full else {}), **ground(True), **dev(d))
        drive("contact_update B%d unknown rule" % B, CD.wholebody_contact_update, ctx, state(False), lift_distance=0.1)
        drive("contact_update_anchored_device B%d bad anchor" % B, CA.wholebody_contact_update_anchored_device, ctx, state(True),
              arr("status", True, B, dtype=np.int32), torch.zeros(B, 11, dtype=torch.float64))
    u = CD.default_update()
    log.append(["default_update", [[name, len(a)] for name, a in calls[-1:]], [n for n, _ in u._fields_]])
    ctx._h = C.c_void_p()
    json.dump(log, open(out_path, "w"), indent=0, sort_keys=True)
    launches = sum(len(c) for _, c, _ in log if isinstance(c, list))
    print("%s: %d wrapper calls, %d entry calls recorded, %d raised, %d unnamed pointers" % (
        tree, len(log), launches, sum(isinstance(c, str) for _, c, _ in log), json.dumps(log).count("UNNAMED POINTER")))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    differ = [x[0] for x, y in zip(a, b) if x != y]
    print("%d and %d wrapper calls compared; %d differ" % (len(a), len(b), len(differ) + abs(len(a) - len(b))))
    for label in differ[:20]:
        print("  differs:", label)
    return 1 if differ or len(a) != len(b) else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else main(*sys.argv[1:3]))

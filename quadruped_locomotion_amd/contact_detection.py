"""ctypes binding of include/qlamd_contact_detection.h (the part of the C-ABI that qlamd.h includes at its end, behind
qlamd_plant_contacts.h) -- ground contact detection for the plant: foot positions and velocities in the world, a terrain, the next
tick's support flags -- on the marshalling helpers of capi.py.  Plumbing only.  Its host marshalling (_host_update) and its kept
call (ContactUpdateCall) are contact_anchor.py's as well, whose entry takes one more struct.

The same layout as capi.py: the header's constants, its structs, its functions (SIGNATURES), the wrappers.
tests/test_contact_update_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

import numpy as np

from . import capi
from .plant_contacts import CONTACT_PULLS

# bits of qlamd_contact_update::events (QLAMD_<name> in the header)
CONTACT_EVENT_TOUCHDOWN, CONTACT_EVENT_RELEASED_PULL, CONTACT_EVENT_RELEASED_GAP = 1, 2, 4


class Heightfield(C.Structure):
    """qlamd_heightfield"""
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("resolution", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("heights", C.c_void_p)]


class ContactUpdate(C.Structure):
    """qlamd_contact_update"""
    _fields_ = [("plane", C.c_void_p), ("heightfield", C.c_void_p), ("contact_report", C.c_void_p), ("release_mask", C.c_uint8),
                ("touchdown_distance", C.c_double), ("approach_speed", C.c_double), ("liftoff_distance", C.c_double),
                ("sensor_distance", C.c_double), ("support_next", C.c_void_p), ("contact_sensor", C.c_void_p), ("events", C.c_void_p),
                ("gap", C.c_void_p), ("surface_normal", C.c_void_p), ("foot_position", C.c_void_p), ("foot_velocity", C.c_void_p)]


_p = C.c_void_p
SIGNATURES = {
    "qlamd_contact_update_default": (None, [_p]),
    "qlamd_wholebody_contact_update_batch": (C.c_int, [_p, _p, _p, _p, C.c_int64, _p, C.c_int, _p]),
}
EXPORTS = tuple(SIGNATURES)

# key of a result / argument -> (member of qlamd_contact_update, elements per robot, dtype)
OUTPUTS = (("support_next", "support_next", 4, np.uint8), ("sensor", "contact_sensor", 4, np.uint8), ("events", "events", 4, np.uint8),
           ("gap", "gap", 4, np.float64), ("normals", "surface_normal", 12, np.float64), ("foot_pos", "foot_position", 12, np.float64),
           ("foot_vel", "foot_velocity", 12, np.float64))
# key of the state dict -> elements per robot: what the entry reads (and "stance", optional)
STATE_KEYS = (("q", 12), ("qd", 12), ("base_quat", 4), ("base_linvel", 3), ("base_angvel", 3), ("base_pos", 3))
RULE = ("release_mask", "touchdown_distance", "approach_speed", "liftoff_distance", "sensor_distance")


def lib():
    """capi.lib() with this header's entries declared; a library without them is an error here (there is no fallback)."""
    return capi.declared(SIGNATURES)


def default_update():
    """A qlamd_contact_update as qlamd_contact_update_default leaves it."""
    u = ContactUpdate()
    lib().qlamd_contact_update_default(C.byref(u))
    return u


def heightfield(origin, resolution, heights):
    """qlamd_heightfield over `heights` [ny, nx] (a C-contiguous float64 numpy array, or a torch tensor for a device call)."""
    ny, nx = heights.shape
    if not capi._is(heights, "float64", nx * ny):
        raise ValueError("heights must be a contiguous float64 array [ny, nx]")
    return Heightfield(float(origin[0]), float(origin[1]), float(resolution), int(nx), int(ny), capi._ptr(heights))


def _update(B, plane, hf, report, rule, outputs):
    """The struct over arrays in the call's memory space, each checked before the library reads or writes behind its pointer.
    -> (ContactUpdate, keep-alives)"""
    for name, a, dtype, n in [("plane", plane, "float64", 4), ("report", report, "uint8", 4)] + [
            (key, outputs.get(key), np.dtype(dtype).name, n) for key, _, n, dtype in OUTPUTS]:
        if a is not None and not capi._is(a, dtype, n * B):
            raise ValueError("%s must be a contiguous %s array of %d x %d elements" % (name, dtype, B, n))
    unknown = set(rule) - set(RULE)
    if unknown:
        raise TypeError("unknown arguments: %s" % ", ".join(sorted(unknown)))
    u = ContactUpdate()
    u.release_mask = int(rule.get("release_mask", CONTACT_PULLS))
    for name in RULE[1:]:
        setattr(u, name, float(rule.get(name, 0.0)))
    u.plane, u.contact_report = capi._ptr(plane), capi._ptr(report)
    u.heightfield = C.addressof(hf) if hf is not None else None
    for key, member, _, _ in OUTPUTS:
        setattr(u, member, capi._ptr(outputs.get(key)))
    return u, [hf]


def _host_update(ctx, entry, anchors, state, plane, hf, report, want, in_place, rule):
    """The host form of both update entries: `entry` with the structs of `anchors` (none for this header's entry; one, or None for
    NULL, for contact_anchor.py's) between the update struct and the batch size."""
    B = state["q"].shape[0]
    keep = []
    st = {k: np.ascontiguousarray(state[k], dtype=np.float64) for k, _ in STATE_KEYS}
    for k, n in STATE_KEYS:
        if st[k].size != B * n:
            raise ValueError("state[%r] must be [%d, %d]" % (k, B, n))
    if state.get("stance") is not None:
        st["stance"] = state["stance"] if in_place else np.ascontiguousarray(state["stance"], dtype=np.uint8)
        if not capi._is(st["stance"], "uint8", 4 * B):
            raise ValueError("state['stance'] must be a contiguous uint8 array [%d, 4]" % B)
    wb = capi._wholebody_batch(st, keep)
    plane = None if plane is None else np.ascontiguousarray(plane, dtype=np.float64)
    report = None if report is None else np.ascontiguousarray(report, dtype=np.uint8)
    out = {key: np.zeros((B, n), dtype) for key, _, n, dtype in OUTPUTS if key in want}
    if in_place:
        if "stance" not in st:
            raise ValueError("in_place needs state['stance']")
        out["support_next"] = st["stance"]
    out["status"] = np.full(B, -1, np.int32)
    u, alive = _update(B, plane, hf, report, rule, out)
    capi._call(entry, ctx._h, C.byref(wb), capi._ptr(st["base_pos"]), C.byref(u), *[C.byref(a) if a is not None else None for a in anchors],
               B, capi._ptr(out["status"]), capi.MEM_HOST, None)
    del alive
    return out


def wholebody_contact_update(ctx, state, plane=None, hf=None, report=None, want=tuple(k for k, _, _, _ in OUTPUTS), in_place=False,
                             **rule):
    """qlamd_wholebody_contact_update_batch on host arrays.  state: q, qd [B,12], base_quat [B,4], base_linvel, base_angvel,
    base_pos [B,3] and, optionally, stance uint8 [B,4] (the current flags; absent: none flagged).  plane [B,4] or hf (heightfield())
    or neither (z = 0); report uint8 [B,4] or None; rule: release_mask, touchdown_distance, approach_speed, liftoff_distance,
    sensor_distance.  -> dict with status [B] and what `want` names: support_next, sensor, events uint8 [B,4], gap [B,4], normals,
    foot_pos, foot_vel [B,12].  in_place: support_next is state["stance"] itself."""
    return _host_update(ctx, lib().qlamd_wholebody_contact_update_batch, (), state, plane, hf, report, want, in_place, rule)


class ContactUpdateCall:
    """One checked device call of qlamd_wholebody_contact_update_batch, kept: calling it launches again on the same tensors with
    nothing re-checked or re-marshalled -- what a loop over ticks or a graph capture wants (the checks of
    wholebody_contact_update_device cost more host time than the launch).  Holds every tensor and struct it points to.
    (contact_anchor.AnchoredContactUpdateCall is this class with its own `_entry` and one struct in `_anchors`.)"""
    _anchors = ()                                               # the structs between the update struct and the batch size

    def _entry(self):
        return lib().qlamd_wholebody_contact_update_batch

    def __init__(self, ctx, dstate, status, plane=None, hf=None, report=None, stream=None, support_next=None, sensor=None, events=None,
                 gap=None, normals=None, foot_pos=None, foot_vel=None, **rule):
        B = dstate["q"].shape[0]
        for k, n in STATE_KEYS:
            if not capi._is(dstate[k], "float64", B * n):
                raise ValueError("dstate[%r] must be a contiguous float64 tensor of %d x %d elements" % (k, B, n))
        if dstate.get("stance") is not None and not capi._is(dstate["stance"], "uint8", 4 * B):
            raise ValueError("dstate['stance'] must be a contiguous uint8 tensor of %d x 4 elements" % B)
        if not capi._is(status, "int32", B):
            raise ValueError("status must be a contiguous int32 tensor of %d elements" % B)
        outputs = dict(support_next=support_next, sensor=sensor, events=events, gap=gap, normals=normals, foot_pos=foot_pos,
                       foot_vel=foot_vel)
        self._wb = capi._wholebody_batch({k: dstate.get(k) for k in [k for k, _ in STATE_KEYS[:5]] + ["stance"]}, [])
        self._update, _ = _update(B, plane, hf, report, rule, outputs)
        self._alive = (dict(dstate), status, plane, hf, report, outputs)
        self._args = (ctx._h, C.byref(self._wb), capi._ptr(dstate["base_pos"]), C.byref(self._update),
                      *[C.byref(a) if a is not None else None for a in self._anchors], B, capi._ptr(status), capi.MEM_DEVICE,
                      capi._stream(stream))
        self._fn = self._entry()

    def __call__(self):
        capi._call(self._fn, *self._args)


def wholebody_contact_update_device(ctx, dstate, status, plane=None, hf=None, report=None, stream=None, support_next=None, sensor=None,
                                    events=None, gap=None, normals=None, foot_pos=None, foot_vel=None, **rule):
    """Same entry on torch CUDA tensors; asynchronous.  dstate as the host form's state, on the device ("stance" optional);
    hf: heightfield() over a device tensor; outputs: preallocated tensors or None.  support_next may be dstate["stance"].
    (One ContactUpdateCall, made and called once.)"""
    ContactUpdateCall(ctx, dstate, status, plane=plane, hf=hf, report=report, stream=stream, support_next=support_next, sensor=sensor,
                      events=events, gap=gap, normals=normals, foot_pos=foot_pos, foot_vel=foot_vel, **rule)()

"""ctypes binding of include/qlamd_swing_task.h (the part of the C-ABI that qlamd.h brings in behind qlamd_contact_anchor.h) -- the
swing-foot task of the closed loop: schedule and footholds in, desired joint accelerations and the solve's support flags out, one
swing record per leg kept by the caller -- on the marshalling helpers of capi.py and contact_detection.py's state keys.  Plumbing
only.  One table (ARRAYS) declares every array of the struct and one function (_task) marshals it, for the host and the device
flavour alike.

The same layout as capi.py: the header's constants, its struct, its functions (SIGNATURES), the wrappers.
tests/test_swing_task_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

import numpy as np

from . import capi
from .contact_detection import STATE_KEYS

# bits of qlamd_swing_task::swing_events (QLAMD_<name> in the header)
SWING_EVENT_BEGAN, SWING_EVENT_LANDED, SWING_EVENT_LATE_LIFTOFF, SWING_EVENT_OVERTIME = 1, 2, 4, 8

SCALARS = ("swing_duration", "profile_height", "touchdown_speed", "touchdown_phase", "position_gain", "velocity_gain", "max_error",
           "damping", "max_joint_acceleration", "dt")
# what qlamd_swing_task_default leaves in them (dt is the caller's to set: the library refuses 0)
DEFAULTS = dict(swing_duration=0.45, profile_height=0.08, touchdown_speed=0.0, touchdown_phase=0.0, position_gain=0.0, velocity_gain=0.0,
                max_error=float("inf"), damping=0.0, max_joint_acceleration=float("inf"), dt=0.0)


class SwingTask(C.Structure):
    """qlamd_swing_task"""
    _fields_ = ([("swing_leg", C.c_void_p), ("foothold", C.c_void_p), ("surface_normal", C.c_void_p)] +
                [(name, C.c_double) for name in SCALARS] +
                [("swing_state", C.c_void_p), ("desired_joint_acceleration", C.c_void_p), ("support_solve", C.c_void_p),
                 ("foot_reference", C.c_void_p), ("swing_events", C.c_void_p)])


_p = C.c_void_p
SIGNATURES = {
    "qlamd_swing_task_default": (None, [_p]),
    "qlamd_wholebody_swing_task_batch": (C.c_int, [_p, _p, _p, _p, C.c_int64, _p, C.c_int, _p]),
}
EXPORTS = tuple(SIGNATURES)

# key of an argument / a result -> (member of qlamd_swing_task, elements per robot, dtype, required)
ARRAYS = (("swing_leg", "swing_leg", 4, np.uint8, True), ("foothold", "foothold", 12, np.float64, True),
          ("normals", "surface_normal", 12, np.float64, False), ("swing_state", "swing_state", 16, np.float64, True),
          ("qdd_des", "desired_joint_acceleration", 12, np.float64, True), ("support_solve", "support_solve", 4, np.uint8, False),
          ("foot_reference", "foot_reference", 36, np.float64, False), ("events", "swing_events", 4, np.uint8, False))
OUTPUTS = ARRAYS[4:]
# what the entry reads of the state dict beside contact_detection.STATE_KEYS, both optional: the detected flags, [v'_d ; w'_d]
STATE_OPTIONAL = (("stance", 4, "uint8"), ("a_des", 6, "float64"))


def lib():
    """capi.lib() with this header's entries declared; a library without them is an error here (there is no fallback)."""
    return capi.declared(SIGNATURES)


def default_task():
    """A qlamd_swing_task as qlamd_swing_task_default leaves it."""
    t = SwingTask()
    lib().qlamd_swing_task_default(C.byref(t))
    return t


def _task(B, arrays, scalars):
    """The struct over arrays in the call's memory space (by key of ARRAYS), each checked before the library reads or writes
    behind its pointer; scalars: members of SCALARS, the rest as qlamd_swing_task_default leaves them (DEFAULTS).  -> SwingTask"""
    unknown = set(scalars) - set(SCALARS)
    if unknown:
        raise TypeError("unknown arguments: %s" % ", ".join(sorted(unknown)))
    t = SwingTask()
    for name in SCALARS:
        setattr(t, name, float(scalars.get(name, DEFAULTS[name])))
    for key, member, n, dtype, required in ARRAYS:
        a = arrays.get(key)
        if a is None and required:
            raise ValueError("%s is required" % key)
        if a is not None and not capi._is(a, np.dtype(dtype).name, n * B):
            raise ValueError("%s must be a contiguous %s array of %d x %d elements" % (key, np.dtype(dtype).name, B, n))
        setattr(t, member, capi._ptr(a))
    return t


def wholebody_swing_task(ctx, state, swing_leg, foothold, swing_state, normals=None, want=tuple(k for k, _, _, _, _ in OUTPUTS[1:]),
                         in_place=False, **scalars):
    """qlamd_wholebody_swing_task_batch on host arrays.  state: q, qd [B,12], base_quat [B,4], base_linvel, base_angvel, base_pos
    [B,3] and, optionally, stance uint8 [B,4] (the detected flags; absent: none) and a_des [B,6] (absent: 0).  swing_leg uint8
    [B,4], foothold [B,12] (or [B,4,3]), normals the same or None; swing_state: a contiguous float64 array of B x 16 elements,
    updated in place; scalars: members of qlamd_swing_task (dt is required by the library).  -> dict with status [B], qdd_des
    [B,12] and what `want` names: support_solve, events uint8 [B,4], foot_reference [B,36].  in_place: support_solve is
    state["stance"] itself."""
    B = state["q"].shape[0]
    st = {k: np.ascontiguousarray(state[k], dtype=np.float64) for k, _ in STATE_KEYS}
    for k, n in STATE_KEYS:
        if st[k].size != B * n:
            raise ValueError("state[%r] must be [%d, %d]" % (k, B, n))
    for k, n, dtype in STATE_OPTIONAL:
        if state.get(k) is not None:
            st[k] = state[k] if in_place and k == "stance" else np.ascontiguousarray(state[k], dtype=dtype)
            if not capi._is(st[k], dtype, n * B):
                raise ValueError("state[%r] must be a contiguous %s array [%d, %d]" % (k, dtype, B, n))
    keep = []
    wb = capi._wholebody_batch(st, keep)
    arrays = dict(swing_leg=np.ascontiguousarray(swing_leg, dtype=np.uint8), foothold=np.ascontiguousarray(foothold, dtype=np.float64),
                  normals=None if normals is None else np.ascontiguousarray(normals, dtype=np.float64), swing_state=swing_state)
    out = {key: np.zeros((B, n), dtype) for key, _, n, dtype, required in OUTPUTS if required or key in want}
    if in_place:
        if "stance" not in st:
            raise ValueError("in_place needs state['stance']")
        out["support_solve"] = st["stance"]
    out["status"] = np.full(B, -1, np.int32)
    task = _task(B, dict(arrays, **out), scalars)
    capi._call(lib().qlamd_wholebody_swing_task_batch, ctx._h, C.byref(wb), capi._ptr(st["base_pos"]), C.byref(task), B,
               capi._ptr(out["status"]), capi.MEM_HOST, None)
    del keep, arrays
    return out


class SwingTaskCall:
    """One checked device call of qlamd_wholebody_swing_task_batch, kept: calling it launches again on the same tensors with
    nothing re-checked or re-marshalled -- what a loop over ticks or a graph capture wants.  Holds every tensor and struct it
    points to.  Arguments as wholebody_swing_task_device's."""

    def __init__(self, ctx, dstate, status, swing_leg, foothold, swing_state, qdd_des, normals=None, support_solve=None,
                 foot_reference=None, events=None, stream=None, **scalars):
        B = dstate["q"].shape[0]
        for k, n in STATE_KEYS:
            if not capi._is(dstate[k], "float64", B * n):
                raise ValueError("dstate[%r] must be a contiguous float64 tensor of %d x %d elements" % (k, B, n))
        for k, n, dtype in STATE_OPTIONAL:
            if dstate.get(k) is not None and not capi._is(dstate[k], dtype, n * B):
                raise ValueError("dstate[%r] must be a contiguous %s tensor of %d x %d elements" % (k, dtype, B, n))
        if not capi._is(status, "int32", B):
            raise ValueError("status must be a contiguous int32 tensor of %d elements" % B)
        arrays = dict(swing_leg=swing_leg, foothold=foothold, normals=normals, swing_state=swing_state, qdd_des=qdd_des,
                      support_solve=support_solve, foot_reference=foot_reference, events=events)
        self._wb = capi._wholebody_batch({k: dstate.get(k) for k in [k for k, _ in STATE_KEYS[:5]] + [k for k, _, _ in STATE_OPTIONAL]}, [])
        self._task = _task(B, arrays, scalars)
        self._alive = (dict(dstate), status, arrays)
        self._args = (ctx._h, C.byref(self._wb), capi._ptr(dstate["base_pos"]), C.byref(self._task), B, capi._ptr(status),
                      capi.MEM_DEVICE, capi._stream(stream))
        self._fn = lib().qlamd_wholebody_swing_task_batch

    def __call__(self):
        capi._call(self._fn, *self._args)


def wholebody_swing_task_device(ctx, dstate, status, swing_leg, foothold, swing_state, qdd_des, **kwargs):
    """Same entry on torch CUDA tensors; asynchronous.  dstate as the host form's state, on the device ("stance" and "a_des"
    optional); swing_state [B,16] float64, updated in place; qdd_des [B,12]; normals, support_solve, foot_reference, events:
    tensors or None; support_solve may be dstate["stance"].  (One SwingTaskCall, made and called once.)"""
    SwingTaskCall(ctx, dstate, status, swing_leg, foothold, swing_state, qdd_des, **kwargs)()

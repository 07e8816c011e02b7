"""ctypes binding of include/qlamd_contact_anchor.h (the part of the C-ABI that qlamd.h brings in behind qlamd_plant_friction.h) --
contact anchors for the plant: the contact update that keeps where each flagged foot is held, and the plant step that holds it
there -- on the marshalling helpers of capi.py and the structs of contact_detection.py, plant_contacts.py and plant_friction.py.
Plumbing only.

The same layout as capi.py: the header's constants, its structs, its functions (SIGNATURES), the wrappers.
tests/test_contact_anchor_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

import numpy as np

from . import capi
from . import contact_detection as CD
from .plant_contacts import OUTPUTS as CONTACT_OUTPUTS, PlantContacts
from .plant_friction import PlantFriction

# bit of qlamd_contact_update::events that this header adds (QLAMD_<name> in the header)
CONTACT_EVENT_REANCHORED = 8


class ContactAnchors(C.Structure):
    """qlamd_contact_anchors"""
    _fields_ = [("anchor", C.c_void_p), ("reanchor_mask", C.c_uint8)]


class PlantAnchor(C.Structure):
    """qlamd_plant_anchor"""
    _fields_ = [("anchor", C.c_void_p), ("position_gain", C.c_double), ("max_error", C.c_double), ("position_error", C.c_void_p)]


_p, _dbl = C.c_void_p, C.c_double
SIGNATURES = {
    "qlamd_wholebody_contact_update_anchored_batch": (C.c_int, [_p, _p, _p, _p, _p, C.c_int64, _p, C.c_int, _p]),
    "qlamd_wholebody_plant_step_anchored_batch": (C.c_int, [_p, _p, _p, _p, _p, _dbl, _dbl, C.c_int64, _p, _p, _p, _p, _p, _p, _p, C.c_int,
                                                            _p]),
}
EXPORTS = tuple(SIGNATURES)


def lib():
    """capi.lib() with this header's entries declared; a library without them is an error here (there is no fallback)."""
    L = capi.lib()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def _anchors(B, anchor, reanchor_mask):
    if anchor is None or not capi._is(anchor, "float64", 12 * B):
        raise ValueError("anchor must be a contiguous float64 array of %d x 12 elements" % B)
    return ContactAnchors(capi._ptr(anchor), int(reanchor_mask))


def _plant_anchor(B, anchor, position_gain, max_error, position_error):
    if anchor is None or not capi._is(anchor, "float64", 12 * B):
        raise ValueError("anchor must be a contiguous float64 array of %d x 12 elements" % B)
    if position_error is not None and not capi._is(position_error, "float64", 12 * B):
        raise ValueError("position_error must be a contiguous float64 array of %d x 12 elements" % B)
    return PlantAnchor(capi._ptr(anchor), float(position_gain), float(max_error), capi._ptr(position_error))


# ---------------------------------------------------------------------------------------------------------------- the update

def wholebody_contact_update_anchored(ctx, state, anchor, reanchor_mask=0, plane=None, hf=None, report=None,
                                      want=tuple(k for k, _, _, _ in CD.OUTPUTS), in_place=False, with_anchors=True, **rule):
    """qlamd_wholebody_contact_update_anchored_batch on host arrays: contact_detection.wholebody_contact_update's arguments and
    result, and anchor float64 [B,12] (or [B,4,3]), updated in place, with reanchor_mask the report bits that move a held foot's
    anchor.  with_anchors=False: the struct is NULL, which is contact_detection.wholebody_contact_update."""
    B = state["q"].shape[0]
    keep = []
    st = {k: np.ascontiguousarray(state[k], dtype=np.float64) for k, _ in CD.STATE_KEYS}
    for k, n in CD.STATE_KEYS:
        if st[k].size != B * n:
            raise ValueError("state[%r] must be [%d, %d]" % (k, B, n))
    if state.get("stance") is not None:
        st["stance"] = state["stance"] if in_place else np.ascontiguousarray(state["stance"], dtype=np.uint8)
        if not capi._is(st["stance"], "uint8", 4 * B):
            raise ValueError("state['stance'] must be a contiguous uint8 array [%d, 4]" % B)
    wb = capi._wholebody_batch(st, keep)
    plane = None if plane is None else np.ascontiguousarray(plane, dtype=np.float64)
    report = None if report is None else np.ascontiguousarray(report, dtype=np.uint8)
    out = {key: np.zeros((B, n), dtype) for key, _, n, dtype in CD.OUTPUTS if key in want}
    if in_place:
        if "stance" not in st:
            raise ValueError("in_place needs state['stance']")
        out["support_next"] = st["stance"]
    out["status"] = np.full(B, -1, np.int32)
    u, alive = CD._update(B, plane, hf, report, rule, out)
    ca = _anchors(B, anchor, reanchor_mask) if with_anchors else None
    capi._call(lib().qlamd_wholebody_contact_update_anchored_batch, ctx._h, C.byref(wb), capi._ptr(st["base_pos"]), C.byref(u),
               C.byref(ca) if ca is not None else None, B, capi._ptr(out["status"]), capi.MEM_HOST, None)
    del alive
    return out


class AnchoredContactUpdateCall:
    """One checked device call of qlamd_wholebody_contact_update_anchored_batch, kept, as contact_detection.ContactUpdateCall:
    calling it launches again on the same tensors with nothing re-checked or re-marshalled.  anchor: float64 tensor of B x 12
    elements, updated in place (None: the struct is NULL).  Holds every tensor and struct it points to."""

    def __init__(self, ctx, dstate, status, anchor, reanchor_mask=0, plane=None, hf=None, report=None, stream=None, support_next=None,
                 sensor=None, events=None, gap=None, normals=None, foot_pos=None, foot_vel=None, **rule):
        B = dstate["q"].shape[0]
        for k, n in CD.STATE_KEYS:
            if not capi._is(dstate[k], "float64", B * n):
                raise ValueError("dstate[%r] must be a contiguous float64 tensor of %d x %d elements" % (k, B, n))
        if dstate.get("stance") is not None and not capi._is(dstate["stance"], "uint8", 4 * B):
            raise ValueError("dstate['stance'] must be a contiguous uint8 tensor of %d x 4 elements" % B)
        if not capi._is(status, "int32", B):
            raise ValueError("status must be a contiguous int32 tensor of %d elements" % B)
        outputs = dict(support_next=support_next, sensor=sensor, events=events, gap=gap, normals=normals, foot_pos=foot_pos,
                       foot_vel=foot_vel)
        self._wb = capi._wholebody_batch({k: dstate.get(k) for k in [k for k, _ in CD.STATE_KEYS[:5]] + ["stance"]}, [])
        self._update, _ = CD._update(B, plane, hf, report, rule, outputs)
        self._anchors = _anchors(B, anchor, reanchor_mask) if anchor is not None else None
        self._alive = (dict(dstate), status, anchor, plane, hf, report, outputs)
        self._args = (ctx._h, C.byref(self._wb), capi._ptr(dstate["base_pos"]), C.byref(self._update),
                      C.byref(self._anchors) if self._anchors is not None else None, B, capi._ptr(status), capi.MEM_DEVICE,
                      capi._stream(stream))
        self._fn = lib().qlamd_wholebody_contact_update_anchored_batch

    def __call__(self):
        capi._call(self._fn, *self._args)


def wholebody_contact_update_anchored_device(ctx, dstate, status, anchor, **kwargs):
    """Same entry on torch CUDA tensors; asynchronous.  (One AnchoredContactUpdateCall, made and called once.)"""
    AnchoredContactUpdateCall(ctx, dstate, status, anchor, **kwargs)()


# ------------------------------------------------------------------------------------------------------------ the plant step

def _entry():
    """the declared entry: what capi._plant_call is handed, so that it never reaches an undeclared function"""
    return lib().qlamd_wholebody_plant_step_anchored_batch


def wholebody_plant_step_anchored(ctx, state, tau, anchor, position_gain, max_error=float("inf"), friction=None, cone=False, g_ext=None,
                                  gravity=9.81, dt=None, free_flight=False, in_place=False, prev_stance=None, velocity_gain=0.0,
                                  want=("nu_plus", "impulse", "report", "iterations", "position_error"), with_anchor=True):
    """qlamd_wholebody_plant_step_anchored_batch on host buffers.  plant_contacts.wholebody_plant_step's arguments and result with
    anchor float64 [B,12] (world), position_gain k_p and max_error e_max; cone=True: the friction struct is given (friction = mu > 0
    is then the constraint, and iterations int32 [B,2] a result), else it is NULL (hard contacts; friction = mu or None for the
    report).  The result also has position_error [B,12] when `want` names it.  base_pos is passed with or without dt.
    with_anchor=False: the anchor struct is NULL, which is plant_friction.wholebody_plant_step_friction."""
    B = state["q"].shape[0]
    if prev_stance is not None:
        prev_stance = np.ascontiguousarray(prev_stance, dtype=np.uint8)
        if prev_stance.shape != (B, 4):
            raise ValueError("prev_stance must be [%d, 4]" % B)
    extra = {key: np.zeros((B, n), dtype) for key, _, n, dtype in CONTACT_OUTPUTS
             if key in want and (key != "report" or friction is not None)}
    pc = PlantContacts(capi._ptr(prev_stance), float(velocity_gain), float(friction) if friction is not None else 0.0,
                       *[capi._ptr(extra.get(key)) for key, _, _, _ in CONTACT_OUTPUTS])
    pf = None
    if cone:
        if "iterations" in want:
            extra["iterations"] = np.zeros((B, 2), np.int32)
        pf = PlantFriction(capi._ptr(extra.get("iterations")))
    pa = None
    if with_anchor:
        anchor = None if anchor is None else np.ascontiguousarray(anchor, dtype=np.float64)
        if "position_error" in want:
            extra["position_error"] = np.zeros((B, 12))
        pa = _plant_anchor(B, anchor, position_gain, max_error, extra.get("position_error"))
    # capi._plant_host's marshalling, with base_pos handed over whether or not there is a state update
    keep = []
    if in_place:
        for _, key, n in capi.PLANT_NEXT_FIELDS:
            a = state[key]
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.size == B * n):
                raise ValueError("in_place needs state[%r] as a C-contiguous float64 array of %d x %d" % (key, B, n))
    wb = capi._wholebody_batch(state, keep)
    if free_flight:
        wb.support_leg = None
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    g_ext = None if g_ext is None else np.ascontiguousarray(g_ext, dtype=np.float64)
    if tau.shape != (B, 12) or (g_ext is not None and g_ext.shape != (B, 18)):
        raise ValueError("tau must be [%d, 12] and g_ext [%d, 18]" % (B, B))
    out = dict(acc=np.zeros((B, 18)), f=np.zeros((B, 12)), status=np.full(B, -1, np.int32))
    out.update(extra)
    pos = state["base_pos"] if in_place else np.ascontiguousarray(state["base_pos"], dtype=np.float64)
    nxt = None
    if dt is not None:
        out["next"] = {key: (state[key] if in_place else np.zeros((B, n))) for _, key, n in capi.PLANT_NEXT_FIELDS}
        nxt = capi.PlantNext(*[capi._ptr(out["next"][key]) for _, key, _ in capi.PLANT_NEXT_FIELDS])
    capi._plant_call(ctx, wb, B, tau, g_ext, pos, float(gravity), float(dt) if dt is not None else 0.0, out["acc"], out["f"], nxt,
                     out["status"], capi.MEM_HOST, None, (_entry(), pc, pf, pa))
    return out


class AnchoredPlantStepCall:
    """One checked device call of qlamd_wholebody_plant_step_anchored_batch, kept: calling it launches again on the same tensors
    with nothing re-checked or re-marshalled.  Arguments as wholebody_plant_step_anchored_device's."""

    def __init__(self, ctx, dstate, tau, status, anchor, position_gain, max_error=float("inf"), friction=0.0, cone=False, acc=None, f=None,
                 g_ext=None, gravity=9.81, dt=0.0, next=None, free_flight=False, stream=None, prev_stance=None, velocity_gain=0.0,
                 nu_plus=None, impulse=None, report=None, iterations=None, position_error=None):
        B = dstate["q"].shape[0]
        for name, a, dtype, n in (("prev_stance", prev_stance, "uint8", 4), ("nu_plus", nu_plus, "float64", 18),
                                  ("impulse", impulse, "float64", 12), ("report", report, "uint8", 4),
                                  ("iterations", iterations, "int32", 2)):
            if a is not None and not capi._is(a, dtype, n * B):
                raise ValueError("%s must be a contiguous %s tensor of %d x %d elements" % (name, dtype, B, n))
        if dstate.get("base_pos") is None or not capi._is(dstate["base_pos"], "float64", 3 * B):
            raise ValueError("dstate['base_pos'] must be a contiguous float64 tensor of %d x 3 elements: this entry always reads it" % B)
        self._pc = PlantContacts(capi._ptr(prev_stance), float(velocity_gain), float(friction), capi._ptr(nu_plus), capi._ptr(impulse),
                                 capi._ptr(report))
        self._pf = PlantFriction(capi._ptr(iterations)) if cone else None
        self._pa = _plant_anchor(B, anchor, position_gain, max_error, position_error) if anchor is not None else None
        self._wb = capi._wholebody_batch(dstate, [])
        if free_flight:
            self._wb.support_leg = None
        self._nxt = None if next is None else capi.PlantNext(*[capi._ptr(next[key]) for _, key, _ in capi.PLANT_NEXT_FIELDS])
        self._alive = (dict(dstate), tau, status, anchor, acc, f, g_ext, next, prev_stance, nu_plus, impulse, report, iterations,
                       position_error)
        self._args = (ctx, self._wb, B, tau, g_ext, dstate["base_pos"], float(gravity), float(dt), acc, f, self._nxt, status,
                      capi.MEM_DEVICE, stream, (_entry(), self._pc, self._pf, self._pa))

    def __call__(self):
        capi._plant_call(*self._args)


def wholebody_plant_step_anchored_device(ctx, dstate, tau, status, anchor, position_gain, **kwargs):
    """Same entry on torch CUDA tensors; asynchronous.  plant_friction.wholebody_plant_step_friction_device's arguments (cone=True:
    the friction struct is given), anchor float64 B x 12 (None: the struct is NULL), position_gain, max_error and position_error:
    a preallocated output or None.  dstate needs "base_pos".  (One AnchoredPlantStepCall, made and called once.)"""
    AnchoredPlantStepCall(ctx, dstate, tau, status, anchor, position_gain, **kwargs)()

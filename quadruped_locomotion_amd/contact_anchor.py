"""ctypes binding of include/qlamd_contact_anchor.h (the part of the C-ABI that qlamd.h brings in behind qlamd_plant_friction.h) --
contact anchors for the plant: the contact update that keeps where each flagged foot is held, and the plant step that holds it
there -- on the marshalling helpers of capi.py (capi._plant_host / capi._plant_device_args), contact_detection.py's update marshalling
and kept call, and plant_contacts._structs for the plant step's structs.  Plumbing only.

The same layout as capi.py: the header's constants, its structs, its functions (SIGNATURES), the wrappers.
tests/test_contact_anchor_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

from . import capi
from . import contact_detection as CD
from .plant_contacts import _structs
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
    return capi.declared(SIGNATURES)


def _anchors(B, anchor, reanchor_mask):
    if anchor is None or not capi._is(anchor, "float64", 12 * B):
        raise ValueError("anchor must be a contiguous float64 array of %d x 12 elements" % B)
    return ContactAnchors(capi._ptr(anchor), int(reanchor_mask))


# ---------------------------------------------------------------------------------------------------------------- the update

def wholebody_contact_update_anchored(ctx, state, anchor, reanchor_mask=0, plane=None, hf=None, report=None,
                                      want=tuple(k for k, _, _, _ in CD.OUTPUTS), in_place=False, with_anchors=True, **rule):
    """qlamd_wholebody_contact_update_anchored_batch on host arrays: contact_detection.wholebody_contact_update's arguments and
    result, and anchor float64 [B,12] (or [B,4,3]), updated in place, with reanchor_mask the report bits that move a held foot's
    anchor.  with_anchors=False: the struct is NULL, which is contact_detection.wholebody_contact_update."""
    ca = _anchors(state["q"].shape[0], anchor, reanchor_mask) if with_anchors else None
    return CD._host_update(ctx, lib().qlamd_wholebody_contact_update_anchored_batch, (ca,), state, plane, hf, report, want, in_place, rule)


class AnchoredContactUpdateCall(CD.ContactUpdateCall):
    """One checked device call of qlamd_wholebody_contact_update_anchored_batch, kept, as contact_detection.ContactUpdateCall:
    calling it launches again on the same tensors with nothing re-checked or re-marshalled.  anchor: float64 tensor of B x 12
    elements, updated in place (None: the struct is NULL).  Holds every tensor and struct it points to."""

    def _entry(self):
        return lib().qlamd_wholebody_contact_update_anchored_batch

    def __init__(self, ctx, dstate, status, anchor, reanchor_mask=0, plane=None, hf=None, report=None, stream=None, support_next=None,
                 sensor=None, events=None, gap=None, normals=None, foot_pos=None, foot_vel=None, **rule):
        self._anchors = (_anchors(dstate["q"].shape[0], anchor, reanchor_mask) if anchor is not None else None,)
        self._anchor = anchor
        super().__init__(ctx, dstate, status, plane, hf, report, stream, support_next, sensor, events, gap, normals, foot_pos, foot_vel,
                         **rule)


def wholebody_contact_update_anchored_device(ctx, dstate, status, anchor, **kwargs):
    """Same entry on torch CUDA tensors; asynchronous.  (One AnchoredContactUpdateCall, made and called once.)"""
    AnchoredContactUpdateCall(ctx, dstate, status, anchor, **kwargs)()


# ------------------------------------------------------------------------------------------------------------ the plant step

def wholebody_plant_step_anchored(ctx, state, tau, anchor, position_gain, max_error=float("inf"), friction=None, cone=False, g_ext=None,
                                  gravity=9.81, dt=None, free_flight=False, in_place=False, prev_stance=None, velocity_gain=0.0,
                                  want=("nu_plus", "impulse", "report", "iterations", "position_error"), with_anchor=True):
    """qlamd_wholebody_plant_step_anchored_batch on host buffers.  plant_contacts.wholebody_plant_step's arguments and result with
    anchor float64 [B,12] (world), position_gain k_p and max_error e_max; cone=True: the friction struct is given (friction = mu > 0
    is then the constraint, and iterations int32 [B,2] a result), else it is NULL (hard contacts; friction = mu or None for the
    report).  The result also has position_error [B,12] when `want` names it.  base_pos is passed with or without dt.
    with_anchor=False: the anchor struct is NULL, which is plant_friction.wholebody_plant_step_friction."""
    structs, extra = _structs(state["q"].shape[0], friction, velocity_gain, dict(prev_stance=prev_stance, anchor=anchor), want,
                              PlantFriction if cone else None, PlantAnchor if with_anchor else None, position_gain, max_error)
    return capi._plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, lib().qlamd_wholebody_plant_step_anchored_batch,
                            structs, extra, pos_always=True)


class AnchoredPlantStepCall:
    """One checked device call of qlamd_wholebody_plant_step_anchored_batch, kept: calling it launches again on the same tensors
    with nothing re-checked or re-marshalled.  Arguments as wholebody_plant_step_anchored_device's."""

    def __init__(self, ctx, dstate, tau, status, anchor, position_gain, max_error=float("inf"), friction=0.0, cone=False, acc=None, f=None,
                 g_ext=None, gravity=9.81, dt=0.0, next=None, free_flight=False, stream=None, prev_stance=None, velocity_gain=0.0,
                 nu_plus=None, impulse=None, report=None, iterations=None, position_error=None):
        arrays = dict(prev_stance=prev_stance, nu_plus=nu_plus, impulse=impulse, report=report, iterations=iterations,
                      position_error=position_error, anchor=anchor)
        structs, _ = _structs(dstate["q"].shape[0], float(friction), velocity_gain, arrays, None, PlantFriction if cone else None,
                              PlantAnchor if anchor is not None else None, position_gain, max_error)
        self._alive = (dict(dstate), next, arrays)
        self._args = capi._plant_device_args(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream,
                                             lib().qlamd_wholebody_plant_step_anchored_batch, structs, pos_always=True)

    def __call__(self):
        capi._plant_call(*self._args)


def wholebody_plant_step_anchored_device(ctx, dstate, tau, status, anchor, position_gain, **kwargs):
    """Same entry on torch CUDA tensors; asynchronous.  plant_friction.wholebody_plant_step_friction_device's arguments (cone=True:
    the friction struct is given), anchor float64 B x 12 (None: the struct is NULL), position_gain, max_error and position_error:
    a preallocated output or None.  dstate needs "base_pos".  (One AnchoredPlantStepCall, made and called once.)"""
    AnchoredPlantStepCall(ctx, dstate, tau, status, anchor, position_gain, **kwargs)()

"""ctypes binding of include/qlamd_plant_contacts.h (the part of the C-ABI that qlamd.h includes at its end) -- the plant step with touchdown impacts, contact stabilisation and a contact
report -- on the marshalling helpers of capi.py (one path: capi._plant_host / capi._plant_device_args).  Plumbing only.

The same layout as capi.py: the header's constants, its struct, its function (SIGNATURES), the wrappers.  This module is the
base of the plant modules' chain (plant_friction.py, contact_anchor.py): OPTIONAL and _structs() are theirs as well.
tests/test_plant_contacts_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

import numpy as np

from . import capi

# bits of qlamd_plant_contacts::contact_report (QLAMD_<name> in the header)
CONTACT_PULLS, CONTACT_OUTSIDE_CONE, CONTACT_TOUCHDOWN = 1, 2, 4


class PlantContacts(C.Structure):
    """qlamd_plant_contacts"""
    _fields_ = [("previous_support_leg", C.c_void_p), ("velocity_gain", C.c_double), ("friction_coefficient", C.c_double),
                ("post_impact_velocity", C.c_void_p), ("impulse", C.c_void_p), ("contact_report", C.c_void_p)]


_p, _dbl = C.c_void_p, C.c_double
SIGNATURES = {
    "qlamd_wholebody_plant_step_batch": (C.c_int, [_p, _p, _p, _p, _p, _dbl, _dbl, C.c_int64, _p, _p, _p, _p, _p, C.c_int, _p]),
}
EXPORTS = tuple(SIGNATURES)

# key of a result / argument -> (member of qlamd_plant_contacts, elements per robot, dtype)
OUTPUTS = (("nu_plus", "post_impact_velocity", 18, np.float64), ("impulse", "impulse", 12, np.float64),
           ("report", "contact_report", 4, np.uint8))
# every optional array of the plant entries, by the wrappers' keyword -> (dtype, elements per robot): the members of this
# header's struct, of plant_friction.py's (iterations) and of contact_anchor.py's (position_error, anchor)
OPTIONAL = dict(prev_stance=("uint8", 4), nu_plus=("float64", 18), impulse=("float64", 12), report=("uint8", 4), iterations=("int32", 2),
                position_error=("float64", 12), anchor=("float64", 12))


def lib():
    """capi.lib() with this header's entry declared; a library without it is an error here (there is no fallback)."""
    return capi.declared(SIGNATURES)


def _structs(B, friction, velocity_gain, arrays, want=None, friction_struct=None, anchor_struct=None, position_gain=0.0, max_error=0.0):
    """The optional structs of a plant entry from a wrapper's keyword arguments.  arrays: a dict of what was handed in, by key
    of OPTIONAL (None or absent: not given); the host flavour fills it in.  The device flavour (want=None) checks it; the host
    flavour converts the inputs first and allocates the outputs `want` names, the report only with a friction coefficient,
    iterations and position_error only with their struct; anything handed in is checked before the library gets its pointer.
    friction_struct / anchor_struct: plant_friction.PlantFriction / contact_anchor.PlantAnchor where the entry is to get that
    struct (it then needs `anchor`), else NULL.  -> ((PlantContacts, friction struct or None, anchor struct or None), outputs)"""
    a, out, get = arrays, {}, arrays.get
    if want is not None:
        if get("prev_stance") is not None:
            a["prev_stance"] = np.ascontiguousarray(a["prev_stance"], dtype=np.uint8)
            if a["prev_stance"].shape != (B, 4):
                raise ValueError("prev_stance must be [%d, 4]" % B)
        if anchor_struct is not None and get("anchor") is not None:
            a["anchor"] = np.ascontiguousarray(a["anchor"], dtype=np.float64)
        given = [key for key, _, _, _ in OUTPUTS if key != "report" or friction is not None]
        given += ["iterations"] * (friction_struct is not None) + ["position_error"] * (anchor_struct is not None)
        out = {key: np.zeros((B, OPTIONAL[key][1]), OPTIONAL[key][0]) for key in given if key in want}
        a.update(out)
    for key, x in a.items():
        dtype, n = OPTIONAL[key]
        if not capi._is(x, dtype, n * B) if x is not None else key == "anchor" and anchor_struct is not None:
            raise ValueError("%s must be contiguous %s, %d x %d elements" % (key, dtype, B, n))
    ptr = capi._ptr
    pc = PlantContacts(ptr(get("prev_stance")), float(velocity_gain), float(friction) if friction is not None else 0.0,
                       ptr(get("nu_plus")), ptr(get("impulse")), ptr(get("report")))
    if want is not None:
        pc._arrays = a                                         # (converted inputs live as long as the struct that points to them)
    pf = friction_struct(ptr(get("iterations"))) if friction_struct is not None else None
    pa = None
    if anchor_struct is not None:
        pa = anchor_struct(ptr(get("anchor")), float(position_gain), float(max_error), ptr(get("position_error")))
    return (pc, pf, pa), out


def wholebody_plant_step(ctx, state, tau, g_ext=None, gravity=9.81, dt=None, free_flight=False, in_place=False, prev_stance=None,
                         velocity_gain=0.0, friction=None, want=("nu_plus", "impulse", "report"), contacts=True):
    """qlamd_wholebody_plant_step_batch on host buffers: capi.wholebody_forward_dynamics's arguments and result, and
    prev_stance uint8 [B,4] or None (no touchdown), velocity_gain k_v, friction mu (None: no report).  The result also holds what
    `want` names: nu_plus [B,18], impulse [B,12], report uint8 [B,4] (CONTACT_* bits; only with friction).  state["normals"], when
    present, are the world normals of the report.  contacts=False: the struct is NULL, which is capi.wholebody_forward_dynamics."""
    structs, extra = (None,), None
    if contacts:
        structs, extra = _structs(state["q"].shape[0], friction, velocity_gain, dict(prev_stance=prev_stance), want)
    return capi._plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, lib().qlamd_wholebody_plant_step_batch,
                            structs[:1], extra)


def wholebody_plant_step_device(ctx, dstate, tau, status, acc=None, f=None, g_ext=None, gravity=9.81, dt=0.0, next=None,
                                free_flight=False, stream=None, prev_stance=None, velocity_gain=0.0, friction=0.0, nu_plus=None,
                                impulse=None, report=None, contacts=True):
    """Same entry on torch CUDA tensors; asynchronous.  prev_stance uint8 [B,4]; nu_plus [B,18], impulse [B,12] float64 and report
    uint8 [B,4]: preallocated outputs or None.  dstate["normals"], when present, are the world normals of the report."""
    (pc, _, _), _ = _structs(dstate["q"].shape[0], friction, velocity_gain,
                             dict(prev_stance=prev_stance, nu_plus=nu_plus, impulse=impulse, report=report))
    capi._plant_call(*capi._plant_device_args(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream,
                                              lib().qlamd_wholebody_plant_step_batch, (pc if contacts else None,)))

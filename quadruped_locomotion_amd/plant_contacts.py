"""ctypes binding of include/qlamd_plant_contacts.h (the part of the C-ABI that qlamd.h includes at its end) -- the plant step with touchdown impacts, contact stabilisation and a contact
report -- on the marshalling helpers of capi.py (one path: capi._plant_host / capi._plant_device).  Plumbing only.

The same layout as capi.py: the header's constants, its struct, its function (SIGNATURES), the wrappers.
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


def lib():
    """capi.lib() with this header's entry declared; a library without it is an error here (there is no fallback)."""
    L = capi.lib()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def _entry():
    """the declared entry: what capi._plant_call is handed, so that it never reaches an undeclared function"""
    return lib().qlamd_wholebody_plant_step_batch


def wholebody_plant_step(ctx, state, tau, g_ext=None, gravity=9.81, dt=None, free_flight=False, in_place=False, prev_stance=None,
                         velocity_gain=0.0, friction=None, want=("nu_plus", "impulse", "report"), contacts=True):
    """qlamd_wholebody_plant_step_batch on host buffers: capi.wholebody_forward_dynamics's arguments and result, and
    prev_stance uint8 [B,4] or None (no touchdown), velocity_gain k_v, friction mu (None: no report).  The result also holds what
    `want` names: nu_plus [B,18], impulse [B,12], report uint8 [B,4] (CONTACT_* bits; only with friction).  state["normals"], when
    present, are the world normals of the report.  contacts=False: the struct is NULL, which is capi.wholebody_forward_dynamics."""
    if not contacts:
        return capi._plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, contacts=(_entry(), None))
    B = state["q"].shape[0]
    if prev_stance is not None:
        prev_stance = np.ascontiguousarray(prev_stance, dtype=np.uint8)
        if prev_stance.shape != (B, 4):
            raise ValueError("prev_stance must be [%d, 4]" % B)
    extra = {key: np.zeros((B, n), dtype) for key, _, n, dtype in OUTPUTS if key in want and (key != "report" or friction is not None)}
    pc = PlantContacts(capi._ptr(prev_stance), float(velocity_gain), float(friction) if friction is not None else 0.0,
                       *[capi._ptr(extra.get(key)) for key, _, _, _ in OUTPUTS])
    return capi._plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, contacts=(_entry(), pc), extra=extra)


def wholebody_plant_step_device(ctx, dstate, tau, status, acc=None, f=None, g_ext=None, gravity=9.81, dt=0.0, next=None,
                                free_flight=False, stream=None, prev_stance=None, velocity_gain=0.0, friction=0.0, nu_plus=None,
                                impulse=None, report=None, contacts=True):
    """Same entry on torch CUDA tensors; asynchronous.  prev_stance uint8 [B,4]; nu_plus [B,18], impulse [B,12] float64 and report
    uint8 [B,4]: preallocated outputs or None.  dstate["normals"], when present, are the world normals of the report."""
    B = dstate["q"].shape[0]
    for name, a, dtype, n in (("prev_stance", prev_stance, "uint8", 4), ("nu_plus", nu_plus, "float64", 18),
                              ("impulse", impulse, "float64", 12), ("report", report, "uint8", 4)):
        if a is not None and not capi._is(a, dtype, n * B):
            raise ValueError("%s must be a contiguous %s tensor of %d x %d elements" % (name, dtype, B, n))
    pc = None
    if contacts:
        pc = PlantContacts(capi._ptr(prev_stance), float(velocity_gain), float(friction), capi._ptr(nu_plus), capi._ptr(impulse),
                           capi._ptr(report))
    capi._plant_device(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream, contacts=(_entry(), pc))

"""ctypes binding of include/qlamd_plant_friction.h (the part of the C-ABI that qlamd.h includes at its end) -- the plant step with
friction: contact impulses and forces inside the friction pyramid -- on the marshalling helpers of capi.py (one path:
capi._plant_host / capi._plant_device_args) and the structs of plant_contacts.py (one place: plant_contacts._structs).  Plumbing only.

The same layout as capi.py: the header's constants, its struct, its function (SIGNATURES), the wrappers.
tests/test_plant_friction_cpu.py holds all of them against the header and the C compiler."""
import ctypes as C

from . import capi
from .plant_contacts import _structs, CONTACT_TOUCHDOWN  # noqa: F401  (the report byte is shared)

# bits of qlamd_plant_contacts::contact_report that this entry adds (QLAMD_<name> in the header)
CONTACT_SEPARATING, CONTACT_SLIDING = 8, 16


class PlantFriction(C.Structure):
    """qlamd_plant_friction"""
    _fields_ = [("iterations", C.c_void_p)]


_p, _dbl = C.c_void_p, C.c_double
SIGNATURES = {
    "qlamd_wholebody_plant_step_friction_batch": (C.c_int, [_p, _p, _p, _p, _p, _dbl, _dbl, C.c_int64, _p, _p, _p, _p, _p, _p, C.c_int, _p]),
}
EXPORTS = tuple(SIGNATURES)


def lib():
    """capi.lib() with this header's entry declared; a library without it is an error here (there is no fallback)."""
    return capi.declared(SIGNATURES)


def wholebody_plant_step_friction(ctx, state, tau, friction, g_ext=None, gravity=9.81, dt=None, free_flight=False, in_place=False,
                                  prev_stance=None, velocity_gain=0.0, want=("nu_plus", "impulse", "report", "iterations"),
                                  with_friction=True):
    """qlamd_wholebody_plant_step_friction_batch on host buffers: plant_contacts.wholebody_plant_step's arguments and result, with
    friction = mu > 0 the constraint; the report holds CONTACT_TOUCHDOWN / CONTACT_SEPARATING / CONTACT_SLIDING and the result also
    has iterations int32 [B,2] (impulse QP, force QP) when `want` names it.  with_friction=False: the friction struct is NULL,
    which is plant_contacts.wholebody_plant_step with the same contacts struct."""
    structs, extra = _structs(state["q"].shape[0], float(friction), velocity_gain, dict(prev_stance=prev_stance), want,
                              PlantFriction if with_friction else None)
    return capi._plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, lib().qlamd_wholebody_plant_step_friction_batch,
                            structs[:2], extra)


def wholebody_plant_step_friction_device(ctx, dstate, tau, status, friction, acc=None, f=None, g_ext=None, gravity=9.81, dt=0.0,
                                         next=None, free_flight=False, stream=None, prev_stance=None, velocity_gain=0.0, nu_plus=None,
                                         impulse=None, report=None, iterations=None, with_friction=True):
    """Same entry on torch CUDA tensors; asynchronous.  plant_contacts.wholebody_plant_step_device's arguments, friction = mu > 0,
    and iterations int32 [B,2]: a preallocated output or None."""
    structs, _ = _structs(dstate["q"].shape[0], float(friction), velocity_gain,
                          dict(prev_stance=prev_stance, nu_plus=nu_plus, impulse=impulse, report=report, iterations=iterations),
                          friction_struct=PlantFriction if with_friction else None)
    capi._plant_call(*capi._plant_device_args(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream,
                                              lib().qlamd_wholebody_plant_step_friction_batch, structs[:2]))

"""The record of check 6 of profiles/r18/binding_fold.md: host time per call of the device wrappers, a recorder in the place of the
library and CPU torch tensors in the place of device tensors.  10 000 calls per repeat, 5 repeats; median and spread (largest
minus smallest repeat) in microseconds per call.

    python host_time.py <tree>                      one process per tree (the parent's checkout, this one)"""
import ctypes as C
import sys
import time

import numpy as np

CALLS, REPEATS, B = 10000, 5, 5


def main(tree):
    sys.path.insert(0, tree)
    import torch
    from quadruped_locomotion_amd import capi, contact_anchor as CA, contact_detection as CD, plant_contacts as PC, plant_friction as PF

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("qlamd_"):
                raise AttributeError(name)

            def fn(*args):
                return 0
            fn.__name__ = name
            return fn

    capi._lib = Recorder()
    ctx = capi.Context()
    ctx._h = C.c_void_p(0xC0FFEE)
    t = lambda n, dtype=torch.float64: torch.ones(B, n, dtype=dtype)  # noqa: E731
    d = dict(q=t(12), qd=t(12), base_quat=t(4), base_linvel=t(3), base_angvel=t(3), base_pos=t(3), stance=t(4, torch.uint8), normals=t(12))
    tau, st, anchor, iters = t(12), torch.zeros(B, dtype=torch.int32), t(12), t(2, torch.int32)
    con = dict(prev_stance=t(4, torch.uint8), velocity_gain=400.0, nu_plus=t(18), impulse=t(12), report=t(4, torch.uint8))
    step = dict(dt=0.0025, next=d, stream=0x5151)
    upd = dict(plane=t(4), report=con["report"], support_next=d["stance"], events=t(4, torch.uint8), gap=t(4), liftoff_distance=0.01,
               stream=0x5151)
    kept_update = CD.ContactUpdateCall(ctx, d, st, **upd)
    kept_step = CA.AnchoredPlantStepCall(ctx, d, tau, st, anchor, 16000.0, max_error=0.01, friction=0.6, cone=True, iterations=t(2, torch.int32),
                                         position_error=t(12), **step, **con)
    cases = (
        ("wholebody_plant_step_device", lambda: PC.wholebody_plant_step_device(ctx, d, tau, st, friction=0.6, **step, **con)),
        ("wholebody_plant_step_friction_device",
         lambda: PF.wholebody_plant_step_friction_device(ctx, d, tau, st, 0.6, iterations=iters, **step, **con)),
        ("wholebody_plant_step_anchored_device",
         lambda: CA.wholebody_plant_step_anchored_device(ctx, d, tau, st, anchor, 16000.0, max_error=0.01, friction=0.6, cone=True, **step, **con)),
        ("wholebody_contact_update_device", lambda: CD.wholebody_contact_update_device(ctx, d, st, **upd)),
        ("ContactUpdateCall.__call__", kept_update),
        ("AnchoredPlantStepCall.__call__", kept_step),
    )
    for name, fn in cases:
        for _ in range(1000):
            fn()
        us = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            us.append((time.perf_counter() - t0) / CALLS * 1e6)
        print("%-40s median %7.3f us  spread %6.3f us  (%s)" % (name, float(np.median(us)), max(us) - min(us), " ".join("%.3f" % u for u in us)))
    ctx._h = C.c_void_p()


if __name__ == "__main__":
    main(sys.argv[1])

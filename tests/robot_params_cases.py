"""Inputs shared by tests/test_robot_params_cpu.py and tests/test_robot_params_gpu.py: the batches the GPU tests of
qlamd_balance_solve_robot_params_batch solve, every robot with its own synth.make_robot_params draw, and their oracle results,
robot by robot (oracle.balance_step takes its parameters per call), computed once per process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from quadruped_locomotion_amd import synth  # noqa: E402

B = 1024          # 256 wavefronts: every lane pattern; the workload's 4096 adds nothing
MASK_ROBOTS = 37  # per stance mask, as tests/test_balance_gpu.py draws them (37 robots of the trot batch, all 16 masks)


def normals_for(batch, seed=5):
    """Per-leg surface normals up to ~20 degrees off vertical (the draw of tests/test_balance_gpu.py)."""
    rng = np.random.default_rng(seed)
    nw = np.tile(np.array([0, 0, 1.0]), (batch, 4, 1)) + 0.15 * rng.normal(size=(batch, 4, 3))
    nw /= np.linalg.norm(nw, axis=2, keepdims=True)
    return np.ascontiguousarray(nw.reshape(batch, 12))


def mask_states():
    """All 16 stance masks, MASK_ROBOTS robots each: robots [37 m, 37 m + 37) stand on the legs of mask m."""
    base = synth.make_states(MASK_ROBOTS, "trot")
    parts = []
    for mask in range(16):
        s = {k: v.copy() for k, v in base.items()}
        s["stance"][:] = [(mask >> l) & 1 for l in range(4)]
        parts.append(s)
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=0)) for k in base}


def states(name):
    if name == "static":
        return synth.make_states(B, "static", errors="survey")
    if name == "trot":
        return synth.make_states(B, "trot")
    if name == "masks":
        return mask_states()
    raise ValueError(name)


NAMES = ("static", "trot", "masks")
_cache = {}


def case(name, with_normals):
    """(state, normals or None, robot parameters) of one batch; the parameters are robot i's own draw whatever the batch."""
    s = states(name)
    n = s["q"].shape[0]
    return s, (normals_for(n) if with_normals else None), synth.make_robot_params(n)


def oracle_results(O, name, with_normals):
    """(tau [B, 12], grf [B, 12], status [B]) of the oracle, every robot under its own parameters."""
    key = (name, bool(with_normals))
    if key not in _cache:
        s, nw, rp = case(name, with_normals)
        n = s["q"].shape[0]
        tau, grf, status = np.zeros((n, 12)), np.zeros((n, 12)), np.zeros(n, dtype=np.int32)
        for i in range(n):
            r = O.balance_step(s, i, params=synth.robot_params_struct(rp, i, O.BalanceParams), normals_world=nw)
            tau[i], grf[i], status[i] = r["tau"], r["grf"], r["status"]
        for a in (tau, grf, status):
            a.setflags(write=False)
        _cache[key] = (tau, grf, status)
    return _cache[key]


def records(capi, rp):
    """The folded records [B, 32] of a make_robot_params dict."""
    n = rp["friction"].shape[0]
    return capi.robot_params_fill([synth.robot_params_struct(rp, i, capi.BalanceParams) for i in range(n)])

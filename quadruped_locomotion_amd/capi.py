"""ctypes binding of the C-ABI (include/qlamd.h) -- plumbing only.

The arithmetic lives in the HIP kernels of libqlamd.so.  There is no Python or
CPU fallback: a missing library or a missing GPU raises.

Layout of this file: the header's constants, its structs, its functions (SIGNATURES: the one place an entry's
restype / argtypes are written), then one helper per marshalling job, then the wrappers.  tests/test_capi_cpu.py holds
constants, struct layouts and signatures against the header and the C compiler.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libqlamd.so")

# ---- the constants of include/qlamd.h (QLAMD_<name> there), grouped as the header groups them ---------------------------
# return codes of the API calls
OK = 0
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_LOADED, ERR_OUT_OF_MEMORY, ERR_BUSY, ERR_NEEDS_RESERVE = -1, -2, -3, -4, -5, -6, -7
# per-robot status words
STATUS_OK, STATUS_INFEASIBLE, STATUS_NOT_PD, STATUS_MAX_ITER, STATUS_NO_COMMAND, STATUS_DEPENDENT_EQUALITY, STATUS_WARM_REJECTED = range(7)
# where caller buffers live
MEM_DEVICE, MEM_HOST = 0, 1
STATE_RECORD_DOUBLES = 48
# context options and their values
OPT_ON_FAILURE, OPT_REFINE_PASSES, OPT_DYNAMICS_FORM, OPT_PLACEMENT_WAIT, OPT_WARM_FALLBACK, OPT_STATE_LAYOUT = 1, 2, 5, 6, 7, 8
STATE_FIELDS, STATE_RECORDS = 0, 1
ON_FAILURE_ZERO, ON_FAILURE_KEEP = 0, 1
DYNAMICS_AUTO, DYNAMICS_LEG, DYNAMICS_ROW = 0, 1, 2
# event counters
COUNTER_PLACEMENT_GIVE_UPS, COUNTER_WARM_RETRIES = 0, 1
# placement policies
PLACEMENT_AUTO, PLACEMENT_LATENCY, PLACEMENT_THROUGHPUT, PLACEMENT_NONE = 0, 1, 2, 3
ROBOT_PARAMS_DOUBLES = 32
NO_BOUND = 1.7976931348623157e308   # std::numeric_limits<double>::max(): what the reference writes for "no bound"


# ---- the structs of include/qlamd.h, in its order: class <Name> mirrors qlamd_<name> -------------------------------------
class BalanceParams(C.Structure):
    _fields_ = [
        ("kp_trans", C.c_double * 3), ("kd_trans", C.c_double * 3), ("kff_trans", C.c_double * 3),
        ("kp_rot", C.c_double * 3), ("kd_rot", C.c_double * 3), ("kff_rot", C.c_double * 3),
        ("force_weights", C.c_double * 6),
        ("regularizer", C.c_double), ("friction", C.c_double), ("min_normal_force", C.c_double),
        ("torque_limit", C.c_double), ("torso_mass", C.c_double), ("leg_mass", C.c_double * 4),
        ("gravity", C.c_double), ("grav_comp_percentage", C.c_double),
        ("com_in_base", C.c_double * 3), ("hip_in_base", (C.c_double * 3) * 4),
    ]


class RobotModel(C.Structure):
    _fields_ = [
        ("joint_xyz", ((C.c_double * 3) * 4) * 4), ("joint_rpy", ((C.c_double * 3) * 4) * 4),
        ("link_mass", (C.c_double * 4) * 4), ("link_com", ((C.c_double * 3) * 4) * 4),
        ("link_inertia", ((C.c_double * 6) * 4) * 4),
        ("base_mass", C.c_double), ("base_com", C.c_double * 3), ("base_inertia", C.c_double * 6),
    ]


class StateBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "joint_position", "base_position", "base_orientation", "base_linear_velocity",
        "base_angular_velocity", "desired_position", "desired_orientation",
        "desired_linear_velocity", "desired_angular_velocity", "support_leg", "surface_normal")]


# state-dict key -> StateBatch field (keys as produced by synth.make_states)
FIELD_OF_KEY = (
    ("q", "joint_position", 12), ("base_pos", "base_position", 3), ("base_quat", "base_orientation", 4),
    ("base_linvel", "base_linear_velocity", 3), ("base_angvel", "base_angular_velocity", 3),
    ("des_pos", "desired_position", 3), ("des_quat", "desired_orientation", 4),
    ("des_linvel", "desired_linear_velocity", 3), ("des_angvel", "desired_angular_velocity", 3),
)
# offsets (doubles) of the fields inside a qlamd_state_record (include/qlamd.h), by the keys of synth.make_states
STATE_RECORD_OFFSETS = {"q": 0, "base_pos": 12, "base_quat": 16, "base_linvel": 20, "base_angvel": 23, "des_pos": 26, "des_quat": 30,
                        "des_linvel": 34, "des_angvel": 37}


class Placement(C.Structure):
    """qlamd_placement"""
    _fields_ = [("robot_order", C.c_void_p), ("iterations", C.c_void_p), ("prev_iterations", C.c_void_p),
                ("next_robot_order", C.c_void_p), ("policy", C.c_int), ("prev_working_set", C.c_void_p),
                ("working_set", C.c_void_p), ("set_memory", C.c_void_p)]


class RobotParams(C.Structure):
    """qlamd_robot_params: the folded controller parameters of one robot, ROBOT_PARAMS_DOUBLES doubles"""
    _fields_ = [
        ("kp_trans", C.c_double * 3), ("kd_trans", C.c_double * 3), ("kff_trans", C.c_double * 3),
        ("kp_rot", C.c_double * 3), ("kd_rot", C.c_double * 3), ("kff_rot", C.c_double * 3),
        ("force_weights", C.c_double * 6),
        ("regularizer", C.c_double), ("friction", C.c_double), ("min_normal_force", C.c_double),
        ("torque_limit", C.c_double), ("gravity_force_scale", C.c_double), ("gravity_torque_arm", C.c_double * 3),
    ]


class SwingParams(C.Structure):
    _fields_ = [("kp", C.c_double * 3), ("kd", C.c_double * 3), ("period", C.c_double), ("accel_window", C.c_double),
                ("accel_scale", C.c_double), ("gravity", C.c_double)]


class SwingBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("joint_position", "joint_velocity", "joint_velocity_oldest",
                                           "target_foot_position", "target_foot_velocity", "support_leg",
                                           "id_joint_position")]


class PoseParams(C.Structure):
    _fields_ = [("hip_in_base", (C.c_double * 3) * 4), ("com_weight", C.c_double), ("tolerance", C.c_double),
                ("max_iterations", C.c_int), ("dummy_equality", C.c_int), ("leg_order", C.c_int * 4)]


class PoseBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("stance", "stance_mask", "nominal_stance", "support_polygon",
                                           "n_vertices", "center_of_mass", "max_limb_length", "pose")]


# problem-dict key (synth.make_pose_problems) -> PoseBatch field
POSE_FIELD_OF_KEY = (("stance", "stance"), ("stance_mask", "stance_mask"), ("nominal", "nominal_stance"),
                     ("polygon", "support_polygon"), ("n_vertices", "n_vertices"), ("r_com", "center_of_mass"),
                     ("max_len", "max_limb_length"), ("pose", "pose"))


class LegStateBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("support_leg", "phase", "is_footstep", "contact", "joint_position", "limb_state",
                                          "store_flag", "stored_joint_position", "joint_command", "foot_target", "support",
                                          "leg_state_code")]


LEG_STATE_DTYPES = dict(support_leg=np.uint8, phase=np.float64, is_footstep=np.uint8, contact=np.uint8,
                        joint_position=np.float64, limb_state=np.int8, store_flag=np.uint8,
                        stored_joint_position=np.float64, joint_command=np.float64, foot_target=np.float64,
                        support=np.uint8, leg_state_code=np.int8)


ROBOT_STATE_FIELDS = (("des_pos", 3), ("des_quat", 4), ("des_linvel", 3), ("des_angvel", 3), ("joint_command", 12),
                      ("foot_position", 12), ("foot_velocity", 12), ("foot_acceleration", 12), ("surface_normal", 12),
                      ("phase", 4))


class RobotStateFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in ROBOT_STATE_FIELDS] + [("support_leg", C.c_void_p), ("leg_mode", C.c_void_p)]


class IkParams(C.Structure):
    _fields_ = [("d", C.c_double), ("l1", C.c_double), ("l2", C.c_double), ("limb_config", C.c_uint8 * 4)]


class JointPidParams(C.Structure):
    _fields_ = [(n, C.c_double * 12) for n in ("p", "i", "d", "i_max", "i_min", "lower", "upper")] + [("antiwindup", C.c_int)]


class SwingBranchExtra(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("base_orientation", "joint_command", "leg_mode", "pid_error_last", "pid_error_integral")]


class WholebodyBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("joint_position", "joint_velocity", "base_orientation", "base_linear_velocity",
                                           "base_angular_velocity", "desired_base_acceleration",
                                           "desired_joint_acceleration", "support_leg", "surface_normal")]


# key of a synth.make_wholebody_states dict -> field of qlamd_wholebody_batch
WHOLEBODY_FIELDS = (("q", "joint_position"), ("qd", "joint_velocity"), ("base_quat", "base_orientation"),
                    ("base_linvel", "base_linear_velocity"), ("base_angvel", "base_angular_velocity"),
                    ("a_des", "desired_base_acceleration"), ("qdd_des", "desired_joint_acceleration"),
                    ("stance", "support_leg"), ("normals", "surface_normal"))


class WholebodyParams(C.Structure):
    _fields_ = [("torque_weight", C.c_double), ("torque_limit", C.c_double), ("gravity", C.c_double)]


class PlantNext(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("joint_position", "joint_velocity", "base_position", "base_orientation",
                                           "base_linear_velocity", "base_angular_velocity")]


# field of qlamd_plant_next -> (key of the state dict, elements per robot)
PLANT_NEXT_FIELDS = (("joint_position", "q", 12), ("joint_velocity", "qd", 12), ("base_position", "base_pos", 3),
                     ("base_orientation", "base_quat", 4), ("base_linear_velocity", "base_linvel", 3),
                     ("base_angular_velocity", "base_angvel", 3))


TICK_FIELDS = (("messages", np.uint8), ("offsets", np.int64), ("joint_position", np.float64), ("joint_velocity", np.float64),
               ("joint_velocity_oldest", np.float64), ("base_position", np.float64), ("base_orientation", np.float64),
               ("base_linear_velocity", np.float64), ("base_angular_velocity", np.float64), ("contact", np.uint8),
               ("limb_state", np.int8), ("store_flag", np.uint8), ("stored_joint_position", np.float64), ("leg_mode", np.uint8), ("support", np.uint8),
               ("pid_error_last", np.float64), ("pid_error_integral", np.float64), ("joint_effort", np.float64),
               ("leg_state_code", np.int8), ("status", np.int32), ("message_status", np.int32), ("command", np.uint8),
               ("working_set", np.uint32), ("placement_state", np.int32), ("set_memory", np.uint32), ("iterations", np.int32))


class TickBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _ in TICK_FIELDS]


# ---- the functions of include/qlamd.h, in its order: entry -> (restype, argtypes) -----------------------------------------
# A pointer to a struct is POINTER(mirror) where callers hand over byref(mirror), c_void_p where they hand over addresses
# (ctypes takes a byref for either); arrays, the context and the stream are c_void_p.
_p, _int, _i64, _dbl, _ref = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.POINTER
_where = [_int, _p]     # `memory` and `stream`, the tail of every batch entry
SIGNATURES = {
    "qlamd_balance_default_params": (None, [_ref(BalanceParams)]),
    "qlamd_default_robot_model": (None, [_ref(RobotModel)]),
    "qlamd_context_create": (_int, [_ref(BalanceParams), _ref(RobotModel), _int, _ref(_p)]),
    "qlamd_context_destroy": (None, [_p]),
    "qlamd_reserve": (_int, [_p, _i64]),
    "qlamd_set_robots_per_wave": (_int, [_p, _int]),
    "qlamd_set_option": (_int, [_p, _int, _int]),
    "qlamd_get_counter": (_int, [_p, _int, _ref(_i64)]),
    "qlamd_balance_solve_batch": (_int, [_p, _ref(StateBatch), _i64, _p, _p, _p] + _where),
    "qlamd_force_distribution_batch": (_int, [_p] + [_p] * 5 + [_i64, _p, _p, _p] + _where),
    "qlamd_set_memory_slot": (C.c_uint, [C.c_uint]),
    "qlamd_balance_solve_placed_batch": (_int, [_p, _ref(StateBatch), _i64, _ref(Placement), _p, _p, _p] + _where),
    "qlamd_force_distribution_placed_batch": (_int, [_p] + [_p] * 5 + [_i64, _ref(Placement), _p, _p, _p] + _where),
    "qlamd_robot_params_fill": (_int, [_p, _i64, _p]),
    "qlamd_balance_solve_robot_params_batch": (_int, [_p, _ref(StateBatch), _p, _i64, _ref(Placement), _p, _p, _p] + _where),
    "qlamd_place_next_call": (_int, [_p, _ref(Placement)]),
    "qlamd_placement_from_iterations": (_int, [_p, _p, _i64, _int, _p] + _where),
    "qlamd_swing_default_params": (None, [_ref(SwingParams)]),
    "qlamd_swing_leg_torque_batch": (_int, [_p, _ref(SwingParams), _ref(SwingBatch), _i64, _p] + _where),
    "qlamd_virtual_wrench_batch": (_int, [_p, _ref(StateBatch), _i64, _p] + _where),
    "qlamd_leg_kinematics_batch": (_int, [_p, _p, _p, _i64, _p, _p, _p] + _where),
    "qlamd_qp_solve_batch": (_int, [_p, _int, _int, _int] + [_p] * 6 + [_i64, _p, _p, _p] + _where),
    "qlamd_weighted_lsq_qp_batch": (_int, [_p, _int, _int, _int, _int] + [_p] * 9 + [_i64, _p, _p] + _where),
    "qlamd_pose_default_params": (None, [_ref(PoseParams)]),
    "qlamd_pose_sqp_batch": (_int, [_p, _ref(PoseParams), _ref(PoseBatch), _i64, _p, _p, _p] + _where),
    "qlamd_pose_qp_batch": (_int, [_p, _ref(PoseParams), _ref(PoseBatch), _i64, _p, _p] + _where),
    "qlamd_pose_check_batch": (_int, [_p, _ref(PoseParams), _ref(PoseBatch), _p, _dbl, _i64, _p] + _where),
    "qlamd_pose_geometric_batch": (_int, [_p, _ref(PoseParams), _ref(PoseBatch), _p, _i64, _p] + _where),
    "qlamd_base_auto_optimize_pose_batch": (_int, [_p, _ref(PoseParams), _ref(PoseBatch), _p, _p, _dbl, _i64, _p, _p, _p, _p] + _where),
    "qlamd_leg_state_machine_batch": (_int, [_p, _ref(LegStateBatch), _int, _i64] + _where),
    "qlamd_robot_state_unpack_batch": (_int, [_p, _p, _p, _i64, _ref(RobotStateFields), _p] + _where),
    "qlamd_ik_default_params": (None, [_ref(IkParams)]),
    "qlamd_leg_inverse_kinematics_batch": (_int, [_p, _ref(IkParams), _p, _p, _i64, _p, _p] + _where),
    "qlamd_joint_pid_default_params": (None, [_ref(JointPidParams)]),
    "qlamd_swing_branch_batch": (_int, [_p, _ref(SwingParams), _ref(JointPidParams), _ref(SwingBatch), _ref(SwingBranchExtra), _dbl, _i64,
                                        _p] + _where),
    "qlamd_wholebody_default_params": (None, [_ref(WholebodyParams)]),
    "qlamd_wholebody_dynamics_batch": (_int, [_p, _ref(WholebodyBatch), _dbl, _i64, _p, _p, _p] + _where),
    "qlamd_wholebody_solve_batch": (_int, [_p, _ref(WholebodyParams), _ref(WholebodyBatch), _i64, _p, _p, _p] + _where),
    "qlamd_wholebody_solve_placed_batch": (_int, [_p, _p, _p, _i64, _p, _p, _p, _p, _p] + _where),
    "qlamd_wholebody_forward_dynamics_batch": (_int, [_p, _p, _p, _p, _p, _dbl, _dbl, _i64, _p, _p, _p, _p] + _where),
    "qlamd_tick_command_bytes": (C.c_size_t, [_i64]),
    "qlamd_full_tick_batch": (_int, [_p, _ref(SwingParams), _ref(JointPidParams), _ref(TickBatch), _dbl, _int, _i64] + _where),
    "qlamd_strerror": (C.c_char_p, [_int]),
    "qlamd_version": (_int, []),
}
EXPORTS = tuple(SIGNATURES)


class QlamdError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed: %s (%d)" % (what, strerror(code), code))
        self.code = code


_lib = None


def lib():
    """Load libqlamd.so; raise loudly if the HIP extension was not built."""
    global _lib
    if _lib is None:
        # torch (device tensors, streams) carries its own HIP runtime: it has to be the one that initialises, or a later
        # `import torch` in the same process finds no GPU.  Plumbing only -- nothing of torch is used by the library.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "HIP extension missing: %s (run `python -c 'import __graft_entry__ as g; g.build()'`). "
                "There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            # (an entry may be absent: tools/ab, tools/experiments/variants.py and tools/set_memory_probe.py --lib run builds of
            # earlier revisions through this module; calling what such a build lacks is an AttributeError there)
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def declared(signatures):
    """lib() with the entries of an extension header's table (the SIGNATURES of plant_contacts.py, contact_detection.py, ...)
    declared: the lib() of those modules.  A library without one of them is an error here (there is no fallback)."""
    L = lib()
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


# ---- one helper per marshalling job ------------------------------------------------------------------------------------------
def _call(fn, *args):
    """Call an entry that returns a QLAMD_* code: anything but OK raises QlamdError under the entry's own name."""
    rc = fn(*args)
    if rc != OK:
        raise QlamdError(rc, fn.__name__)


def _stream(stream):
    """hipStream_t handle (an integer, e.g. torch's cuda_stream) or None -> the `stream` argument."""
    return C.c_void_p(stream) if stream else None


def _ptr(a):
    """data pointer of a numpy array or a torch tensor (None -> NULL)."""
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _filled(mirror, entry):
    """A parameter struct filled by the library's qlamd_*_default_params / qlamd_default_robot_model."""
    p = mirror()
    getattr(lib(), entry)(C.byref(p))
    return p


def _is(a, dtype, count):
    """a (torch tensor or numpy array) is contiguous and holds `count` elements of `dtype` ("int32", ...)."""
    contiguous = a.is_contiguous() if hasattr(a, "is_contiguous") else a.flags["C_CONTIGUOUS"]
    return str(a.dtype).split(".")[-1] == dtype and (a.numel() if hasattr(a, "numel") else a.size) == count and contiguous


def _host_out(a, B, name):
    """A caller-supplied host output array the library writes B * 96 bytes into: float64, C-contiguous, [B, 12] -- or a
    fresh one.  (The library cannot see a numpy array's dtype or strides: a float32 or transposed array would be
    overrun.)"""
    if a is None:
        return np.zeros((B, 12))
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.shape == (B, 12)):
        raise ValueError("%s must be a C-contiguous float64 array of shape (%d, 12)" % (name, B))
    return a


def _state_batch(state, normals, memory, skip=()):
    """qlamd_state_batch over a state dict (keys of synth.make_states) and `normals` (or None) -> (StateBatch, keep-alives, B).
    MEM_HOST: every field as a C-contiguous float64 (support flags: uint8) array [B, k], B from the first field; MEM_DEVICE:
    torch tensors, used in place.  Fields whose key is in `skip` stay NULL."""
    arrays = dict(state, normals=normals)
    if normals is None:
        skip = tuple(skip) + ("normals",)
    sb, keep, B = StateBatch(), [], None
    for key, field, k in FIELD_OF_KEY + (("stance", "support_leg", 4), ("normals", "surface_normal", 12)):
        if key in skip:
            continue
        a = arrays[key]
        if memory == MEM_HOST:
            a = np.asarray(a, dtype=np.uint8 if key == "stance" else np.float64)
            a = np.ascontiguousarray(a.reshape(-1 if B is None else B, k))
            keep.append(a)
            setattr(sb, field, a.ctypes.data)
        else:
            setattr(sb, field, a.data_ptr())
        if B is None:
            B = int(a.shape[0])
    return sb, keep, B


def _placement(B, policy=0, order=None, iterations=None, prev_iterations=None, next_order=None, prev_working_set=None,
               working_set=None, set_memory=None, wholebody=False):
    """qlamd_placement over torch tensors (or numpy arrays) in the memory space of the call, each checked before the library
    reads or writes B elements behind its pointer: order / iterations / prev_iterations / next_order int32 [B].  The balance
    step's warm start: prev_working_set / working_set int32 [B] and set_memory int32 [B, 4] (the bits of uint32 words).
    wholebody: the whole-body step's 64-bit sets, 8 bytes per robot (int32 [B, 2] or int64 [B]), and its table int64 [B, 4],
    which is an argument of its own there (the struct's member stays NULL); None when no array of the struct is given."""
    for name, a in (("order", order), ("iterations", iterations), ("prev_iterations", prev_iterations), ("next_order", next_order)):
        if a is not None and not _is(a, "int32", B):
            raise ValueError("%s must be a contiguous int32 tensor of %d elements" % (name, B))
    for name, a in (("prev_working_set", prev_working_set), ("working_set", working_set)):
        if a is None:
            continue
        if wholebody and (a.numel() * a.element_size() != 8 * B or not a.is_contiguous()):
            raise ValueError("%s must be a contiguous tensor of 8 bytes per robot" % name)
        if not wholebody and not _is(a, "int32", B):
            raise ValueError("%s must be a contiguous int32 tensor of %d elements (the 32 bits of a uint32)" % (name, B))
    bits = "64" if wholebody else "32"
    if set_memory is not None and not _is(set_memory, "int" + bits, 4 * B):
        raise ValueError("set_memory must be a contiguous int%s tensor of %d x 4 elements (the %s bits of a uint%s)" % (bits, B, bits, bits))
    arrays = (order, iterations, prev_iterations, next_order, prev_working_set, working_set)
    if wholebody and all(a is None for a in arrays):
        return None
    ptrs = [_ptr(a) for a in arrays]
    return Placement(*ptrs[:4], int(policy), *ptrs[4:], None if wholebody else _ptr(set_memory))


def _pose_batch(problems, memory):
    pb, keep = PoseBatch(), []
    for key, field in POSE_FIELD_OF_KEY:
        a = problems.get(key)
        if a is not None and memory == MEM_HOST:
            a = np.ascontiguousarray(a)
            keep.append(a)
        setattr(pb, field, _ptr(a))
    return pb, keep


def _wholebody_batch(state, keep):
    """qlamd_wholebody_batch over numpy arrays (kept alive in `keep`) or torch CUDA tensors."""
    wb = WholebodyBatch()
    for key, field in WHOLEBODY_FIELDS:
        v = state.get(key)
        if v is None:
            continue
        if not hasattr(v, "data_ptr"):
            v = np.ascontiguousarray(v, dtype=np.uint8 if key == "stance" else np.float64)
            keep.append(v)
        setattr(wb, field, _ptr(v))
    return wb


def _robot_state_fields(zeros, want=None):
    """qlamd_robot_state_fields over fresh outputs, zeros(width, dtype name) making each: -> (RobotStateFields, dict of them)."""
    f, out = RobotStateFields(), {}
    for name, w, dtype in [(n, w, "float64") for n, w in ROBOT_STATE_FIELDS] + [("support_leg", 4, "uint8"), ("leg_mode", 4, "uint8")]:
        if want is None or name in want:
            out[name] = zeros(w, dtype)
            setattr(f, name, _ptr(out[name]))
    return f, out


# ---- the wrappers ------------------------------------------------------------------------------------------------------------
def strerror(code):
    return lib().qlamd_strerror(int(code)).decode()


def set_memory_slot(support_mask):
    """qlamd_set_memory_slot: the slot of qlamd_placement::set_memory [B][4] that belongs to a support mask (LF = bit 0, RF = 1,
    RH = 2, LH = 3) -- the library's own table, the one its kernels use."""
    return int(lib().qlamd_set_memory_slot(int(support_mask)))


def tick_command_bytes(batch):
    """Size of the opaque `command` block of qlamd_tick_batch (zero-filled before the first tick)."""
    return int(lib().qlamd_tick_command_bytes(int(batch)))


def default_params():
    return _filled(BalanceParams, "qlamd_balance_default_params")


def default_robot_model():
    return _filled(RobotModel, "qlamd_default_robot_model")


def default_swing_params():
    return _filled(SwingParams, "qlamd_swing_default_params")


def default_pose_params():
    return _filled(PoseParams, "qlamd_pose_default_params")


def default_ik_params():
    return _filled(IkParams, "qlamd_ik_default_params")


def default_joint_pid_params():
    return _filled(JointPidParams, "qlamd_joint_pid_default_params")


def default_wholebody_params():
    return _filled(WholebodyParams, "qlamd_wholebody_default_params")


def robot_params_fill(params):
    """qlamd_robot_params_fill: a BalanceParams, a list of them or a ctypes array of them -> numpy float64 [B, 32], one folded
    record per robot (row i viewed as a RobotParams: RobotParams.from_buffer(records[i])).  `gravity` is not part of a record:
    it stays the context's.  A host function: no device is needed."""
    if isinstance(params, BalanceParams):
        params = [params]
    arr = params if isinstance(params, C.Array) else (BalanceParams * len(params))(*params)
    out = np.zeros((len(arr), ROBOT_PARAMS_DOUBLES), dtype=np.float64)
    if len(arr):
        _call(lib().qlamd_robot_params_fill, C.addressof(arr), len(arr), out.ctypes.data)
    return out


class Context:
    """RAII wrapper of qlamd_context."""

    def __init__(self, params=None, model=None, device=0):
        self._h = C.c_void_p()
        self.params = params if params is not None else default_params()
        _call(lib().qlamd_context_create, C.byref(self.params), C.byref(model) if model is not None else None, int(device),
              C.byref(self._h))
        self.device = device

    def close(self):
        if self._h:
            lib().qlamd_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        """qlamd_set_option (OPT_* and their values above)."""
        _call(lib().qlamd_set_option, self._h, int(option), int(value))

    def counter(self, which):
        """qlamd_get_counter (COUNTER_* above); waits for the device.  0 from a build that has no counters yet."""
        v = C.c_int64(0)
        if not hasattr(lib(), "qlamd_get_counter"):
            return 0
        _call(lib().qlamd_get_counter, self._h, int(which), C.byref(v))
        return int(v.value)

    def reserve(self, max_batch):
        """Size the context's device scratch for batches up to max_batch (qlamd_reserve): before capturing the whole tick."""
        _call(lib().qlamd_reserve, self._h, int(max_batch))

    def set_robots_per_wave(self, rpw):
        _call(lib().qlamd_set_robots_per_wave, self._h, int(rpw))

    # ---- host (numpy) buffers -------------------------------------------------
    def balance_solve_host(self, state, normals=None, want_forces=True, tau=None, grf=None):
        """tau / grf: C-contiguous float64 [B,12] arrays to write into (what QLAMD_ON_FAILURE_KEEP leaves alone is the
        caller's), fresh zeros otherwise."""
        sb, keep, B = _state_batch(state, normals, MEM_HOST)
        tau = _host_out(tau, B, "tau")
        grf = _host_out(grf, B, "grf") if want_forces else None
        status = np.full(B, -1, dtype=np.int32)
        _call(lib().qlamd_balance_solve_batch, self._h, C.byref(sb), B, _ptr(tau), _ptr(grf), _ptr(status), MEM_HOST, None)
        return tau, grf, status

    def balance_solve_placed_host(self, state, order=None, normals=None, want_forces=True, prev_iterations=None, policy=0):
        """qlamd_balance_solve_placed_batch with host (numpy) buffers -> (tau, grf, status, iterations[, next_order])."""
        sb, keep, B = _state_batch(state, normals, MEM_HOST)
        if order is not None:
            order = np.ascontiguousarray(np.asarray(order, dtype=np.int32).reshape(B))
        nxt = None
        if prev_iterations is not None:
            prev_iterations = np.ascontiguousarray(np.asarray(prev_iterations, dtype=np.int32).reshape(B))
            nxt = np.full(B, -1, dtype=np.int32)
        tau = np.zeros((B, 12))
        grf = np.zeros((B, 12)) if want_forces else None
        status = np.full(B, -1, dtype=np.int32)
        iters = np.full(B, -1, dtype=np.int32)
        pl = _placement(B, policy, order, iters, prev_iterations, nxt)
        _call(lib().qlamd_balance_solve_placed_batch, self._h, C.byref(sb), B, C.byref(pl), _ptr(tau), _ptr(grf), _ptr(status),
              MEM_HOST, None)
        return (tau, grf, status, iters) if nxt is None else (tau, grf, status, iters, nxt)

    def balance_solve_robot_params_host(self, state, robot_params, order=None, normals=None, want_forces=True):
        """qlamd_balance_solve_robot_params_batch with host (numpy) buffers: robot_params float64 [B, 32] -> (tau, grf, status,
        iterations)."""
        sb, keep, B = _state_batch(state, normals, MEM_HOST)
        if order is not None:
            order = np.ascontiguousarray(np.asarray(order, dtype=np.int32).reshape(B))
        if robot_params is not None:
            robot_params = np.ascontiguousarray(np.asarray(robot_params, dtype=np.float64).reshape(B, ROBOT_PARAMS_DOUBLES))
        tau = np.zeros((B, 12))
        grf = np.zeros((B, 12)) if want_forces else None
        status = np.full(B, -1, dtype=np.int32)
        iters = np.full(B, -1, dtype=np.int32)
        pl = _placement(B, 0, order, iters)
        _call(lib().qlamd_balance_solve_robot_params_batch, self._h, C.byref(sb), _ptr(robot_params), B, C.byref(pl), _ptr(tau),
              _ptr(grf), _ptr(status), MEM_HOST, None)
        return tau, grf, status, iters

    # ---- device (torch) buffers ------------------------------------------------
    def balance_solve_device(self, dstate, tau, grf, status, stream=None):
        """dstate: dict of torch CUDA tensors (keys of synth.make_states, plus optional
        'normals'); tau/grf/status: preallocated CUDA tensors.  Asynchronous."""
        sb, _, B = _state_batch(dstate, dstate.get("normals"), MEM_DEVICE)
        _call(lib().qlamd_balance_solve_batch, self._h, C.byref(sb), B, tau.data_ptr(), _ptr(grf), status.data_ptr(), MEM_DEVICE,
              _stream(stream))

    def balance_solve_placed_device(self, dstate, tau, grf, status, order=None, iterations=None, prev_iterations=None,
                                    next_order=None, policy=0, stream=None, prev_working_set=None, working_set=None,
                                    set_memory=None):
        """qlamd_balance_solve_placed_batch on torch CUDA tensors: order = int32 [B] permutation (slot -> robot) or None,
        iterations = int32 [B] output or None; prev_iterations / next_order = the counts of the previous call and the
        placement for the next one (both or neither); set_memory = int32 [B, 4], the working set per support set, updated in
        place (instead of prev_working_set).  Asynchronous."""
        sb, _, B = _state_batch(dstate, dstate.get("normals"), MEM_DEVICE)
        pl = _placement(B, policy, order, iterations, prev_iterations, next_order, prev_working_set, working_set, set_memory)
        _call(lib().qlamd_balance_solve_placed_batch, self._h, C.byref(sb), B, C.byref(pl), tau.data_ptr(), _ptr(grf),
              status.data_ptr(), MEM_DEVICE, _stream(stream))

    def force_distribution_placed_device(self, q, quat, support, wrench, tau, grf, status, normals=None, order=None, iterations=None,
                                         prev_iterations=None, next_order=None, policy=0, stream=None, prev_working_set=None,
                                         working_set=None, set_memory=None):
        """qlamd_force_distribution_placed_batch on torch CUDA tensors (q [B, 12], quat [B, 4], support uint8 [B, 4], wrench
        [B, 6]); the placement's arguments as balance_solve_placed_device.  Asynchronous."""
        B = q.shape[0]
        pl = _placement(B, policy, order, iterations, prev_iterations, next_order, prev_working_set, working_set, set_memory)
        _call(lib().qlamd_force_distribution_placed_batch, self._h, _ptr(q), _ptr(quat), _ptr(support), _ptr(normals), _ptr(wrench), B,
              C.byref(pl), _ptr(tau), _ptr(grf), _ptr(status), MEM_DEVICE, _stream(stream))

    def balance_solve_robot_params_device(self, dstate, robot_params, tau, grf, status, order=None, iterations=None,
                                          prev_iterations=None, next_order=None, policy=0, stream=None, prev_working_set=None,
                                          working_set=None, set_memory=None):
        """qlamd_balance_solve_robot_params_batch on torch CUDA tensors: robot_params = float64 [B, 32], robot i's folded record
        (robot_params_fill) in row i; the other arguments as balance_solve_placed_device (prev_iterations / next_order are
        passed on for the library to refuse).  Asynchronous."""
        sb, _, B = _state_batch(dstate, dstate.get("normals"), MEM_DEVICE)
        if robot_params is not None and not _is(robot_params, "float64", ROBOT_PARAMS_DOUBLES * B):
            raise ValueError("robot_params must be a contiguous float64 tensor of %d x %d elements" % (B, ROBOT_PARAMS_DOUBLES))
        pl = _placement(B, policy, order, iterations, prev_iterations, next_order, prev_working_set, working_set, set_memory)
        _call(lib().qlamd_balance_solve_robot_params_batch, self._h, C.byref(sb), _ptr(robot_params), B, C.byref(pl), tau.data_ptr(),
              _ptr(grf), status.data_ptr(), MEM_DEVICE, _stream(stream))

    def place_next_call(self, order=None, iterations=None, prev_iterations=None, next_order=None, policy=0):
        """qlamd_place_next_call with torch int32 CUDA tensors (or all None to withdraw a pending placement)."""
        given = [a for a in (order, iterations, next_order) if a is not None]
        pl = _placement(given[0].numel(), policy, order, iterations, prev_iterations, next_order) if given else None
        _call(lib().qlamd_place_next_call, self._h, C.byref(pl) if pl is not None else None)

    def placement_from_iterations(self, iterations, order=None, policy=0, stream=None):
        """qlamd_placement_from_iterations: numpy int32 [B] -> numpy order (synchronous), or torch int32 CUDA tensors
        (order preallocated, asynchronous on `stream`)."""
        if hasattr(iterations, "data_ptr"):
            B, memory = iterations.numel(), MEM_DEVICE
            if order is None or str(order.dtype) != "torch.int32" or order.numel() != B or str(iterations.dtype) != "torch.int32":
                raise ValueError("device memory: pass int32 tensors iterations and order of equal length")
        else:
            iterations = np.ascontiguousarray(np.asarray(iterations, dtype=np.int32).reshape(-1))
            B, memory, stream = iterations.shape[0], MEM_HOST, None
            order = np.full(B, -1, dtype=np.int32)
        _call(lib().qlamd_placement_from_iterations, self._h, _ptr(iterations), B, int(policy), _ptr(order), memory, _stream(stream))
        return order

    def virtual_wrench_device(self, dstate, wrench, stream=None):
        sb, _, B = _state_batch(dstate, None, MEM_DEVICE)
        _call(lib().qlamd_virtual_wrench_batch, self._h, C.byref(sb), B, wrench.data_ptr(), MEM_DEVICE, _stream(stream))

    def leg_kinematics_device(self, q, quat, foot=None, jac=None, grav=None, stream=None):
        _call(lib().qlamd_leg_kinematics_batch, self._h, q.data_ptr(), quat.data_ptr(), q.shape[0], _ptr(foot), _ptr(jac), _ptr(grav),
              MEM_DEVICE, _stream(stream))


def virtual_wrench(ctx, state):
    """qlamd_virtual_wrench_batch on host buffers (state dict as synth.make_states) -> wrench [B,6]."""
    sb, keep, B = _state_batch(state, None, MEM_HOST, skip=("q", "stance"))   # (the entry reads the base and desired-base fields only)
    w = np.zeros((B, 6))
    _call(lib().qlamd_virtual_wrench_batch, ctx._h, C.byref(sb), B, w.ctypes.data, MEM_HOST, None)
    return w


def leg_kinematics(ctx, q, quat):
    """qlamd_leg_kinematics_batch on host buffers -> (foot [B,4,3], jacobian [B,4,9], gravity torque [B,4,3])."""
    q = np.ascontiguousarray(q, dtype=np.float64); quat = np.ascontiguousarray(quat, dtype=np.float64)
    B = q.shape[0]
    foot, jac, grav = np.zeros((B, 4, 3)), np.zeros((B, 4, 9)), np.zeros((B, 4, 3))
    _call(lib().qlamd_leg_kinematics_batch, ctx._h, _ptr(q), _ptr(quat), B, _ptr(foot), _ptr(jac), _ptr(grav), MEM_HOST, None)
    return foot, jac, grav


def force_distribution(ctx, q, quat, support, wrench, normals=None, memory=MEM_HOST, tau=None, grf=None):
    """qlamd_force_distribution_batch with host (numpy) buffers -> (tau, grf, status)."""
    q = np.ascontiguousarray(q, dtype=np.float64); quat = np.ascontiguousarray(quat, dtype=np.float64)
    support = np.ascontiguousarray(support, dtype=np.uint8); wrench = np.ascontiguousarray(wrench, dtype=np.float64)
    normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    B = q.shape[0]
    if memory == MEM_HOST:
        tau, grf = _host_out(tau, B, "tau"), _host_out(grf, B, "grf")
    elif tau is None or grf is None:
        raise ValueError("device memory: pass preallocated tau / grf tensors")
    st = np.full(B, -1, dtype=np.int32)
    _call(lib().qlamd_force_distribution_batch, ctx._h, _ptr(q), _ptr(quat), _ptr(support), _ptr(normals), _ptr(wrench), B, _ptr(tau),
          _ptr(grf), _ptr(st), memory, None)
    return tau, grf, st


def swing_leg_torque(ctx, q, qd, qd_oldest, target_pos, target_vel, support, q_id=None, params=None, memory=MEM_HOST,
                     out=None, stream=None):
    """qlamd_swing_leg_torque_batch; numpy arrays for MEM_HOST (returns tau [B,12]), torch tensors + out for MEM_DEVICE."""
    prm = params if params is not None else default_swing_params()
    arrs = [q, qd, qd_oldest, target_pos, target_vel, support, q_id]
    if memory == MEM_HOST:
        arrs = [None if a is None else np.ascontiguousarray(a) for a in arrs]
    sb = SwingBatch(*[_ptr(a) for a in arrs])
    B = int(arrs[0].shape[0])
    tau = np.zeros((B, 12)) if memory == MEM_HOST else out
    _call(lib().qlamd_swing_leg_torque_batch, ctx._h, C.byref(prm), C.byref(sb), B, _ptr(tau), memory, _stream(stream))
    return tau


def swing_branch(ctx, joint_effort, q, qd, qd_oldest, target_pos, target_vel, support, base_orientation, joint_command,
                 leg_mode, pid_error_last, pid_error_integral, period, q_id=None, params=None, pid=None, memory=MEM_HOST,
                 stream=None):
    """qlamd_swing_branch_batch.  joint_effort, pid_error_last, pid_error_integral are updated in place (host:
    C-contiguous float64 numpy arrays; device: torch CUDA tensors)."""
    prm = params if params is not None else default_swing_params()
    pidp = pid if pid is not None else default_joint_pid_params()
    arrs = [q, qd, qd_oldest, target_pos, target_vel, support, q_id]
    ext = [base_orientation, joint_command, leg_mode, pid_error_last, pid_error_integral]
    if memory == MEM_HOST:
        arrs = [None if a is None else np.ascontiguousarray(a) for a in arrs]
        ext[:3] = [None if a is None else np.ascontiguousarray(a) for a in ext[:3]]
        for a in (joint_effort, pid_error_last, pid_error_integral):
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    sb = SwingBatch(*[_ptr(a) for a in arrs])
    ex = SwingBranchExtra(*[_ptr(a) for a in ext])
    B = int(arrs[0].shape[0])
    _call(lib().qlamd_swing_branch_batch, ctx._h, C.byref(prm), C.byref(pidp), C.byref(sb), C.byref(ex), float(period), B,
          _ptr(joint_effort), memory, _stream(stream))
    return joint_effort


def pose_sqp(ctx, problems, params=None, memory=MEM_HOST, out=None, stream=None):
    """problems: dict as synth.make_pose_problems (numpy for MEM_HOST, torch CUDA tensors for
    MEM_DEVICE).  Returns (pose [B,7], iterations [B], status [B]) -- numpy arrays for host
    memory; for device memory the preallocated tensors passed in `out`."""
    prm = params if params is not None else default_pose_params()
    B = int(problems["pose"].shape[0])
    pb, keep = _pose_batch(problems, memory)
    if memory == MEM_HOST:
        pose = np.zeros((B, 7)); it = np.zeros(B, dtype=np.int32); st = np.full(B, -1, dtype=np.int32)
    else:
        pose, it, st = out
    _call(lib().qlamd_pose_sqp_batch, ctx._h, C.byref(prm), C.byref(pb), B, _ptr(pose), _ptr(it), _ptr(st), memory, _stream(stream))
    return pose, it, st


def pose_qp(ctx, problems, params=None):
    """qlamd_pose_qp_batch, host buffers -> (pose [B,7], status [B])."""
    prm = params if params is not None else default_pose_params()
    B = int(problems["pose"].shape[0])
    pb, keep = _pose_batch(problems, MEM_HOST)
    pose = np.zeros((B, 7)); st = np.full(B, -1, dtype=np.int32)
    _call(lib().qlamd_pose_qp_batch, ctx._h, C.byref(prm), C.byref(pb), B, _ptr(pose), _ptr(st), MEM_HOST, None)
    return pose, st


def pose_check(ctx, problems, min_len=None, leg_tol=0.0, params=None):
    """qlamd_pose_check_batch for the poses in problems['pose'], host buffers -> ok [B] uint8."""
    prm = params if params is not None else default_pose_params()
    B = int(problems["pose"].shape[0])
    pb, keep = _pose_batch(problems, MEM_HOST)
    mn = None if min_len is None else np.ascontiguousarray(min_len, dtype=np.float64)
    ok = np.zeros(B, dtype=np.uint8)
    _call(lib().qlamd_pose_check_batch, ctx._h, C.byref(prm), C.byref(pb), _ptr(mn), float(leg_tol), B, _ptr(ok), MEM_HOST, None)
    return ok


def pose_geometric(ctx, problems, stance_for_orientation=None, params=None):
    """qlamd_pose_geometric_batch, host buffers -> pose [B,7]."""
    prm = params if params is not None else default_pose_params()
    B = int(problems["stance"].shape[0])
    pb, keep = _pose_batch(problems, MEM_HOST)
    sfo = None if stance_for_orientation is None else np.ascontiguousarray(stance_for_orientation, dtype=np.float64)
    pose = np.zeros((B, 7))
    _call(lib().qlamd_pose_geometric_batch, ctx._h, C.byref(prm), C.byref(pb), _ptr(sfo), B, _ptr(pose), MEM_HOST, None)
    return pose


def base_auto_optimize_pose(ctx, problems, stance_for_orientation=None, min_len=None, leg_tol=0.0, params=None,
                            memory=MEM_HOST, out=None, stream=None):
    """qlamd_base_auto_optimize_pose_batch -> (pose [B,7], stage [B], iterations [B], status [B]).  Host buffers by
    default; for device memory pass torch CUDA tensors in `problems` and preallocated outputs in `out`."""
    prm = params if params is not None else default_pose_params()
    B = int(problems["stance"].shape[0])
    pb, keep = _pose_batch(problems, memory)
    if memory == MEM_HOST:
        sfo = None if stance_for_orientation is None else np.ascontiguousarray(stance_for_orientation, dtype=np.float64)
        mn = None if min_len is None else np.ascontiguousarray(min_len, dtype=np.float64)
        pose = np.zeros((B, 7)); stage = np.zeros(B, np.int32); it = np.zeros(B, np.int32); st = np.full(B, -1, np.int32)
    else:
        sfo, mn = stance_for_orientation, min_len
        pose, stage, it, st = out
    _call(lib().qlamd_base_auto_optimize_pose_batch, ctx._h, C.byref(prm), C.byref(pb), _ptr(sfo), _ptr(mn), float(leg_tol), B,
          _ptr(pose), _ptr(stage), _ptr(it), _ptr(st), memory, _stream(stream))
    return pose, stage, it, st


def leg_state_machine(ctx, io, index_quirk=1, memory=MEM_HOST, stream=None):
    """qlamd_leg_state_machine_batch.  `io`: dict with the fields of qlamd_leg_state_batch (numpy arrays of the
    dtypes in LEG_STATE_DTYPES for host memory, torch CUDA tensors for device memory); the in/out and out arrays
    are updated in place."""
    b = LegStateBatch()
    for name, dt in LEG_STATE_DTYPES.items():
        a = io[name]
        if memory == MEM_HOST:
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], name
        setattr(b, name, _ptr(a))
    B = int(io["phase"].shape[0])
    _call(lib().qlamd_leg_state_machine_batch, ctx._h, C.byref(b), int(index_quirk), B, memory, _stream(stream))
    return io


def robot_state_unpack(ctx, messages, offsets, want=None):
    """qlamd_robot_state_unpack_batch on host buffers.  messages: bytes / uint8 array, offsets: int64 [B+1].
    Returns (dict of arrays, status [B]); `want` limits the outputs (default: all)."""
    buf = np.frombuffer(messages, dtype=np.uint8) if isinstance(messages, (bytes, bytearray)) else np.ascontiguousarray(messages, np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    B = off.shape[0] - 1
    f, out = _robot_state_fields(lambda w, dtype: np.zeros((B, w), dtype), want)
    st = np.full(B, -1, np.int32)
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)
    _call(lib().qlamd_robot_state_unpack_batch, ctx._h, _ptr(buf), _ptr(off), B, C.byref(f), _ptr(st), MEM_HOST, None)
    return out, st


def robot_state_unpack_device(ctx, messages, offsets, stream=None):
    """qlamd_robot_state_unpack_batch on device buffers (torch CUDA tensors: uint8 blob, int64 [B+1] offsets) ->
    (dict of CUDA tensors, status tensor).  Asynchronous."""
    import torch
    B = offsets.numel() - 1
    f, out = _robot_state_fields(lambda w, dtype: torch.zeros(B, w, dtype=getattr(torch, dtype), device=messages.device))
    st = torch.full((B,), -1, dtype=torch.int32, device=messages.device)
    _call(lib().qlamd_robot_state_unpack_batch, ctx._h, messages.data_ptr(), offsets.data_ptr(), B, C.byref(f), st.data_ptr(),
          MEM_DEVICE, _stream(stream))
    return out, st


def leg_inverse_kinematics(ctx, foot_position, joint_position_last=None, params=None):
    """qlamd_leg_inverse_kinematics_batch on host buffers -> (q [B,12], ok [B,4])."""
    prm = params if params is not None else default_ik_params()
    foot = np.ascontiguousarray(foot_position, dtype=np.float64)
    last = None if joint_position_last is None else np.ascontiguousarray(joint_position_last, dtype=np.float64)
    B = foot.shape[0]
    q = np.zeros((B, 12)); ok = np.zeros((B, 4), np.uint8)
    _call(lib().qlamd_leg_inverse_kinematics_batch, ctx._h, C.byref(prm), _ptr(foot), _ptr(last), B, _ptr(q), _ptr(ok), MEM_HOST, None)
    return q, ok


def qp_solve(ctx, G, g0, CE, ce0, CI, ci0):
    """Batch of dense QPs with host (numpy) buffers: G [B,n,n], g0 [B,n], CE [B,n,p] or None, CI [B,n,m]."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    B, n = G.shape[0], G.shape[1]
    g0 = np.ascontiguousarray(g0, dtype=np.float64)
    p = 0 if CE is None else int(np.asarray(CE).shape[2])
    m = 0 if CI is None else int(np.asarray(CI).shape[2])
    CE = None if p == 0 else np.ascontiguousarray(CE, dtype=np.float64)
    ce0 = None if p == 0 else np.ascontiguousarray(ce0, dtype=np.float64)
    CI = None if m == 0 else np.ascontiguousarray(CI, dtype=np.float64)
    ci0 = None if m == 0 else np.ascontiguousarray(ci0, dtype=np.float64)
    x = np.zeros((B, n)); f = np.zeros(B); st = np.full(B, -1, dtype=np.int32)
    _call(lib().qlamd_qp_solve_batch, ctx._h, n, p, m, _ptr(G), _ptr(g0), _ptr(CE), _ptr(ce0), _ptr(CI), _ptr(ci0), B, _ptr(x), _ptr(f),
          _ptr(st), MEM_HOST, None)
    return x, f, st


def weighted_lsq_qp(ctx, A, S, b, W, Ceq=None, ceq=None, D=None, d=None, f=None, memory=MEM_HOST, out=None, stream=None):
    """qlamd_weighted_lsq_qp_batch: min (Ax-b)'S(Ax-b) + x'Wx  s.t. Cx = c, d <= Dx <= f  (the argument list of
    ooqpei::QuadraticProblemFormulation::solve).  A [B,k,n], S [B,k], b [B,k], W [B,n] (diagonals), Ceq [B,p,n],
    ceq [B,p], D [B,m,n], d / f [B,m].  Host: numpy in, (x, status) out; device: torch tensors and out = (x, status)."""
    arrs = [A, S, b, W, Ceq, ceq, D, d, f]
    if memory == MEM_HOST:
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
    A = arrs[0]
    B, k, n = int(A.shape[0]), int(A.shape[1]), int(A.shape[2])
    p = 0 if arrs[4] is None else int(arrs[4].shape[1])
    m = 0 if arrs[6] is None else int(arrs[6].shape[1])
    if memory == MEM_HOST:
        x, st = np.zeros((B, n)), np.full(B, -1, dtype=np.int32)
    else:
        if out is None:
            raise ValueError("device memory: pass out=(x [B,n] float64, status [B] int32) as preallocated CUDA tensors")
        x, st = out
    _call(lib().qlamd_weighted_lsq_qp_batch, ctx._h, n, k, p, m, *[_ptr(a) for a in arrs], B, _ptr(x), _ptr(st), memory, _stream(stream))
    return x, st


def to_device(state, device="cuda:0"):
    """numpy state dict -> dict of torch tensors resident in HBM."""
    import torch
    out = {}
    for k, v in state.items():
        out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    return out


def to_device_records(state, device="cuda:0"):
    """numpy state dict -> dict of torch tensors for a context with OPT_STATE_LAYOUT = STATE_RECORDS: the nine double fields are
    views into ONE [B][48] tensor of qlamd_state_record's (data_ptr() of a view = the field's first element of robot 0), the
    support flags (and normals, if any) arrays of their own."""
    import torch
    B = state["q"].shape[0]
    rec = np.zeros((B, STATE_RECORD_DOUBLES))
    for k, o in STATE_RECORD_OFFSETS.items():
        rec[:, o:o + state[k].shape[1]] = state[k]
    t = torch.from_numpy(rec).to(device)
    out = {k: t[:, o:] for k, o in STATE_RECORD_OFFSETS.items()}
    out["_records"] = t
    for k, v in state.items():
        if k not in STATE_RECORD_OFFSETS:
            out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    return out


def wholebody_dynamics(ctx, state, gravity=9.81, want=("M", "h", "Jc")):
    """qlamd_wholebody_dynamics_batch on host buffers -> dict with M [B,18,18], h [B,18], Jc [B,12,18]."""
    keep = []
    wb = _wholebody_batch(state, keep)
    B = state["q"].shape[0]
    out = dict(M=np.zeros((B, 18, 18)) if "M" in want else None, h=np.zeros((B, 18)) if "h" in want else None,
               Jc=np.zeros((B, 12, 18)) if "Jc" in want else None)
    _call(lib().qlamd_wholebody_dynamics_batch, ctx._h, C.byref(wb), float(gravity), B, _ptr(out["M"]), _ptr(out["h"]), _ptr(out["Jc"]),
          MEM_HOST, None)
    return out


def wholebody_dynamics_device(ctx, dstate, M, h, Jc, gravity=9.81, stream=None):
    wb = _wholebody_batch(dstate, [])
    _call(lib().qlamd_wholebody_dynamics_batch, ctx._h, C.byref(wb), float(gravity), dstate["q"].shape[0], _ptr(M), _ptr(h), _ptr(Jc),
          MEM_DEVICE, _stream(stream))


def wholebody_solve(ctx, state, params=None, tau=None, grf=None):
    """qlamd_wholebody_solve_batch on host buffers -> (tau [B,12], grf [B,12], status [B])."""
    prm = params if params is not None else default_wholebody_params()
    keep = []
    wb = _wholebody_batch(state, keep)
    B = state["q"].shape[0]
    tau, grf = _host_out(tau, B, "tau"), _host_out(grf, B, "grf")
    st = np.full(B, -1, np.int32)
    _call(lib().qlamd_wholebody_solve_batch, ctx._h, C.byref(prm), C.byref(wb), B, _ptr(tau), _ptr(grf), _ptr(st), MEM_HOST, None)
    return tau, grf, st


def wholebody_solve_device(ctx, dstate, tau, grf, status, params=None, stream=None):
    """Same entry on torch CUDA tensors (dstate: dict from to_device); asynchronous."""
    prm = params if params is not None else default_wholebody_params()
    wb = _wholebody_batch(dstate, [])
    _call(lib().qlamd_wholebody_solve_batch, ctx._h, C.byref(prm), C.byref(wb), dstate["q"].shape[0], tau.data_ptr(), _ptr(grf),
          status.data_ptr(), MEM_DEVICE, _stream(stream))


def wholebody_solve_placed_device(ctx, dstate, tau, grf, status, params=None, stream=None, order=None, iterations=None,
                                  prev_iterations=None, next_order=None, policy=0, prev_working_set=None, working_set=None,
                                  set_memory=None):
    """qlamd_wholebody_solve_placed_batch on torch CUDA tensors; asynchronous.  order / iterations / prev_iterations / next_order:
    int32 [B]; prev_working_set / working_set: the 64-bit sets as int32 [B, 2] or int64 [B]; set_memory: the working set per support
    set, int64 [B, 4] (32-byte aligned: the library refuses another), updated in place, instead of prev_working_set."""
    prm = params if params is not None else default_wholebody_params()
    wb = _wholebody_batch(dstate, [])
    B = dstate["q"].shape[0]
    pl = _placement(B, policy, order, iterations, prev_iterations, next_order, prev_working_set, working_set, set_memory, wholebody=True)
    _call(lib().qlamd_wholebody_solve_placed_batch, ctx._h, C.byref(prm), C.byref(wb), B, C.byref(pl) if pl is not None else None,
          _ptr(set_memory), tau.data_ptr(), _ptr(grf), status.data_ptr(), MEM_DEVICE, _stream(stream))


def _plant_call(ctx, wb, B, tau, g_ext, base_pos, gravity, dt, acc, f, nxt, status, memory, stream, entry, *structs):
    """One call of a plant entry: the eleven arguments every plant entry begins with, the entry's own optional structs (zero to
    three; None: NULL) in front of `status`, and the three every entry ends with.  `entry` is a declared function of the library."""
    _call(entry, ctx._h, C.byref(wb), _ptr(tau), _ptr(g_ext), _ptr(base_pos), gravity, dt, B, _ptr(acc), _ptr(f),
          C.byref(nxt) if nxt is not None else None, *[C.byref(struct) if struct is not None else None for struct in structs],
          _ptr(status), memory, _stream(stream))


def _plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, entry, structs=(), extra=None, pos_always=False):
    """The host form of every plant entry (entry, structs: _plant_call's) -> dict with acc, f, status, `next` with dt, and `extra`.
    base_pos goes over with dt only, unless the entry reads it in any case (pos_always, as plant_check's in
    csrc/plant_step_body.hpp); in_place: it is the state's own array."""
    keep = []
    B = state["q"].shape[0]
    if in_place:
        for _, key, n in PLANT_NEXT_FIELDS:
            a = state[key]
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.size == B * n):
                raise ValueError("in_place needs state[%r] as a C-contiguous float64 array of %d x %d" % (key, B, n))
    wb = _wholebody_batch(state, keep)
    if free_flight:
        wb.support_leg = None
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    g_ext = None if g_ext is None else np.ascontiguousarray(g_ext, dtype=np.float64)
    if tau.shape != (B, 12) or (g_ext is not None and g_ext.shape != (B, 18)):
        raise ValueError("tau must be [%d, 12] and g_ext [%d, 18]" % (B, B))
    out = dict(acc=np.zeros((B, 18)), f=np.zeros((B, 12)), status=np.full(B, -1, np.int32))
    out.update(extra or {})
    nxt = None
    pos = np.ascontiguousarray(state["base_pos"], dtype=np.float64) if dt is not None or pos_always else None
    if dt is not None:
        out["next"] = {key: (state[key] if in_place else np.zeros((B, n))) for _, key, n in PLANT_NEXT_FIELDS}
        nxt = PlantNext(*[_ptr(out["next"][key]) for _, key, _ in PLANT_NEXT_FIELDS])
    _plant_call(ctx, wb, B, tau, g_ext, pos, float(gravity), float(dt) if dt is not None else 0.0, out["acc"], out["f"], nxt,
                out["status"], MEM_HOST, None, entry, *structs)
    return out


def wholebody_forward_dynamics(ctx, state, tau, g_ext=None, gravity=9.81, dt=None, free_flight=False, in_place=False):
    """qlamd_wholebody_forward_dynamics_batch on host buffers -> dict with acc [B,18], f [B,12], status [B] and, with dt, `next`:
    the state after dt under the keys of `state` (q, qd, base_pos, base_quat, base_linvel, base_angvel).  state["stance"] flags the
    held feet (free_flight: support_leg = NULL); in_place: the next state is written over `state`'s own arrays."""
    return _plant_host(ctx, state, tau, g_ext, gravity, dt, free_flight, in_place, lib().qlamd_wholebody_forward_dynamics_batch)


def _plant_device_args(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream, entry, structs=(),
                       pos_always=False):
    """_plant_call's arguments for the device form of every plant entry: marshalled once, they are what a kept call launches
    again.  They hold the structs; the tensors behind the structs' pointers are the caller's to keep.  base_pos goes over with
    `next` only, unless the entry reads it in any case (pos_always: dstate then needs it)."""
    B = dstate["q"].shape[0]
    if pos_always and (dstate.get("base_pos") is None or not _is(dstate["base_pos"], "float64", 3 * B)):
        raise ValueError("dstate['base_pos'] must be a contiguous float64 tensor of %d x 3 elements: this entry always reads it" % B)
    wb = _wholebody_batch(dstate, [])
    if free_flight:
        wb.support_leg = None
    nxt = None if next is None else PlantNext(*[_ptr(next[key]) for _, key, _ in PLANT_NEXT_FIELDS])
    return (ctx, wb, B, tau, g_ext, dstate.get("base_pos") if next is not None or pos_always else None, float(gravity), float(dt),
            acc, f, nxt, status, MEM_DEVICE, stream, entry, *structs)


def wholebody_forward_dynamics_device(ctx, dstate, tau, status, acc=None, f=None, g_ext=None, gravity=9.81, dt=0.0, next=None,
                                      free_flight=False, stream=None):
    """Same entry on torch CUDA tensors; asynchronous.  next: dict of tensors under the state's keys (q, qd, base_pos, base_quat,
    base_linvel, base_angvel) or NULL; it may be `dstate` itself, which then needs "base_pos" (a rollout in place)."""
    _plant_call(*_plant_device_args(ctx, dstate, tau, status, acc, f, g_ext, gravity, dt, next, free_flight, stream,
                                    lib().qlamd_wholebody_forward_dynamics_batch))


def full_tick(ctx, io, period, index_quirk=1, params=None, pid=None, memory=MEM_HOST, stream=None):
    """qlamd_full_tick_batch.  `io`: dict with the fields of qlamd_tick_batch (TICK_FIELDS: C-contiguous numpy arrays of
    those dtypes for host memory, torch CUDA tensors for device memory; `leg_state_code` and `command` may be None);
    in/out and out arrays are updated in place.  `set_memory` ([B, 4], in the place of `working_set`) and `iterations` ([B]) are
    the optional last members; a torch tensor holds their 32-bit words as int32."""
    prm = params if params is not None else default_swing_params()
    pidp = pid if pid is not None else default_joint_pid_params()
    tb = TickBatch()
    for name, dt in TICK_FIELDS:
        a = io.get(name)
        if a is None:
            continue
        if memory == MEM_HOST:
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], name
        setattr(tb, name, _ptr(a))
    B = int(io["offsets"].shape[0]) - 1
    sm = io.get("set_memory")
    if sm is not None:
        words = sm.numel() if hasattr(sm, "numel") else sm.size
        if words != 4 * B or (sm.element_size() if hasattr(sm, "element_size") else sm.itemsize) != 4:
            raise ValueError("set_memory must hold %d x 4 words of 32 bits" % B)
        if hasattr(sm, "is_contiguous") and not sm.is_contiguous():
            raise ValueError("set_memory must be contiguous")
    _call(lib().qlamd_full_tick_batch, ctx._h, C.byref(prm), C.byref(pidp), C.byref(tb), float(period), int(index_quirk), B, memory,
          _stream(stream))
    return io

"""ctypes view of libqc_balance.so (C ABI: include/qc_balance.h).

There is NO fallback: if the HIP library is missing or cannot be loaded the
import of the controller fails loudly.  The .so is built in-tree by
__graft_entry__.build() (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QC_LIB_PATH") or os.path.join(_HERE, "libqc_balance.so")  # QC_LIB_PATH: development builds (tools/)

QC_OK = 0
QC_ERR_INVALID = -1
QC_ERR_ABI = -4
ABI_VERSION = 6  # the revision of include/qc_balance.h these ctypes structures were written against
STATUS_NAMES = {0: "solved", 1: "max_iter", 2: "infeasible", 3: "not_pd"}


class QcParams(C.Structure):
    _fields_ = [("mu", C.c_double), ("mass", C.c_double), ("fzmin", C.c_double), ("fzmax", C.c_double),
                ("Ib", C.c_double * 9), ("S", C.c_double * 36), ("W", C.c_double * 144),
                ("kff", C.c_double * 6), ("kp_p", C.c_double * 3), ("kd_p", C.c_double * 3),
                ("kp_w", C.c_double * 3), ("kd_w", C.c_double * 3),
                ("max_iter", C.c_int32), ("reserved", C.c_int32)]


class QcBatchIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in
                ("Rwb", "Rwb_d", "x", "xdot", "w", "x_d", "xdot_d", "w_d", "feet", "stance", "joint_q", "gait_phase", "gait_duty",
                 "swing_pos", "swing_vel", "joint_qdot", "swing_state", "gait_dt")]


class QcBatchOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("grf_body", "status", "active_set", "iterations", "joint_tau")]


class QcKinematics(C.Structure):
    _fields_ = [("hip", C.c_double * 12), ("links", C.c_double * 12), ("tau_min", C.c_double), ("tau_max", C.c_double),
                ("jc_kff", C.c_double * 3), ("jc_kp", C.c_double * 3), ("jc_kd", C.c_double * 3),
                ("planner_hip", C.c_double * 12), ("planner_k", C.c_double), ("swing_height", C.c_double)]


class QcSwingState(C.Structure):
    _fields_ = [("leg_state", C.c_int32 * 4), ("has_traj", C.c_int32 * 4), ("p_start", C.c_double * 12), ("p_final", C.c_double * 12)]


class QcCommanderState(C.Structure):
    _fields_ = [("standing", C.c_int32), ("gait_running", C.c_int32), ("cmd_pending", C.c_int32), ("reserved", C.c_int32),
                ("Vb", C.c_double * 6), ("Rwb_d", C.c_double * 9), ("x_d", C.c_double * 3), ("xdot_d", C.c_double * 3), ("w_d", C.c_double * 3)]


class QcCommandIn(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("twist", C.c_void_p), ("fresh", C.c_void_p), ("state", C.c_void_p),
                ("stand_height", C.c_double), ("stand_tol", C.c_double), ("cmd_dt", C.c_double)]


class QcPlantIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("Rwb", C.c_void_p), ("x", C.c_void_p), ("xdot", C.c_void_p), ("w", C.c_void_p),
                ("grf_body", C.c_void_p), ("foot_world", C.c_void_p), ("feet", C.c_void_p), ("dt", C.c_double)]


class QcPlantAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("Rwb", "x", "xdot", "w", "grf_body", "foot_world", "Rwb_next_bar", "x_next_bar", "xdot_next_bar", "w_next_bar", "feet_next_bar",
                 "Rwb_bar", "x_bar", "xdot_bar", "w_bar", "grf_bar", "foot_world_bar")] + [("dt", C.c_double)]


class QcLegPlantIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "joint_tau", "stance", "gait_phase", "gait_duty", "cmd_state",
                 "foot_world", "flags")] + [("leg_inertia", C.c_double * 3), ("dt", C.c_double)]


class QcLegPlantAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "joint_tau", "stance", "gait_phase", "gait_duty", "cmd_state",
                 "Rwb_next_bar", "x_next_bar", "xdot_next_bar", "w_next_bar", "joint_q_next_bar", "joint_qdot_next_bar",
                 "Rwb_bar", "x_bar", "xdot_bar", "w_bar", "joint_q_bar", "joint_qdot_bar", "joint_tau_bar", "flags")] + [
                ("leg_inertia", C.c_double * 3), ("dt", C.c_double)]


class QcCertifySummary(C.Structure):
    _fields_ = [("n_fail", C.c_int64), ("n_nonfinite", C.c_int64), ("n_swing_nonzero", C.c_int64), ("worst_primal", C.c_double),
                ("worst_stationarity", C.c_double), ("arg_primal", C.c_int64), ("arg_stationarity", C.c_int64)]


class QcCertifyIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("act_tol", C.c_double), ("primal_tol", C.c_double),
                ("stat_tol", C.c_double)] + [(k, C.c_void_p) for k in
                ("primal", "stationarity", "lambda", "grad", "active", "flags", "summary")]


class QcSensitivityIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("grf_bar", C.c_void_p), ("act_tol", C.c_double)] + [(k, C.c_void_p) for k in
                ("adjoint", "b_bar", "feet_bar", "x_bar", "xdot_bar", "w_bar", "x_d_bar", "xdot_d_bar", "w_d_bar", "flags")]


class QcSensitivityRotIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("grf_body", "grf_bar", "b_bar", "feet_bar", "Rwb_bar", "Rwb_d_bar", "Rwb_rot_bar", "Rwb_d_rot_bar")]


class QcSensitivityParamIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("grf_bar", C.c_void_p), ("adjoint", C.c_void_p), ("act_tol", C.c_double),
                ("param_bar_rows", C.c_void_p), ("param_bar", C.c_void_p)]


class QcSensitivityKinIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("grf_body", "status", "joint_tau_bar", "feet_bar", "grf_bar_in", "joint_q_bar_in", "grf_bar", "joint_q_bar")]


class QcSensitivitySwingIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("joint_tau_bar", "joint_q_bar_in", "Rwb_bar_in", "x_bar_in", "swing_pos_bar", "swing_vel_bar", "joint_q_bar", "joint_qdot_bar",
                 "gain_bar", "Rwb_bar", "x_bar", "flags")]


class QcSwingReferenceIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in ("swing_pos", "swing_vel", "planned")]


class QcSwingReferenceAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("state_before", "swing_pos_bar", "swing_vel_bar", "p_start_next_bar", "p_final_next_bar", "Rwb_bar_in", "x_bar_in", "xdot_bar_in",
                 "w_bar_in", "joint_q_bar_in", "Rwb_bar", "x_bar", "xdot_bar", "w_bar", "xdot_d_bar", "joint_q_bar", "p_start_bar", "p_final_bar",
                 "flags")]


class QcCommanderStepIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in ("Rwb_d", "x_d", "xdot_d", "w_d", "run", "applied")]


class QcCommanderStepAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in
                ("state_before", "Rwb_d_bar", "x_d_bar", "xdot_d_bar", "w_d_bar", "Vb_next_bar", "Rwb_bar_in", "x_bar_in", "twist_bar", "Vb_bar",
                 "Rwb_bar", "x_bar", "Rwb_d_prev_bar", "x_d_prev_bar", "xdot_d_prev_bar", "w_d_prev_bar", "flags")]


class QcSupportPolygonIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("schedule", C.c_void_p), ("schedule_shared", C.c_int32), ("world", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("com_xy", "weights", "flags")]


class QcSupportPolygonAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("schedule", C.c_void_p), ("schedule_shared", C.c_int32), ("world", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("com_xy_bar", "feet_bar_in", "Rwb_bar_in", "x_bar_in", "phase_bar_in", "schedule_bar_in", "feet_bar",
                                          "Rwb_bar", "x_bar", "phase_bar", "schedule_bar", "flags")]


COM_MODES = {"replace": 0, "offset": 1}  # QC_COM_REPLACE, QC_COM_OFFSET


class QcComReferenceIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("schedule", C.c_void_p), ("schedule_shared", C.c_int32), ("mode", C.c_int32), ("gain", C.c_double)] + \
               [(k, C.c_void_p) for k in ("x_d_in", "x_d_out", "com_xy", "flags")]


class QcComReferenceAdjointIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("schedule", C.c_void_p), ("schedule_shared", C.c_int32), ("mode", C.c_int32), ("gain", C.c_double)] + \
               [(k, C.c_void_p) for k in ("x_d_out_bar", "feet_bar_in", "Rwb_bar_in", "x_bar_in", "phase_bar_in", "schedule_bar_in", "x_d_in_bar",
                                          "feet_bar", "Rwb_bar", "x_bar", "phase_bar", "schedule_bar", "schedule_bar_sum", "flags")]


PARAM_COUNT = 211  # QC_PARAM_COUNT: the doubles of QcParams, in its order


class QcLaunchInfo(C.Structure):
    _fields_ = [("lanes_per_robot", C.c_int32), ("mode", C.c_int32), ("form", C.c_int32), ("strategies", C.c_int32),
                ("chunk", C.c_int64), ("blocks", C.c_int64), ("resident_workgroups", C.c_int64), ("lds_bytes", C.c_int64)]


EXPORTS = ("qc_create_abi", "qc_destroy", "qc_control_batch", "qc_control_batch_host", "qc_control",
           "qc_last_error", "qc_kernel_name", "qc_abi_version", "qc_default_kinematics", "qc_set_kinematics", "qc_set_gait", "qc_swing_state_init",
           "qc_set_tuning", "qc_query_launch", "qc_check_abi", "qc_default_command", "qc_commander_state_init", "qc_tick_batch",
           "qc_default_plant", "qc_plant_step_batch", "qc_default_leg_plant", "qc_leg_plant_step_batch",
           "qc_default_certify", "qc_certify_batch", "qc_default_sensitivity", "qc_sensitivity_batch",
           "qc_default_sensitivity_rot", "qc_sensitivity_rot_batch", "qc_default_plant_adjoint", "qc_plant_step_adjoint_batch",
           "qc_default_sensitivity_param", "qc_sensitivity_param_batch", "qc_default_sensitivity_kin", "qc_sensitivity_kin_batch",
           "qc_default_leg_plant_adjoint", "qc_leg_plant_step_adjoint_batch", "qc_default_sensitivity_swing", "qc_sensitivity_swing_batch",
           "qc_default_swing_reference", "qc_swing_reference_batch", "qc_default_swing_reference_adjoint", "qc_swing_reference_adjoint_batch",
           "qc_default_commander_step", "qc_commander_step_batch", "qc_default_commander_step_adjoint", "qc_commander_step_adjoint_batch",
           "qc_default_support_polygon", "qc_support_polygon_batch", "qc_default_support_polygon_adjoint", "qc_support_polygon_adjoint_batch",
           "qc_default_com_reference", "qc_com_reference_batch", "qc_default_com_reference_adjoint", "qc_com_reference_adjoint_batch")

_lib = None


def load():
    """Load the HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 /
    # libhsa-runtime64 (same SONAME as /opt/rocm's).  If our library were loaded
    # first it would pull in /opt/rocm's copy and a later `import torch` would
    # bring up a second HSA runtime that sees no GPU.  Importing torch first
    # makes the dynamic loader resolve our NEEDED libamdhip64.so.7 to the copy
    # torch already mapped.  (A C++ host that never loads torch simply uses
    # /opt/rocm's runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - torch is optional plumbing
        pass
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"{LIB_PATH} does not export {name}")
    # (ABI v6: the exported constructor takes the caller's ABI revision and struct sizes; `qc_create` is an inline wrapper in the header)
    lib.qc_create_abi.argtypes = [C.POINTER(QcParams), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_size_t, C.c_size_t]
    lib.qc_create_abi.restype = C.c_int
    lib.qc_destroy.argtypes = [C.c_void_p]
    lib.qc_destroy.restype = None
    lib.qc_control_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.c_void_p,
                                     C.POINTER(QcBatchOut), C.c_void_p]
    lib.qc_control_batch.restype = C.c_int
    lib.qc_control_batch_host.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.c_void_p,
                                          C.POINTER(QcBatchOut)]
    lib.qc_control_batch_host.restype = C.c_int
    lib.qc_control.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_void_p, C.c_void_p]
    lib.qc_control.restype = C.c_int
    lib.qc_last_error.restype = C.c_char_p
    lib.qc_kernel_name.argtypes = [C.c_void_p]
    lib.qc_kernel_name.restype = C.c_char_p
    lib.qc_abi_version.restype = C.c_int
    lib.qc_default_kinematics.argtypes = [C.POINTER(QcKinematics)]
    lib.qc_default_kinematics.restype = None
    lib.qc_set_kinematics.argtypes = [C.c_void_p, C.POINTER(QcKinematics)]
    lib.qc_set_kinematics.restype = C.c_int
    lib.qc_set_gait.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.qc_set_gait.restype = C.c_int
    lib.qc_swing_state_init.argtypes = [C.c_void_p, C.c_size_t]
    lib.qc_swing_state_init.restype = None
    lib.qc_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    lib.qc_set_tuning.restype = C.c_int
    lib.qc_query_launch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(QcLaunchInfo)]
    lib.qc_query_launch.restype = C.c_int
    lib.qc_check_abi.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t]
    lib.qc_check_abi.restype = C.c_int
    lib.qc_default_command.argtypes = [C.POINTER(QcCommandIn)]
    lib.qc_default_command.restype = None
    lib.qc_commander_state_init.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.qc_commander_state_init.restype = None
    lib.qc_tick_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcCommandIn), C.c_void_p,
                                  C.POINTER(QcBatchOut), C.c_void_p]
    lib.qc_tick_batch.restype = C.c_int
    lib.qc_default_plant.argtypes = [C.POINTER(QcPlantIo)]
    lib.qc_default_plant.restype = None
    lib.qc_plant_step_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcPlantIo), C.c_void_p]
    lib.qc_plant_step_batch.restype = C.c_int
    lib.qc_default_leg_plant.argtypes = [C.POINTER(QcLegPlantIo)]
    lib.qc_default_leg_plant.restype = None
    lib.qc_leg_plant_step_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcLegPlantIo), C.c_void_p]
    lib.qc_leg_plant_step_batch.restype = C.c_int
    lib.qc_default_certify.argtypes = [C.POINTER(QcCertifyIo)]
    lib.qc_default_certify.restype = None
    lib.qc_certify_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcCertifyIo), C.c_void_p]
    lib.qc_certify_batch.restype = C.c_int
    lib.qc_default_sensitivity.argtypes = [C.POINTER(QcSensitivityIo)]
    lib.qc_default_sensitivity.restype = None
    lib.qc_sensitivity_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSensitivityIo), C.c_void_p]
    lib.qc_sensitivity_batch.restype = C.c_int
    lib.qc_default_sensitivity_rot.argtypes = [C.POINTER(QcSensitivityRotIo)]
    lib.qc_default_sensitivity_rot.restype = None
    lib.qc_sensitivity_rot_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSensitivityRotIo), C.c_void_p]
    lib.qc_sensitivity_rot_batch.restype = C.c_int
    lib.qc_default_sensitivity_param.argtypes = [C.POINTER(QcSensitivityParamIo)]
    lib.qc_default_sensitivity_param.restype = None
    lib.qc_sensitivity_param_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSensitivityParamIo), C.c_void_p]
    lib.qc_sensitivity_param_batch.restype = C.c_int
    lib.qc_default_sensitivity_kin.argtypes = [C.POINTER(QcSensitivityKinIo)]
    lib.qc_default_sensitivity_kin.restype = None
    lib.qc_sensitivity_kin_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSensitivityKinIo), C.c_void_p]
    lib.qc_sensitivity_kin_batch.restype = C.c_int
    lib.qc_default_plant_adjoint.argtypes = [C.POINTER(QcPlantAdjointIo)]
    lib.qc_default_plant_adjoint.restype = None
    lib.qc_plant_step_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcPlantAdjointIo), C.c_void_p]
    lib.qc_plant_step_adjoint_batch.restype = C.c_int
    lib.qc_default_leg_plant_adjoint.argtypes = [C.POINTER(QcLegPlantAdjointIo)]
    lib.qc_default_leg_plant_adjoint.restype = None
    lib.qc_leg_plant_step_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcLegPlantAdjointIo), C.c_void_p]
    lib.qc_leg_plant_step_adjoint_batch.restype = C.c_int
    lib.qc_default_sensitivity_swing.argtypes = [C.POINTER(QcSensitivitySwingIo)]
    lib.qc_default_sensitivity_swing.restype = None
    lib.qc_sensitivity_swing_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSensitivitySwingIo), C.c_void_p]
    lib.qc_sensitivity_swing_batch.restype = C.c_int
    lib.qc_default_swing_reference.argtypes = [C.POINTER(QcSwingReferenceIo)]
    lib.qc_default_swing_reference.restype = None
    lib.qc_swing_reference_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSwingReferenceIo), C.c_void_p]
    lib.qc_swing_reference_batch.restype = C.c_int
    lib.qc_default_swing_reference_adjoint.argtypes = [C.POINTER(QcSwingReferenceAdjointIo)]
    lib.qc_default_swing_reference_adjoint.restype = None
    lib.qc_swing_reference_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSwingReferenceAdjointIo), C.c_void_p]
    lib.qc_swing_reference_adjoint_batch.restype = C.c_int
    lib.qc_default_commander_step.argtypes = [C.POINTER(QcCommanderStepIo)]
    lib.qc_default_commander_step.restype = None
    lib.qc_commander_step_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcCommandIn), C.POINTER(QcCommanderStepIo), C.c_void_p]
    lib.qc_commander_step_batch.restype = C.c_int
    lib.qc_default_commander_step_adjoint.argtypes = [C.POINTER(QcCommanderStepAdjointIo)]
    lib.qc_default_commander_step_adjoint.restype = None
    lib.qc_commander_step_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcCommandIn), C.POINTER(QcCommanderStepAdjointIo),
                                                    C.c_void_p]
    lib.qc_commander_step_adjoint_batch.restype = C.c_int
    lib.qc_default_support_polygon.argtypes = [C.POINTER(QcSupportPolygonIo)]
    lib.qc_default_support_polygon.restype = None
    lib.qc_support_polygon_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSupportPolygonIo), C.c_void_p]
    lib.qc_support_polygon_batch.restype = C.c_int
    lib.qc_default_support_polygon_adjoint.argtypes = [C.POINTER(QcSupportPolygonAdjointIo)]
    lib.qc_default_support_polygon_adjoint.restype = None
    lib.qc_support_polygon_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcSupportPolygonAdjointIo), C.c_void_p]
    lib.qc_support_polygon_adjoint_batch.restype = C.c_int
    lib.qc_default_com_reference.argtypes = [C.POINTER(QcComReferenceIo)]
    lib.qc_default_com_reference.restype = None
    lib.qc_com_reference_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcComReferenceIo), C.c_void_p]
    lib.qc_com_reference_batch.restype = C.c_int
    lib.qc_default_com_reference_adjoint.argtypes = [C.POINTER(QcComReferenceAdjointIo)]
    lib.qc_default_com_reference_adjoint.restype = None
    lib.qc_com_reference_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcBatchIn), C.POINTER(QcComReferenceAdjointIo), C.c_void_p]
    lib.qc_com_reference_adjoint_batch.restype = C.c_int
    # the structures above are hand-written mirrors of the header: a library built from another revision is refused here,
    # before any of them crosses the boundary
    rc = lib.qc_check_abi(ABI_VERSION, C.sizeof(QcParams), C.sizeof(QcBatchIn), C.sizeof(QcBatchOut))
    if rc != QC_OK:
        raise ImportError(f"{LIB_PATH}: {lib.qc_last_error().decode()}")
    _lib = lib
    return lib


def create(lib, params, device, handle):
    """qc_create for this binding: qc_create_abi with the revision and the sizes of the ctypes mirrors above."""
    return lib.qc_create_abi(C.byref(params), int(device), C.byref(handle), ABI_VERSION, C.sizeof(QcParams), C.sizeof(QcBatchIn), C.sizeof(QcBatchOut))


def last_error():
    return load().qc_last_error().decode()

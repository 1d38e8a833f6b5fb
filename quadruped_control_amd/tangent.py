"""Forward mode of the balance QP (include/qc_tangent.h, csrc/qc_tangent.hpp): tangents of the inputs of a solved batch pushed
through the QP on its active face, and the Jacobian d grf_body / d inputs as the tangent call on unit seeds.

The plant step's forward mode (qc_plant_step_tangent_batch, csrc/qc_plant_tangent.hpp) follows it: plant_step_tangent(), and the two
chained step after step - rollout_tangent(), the forward-mode twin of rollout(), and rollout_transition(), the 12 x 12
state-transition matrix of a closed-loop rollout.

The loop around the complete tick has its forward mode too: torque_tangent() (qc_torque_tangent_batch, csrc/qc_torque_tangent.hpp),
the clamped J^T torque map, and leg_plant_step_tangent() (qc_leg_plant_step_tangent_batch, csrc/qc_leg_plant_tangent.hpp), the legged
plant; rollout_tick_tangent() chains them with tangent_batch() into the forward-mode twin of ctl.rollout_tick(batch, None, ...), and
rollout_tick_transition() is its 36 x 36 state-transition matrix.

A trot has its forward mode as well: swing_torque_tangent() (qc_swing_torque_tangent_batch, csrc/qc_swing_tangent.hpp), the swing legs'
PD torques on references that are given, chained in place behind torque_tangent(); rollout_swing_tangent() is the forward-mode twin of
ctl.rollout_tick(batch, None, ...) for a batch with swing_pos and swing_vel, rollout_swing_transition() its 36 x 36 matrix.

The planner has its forward mode too: swing_reference_tangent() (qc_swing_reference_tangent_batch, csrc/qc_swing_reference_tangent.hpp),
the foothold planner and the sextic swing trajectory at held plan decisions; rollout_gait_tangent() is the forward-mode twin of
ctl.rollout_tick(batch, None, ...) for a batch with swing_state and a running clock - of rollout_gait_autograd() -, and
rollout_gait_transition() its 60 x 60 matrix: the 36 coordinates of the tick and the record's p_start[12], p_final[12].

The functions take the controller as their first argument, as autograd.py's do.  The symbols of the library are bound here, on
the CDLL that _lib.load() returns, with this module's own ctypes records: _lib.EXPORTS and BalanceController are not touched.

The two stages a rollout is steered through have theirs: commander_step_tangent() (qc_commander_step_tangent_batch) - the twist
command, the held command, the pose and the record's desired state to the desired state the QP and the planner are fed - and
com_reference_tangent() (qc_com_reference_tangent_batch) - the feet, the pose, the phases and the schedule of the lean to x_d; both in
csrc/qc_command_tangent.hpp.

rollout_commander_tangent() - the forward-mode twin of ctl.rollout_tick(batch, command, ...) and of
rollout_commander_autograd() - and rollout_lean_tangent() - that of ctl.rollout_tick(batch, None, ..., lean=...) and of
rollout_gait_autograd(lean=...) - chain them in front of rollout_gait_tangent()'s step.

The handle's own parameters have their forward mode too: param_tangent() (qc_param_tangent_batch, csrc/qc_param_tangent.hpp) pushes
K directions in the 211 doubles of PARAM_LAYOUT through the QP - the transpose of autograd.py's params=theta -,
param_jacobian_batch() is d grf_body / d theta on unit seeds, and every rollout here takes `params_tan`.

Not covered: tangents of the gait clock (the phases, the contact mask and the plan decisions are held), tangents of the kinematic
model, the joint gains and the plant's use of mass and Ib, and a jvp on the torch.autograd.Functions of autograd.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .balance_controller import _KINEMATICS_FIELDS, _READONLY_FIELDS, COMMANDER_STATE_DTYPE, _check_tensor, _fill, _RolloutPlans, _outputs

# name -> values per robot; the names are the record's fields
TANGENTS = {"x_tan": 3, "xdot_tan": 3, "w_tan": 3, "x_d_tan": 3, "xdot_d_tan": 3, "w_d_tan": 3, "Rwb_rot_tan": 3, "Rwb_d_rot_tan": 3,
            "feet_tan": 12, "joint_q_tan": 12}
_TANGENT_OUTPUTS = {"grf_tan": ((4, 3), "float64"), "b_tan": ((6,), "float64")}
JACOBIAN_WRT = ("x", "xdot", "w", "x_d", "xdot_d", "w_d", "Rwb_rot", "Rwb_d_rot")  # jacobian_batch's default; "feet" and "joint_q" are allowed too
# the plant step's forward mode (qc_plant_tangent_io): its input tangents and its outputs
PLANT_TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "xdot_tan": 3, "w_tan": 3, "grf_tan": 12, "foot_world_tan": 12}
_PLANT_TANGENT_OUTPUTS = {"Rwb_rot_next_tan": ((3,), "float64"), "x_next_tan": ((3,), "float64"), "xdot_next_tan": ((3,), "float64"),
                          "w_next_tan": ((3,), "float64"), "feet_next_tan": ((4, 3), "float64")}
PLANT_TANGENT_WANT = tuple(_PLANT_TANGENT_OUTPUTS)
# rollout_tangent(): what `tangents` may hold - the start state's, step 0's feet_tan, and the held ones, applied at every step
_ROLLOUT_STATE = ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan")
_ROLLOUT_HELD = ("x_d_tan", "xdot_d_tan", "w_d_tan", "Rwb_d_rot_tan")
ROLLOUT_TANGENTS = {**{k: 3 for k in _ROLLOUT_STATE}, "feet_tan": 12, "foot_world_tan": 12, **{k: 3 for k in _ROLLOUT_HELD}}
TRANSITION_COLUMNS = tuple((name, c) for name in ("Rwb_rot", "x", "xdot", "w") for c in range(3))  # rollout_transition's rows and columns


# the torque map's forward mode (qc_torque_tangent_io) and the leg plant's (qc_leg_plant_tangent_io)
TORQUE_TANGENTS = {"grf_tan": 12, "joint_q_tan": 12}
_TORQUE_TANGENT_OUTPUTS = {"joint_tau_tan": ((4, 3), "float64")}
LEG_PLANT_TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "xdot_tan": 3, "w_tan": 3, "joint_q_tan": 12, "joint_qdot_tan": 12, "joint_tau_tan": 12}
_LEG_PLANT_TANGENT_OUTPUTS = {**{k: ((3,), "float64") for k in ("Rwb_rot_next_tan", "x_next_tan", "xdot_next_tan", "w_next_tan")},
                              "joint_q_next_tan": ((4, 3), "float64"), "joint_qdot_next_tan": ((4, 3), "float64")}
LEG_PLANT_TANGENT_WANT = tuple(_LEG_PLANT_TANGENT_OUTPUTS)
# rollout_tick_tangent(): the start state's six tangents and the held ones; rollout_tick_transition()'s 36 coordinates
_TICK_STATE = ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan", "joint_qdot_tan")
ROLLOUT_TICK_TANGENTS = {**{k: LEG_PLANT_TANGENTS[k] for k in _TICK_STATE}, **{k: 3 for k in _ROLLOUT_HELD}}
TICK_TRANSITION_COLUMNS = tuple((name, c) for name in ("Rwb_rot", "x", "xdot", "w") for c in range(3)) + \
    tuple((name, c) for name in ("joint_q", "joint_qdot") for c in range(12))
TICK_PLANT_FLAGS_SHIFT = 8  # rollout_tick_tangent()'s flags: tangent_batch()'s bits | the plant's bits << 8

# the swing legs' PD torques (qc_swing_tangent_io): the record's tangents in its order, and rollout_swing_tangent()'s - the tick's
# and the two held references'
SWING_TORQUE_TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "swing_pos_tan": 12, "swing_vel_tan": 12, "joint_q_tan": 12, "joint_qdot_tan": 12,
                         "joint_tau_tan_in": 12}
_SWING_TORQUE_TANGENT_OUTPUTS = {"joint_tau_tan": ((4, 3), "float64")}
_SWING_HELD = ("swing_pos_tan", "swing_vel_tan")
ROLLOUT_SWING_TANGENTS = {**ROLLOUT_TICK_TANGENTS, **{k: 12 for k in _SWING_HELD}}
SWING_FLAGS_SHIFT = 16  # rollout_swing_tangent()'s flags: rollout_tick_tangent()'s word | swing_torque_tangent()'s bits << 16

# the planner and the swing trajectory (qc_swing_reference_tangent_io): the record's tangents and outputs in its order;
# rollout_gait_tangent()'s tangents - the tick's and the two of the start record - and rollout_gait_transition()'s 60 coordinates
SWING_REFERENCE_TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "xdot_tan": 3, "w_tan": 3, "xdot_d_tan": 3, "joint_q_tan": 12, "p_start_tan": 12, "p_final_tan": 12}
_SWING_REFERENCE_TANGENT_OUTPUTS = {"swing_pos_tan": ((4, 3), "float64"), "swing_vel_tan": ((4, 3), "float64"),
                                    "p_start_next_tan": ((12,), "float64"), "p_final_next_tan": ((12,), "float64")}
SWING_REFERENCE_TANGENT_WANT = tuple(_SWING_REFERENCE_TANGENT_OUTPUTS)
_GAIT_RECORD = ("p_start_tan", "p_final_tan")
ROLLOUT_GAIT_TANGENTS = {**ROLLOUT_TICK_TANGENTS, **{k: 12 for k in _GAIT_RECORD}}
GAIT_TRANSITION_COLUMNS = TICK_TRANSITION_COLUMNS + tuple((name, c) for name in ("p_start", "p_final") for c in range(12))
REFERENCE_FLAGS_SHIFT = 20  # rollout_gait_tangent()'s flags: rollout_swing_tangent()'s word | swing_reference_tangent()'s bits << 20

# the commander step (qc_commander_step_tangent_io) and the com reference (qc_com_reference_tangent_io): the records' tangents and
# outputs in their order
COMMANDER_STEP_TANGENTS = {"twist_tan": 6, "Vb_tan": 6, "Rwb_rot_tan": 3, "x_tan": 3, "Rwb_d_rot_prev_tan": 3, "x_d_prev_tan": 3, "xdot_d_prev_tan": 3,
                           "w_d_prev_tan": 3}
_COMMANDER_STEP_TANGENT_OUTPUTS = {**{k: ((3,), "float64") for k in ("Rwb_d_rot_tan", "x_d_tan", "xdot_d_tan", "w_d_tan")}, "Vb_next_tan": ((6,), "float64")}
COMMANDER_STEP_TANGENT_WANT = tuple(_COMMANDER_STEP_TANGENT_OUTPUTS)
COM_REFERENCE_TANGENTS = {"x_d_in_tan": 3, "feet_tan": 12, "joint_q_tan": 12, "Rwb_rot_tan": 3, "x_tan": 3, "phase_tan": 4, "schedule_tan": 16}
_COM_REFERENCE_TANGENT_OUTPUTS = {"x_d_out_tan": ((3,), "float64"), "com_xy_tan": ((2,), "float64")}


class QcCommanderStepTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("state_before", C.c_void_p), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in tuple(COMMANDER_STEP_TANGENTS) + COMMANDER_STEP_TANGENT_WANT + ("flags",)]


class QcComReferenceTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("schedule", C.c_void_p), ("schedule_shared", C.c_int32), ("mode", C.c_int32), ("gain", C.c_double),
                ("n_dir", C.c_size_t)] + [(k, C.c_void_p) for k in tuple(COM_REFERENCE_TANGENTS) + tuple(_COM_REFERENCE_TANGENT_OUTPUTS) + ("flags",)]


class QcSwingReferenceTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("state_before", C.c_void_p), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in tuple(SWING_REFERENCE_TANGENTS) + SWING_REFERENCE_TANGENT_WANT + ("flags",)]


class QcSwingTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("n_dir", C.c_size_t)] + [(k, C.c_void_p) for k in tuple(SWING_TORQUE_TANGENTS) + ("joint_tau_tan", "flags")]


class QcTorqueTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("status", C.c_void_p), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in ("grf_tan", "joint_q_tan", "joint_tau_tan")]


class QcLegPlantTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + \
               [(k, C.c_void_p) for k in ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "joint_tau", "stance", "gait_phase", "gait_duty", "cmd_state")] + \
               [("leg_inertia", C.c_double * 3), ("dt", C.c_double), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in tuple(LEG_PLANT_TANGENTS) + LEG_PLANT_TANGENT_WANT + ("flags",)]


class QcTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("act_tol", C.c_double), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in tuple(TANGENTS) + ("grf_tan", "b_tan", "flags")]


class QcParamTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("act_tol", C.c_double), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in ("param_tan", "grf_tan_in", "b_tan_in", "grf_tan", "b_tan", "flags")]


class QcPlantTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in ("Rwb", "x", "xdot", "w", "grf_body", "foot_world")] + \
               [("dt", C.c_double), ("n_dir", C.c_size_t)] + [(k, C.c_void_p) for k in tuple(PLANT_TANGENTS) + PLANT_TANGENT_WANT]


_bound = None


def _library():
    """the library with this module's symbols bound"""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name in ("qc_default_tangent", "qc_tangent_batch", "qc_default_plant_tangent", "qc_plant_step_tangent_batch", "qc_default_torque_tangent",
                     "qc_torque_tangent_batch", "qc_default_leg_plant_tangent", "qc_leg_plant_step_tangent_batch", "qc_default_swing_tangent",
                     "qc_swing_torque_tangent_batch", "qc_default_swing_reference_tangent", "qc_swing_reference_tangent_batch",
                     "qc_default_commander_step_tangent", "qc_commander_step_tangent_batch", "qc_default_com_reference_tangent",
                     "qc_com_reference_tangent_batch", "qc_default_param_tangent", "qc_param_tangent_batch"):
            if not hasattr(lib, name):
                raise ImportError(f"{_lib.LIB_PATH} does not export {name}")
        lib.qc_default_tangent.argtypes = [C.POINTER(QcTangentIo)]
        lib.qc_default_tangent.restype = None
        lib.qc_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcTangentIo), C.c_void_p]
        lib.qc_tangent_batch.restype = C.c_int
        lib.qc_default_plant_tangent.argtypes = [C.POINTER(QcPlantTangentIo)]
        lib.qc_default_plant_tangent.restype = None
        lib.qc_plant_step_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcPlantTangentIo), C.c_void_p]
        lib.qc_plant_step_tangent_batch.restype = C.c_int
        lib.qc_default_torque_tangent.argtypes = [C.POINTER(QcTorqueTangentIo)]
        lib.qc_default_torque_tangent.restype = None
        lib.qc_torque_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcTorqueTangentIo), C.c_void_p]
        lib.qc_torque_tangent_batch.restype = C.c_int
        lib.qc_default_leg_plant_tangent.argtypes = [C.POINTER(QcLegPlantTangentIo)]
        lib.qc_default_leg_plant_tangent.restype = None
        lib.qc_leg_plant_step_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(QcLegPlantTangentIo), C.c_void_p]
        lib.qc_leg_plant_step_tangent_batch.restype = C.c_int
        lib.qc_default_swing_tangent.argtypes = [C.POINTER(QcSwingTangentIo)]
        lib.qc_default_swing_tangent.restype = None
        lib.qc_swing_torque_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcSwingTangentIo), C.c_void_p]
        lib.qc_swing_torque_tangent_batch.restype = C.c_int
        lib.qc_default_swing_reference_tangent.argtypes = [C.POINTER(QcSwingReferenceTangentIo)]
        lib.qc_default_swing_reference_tangent.restype = None
        lib.qc_swing_reference_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcSwingReferenceTangentIo), C.c_void_p]
        lib.qc_swing_reference_tangent_batch.restype = C.c_int
        lib.qc_default_commander_step_tangent.argtypes = [C.POINTER(QcCommanderStepTangentIo)]
        lib.qc_default_commander_step_tangent.restype = None
        lib.qc_commander_step_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(_lib.QcCommandIn),
                                                        C.POINTER(QcCommanderStepTangentIo), C.c_void_p]
        lib.qc_commander_step_tangent_batch.restype = C.c_int
        lib.qc_default_com_reference_tangent.argtypes = [C.POINTER(QcComReferenceTangentIo)]
        lib.qc_default_com_reference_tangent.restype = None
        lib.qc_com_reference_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcComReferenceTangentIo), C.c_void_p]
        lib.qc_com_reference_tangent_batch.restype = C.c_int
        lib.qc_default_param_tangent.argtypes = [C.POINTER(QcParamTangentIo)]
        lib.qc_default_param_tangent.restype = None
        lib.qc_param_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcParamTangentIo), C.c_void_p]
        lib.qc_param_tangent_batch.restype = C.c_int
        _bound = lib
    return _bound


def _directions(tangents, table, n, dev, io=None):
    """The tangents that are given (not None), validated against `table` (name -> values per robot): contiguous float64 on `dev`,
    each [n, ...] (one direction, squeezed) or [K, n, ...], all agreeing.  Sets each pointer in `io`.  Returns (given, K, squeeze);
    K is 1 when there is none (no tangent at all is the library's refusal)."""
    import torch

    given = {k: t for k, t in tangents.items() if t is not None}
    K, squeeze = None, False
    for k, t in given.items():
        m = table[k]
        bad = ValueError(f"{k}: need contiguous float64 [{n},{m}] or [K,{n},{m}] on {dev}")
        if t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev or t.dim() < 1 or t.numel() == 0:
            raise bad
        stacked = t.dim() >= 2 and t.shape[1] == n and t.shape[0] * n * m == t.numel()  # [K, n, ...]
        flat = not stacked and t.shape[0] == n and t.numel() == n * m                   # [n, ...]: K = 1, squeezed
        if not stacked and not flat:
            raise bad
        lead = t.shape[0] if stacked else 1
        if K is None:
            K, squeeze = lead, flat
        elif K != lead or squeeze != flat:
            raise ValueError(f"{k}: the tangents must agree on the number of directions and on the [n, ...] / [K, n, ...] form")
        if io is not None:
            setattr(io, k, t.data_ptr())
    return given, (1 if K is None else K), squeeze


def plan_tangent(ctl, batch, grf_body, tangents, want=("grf_tan",), act_tol=1e-7, out=None, stream=None):
    """tangent_batch() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_tangent_batch call (graph-capturable)
    on tensors that are read in place; `out` holds [K, n, ...] tensors and squeeze says whether the tangents came as [n, ...].
    Planning launches nothing."""
    _library()
    unknown = [k for k in tangents if k not in TANGENTS]
    if unknown:
        raise ValueError(f"tangent: unknown tangent(s) {unknown}; the tangents are {tuple(TANGENTS)}")
    io = QcTangentIo()
    ctl._lib.qc_default_tangent(C.byref(io))
    n, dev, bi = ctl._readonly_batch("tangent", batch, _READONLY_FIELDS, io, [("grf_body", grf_body, 12)])
    given, K, squeeze = _directions(tangents, TANGENTS, n, dev, io)
    io.n_dir = K
    io.act_tol = float(act_tol)
    wanted = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("tangent", _TANGENT_OUTPUTS, wanted, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)), (batch, grf_body, given, res, bi, io), ValueError)
    return launch, res, squeeze


def tangent_batch(ctl, batch, grf_body, tangents, want=("grf_tan",), act_tol=1e-7, out=None, stream=None):
    """Forward mode of the balance QP on the active face of `grf_body` [n,12] (as control_batch() wrote it) for the batch the solve
    read (qc_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode: tangents and the Jacobian").  `tangents`: a dict of
    device tensors named as the record's fields - "x_tan", "xdot_tan", "w_tan", "x_d_tan", "xdot_d_tan", "w_d_tan", "Rwb_rot_tan",
    "Rwb_d_rot_tan" ([n,3]; the rotation tangents are world-frame left tangents, R <- exp([d]x) R), "feet_tan" [n,4,3] (body frame)
    and "joint_q_tan" [n,12] (only for a batch with joint_q) - each [n, ...] for one direction or [K, n, ...] for K, all agreeing on
    K; a missing one is zero.  `want`: any of "grf_tan" [K,n,4,3] (body frame), "b_tan" [K,n,6] and "flags" int32 [n] (bit 0: a foot
    on both rows of an axis, the derivative is one-sided; bit 1: a bad pivot, the robot's outputs are NaN in every direction).
    The reduced system is factorised once per robot and substituted K times in one launch.  Nothing of `batch` is written.
    Asynchronous on `stream`, no synchronisation.  Returns the dict of device tensors, [K, n, ...] - squeezed to [n, ...] where the
    tangents came that way; `out`: a dict of tensors with K * n rows to write into.  ValueError with the library's message for a
    call it refuses.  Not covered: entrywise rotation tangents, tangents of the handle's parameters and of the swing pipeline (the
    torque map and the leg plant have their own calls, torque_tangent() and leg_plant_step_tangent())."""
    launch, res, squeeze = plan_tangent(ctl, batch, grf_body, tangents, want, act_tol, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def jacobian_columns(wrt=JACOBIAN_WRT):
    """the columns of jacobian_batch(): the list of (name, component)"""
    unknown = [w for w in wrt if w + "_tan" not in TANGENTS]
    if unknown:
        raise ValueError(f"jacobian: unknown input(s) {unknown}; wrt is a subset of {tuple(k[:-4] for k in TANGENTS)}")
    return [(w, c) for w in wrt for c in range(TANGENTS[w + "_tan"])]


def jacobian_batch(ctl, batch, grf_body, wrt=JACOBIAN_WRT, act_tol=1e-7, chunk=None, stream=None):
    """The Jacobian d grf_body / d inputs of a solved batch on its active face: tangent_batch() on unit seeds built on the device,
    `chunk` directions per launch (None: all in one).  `wrt`: any of "x", "xdot", "w", "x_d", "xdot_d", "w_d", "Rwb_rot", "Rwb_d_rot"
    (3 columns each) and "feet", "joint_q" (12 each; "joint_q" only for a batch with joint_q).  Returns dict(jac [n, 12, C] - column c
    is d grf_body / d (columns[c]) -, columns: the list of (name, component), flags int32 [n]).  Column c equals tangent_batch() on
    the unit seed of columns[c] bit for bit, however the columns are chunked.  ValueError as tangent_batch()."""
    import torch

    cols = jacobian_columns(wrt)
    n = grf_body.shape[0]
    dev = grf_body.device
    total = len(cols)
    step = total if chunk is None else int(chunk)
    if step < 1:
        raise ValueError("jacobian: chunk must be >= 1")
    jac = torch.empty((n, 12, total), dtype=torch.float64, device=dev)
    flags = None
    for c0 in range(0, total, step):
        part = cols[c0:c0 + step]
        seeds = {}
        for j, (name, comp) in enumerate(part):
            key = name + "_tan"
            if key not in seeds:
                seeds[key] = torch.zeros((len(part), n, TANGENTS[key]), dtype=torch.float64, device=dev)
            seeds[key][j, :, comp] = 1.0
        res = tangent_batch(ctl, batch, grf_body, seeds, want=("grf_tan", "flags"), act_tol=act_tol, stream=stream)
        jac[:, :, c0:c0 + len(part)] = res["grf_tan"].reshape(len(part), n, 12).permute(1, 2, 0)
        flags = res["flags"]
    return dict(jac=jac, columns=cols, flags=flags)


# ------------------------------------------------------------------ forward mode in the handle's parameters
PARAM_JACOBIAN_WRT = ("mu", "mass", "fzmin", "fzmax", "Ib", "kff", "kp_p", "kd_p", "kp_w", "kd_w")  # param_jacobian_batch's default: all groups but S and W


def _param_directions(who, param_tan, dev):
    """param_tan validated: contiguous float64 [211] (one direction, squeezed) or [K, 211] on `dev`.  Returns (K, squeeze)."""
    import torch

    if param_tan is None or param_tan.dtype != torch.float64 or not param_tan.is_contiguous() or param_tan.device != dev or param_tan.dim() not in (1, 2) or \
            param_tan.shape[-1] != _lib.PARAM_COUNT or param_tan.numel() == 0:
        raise ValueError(f"{who}: param_tan: need contiguous float64 [{_lib.PARAM_COUNT}] or [K,{_lib.PARAM_COUNT}] on {dev} (PARAM_LAYOUT's order)")
    return (1, True) if param_tan.dim() == 1 else (param_tan.shape[0], False)


def plan_param_tangent(ctl, batch, grf_body, param_tan, want=("grf_tan",), act_tol=1e-7, out=None, add_to=None, stream=None):
    """param_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_param_tangent_batch call
    (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors and squeeze says whether param_tan came as
    [211].  Planning launches nothing."""
    import torch

    _library()
    who = "param_tangent"
    dev = torch.device("cuda", ctl.device)
    K, squeeze = _param_directions(who, param_tan, dev)
    io = QcParamTangentIo()
    ctl._lib.qc_default_param_tangent(C.byref(io))
    n, dev, bi = ctl._readonly_batch(who, batch, _READONLY_FIELDS, io, [("grf_body", grf_body, 12)])
    io.param_tan = param_tan.data_ptr()
    io.n_dir = K
    io.act_tol = float(act_tol)
    add_to = dict(add_to or {})
    unknown = [k for k in add_to if k not in _TANGENT_OUTPUTS]
    if unknown:
        raise ValueError(f"{who}: add_to names {unknown}; it may hold {tuple(_TANGENT_OUTPUTS)}")
    wanted = tuple(w for w in want if w != "flags")
    missing = [k for k in add_to if k not in wanted]
    if missing:
        raise ValueError(f"{who}: add_to names {missing}, which `want` does not ask for")
    if add_to:  # accumulated onto in place: the buffer is the input AND the output of its name
        if out is not None and any(out.get(k) is not None for k in add_to):
            raise ValueError(f"{who}: a buffer of add_to IS the output of its name - give it in add_to alone")
        for k, t in add_to.items():
            m = int(np.prod(_TANGENT_OUTPUTS[k][0]))
            _check_tensor(k, t, K * n, m, torch.float64, dev, True, msg=f"add_to['{k}']: need contiguous float64 with {K * n * m} elements on {dev}")
            setattr(io, k + "_in", t.data_ptr())
        rest = {w: torch.zeros((K * n,) + _TANGENT_OUTPUTS[w][0], dtype=torch.float64, device=dev) for w in wanted if w not in add_to}
        if "flags" in want:
            rest["flags"] = torch.zeros((n,), dtype=torch.int32, device=dev)
        out = dict(rest, **{k: v for k, v in (out or {}).items() if v is not None}, **add_to)
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs(who, _TANGENT_OUTPUTS, wanted, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_param_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)), (batch, grf_body, param_tan, res, bi, io), ValueError)
    return launch, res, squeeze


def param_tangent(ctl, batch, grf_body, param_tan, want=("grf_tan",), act_tol=1e-7, out=None, add_to=None, stream=None):
    """Forward mode of the balance QP in the handle's own parameters, on the active face of `grf_body` [n,12] (as control_batch()
    wrote it) for the batch the solve read (qc_param_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode in the
    parameters").  `param_tan`: a device tensor [211] (one direction, squeezed) or [K, 211] in PARAM_LAYOUT's order - mu, mass,
    fzmin, fzmax, Ib, S, W, kff, kp_p, kd_p, kp_w, kd_w, matrices entrywise and row-major, NOT symmetrised (a direction in S or W
    means something only where it is symmetric) - SHARED by the batch, as the handle's parameters are.  `want`: any of "grf_tan"
    [K,n,4,3] (body frame), "b_tan" [K,n,6] and "flags" int32 [n] (tangent_batch()'s bits).  `add_to`: a dict with the "grf_tan" /
    "b_tan" buffers ([K,n,...], as tangent_batch() wrote them) to accumulate onto IN PLACE - they are the outputs of their names; the
    sum is the one IEEE addition of the two calls' results.  The transpose of sensitivity_params_batch(): <grf_bar, grf_tan_k> per
    robot equals <param_bar_rows, param_tan_k>.  It repeats tangent_batch()'s factorisation (once per robot, substituted K times).
    Nothing of `batch` is written.  Asynchronous on `stream`, no synchronisation.  Returns the dict of device tensors, [K, n, ...] -
    squeezed to [n, ...] where param_tan came as [211].  ValueError with the library's message for a call it refuses.  Not covered:
    per-robot directions, tangents of the kinematic model, of tau_min / tau_max, of the joint gains and of the plant's use of mass and
    Ib."""
    launch, res, squeeze = plan_param_tangent(ctl, batch, grf_body, param_tan, want, act_tol, out, add_to, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def param_jacobian_columns(wrt=None):
    """the columns of param_jacobian_batch(): the list of (group, index) - index a tuple into the group's shape; for "S" and "W" the
    upper triangle (i, j), i <= j, row by row: the column of the symmetric pair"""
    from .balance_controller import PARAM_LAYOUT

    wrt = PARAM_JACOBIAN_WRT if wrt is None else tuple(wrt)
    unknown = [w for w in wrt if w not in PARAM_LAYOUT]
    if unknown:
        raise ValueError(f"param_jacobian: unknown group(s) {unknown}; wrt is a subset of {tuple(PARAM_LAYOUT)}")
    cols = []
    for w in wrt:
        shape = PARAM_LAYOUT[w][1]
        if w in ("S", "W"):
            cols += [(w, (i, j)) for i in range(shape[0]) for j in range(i, shape[1])]
        else:
            cols += [(w, tuple(int(v) for v in idx)) for idx in np.ndindex(*shape)]
    return cols


def param_jacobian_seeds(cols, dev):
    """the unit seeds [len(cols), 211] of param_jacobian_columns()' columns, on `dev`: one 1 per column, and for an off-diagonal (i, j)
    of "S" / "W" the symmetric pair E_ij + E_ji (E_ii on the diagonal)"""
    import torch

    from .balance_controller import PARAM_LAYOUT

    seeds = np.zeros((len(cols), _lib.PARAM_COUNT))
    for c, (group, idx) in enumerate(cols):
        sl, shape = PARAM_LAYOUT[group]
        E = np.zeros(shape if shape else (1,))
        E[idx if shape else 0] = 1.0
        if group in ("S", "W"):
            E[idx[::-1]] = 1.0
        seeds[c, sl] = E.reshape(-1)
    return torch.from_numpy(seeds).to(dev)


def param_jacobian_batch(ctl, batch, grf_body, wrt=None, chunk=None, act_tol=1e-7, stream=None):
    """The Jacobian d grf_body / d theta of a solved batch on its active face, in the handle's own parameters: param_tangent() on unit
    seeds, `chunk` directions per launch (None: all in one).  `wrt`: PARAM_LAYOUT groups (None: PARAM_JACOBIAN_WRT - every group but
    "S" and "W").  A column of a vector or of Ib is the derivative in ONE entry; for "S" and "W" the seeds are the SYMMETRIC pairs
    E_ij + E_ji, i <= j (E_ii on the diagonal) - the derivative along a matrix that stays symmetric, 21 columns for S and 78 for W.
    Returns dict(jac [n, 12, C] - column c is d grf_body / d (columns[c]) -, columns: the list of (group, index), flags int32 [n]).
    Column c equals param_tangent() on the seed of columns[c] bit for bit, however the columns are chunked.  ValueError as
    param_tangent()."""
    import torch

    cols = param_jacobian_columns(wrt)
    n, dev = grf_body.shape[0], grf_body.device
    total = len(cols)
    step = total if chunk is None else int(chunk)
    if step < 1:
        raise ValueError("param_jacobian: chunk must be >= 1")
    seeds = param_jacobian_seeds(cols, dev)
    jac = torch.empty((n, 12, total), dtype=torch.float64, device=dev)
    flags = None
    for c0 in range(0, total, step):
        part = seeds[c0:c0 + step].contiguous()
        res = param_tangent(ctl, batch, grf_body, part, want=("grf_tan", "flags"), act_tol=act_tol, stream=stream)
        jac[:, :, c0:c0 + part.shape[0]] = res["grf_tan"].reshape(part.shape[0], n, 12).permute(1, 2, 0)
        flags = res["flags"]
    return dict(jac=jac, columns=cols, flags=flags)


# ------------------------------------------------------------------ the plant step's forward mode and the closed loop
def plan_plant_step_tangent(ctl, state, grf_body, foot_world, dt, tangents, want=PLANT_TANGENT_WANT, out=None, stream=None):
    """plant_step_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_plant_step_tangent_batch call
    (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors and squeeze says whether the tangents came
    as [n, ...].  A tensor of `out` may be a tensor of `tangents` of the same layout (the aliasing contract of include/qc_tangent.h).
    Planning launches nothing."""
    _library()
    unknown = [k for k in tangents if k not in PLANT_TANGENTS]
    if unknown:
        raise ValueError(f"plant_step_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(PLANT_TANGENTS)}")
    io = QcPlantTangentIo()
    ctl._lib.qc_default_plant_tangent(C.byref(io))
    n, dev = ctl._plant_arrays(io, state, grf_body, foot_world)
    given, K, squeeze = _directions(tangents, PLANT_TANGENTS, n, dev, io)
    io.n_dir = K
    io.dt = float(dt)
    res = _outputs("plant_step_tangent", _PLANT_TANGENT_OUTPUTS, tuple(want), out, K * n, dev, io)
    res = {k: v.view((K, n) + _PLANT_TANGENT_OUTPUTS[k][0]) for k, v in res.items()}
    launch = ctl._launcher("qc_plant_step_tangent_batch", (n, C.byref(io), ctl._stream_ptr(stream)), (state, grf_body, foot_world, given, res, io), ValueError)
    return launch, res, squeeze


def plant_step_tangent(ctl, state, grf_body, foot_world, dt, tangents, want=PLANT_TANGENT_WANT, out=None, stream=None):
    """Forward mode of plant_step() (qc_plant_step_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode: the plant step
    and the closed loop").  `state`: the tensors Rwb [n,9], x, xdot, w [n,3] as they are BEFORE the step; `grf_body`, `foot_world`
    [n,12] and `dt` as the step reads them.  `tangents`: a dict with any of "Rwb_rot_tan" (the world-frame left tangent,
    Rwb <- exp([d]x) Rwb), "x_tan", "xdot_tan", "w_tan" ([n,3]), "grf_tan" (what tangent_batch() wrote) and "foot_world_tan" ([n,4,3]) -
    each [n, ...] for one direction or [K, n, ...] for K, all agreeing on K; a missing one is zero, at least one given.  `want`: any of
    "Rwb_rot_next_tan", "x_next_tan", "xdot_next_tan", "w_next_tan" [K,n,3] and "feet_next_tan" [K,n,4,3], the tangent of the `feet`
    plant_step() writes.  The step is recomputed from `state`; nothing of it is written.  `out`: a dict of tensors with K * n rows
    to write into - each may be the input tangent of its layout.  Asynchronous on `stream`, no synchronisation.  Returns the dict of
    device tensors, squeezed to [n, ...] where the tangents came that way.  ValueError with the library's message for a call it
    refuses.  Not covered: tangents of mass, Ib and dt (the leg plant: leg_plant_step_tangent())."""
    launch, res, squeeze = plan_plant_step_tangent(ctl, state, grf_body, foot_world, dt, tangents, want, out, stream)
    launch()
    return {k: (v[0] if squeeze else v) for k, v in res.items()}


def _rollout_params_tan(who, params_tan, dev, given, K, squeeze):
    """`params_tan` of a rollout (None, [211] or [K, 211]) against the form of the other tangents: returns (K, squeeze) - params_tan's
    own where it is the only seed."""
    if params_tan is None:
        return K, squeeze
    lead = _param_directions(who, params_tan, dev)
    if given and lead != (K, squeeze):
        raise ValueError(f"{who}: params_tan must agree with the tangents on the number of directions and on the squeezed / [K, ...] form")
    return lead


def rollout_tangent(ctl, batch, foot_world, steps, dt, tangents, act_tol=1e-7, warm=True, stream=None, params_tan=None):
    """The forward-mode twin of ctl.rollout(): `steps` times control_batch(), tangent_batch(), plant_step_tangent() (it reads the state
    before the step) and plant_step(), everything planned once, on one stream and without a host round trip.  `batch` is advanced IN
    PLACE and ends bit for bit where ctl.rollout() leaves it.  `tangents`: any of the start state's "Rwb_rot_tan", "x_tan",
    "xdot_tan", "w_tan" [n,3], step 0's "feet_tan" [n,4,3] (body frame), and - held, applied at every step - "foot_world_tan" [n,4,3]
    and the desired state's "x_d_tan", "xdot_d_tan", "w_d_tan", "Rwb_d_rot_tan"; each [n, ...] or [K, n, ...], all agreeing; none is
    written.  Returns (state, res): `state` the tensors of `batch`, `res` the final "Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan",
    "feet_tan", the last solve's "grf_tan" ([K, n, ...], squeezed where the tangents came as [n, ...]) and "flags" int32 [n],
    tangent_batch()'s flags OR-ed over the steps on the device.  The derivative is the one on the active face of every solve at
    `act_tol`, as rollout_autograd()'s.  Tangent memory is one set of buffers whatever `steps` is.
    `params_tan` ([211] or [K, 211], PARAM_LAYOUT's order, agreeing with `tangents` on K): directions in the handle's parameters, held
    over the rollout - every step launches param_tangent() in place on grf_tan behind tangent_batch() and ORs its flags into the same
    word; it is a seed of its own (`tangents` may then be empty).  The plant's mass and Ib stay held, as in
    rollout_autograd(params=...).  params_tan=None launches exactly what the rollout launched without the keyword."""
    import contextlib

    import torch

    if batch.get("joint_q") is not None or batch.get("feet") is None:
        raise ValueError("rollout: the plant is a single rigid body - the batch carries `feet`, not joint_q")
    steps = int(steps)
    if steps < 0:
        raise ValueError("rollout: steps must be >= 0")
    unknown = [k for k in tangents if k not in ROLLOUT_TANGENTS]
    if unknown:
        raise ValueError(f"rollout_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(ROLLOUT_TANGENTS)}")
    n = batch["x"].shape[0]
    dev = torch.device("cuda", ctl.device)
    given, K, squeeze = _directions(tangents, ROLLOUT_TANGENTS, n, dev)
    if not given and params_tan is None:
        raise ValueError("rollout_tangent: no tangent given")
    K, squeeze = _rollout_params_tan("rollout_tangent", params_tan, dev, given, K, squeeze)
    on_stream = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with on_stream:
        # one set of buffers: the state's tangents and feet_tan are advanced in place, grf_tan is rewritten by every step
        buf = {k: (given[k].reshape((K, n) + ((4, 3) if m == 12 else (3,))).clone() if k in given else
                   torch.zeros((K, n) + ((4, 3) if m == 12 else (3,)), dtype=torch.float64, device=dev))
               for k, m in ROLLOUT_TANGENTS.items() if k in _ROLLOUT_STATE or k == "feet_tan"}
        grf_tan = torch.zeros((K, n, 4, 3), dtype=torch.float64, device=dev)
        flags, step_flags = (torch.zeros((n,), dtype=torch.int32, device=dev) for _ in range(2))
        param_flags = torch.zeros((n,), dtype=torch.int32, device=dev) if params_tan is not None else None
    held = {k: given[k].reshape(K, n, 3) for k in _ROLLOUT_HELD if k in given}
    fw_tan = given["foot_world_tan"].reshape(K, n, 4, 3) if "foot_world_tan" in given else None
    state = {k: batch[k] for k in ("Rwb", "x", "xdot", "w")}
    r = _RolloutPlans(ctl, "rollout_tangent", batch, n, warm, lambda first, w, o: ctl.plan_batch(batch, w, o, want_active_set=warm, stream=stream)[0],
                      None, stream)
    if steps > 0 and n > 0:
        solve_tan, _, _ = plan_tangent(ctl, batch, r.out["grf_body"], dict(buf, **held), ("grf_tan", "flags"), act_tol,
                                       {"grf_tan": grf_tan, "flags": step_flags}, stream)
        param_tan = None
        if params_tan is not None:
            param_tan, _, _ = plan_param_tangent(ctl, batch, r.out["grf_body"], params_tan, ("grf_tan", "flags"), act_tol, {"flags": param_flags},
                                                 {"grf_tan": grf_tan}, stream)
        plant_in = {k: buf[k] for k in _ROLLOUT_STATE}
        plant_in["grf_tan"] = grf_tan
        if fw_tan is not None:
            plant_in["foot_world_tan"] = fw_tan
        plant_out = {k[:-4] + "_next_tan": buf[k] for k in _ROLLOUT_STATE}
        plant_out["feet_next_tan"] = buf["feet_tan"]
        step_tan, _, _ = plan_plant_step_tangent(ctl, state, r.out["grf_body"], foot_world, dt, plant_in, PLANT_TANGENT_WANT, plant_out, stream)
        step = ctl.plan_plant(state, r.out["grf_body"], foot_world, dt, batch["feet"], stream)
        for k in range(steps):
            r.solve(k)
            solve_tan()
            if param_tan is not None:
                param_tan()
            with on_stream:
                flags.bitwise_or_(step_flags)
                if param_flags is not None:
                    flags.bitwise_or_(param_flags)
            step_tan()
            step()
    res = dict(buf, grf_tan=grf_tan)
    res = {k: (v[0] if squeeze else v) for k, v in res.items()}
    res["flags"] = flags
    return state, res


def transition_seeds(batch, foot_world, columns=TRANSITION_COLUMNS):
    """rollout_tangent()'s `tangents` for unit seeds on the start state: direction j moves coordinate columns[j] - (name, component)
    with name in "Rwb_rot", "x", "xdot", "w" - by one, and step 0's feet_tan follows from the pinned feet,
    Rwb^T (-dx - delta x (foot_world - x)).  [K, n, ...] device tensors."""
    import torch

    n, dev = batch["x"].shape[0], batch["x"].device
    K = len(columns)
    seeds = {k: torch.zeros((K, n, 3), dtype=torch.float64, device=dev) for k in _ROLLOUT_STATE}
    for j, (name, comp) in enumerate(columns):
        if name + "_tan" not in seeds:
            raise ValueError(f"rollout_transition: unknown coordinate {name!r}; the coordinates are {tuple(k[:-4] for k in _ROLLOUT_STATE)}")
        seeds[name + "_tan"][j, :, comp] = 1.0
    R = batch["Rwb"].reshape(1, n, 1, 3, 3)
    arm = (foot_world.reshape(n, 4, 3) - batch["x"].reshape(n, 1, 3)).unsqueeze(0)
    delta, dx = seeds["Rwb_rot_tan"].unsqueeze(2), seeds["x_tan"].unsqueeze(2)
    world = -dx - torch.cross(delta.expand(K, n, 4, 3), arm.expand(K, n, 4, 3), dim=-1)
    seeds["feet_tan"] = (R.transpose(-1, -2) * world.unsqueeze(-2)).sum(-1).contiguous()  # Rwb^T world, elementwise: the same bits however the seeds are chunked
    return seeds


def rollout_transition(ctl, batch, foot_world, steps, dt, act_tol=1e-7, warm=True, chunk=None, stream=None):
    """The 12 x 12 state-transition matrix of `steps` closed-loop steps in minimal coordinates (rotation tangent, x, xdot, w):
    rollout_tangent() on the 12 unit seeds of the start state (transition_seeds), `chunk` seeds per rollout (None: all in one; the
    start state is restored between the chunks).  `batch` is advanced in place, as by ctl.rollout().  Returns dict(phi [n,12,12] -
    phi[:, r, c] = d (coordinate r after the steps) / d (coordinate c at the start), rows and columns in the order of `columns` -,
    columns: the list of (name, component), flags int32 [n]: OR-ed over the steps and the chunks).  Column c equals rollout_tangent()
    on seed c bit for bit, however the columns are chunked; steps = 0 gives the identity."""
    import contextlib

    import torch

    cols = list(TRANSITION_COLUMNS)
    n, dev = batch["x"].shape[0], batch["x"].device
    size = len(cols) if chunk is None else int(chunk)
    if size < 1:
        raise ValueError("rollout_transition: chunk must be >= 1")
    on_stream = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    moved = ("Rwb", "x", "xdot", "w", "feet")
    with on_stream:
        phi = torch.empty((n, 12, 12), dtype=torch.float64, device=dev)
        flags = torch.zeros((n,), dtype=torch.int32, device=dev)
        start = {k: batch[k].clone() for k in moved} if size < len(cols) else None
    for c0 in range(0, len(cols), size):
        part = cols[c0:c0 + size]
        with on_stream:
            if c0 > 0:
                for k in moved:
                    batch[k].copy_(start[k])
            seeds = transition_seeds(batch, foot_world, part)
        _, res = rollout_tangent(ctl, batch, foot_world, steps, dt, seeds, act_tol, warm, stream)
        with on_stream:
            rows = torch.cat([res[k] for k in _ROLLOUT_STATE], dim=-1)  # [len(part), n, 12]
            phi[:, :, c0:c0 + len(part)] = rows.permute(1, 2, 0)
            flags.bitwise_or_(res["flags"])
    return dict(phi=phi, columns=cols, flags=flags)


# ------------------------------------------------------------------ forward mode around the tick: the torque map, the leg plant, the loop
def plan_torque_tangent(ctl, batch, grf_body, status, tangents, out=None, stream=None):
    """torque_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_torque_tangent_batch call
    (graph-capturable) on tensors that are read in place; `out` holds the [K, n, 4, 3] tensor and squeeze says whether the tangents
    came as [n, ...].  out["joint_tau_tan"] may be a tensor of `tangents`.  Planning launches nothing."""
    import torch

    _library()
    unknown = [k for k in tangents if k not in TORQUE_TANGENTS]
    if unknown:
        raise ValueError(f"torque_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(TORQUE_TANGENTS)}")
    io = QcTorqueTangentIo()
    ctl._lib.qc_default_torque_tangent(C.byref(io))
    sizing = [batch.get("joint_q"), grf_body, status] + [t for t in tangents.values() if t is not None and t.dim() == 2]
    n, dev, bi = ctl._readonly_batch("torque_tangent", batch, _KINEMATICS_FIELDS, io, [("grf_body", grf_body, 12)], sizing,
                                     "neither joint_q, grf_body nor status is there to size the call")
    if _check_tensor("status", status, n, None, torch.int32, dev, False):
        io.status = status.data_ptr()
    given, K, squeeze = _directions(tangents, TORQUE_TANGENTS, n, dev, io)
    io.n_dir = K
    res = _outputs("torque_tangent", _TORQUE_TANGENT_OUTPUTS, ("joint_tau_tan",), out, K * n, dev, io)
    res = {k: v.view((K, n) + _TORQUE_TANGENT_OUTPUTS[k][0]) for k, v in res.items()}
    launch = ctl._launcher("qc_torque_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)), (batch, grf_body, status, given, res, bi, io), ValueError)
    return launch, res, squeeze


def torque_tangent(ctl, batch, grf_body, status, tangents, out=None, stream=None):
    """Forward mode of the clamped J^T torque map (qc_torque_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode around
    the tick"): joint_tau_tan = m o (J^T grf_tan + (sum_r g_r H_r) joint_q_tan), the map sensitivity_kinematics_batch() transposes.
    `batch`: the one control_batch(want_torques=True) read - joint_q and the contact mask (stance, else the phase rule on gait_phase,
    else all stance) are all that is read of it; `grf_body` [n,12] and `status` int32 [n] as the solve wrote them.  `tangents`: a dict
    with "grf_tan" (what tangent_batch() wrote) and / or "joint_q_tan", each [n, ...] for one direction or [K, n, ...] for K, agreeing;
    a missing one is zero, at least one given.  m is 1 where the forward torque passed through the clamp, 0 where it was clamped, for
    swing legs and for robots with status != 0.  Returns dict(joint_tau_tan [K, n, 4, 3]), squeezed to [n, 4, 3] where the tangents
    came that way; `out`: a dict with a tensor of K * n * 12 values to write into - it may be one of the tangents.  Nothing of
    `batch` is written.  Asynchronous on `stream`, no synchronisation.  ValueError with the library's message for a call it refuses.
    Not covered: the swing legs' PD torques (tangent 0), tangents of the kinematic constants and the torque limits."""
    launch, res, squeeze = plan_torque_tangent(ctl, batch, grf_body, status, tangents, out, stream)
    launch()
    return {k: (v[0] if squeeze else v) for k, v in res.items()}


def plan_leg_plant_step_tangent(ctl, state, joint_tau, dt, leg_inertia, tangents, stance=None, gait_phase=None, gait_duty=None, cmd_state=None,
                                want=LEG_PLANT_TANGENT_WANT, out=None, stream=None):
    """leg_plant_step_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_leg_plant_step_tangent_batch
    call (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors (and "flags" int32 [n] where asked for)
    and squeeze says whether the tangents came as [n, ...].  A tensor of `out` may be a tensor of `tangents` of the same layout (the
    aliasing contract of include/qc_tangent.h).  Planning launches nothing."""
    import torch

    _library()
    unknown = [k for k in tangents if k not in LEG_PLANT_TANGENTS]
    if unknown:
        raise ValueError(f"leg_plant_step_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(LEG_PLANT_TANGENTS)}")
    dev = torch.device("cuda", ctl.device)
    n = state["x"].shape[0]
    io = QcLegPlantTangentIo()
    ctl._lib.qc_default_leg_plant_tangent(C.byref(io))
    # (a missing state or torque array is the library's refusal, from launch())
    arrays = [(k, state.get(k), m, torch.float64) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("joint_q", 12), ("joint_qdot", 12))]
    arrays += [("joint_tau", joint_tau, 12, torch.float64), ("stance", stance, 4, torch.uint8), ("gait_phase", gait_phase, 4, torch.float64),
               ("gait_duty", gait_duty, 1, torch.float64), ("cmd_state", cmd_state, COMMANDER_STATE_DTYPE.itemsize, torch.uint8)]
    for name, t, k, dtype in arrays:
        if _check_tensor(name, t, n, k, dtype, dev, False):
            setattr(io, name, t.data_ptr() if n else None)
    given, K, squeeze = _directions(tangents, LEG_PLANT_TANGENTS, n, dev, io)
    io.n_dir = K
    _fill(io.leg_inertia, np.broadcast_to(np.asarray(leg_inertia, dtype=np.float64), (3,)), 3, "leg_inertia")
    io.dt = float(dt)
    rows = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("leg_plant_step_tangent", _LEG_PLANT_TANGENT_OUTPUTS, rows, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _LEG_PLANT_TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    keep = (state, joint_tau, stance, gait_phase, gait_duty, cmd_state, given, res, io)
    launch = ctl._launcher("qc_leg_plant_step_tangent_batch", (n, C.byref(io), ctl._stream_ptr(stream)), keep, ValueError)
    return launch, res, squeeze


def leg_plant_step_tangent(ctl, state, joint_tau, dt, leg_inertia, tangents, stance=None, gait_phase=None, gait_duty=None, cmd_state=None,
                           want=LEG_PLANT_TANGENT_WANT, out=None, stream=None):
    """Forward mode of ctl.leg_plant_step() (qc_leg_plant_step_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode
    around the tick").  `state`: the tensors Rwb [n,9], x, xdot, w [n,3], joint_q, joint_qdot [n,12] as they are BEFORE the step;
    `joint_tau`, `dt`, `leg_inertia` and the contact inputs `stance` / `gait_phase` / `gait_duty` / `cmd_state` as the step reads them.
    `tangents`: a dict with any of "Rwb_rot_tan" (the world-frame left tangent, Rwb <- exp([d]x) Rwb), "x_tan", "xdot_tan", "w_tan"
    ([n,3]), "joint_q_tan", "joint_qdot_tan" and "joint_tau_tan" ([n,12] or [n,4,3]; the last is what torque_tangent() wrote) - each
    [n, ...] for one direction or [K, n, ...] for K, all agreeing on K; a missing one is zero, at least one given.  `want`: any of
    "Rwb_rot_next_tan", "x_next_tan", "xdot_next_tan", "w_next_tan" [K,n,3], "joint_q_next_tan", "joint_qdot_next_tan" [K,n,4,3] and
    "flags" int32 [n] (bit l: J(q_l) of stance leg l singular, bit 4 + l: leg l out of reach or J singular after the step); a robot
    with any bit set has NaN in every output row of every direction.  The step is recomputed from `state`; nothing of it is written.
    `out`: a dict of tensors with K * n rows to write into - each may be the input tangent of its layout, joint_qdot_next_tan also
    joint_tau_tan.  Asynchronous on `stream`, no synchronisation.  Returns the dict of device tensors, squeezed to [n, ...] where the
    tangents came that way.  ValueError with the library's message for a call it refuses.  Not covered: tangents of mass, Ib,
    leg_inertia, dt and the kinematic constants; the contact mask is held."""
    launch, res, squeeze = plan_leg_plant_step_tangent(ctl, state, joint_tau, dt, leg_inertia, tangents, stance, gait_phase, gait_duty, cmd_state,
                                                       want, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def rollout_tick_tangent(ctl, batch, steps, dt, leg_inertia, tangents, act_tol=1e-7, warm=True, stream=None, command=None, lean=None, params_tan=None):
    """The forward-mode twin of ctl.rollout_tick(batch, None, ...): `steps` times control_batch(want_torques=True), tangent_batch()
    (the state's tangents and joint_q_tan), torque_tangent(), leg_plant_step_tangent() (it reads the state before the step) and
    leg_plant_step(), everything planned once, on one stream and without a host round trip.  `batch` is advanced IN PLACE and ends
    bit for bit where ctl.rollout_tick() leaves it.  `tangents`: any of the start state's "Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan"
    [n,3], "joint_q_tan", "joint_qdot_tan" [n,12] and - held, applied at every step - the desired state's "x_d_tan", "xdot_d_tan",
    "w_d_tan", "Rwb_d_rot_tan"; each [n, ...] or [K, n, ...], all agreeing; none is written.  A `stance` / `gait_phase` / `gait_duty`
    contact mask is HELD over the rollout, as in rollout_tick_autograd().  Returns (state, res): `state` the six tensors of `batch`,
    `res` the final six tangents under their input names, the last "grf_tan" and "joint_tau_tan" ([K, n, ...], squeezed where the
    tangents came as [n, ...]) and "flags" int32 [n], OR-ed over the steps on the device: bits 0-1 are tangent_batch()'s (bit 0: a
    one-sided face, bit 1: a bad pivot), bits 8-15 the plant's shifted left by 8 (bit 8 + l: J(q_l) singular, bit 12 + l: leg l out
    of reach or J singular after the step).  The derivative is the one on the active face of every solve at `act_tol`, at every
    tick's torque clamp mask and off the plant's flagged legs, as rollout_tick_autograd()'s.  Tangent memory is one set of buffers
    whatever `steps` is.  ValueError for swing references (swing_state, swing_pos, swing_vel), gait_dt, `lean` and a `command` - in THIS
    rollout: rollout_swing_tangent() and rollout_gait_tangent() take the swing pipeline, rollout_commander_tangent() a `command` and
    rollout_lean_tangent() a `lean`.  `params_tan` ([211] or [K, 211], PARAM_LAYOUT's order): directions in the handle's parameters, held
    over the rollout - param_tangent() in place on grf_tan behind tangent_batch() at every step, a seed of its own; the plant's mass
    and Ib, the joint gains and the kinematic model stay held, as in rollout_tick_autograd(params=...)."""
    who = "rollout_tick_tangent"
    if command is not None:
        raise ValueError(f"{who}: commander mode has no forward mode - command must be None (the desired state is held in the batch)")
    if lean is not None:
        raise ValueError(f"{who}: lean has no forward mode - lean must be None")
    for name, why in (("swing_state", "the swing planner"), ("swing_pos", "the swing legs' PD torques"), ("swing_vel", "the swing legs' PD torques"),
                      ("gait_dt", "the gait clock (the contact mask is held)")):
        if batch.get(name) is not None:
            raise ValueError(f"{who}: batch['{name}'] must be None - {why} has no forward mode")
    if batch.get("joint_q") is None or batch.get("joint_qdot") is None:
        raise ValueError(f"{who}: the batch carries joint_q and joint_qdot (rollout_tangent() steps the bare rigid body)")
    return _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, tangents, ROLLOUT_TICK_TANGENTS, act_tol, warm, stream, False, params_tan=params_tan)


def _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, tangents, table, act_tol, warm, stream, swings, clock=None, hook=None, lead=None,
                       params_tan=None):
    """What rollout_tick_tangent(), rollout_swing_tangent() and rollout_gait_tangent() share, behind their own refusals: the tangents
    validated against `table`, one set of buffers, every launch planned once, the step loop.  swings=False launches exactly what
    rollout_tick_tangent() always did; swings=True hands the whole batch to the tick (joint_qdot and the two references with it, as
    ctl.rollout_tick() does) and adds swing_torque_tangent() in place on joint_tau_tan behind torque_tangent(), its flags at
    SWING_FLAGS_SHIFT.  `clock` (float64 [n], with swings=True): the references are made per step - a copy of the records,
    swing_reference_batch() with `clock` as its gait_dt and swing_reference_tangent() in front of the tick, which reads the references
    and the phases they left; the record's two tangents are carried in place, the flags land at REFERENCE_FLAGS_SHIFT.
    `hook` (rollout_commander_tangent(), rollout_lean_tangent()): hook(ctl, who, batch, n, K, dev, buf, given, stream) is called once,
    behind the buffers, and returns an object whose step(k) is launched in front of every step - it rewrites the desired state the tick
    reads (`desired`: name -> tensor, laid over the batch) and the desired-state tangent buffers (`held`: name -> [K,n,3], in place of
    the held ones) -, whose flags(word) ORs its own bits into the rollout's word after the step's launches and whose `res` joins the
    result; the tangents the hook takes itself are not in `tangents`, `lead` = (K, squeeze) is their form.  Without a hook nothing here
    launches, reads or allocates anything it did not before.
    `params_tan` ([211] or [K, 211], agreeing with the other tangents): directions in the handle's parameters, held over the rollout -
    param_tangent() in place on grf_tan behind tangent_batch(), its flags OR-ed into the word's bits 0-1; a seed of its own.  The
    plant's mass and Ib, the joint gains and the kinematic model stay held.  With None nothing is launched or allocated for it."""
    import contextlib

    import torch

    steps = int(steps)
    if steps < 0:
        raise ValueError(f"{who}: steps must be >= 0")
    unknown = [k for k in tangents if k not in table]
    if unknown:
        raise ValueError(f"{who}: unknown tangent(s) {unknown}; the tangents are {tuple(table)}")
    n = batch["x"].shape[0]
    dev = torch.device("cuda", ctl.device)
    given, K, squeeze = _directions(tangents, table, n, dev)
    if lead is not None:
        if given and (K, squeeze) != tuple(lead):
            raise ValueError(f"{who}: the tangents must agree on the number of directions and on the [n, ...] / [K, n, ...] form")
        K, squeeze = lead
        _rollout_params_tan(who, params_tan, dev, True, K, squeeze)
    elif not given and params_tan is None:
        raise ValueError(f"{who}: no tangent given")
    else:
        K, squeeze = _rollout_params_tan(who, params_tan, dev, given, K, squeeze)
    shape = lambda m: (K, n) + ((4, 3) if m == 12 else (3,))
    on_stream = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with on_stream:
        # one set of buffers: the state's tangents are advanced in place, grf_tan and joint_tau_tan are rewritten by every step
        buf = {k: (given[k].reshape(shape(ROLLOUT_TICK_TANGENTS[k])).clone() if k in given else
                   torch.zeros(shape(ROLLOUT_TICK_TANGENTS[k]), dtype=torch.float64, device=dev)) for k in _TICK_STATE}
        grf_tan, tau_tan = (torch.zeros((K, n, 4, 3), dtype=torch.float64, device=dev) for _ in range(2))
        flags, solve_flags, plant_flags = (torch.zeros((n,), dtype=torch.int32, device=dev) for _ in range(3))
        swing_flags = torch.zeros((n,), dtype=torch.int32, device=dev) if swings else None
        param_flags = torch.zeros((n,), dtype=torch.int32, device=dev) if params_tan is not None else None
        if clock is not None:
            # the record's tangents, advanced in place; the references and their tangents, rewritten by every step; the records before it
            rec = {k: (given[k].reshape(K, n, 12).clone() if k in given else torch.zeros((K, n, 12), dtype=torch.float64, device=dev)) for k in _GAIT_RECORD}
            pos_tan, vel_tan = (torch.zeros((K, n, 4, 3), dtype=torch.float64, device=dev) for _ in range(2))
            pos, vel = (torch.zeros((n, 4, 3), dtype=torch.float64, device=dev) for _ in range(2))
            ref_flags = torch.zeros((n,), dtype=torch.int32, device=dev)
            before = torch.empty_like(batch["swing_state"])
    h = hook(ctl, who, batch, n, K, dev, buf, given, stream) if hook is not None else None
    held = {k: given[k].reshape(K, n, 3) for k in _ROLLOUT_HELD if k in given}
    if h is not None:  # the desired state of a step is made by the hook: its arrays over the batch's, its tangent buffers over the held ones
        held = dict(held, **h.held)
        batch = dict(batch, **h.desired)
    names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
    state = {k: batch[k] for k in names}
    # as rollout_tick(): a tick without swing references takes no joint_qdot
    tick_in = batch if swings else {k: v for k, v in batch.items() if k != "joint_qdot"}
    if clock is not None:  # the tick of a gait step: on the references of this step and the phases they left, no planner and no clock
        tick_in = dict({k: v for k, v in batch.items() if k != "swing_state"}, swing_pos=pos, swing_vel=vel)
    contact = {k: batch.get(k) for k in ("stance", "gait_phase", "gait_duty")}
    r = _RolloutPlans(ctl, who, batch, n, warm, lambda first, w, o: ctl.plan_batch(tick_in, w, o, want_active_set=warm, want_torques=True, stream=stream)[0],
                      None, stream, torques=True)
    if steps > 0 and n > 0:
        solve_in = {k: buf[k] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan")}
        solve_tan, _, _ = plan_tangent(ctl, tick_in, r.out["grf_body"], dict(solve_in, **held), ("grf_tan", "flags"), act_tol,
                                       {"grf_tan": grf_tan, "flags": solve_flags}, stream)
        param_tan = None
        if params_tan is not None:
            param_tan, _, _ = plan_param_tangent(ctl, tick_in, r.out["grf_body"], params_tan, ("grf_tan", "flags"), act_tol, {"flags": param_flags},
                                                 {"grf_tan": grf_tan}, stream)
        torque_tan, _, _ = plan_torque_tangent(ctl, tick_in, r.out["grf_body"], r.out["status"], {"grf_tan": grf_tan, "joint_q_tan": buf["joint_q_tan"]},
                                               {"joint_tau_tan": tau_tan}, stream)
        swing_tan = None
        if swings:
            swing_in = {k: buf[k] for k in ("Rwb_rot_tan", "x_tan", "joint_q_tan", "joint_qdot_tan")}
            swing_in.update({k: given[k].reshape(K, n, 4, 3) for k in _SWING_HELD if k in given}, joint_tau_tan_in=tau_tan)
            if clock is not None:
                swing_in.update(swing_pos_tan=pos_tan, swing_vel_tan=vel_tan)
            swing_tan, _, _ = plan_swing_torque_tangent(ctl, tick_in, swing_in, ("joint_tau_tan", "flags"), {"joint_tau_tan": tau_tan, "flags": swing_flags}, stream)
        plant_out = {k[:-4] + "_next_tan": buf[k] for k in _TICK_STATE}
        plant_out["flags"] = plant_flags
        step_tan, _, _ = plan_leg_plant_step_tangent(ctl, state, r.out["joint_tau"], dt, leg_inertia, dict(buf, joint_tau_tan=tau_tan), want=tuple(plant_out),
                                                     out=plant_out, stream=stream, **contact)
        step = ctl.plan_leg_plant(state, r.out["joint_tau"], dt, leg_inertia, stream=stream, **contact)
        reference = reference_tan = None
        if clock is not None:
            reads = {k: batch[k] for k in ("Rwb", "x", "xdot", "w", "xdot_d", "joint_q", "gait_phase", "gait_duty") if batch.get(k) is not None}
            reference, _ = ctl.plan_swing_reference(dict(reads, swing_state=batch["swing_state"], gait_dt=clock), ("swing_pos", "swing_vel"),
                                                    {"swing_pos": pos, "swing_vel": vel}, stream)
            ref_in = dict({k: buf[k] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan")}, **rec)
            if "xdot_d_tan" in held:
                ref_in["xdot_d_tan"] = held["xdot_d_tan"]
            ref_out = {"swing_pos_tan": pos_tan, "swing_vel_tan": vel_tan, "p_start_next_tan": rec["p_start_tan"], "p_final_next_tan": rec["p_final_tan"],
                       "flags": ref_flags}
            reference_tan, _, _ = plan_swing_reference_tangent(ctl, reads, before, ref_in, tuple(ref_out), ref_out, stream)
        for k in range(steps):
            if h is not None:
                h.step(k)
            if reference is not None:
                with on_stream:
                    before.copy_(batch["swing_state"])
                reference()
                reference_tan()
            r.solve(k)
            solve_tan()
            if param_tan is not None:
                param_tan()
            torque_tan()
            if swing_tan is not None:
                swing_tan()
            step_tan()
            with on_stream:
                flags.bitwise_or_(solve_flags.bitwise_or(plant_flags.bitwise_left_shift(TICK_PLANT_FLAGS_SHIFT)))
                if param_flags is not None:
                    flags.bitwise_or_(param_flags)
                if swing_flags is not None:
                    flags.bitwise_or_(swing_flags.bitwise_left_shift(SWING_FLAGS_SHIFT))
                if reference is not None:
                    flags.bitwise_or_(ref_flags.bitwise_left_shift(REFERENCE_FLAGS_SHIFT))
                if h is not None:
                    h.flags(flags)
            step()
    res = dict(buf, grf_tan=grf_tan, joint_tau_tan=tau_tan)
    if clock is not None:
        res.update(rec, swing_pos_tan=pos_tan, swing_vel_tan=vel_tan)
    if h is not None:
        res.update(h.res)
    res = {k: (v[0] if squeeze else v) for k, v in res.items()}
    res["flags"] = flags
    return state, res


def tick_transition_seeds(n, dev, columns=TICK_TRANSITION_COLUMNS, coordinates=_TICK_STATE):
    """rollout_tick_tangent()'s `tangents` for unit seeds on the start state: direction j moves coordinate columns[j] - (name, component)
    with name in "Rwb_rot", "x", "xdot", "w" (3 components) or "joint_q", "joint_qdot" (12) - by one.  [K, n, m] device tensors; only
    the coordinates that are seeded are returned."""
    import torch

    seeds = {}
    for j, (name, comp) in enumerate(columns):
        key = name + "_tan"
        if key not in coordinates:
            raise ValueError(f"rollout_tick_transition: unknown coordinate {name!r}; the coordinates are {tuple(k[:-4] for k in coordinates)}")
        if key not in seeds:
            seeds[key] = torch.zeros((len(columns), n, ROLLOUT_GAIT_TANGENTS[key]), dtype=torch.float64, device=dev)
        seeds[key][j, :, comp] = 1.0
    return seeds


def rollout_tick_transition(ctl, batch, steps, dt, leg_inertia, act_tol=1e-7, warm=True, chunk=None, stream=None):
    """The 36 x 36 state-transition matrix of `steps` closed-loop steps around the tick in minimal coordinates - the rotation tangent,
    x, xdot, w (3 each), joint_q[12], joint_qdot[12], in this order -: rollout_tick_tangent() on the 36 unit seeds of the start state
    (tick_transition_seeds), `chunk` seeds per rollout (None: all in one; the start state is restored between the chunks).  `batch` is
    advanced in place, as by ctl.rollout_tick().  Returns dict(phi [n,36,36] - phi[:, r, c] = d (coordinate r after the steps) / d
    (coordinate c at the start), rows and columns in the order of `columns` -, columns: the list of (name, component), flags int32
    [n]: rollout_tick_tangent()'s, OR-ed over the chunks).  Column c equals rollout_tick_tangent() on seed c bit for bit, however the
    columns are chunked; steps = 0 gives the identity.  A stance leg's joint_qdot is not read by the step: those columns are 0."""
    return _tick_transition("rollout_tick_transition", rollout_tick_tangent, ctl, batch, steps, dt, leg_inertia, act_tol, warm, chunk, stream)


def _tick_transition(who, rollout, ctl, batch, steps, dt, leg_inertia, act_tol, warm, chunk, stream, columns=TICK_TRANSITION_COLUMNS,
                     coordinates=_TICK_STATE, restored=()):
    """rollout_tick_transition(), rollout_swing_transition() and rollout_gait_transition(): `rollout` on the unit seeds of `columns`
    (over `coordinates`, the tangents that make a row), `chunk` of them at a time; `restored`: what the rollout advances in the batch
    beside the six state arrays"""
    import contextlib

    import torch

    cols = list(columns)
    n, dev = batch["x"].shape[0], batch["x"].device
    size = len(cols) if chunk is None else int(chunk)
    if size < 1:
        raise ValueError(f"{who}: chunk must be >= 1")
    on_stream = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    moved = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot") + tuple(restored)
    with on_stream:
        phi = torch.empty((n, len(cols), len(cols)), dtype=torch.float64, device=dev)
        flags = torch.zeros((n,), dtype=torch.int32, device=dev)
        start = {k: batch[k].clone() for k in moved} if size < len(cols) else None
    for c0 in range(0, len(cols), size):
        part = cols[c0:c0 + size]
        with on_stream:
            if c0 > 0:
                for k in moved:
                    batch[k].copy_(start[k])
            seeds = tick_transition_seeds(n, dev, part, coordinates)
        _, res = rollout(ctl, batch, steps, dt, leg_inertia, seeds, act_tol, warm, stream)
        with on_stream:
            rows = torch.cat([res[k].reshape(len(part), n, -1) for k in coordinates], dim=-1)  # [len(part), n, 36] (60 through the planner)
            phi[:, :, c0:c0 + len(part)] = rows.permute(1, 2, 0)
            flags.bitwise_or_(res["flags"])
    return dict(phi=phi, columns=cols, flags=flags)


# ------------------------------------------------------------------ forward mode through a trot: the swing legs' PD torques
def plan_swing_torque_tangent(ctl, batch, tangents, want=("joint_tau_tan",), out=None, stream=None):
    """swing_torque_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_swing_torque_tangent_batch call
    (graph-capturable) on tensors that are read in place; `out` holds the [K, n, 4, 3] tensor (and "flags" int32 [n] where asked for)
    and squeeze says whether the tangents came as [n, ...].  out["joint_tau_tan"] may be tangents["joint_tau_tan_in"] or any other
    [K, n, 4, 3] tangent (the aliasing contract of include/qc_tangent.h).  Planning launches nothing."""
    from .balance_controller import _SWING_FIELDS, SWING_STATE_DTYPE, _record_tensor

    _library()
    unknown = [k for k in tangents if k not in SWING_TORQUE_TANGENTS]
    if unknown:
        raise ValueError(f"swing_torque_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(SWING_TORQUE_TANGENTS)}")
    io = QcSwingTangentIo()
    ctl._lib.qc_default_swing_tangent(C.byref(io))
    sizing = [batch.get(k) for k in ("x", "Rwb", "joint_q", "joint_qdot", "swing_pos", "swing_vel")] + [t for t in tangents.values() if t is not None and t.dim() == 2]
    n, dev, bi = ctl._readonly_batch("swing_torque_tangent", batch, _SWING_FIELDS, io, [], sizing, "none of the arrays of the swing chain is there to size the call")
    if _record_tensor("swing_state", batch.get("swing_state"), n, SWING_STATE_DTYPE.itemsize, dev):  # (the library names its refusal)
        bi.swing_state = batch["swing_state"].data_ptr()
    given, K, squeeze = _directions(tangents, SWING_TORQUE_TANGENTS, n, dev, io)
    io.n_dir = K
    rows = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("swing_torque_tangent", _SWING_TORQUE_TANGENT_OUTPUTS, rows, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _SWING_TORQUE_TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_swing_torque_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)), (batch, given, res, bi, io), ValueError)
    return launch, res, squeeze


def swing_torque_tangent(ctl, batch, tangents, want=("joint_tau_tan",), out=None, stream=None):
    """Forward mode of the swing legs' PD torques (qc_swing_torque_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode:
    tangents and the Jacobian"), the map ctl.sensitivity_swing_batch() transposes.  `batch`: the one control_batch(want_torques=True)
    read, with swing_pos and swing_vel - Rwb, x, joint_q, joint_qdot, the two references and the contact mask (stance, else the phase
    rule on gait_phase as it is now, else all stance) are all that is read of it; a batch with swing_state or gait_dt is refused.
    `tangents`: a dict with any of "Rwb_rot_tan" (the world-frame left tangent, Rwb <- exp([d]x) Rwb), "x_tan" ([n,3]),
    "swing_pos_tan", "swing_vel_tan", "joint_q_tan", "joint_qdot_tan" and "joint_tau_tan_in" ([n,12] or [n,4,3]; the last is added:
    what torque_tangent() wrote) - each [n, ...] for one direction or [K, n, ...] for K, all agreeing on K; a missing one is zero, at
    least one given.  `want`: "joint_tau_tan" [K,n,4,3] and / or "flags" int32 [n].  A swing leg's row is m o (kp o (dq_ref - dq) +
    kd o (dqd - dqdot)) + joint_tau_tan_in, m the forward tick's clamp mask bit for bit, whatever the QP's status; a stance leg's row
    is joint_tau_tan_in.  flags bit l: swing leg l's reference is out of reach, inside the inner limit, not finite, or at a singular
    J(q_ref) - NaN in its row in every direction, the other legs untouched.  torque_tangent() writes exact zeros in swing rows: the
    two calls in that order on one buffer (out["joint_tau_tan"] = tangents["joint_tau_tan_in"]) give the tangent of the tick's
    complete joint_tau.  Returns the dict of device tensors, squeezed to [n, 4, 3] where the tangents came that way; `out`: a dict of
    tensors to write into - joint_tau_tan may be any of the [K, n, 4, 3] tangents.  Nothing of `batch` is written.  Asynchronous on
    `stream`, no synchronisation.  ValueError with the library's message for a call it refuses.  Not covered: tangents of the gains,
    the torque limits and the kinematic constants; the planner and the gait clock."""
    launch, res, squeeze = plan_swing_torque_tangent(ctl, batch, tangents, want, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def _swing_rollout_refusals(who, batch, command, lean):
    """what the rollouts through a trot refuse before anything is planned"""
    if command is not None:
        raise ValueError(f"{who}: commander mode has no forward mode - command must be None (the desired state is held in the batch)")
    if lean is not None:
        raise ValueError(f"{who}: lean has no forward mode - lean must be None")
    for name, why in (("swing_state", "the swing planner"), ("gait_dt", "the gait clock (the contact mask is held)")):
        if batch.get(name) is not None:
            raise ValueError(f"{who}: batch['{name}'] must be None - {why} has no forward mode")
    if batch.get("swing_pos") is None or batch.get("swing_vel") is None:
        raise ValueError(f"{who}: the batch carries swing_pos and swing_vel, both (rollout_tick_tangent() differentiates a batch without swing references)")
    if batch.get("joint_q") is None or batch.get("joint_qdot") is None:
        raise ValueError(f"{who}: the batch carries joint_q and joint_qdot (rollout_tangent() steps the bare rigid body)")


def rollout_swing_tangent(ctl, batch, steps, dt, leg_inertia, tangents, act_tol=1e-7, warm=True, stream=None, command=None, lean=None, params_tan=None):
    """The forward-mode twin of ctl.rollout_tick(batch, None, ...) for a batch that carries swing_pos AND swing_vel: forward mode
    through a trot.  The two references and the `stance` / `gait_phase` / `gait_duty` contact mask are HELD over the rollout, exactly
    as rollout_tick_autograd() holds them.  Per step: control_batch(want_torques=True), tangent_batch(), torque_tangent(),
    swing_torque_tangent() in place on joint_tau_tan, leg_plant_step_tangent() (it reads the state before the step) and
    leg_plant_step(), everything planned once, on one stream and without a host round trip.  `batch` is advanced IN PLACE and ends bit
    for bit where ctl.rollout_tick() leaves it.  `tangents`: rollout_tick_tangent()'s - the start state's "Rwb_rot_tan", "x_tan",
    "xdot_tan", "w_tan" [n,3], "joint_q_tan", "joint_qdot_tan" [n,12] and the held "x_d_tan", "xdot_d_tan", "w_d_tan", "Rwb_d_rot_tan" -
    plus the held "swing_pos_tan" and "swing_vel_tan" [n,12], applied at every step; each [n, ...] or [K, n, ...], all agreeing; none is
    written.  Returns (state, res) as rollout_tick_tangent() does.  res["flags"] int32 [n], OR-ed over the steps on the device, is
    rollout_tick_tangent()'s word - bits 0-1 tangent_batch()'s, bits 8-15 the plant's shifted left by 8 - with swing_torque_tangent()'s
    bits shifted left by SWING_FLAGS_SHIFT = 16: bit 16 + l, swing leg l's reference had no derivative at some step (its torque
    tangent, and what follows from it, is NaN).  The derivative is the one on the active face of every solve at `act_tol` and at
    every tick's clamp masks, as rollout_tick_autograd()'s.  Tangent memory is one set of buffers whatever `steps` is.  ValueError for
    swing_state, gait_dt, a `command`, `lean`, and for a batch with only one of swing_pos / swing_vel (or neither) - in THIS rollout:
    rollout_gait_tangent() takes the planner, rollout_commander_tangent() a `command` and rollout_lean_tangent() a `lean`.
    `params_tan` ([211] or [K, 211]): directions in the handle's parameters, held over the rollout, as rollout_tick_tangent() takes them."""
    who = "rollout_swing_tangent"
    _swing_rollout_refusals(who, batch, command, lean)
    return _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, tangents, ROLLOUT_SWING_TANGENTS, act_tol, warm, stream, True, params_tan=params_tan)


def rollout_swing_transition(ctl, batch, steps, dt, leg_inertia, act_tol=1e-7, warm=True, chunk=None, stream=None):
    """The 36 x 36 state-transition matrix of `steps` closed-loop steps through a trot: rollout_swing_tangent() on the 36 unit seeds of
    the start state (tick_transition_seeds), in rollout_tick_transition()'s column order and chunked the same way (the start state is
    restored between the chunks; the references and the mask are held).  `batch` is advanced in place, as by ctl.rollout_tick().
    Returns dict(phi [n,36,36], columns, flags int32 [n]: rollout_swing_tangent()'s, OR-ed over the chunks).  Column c equals
    rollout_swing_tangent() on seed c bit for bit, however the columns are chunked; steps = 0 gives the identity.  ValueError as
    rollout_swing_tangent()."""
    who = "rollout_swing_transition"
    _swing_rollout_refusals(who, batch, None, None)
    return _tick_transition(who, rollout_swing_tangent, ctl, batch, steps, dt, leg_inertia, act_tol, warm, chunk, stream)


# ------------------------------------------------------------------ forward mode through the planner: the swing references
def plan_swing_reference_tangent(ctl, batch, state_before, tangents, want=SWING_REFERENCE_TANGENT_WANT, out=None, stream=None):
    """swing_reference_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_swing_reference_tangent_batch
    call (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors (and "flags" int32 [n] where asked for)
    and squeeze says whether the tangents came as [n, ...].  out["p_start_next_tan"] may be tangents["p_start_tan"],
    out["p_final_next_tan"] tangents["p_final_tan"], and out["swing_pos_tan"] / out["swing_vel_tan"] any [K, n, 12] tangent (the aliasing
    contract of include/qc_tangent.h).  Planning launches nothing."""
    from .balance_controller import _SWING_REFERENCE_FIELDS, SWING_STATE_DTYPE, _record_tensor

    _library()
    unknown = [k for k in tangents if k not in SWING_REFERENCE_TANGENTS]
    if unknown:
        raise ValueError(f"swing_reference_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(SWING_REFERENCE_TANGENTS)}")
    io = QcSwingReferenceTangentIo()
    ctl._lib.qc_default_swing_reference_tangent(C.byref(io))
    sizing = [batch.get(k) for k in ("x", "Rwb", "xdot", "w", "joint_q", "gait_phase")] + [t for t in tangents.values() if t is not None and t.dim() == 2]
    n, dev, bi = ctl._readonly_batch("swing_reference_tangent", batch, _SWING_REFERENCE_FIELDS, io, [], sizing,
                                     "none of the arrays the planner reads is there to size the call")
    if _record_tensor("swing_state", batch.get("swing_state"), n, SWING_STATE_DTYPE.itemsize, dev):  # (not read: the records come as state_before)
        bi.swing_state = batch["swing_state"].data_ptr()
    if _record_tensor("state_before", state_before, n, SWING_STATE_DTYPE.itemsize, dev):  # (a missing one is the library's refusal)
        io.state_before = state_before.data_ptr()
    given, K, squeeze = _directions(tangents, SWING_REFERENCE_TANGENTS, n, dev, io)
    io.n_dir = K
    rows = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("swing_reference_tangent", _SWING_REFERENCE_TANGENT_OUTPUTS, rows, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _SWING_REFERENCE_TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_swing_reference_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)),
                           (batch, state_before, given, res, bi, io), ValueError)
    return launch, res, squeeze


def swing_reference_tangent(ctl, batch, state_before, tangents, want=SWING_REFERENCE_TANGENT_WANT, out=None, stream=None):
    """Forward mode of ctl.swing_reference_batch() (qc_swing_reference_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode
    through the planner"), the map ctl.swing_reference_adjoint_batch() transposes, under that call's contract: `batch` is the one the
    forward call read, with gait_phase AS THAT CALL LEFT IT and without gait_dt - Rwb, x, xdot, w, joint_q, gait_phase and the optional
    stance / gait_duty are all that is read of it -, `state_before` a copy of the swing_state tensor from BEFORE the forward call: the
    plan decisions are recomputed from it and held, as are the clock and the contact mask.  `tangents`: a dict with any of
    "Rwb_rot_tan" (the world-frame left tangent, Rwb <- exp([d]x) Rwb), "x_tan", "xdot_tan", "w_tan", "xdot_d_tan" ([n,3]),
    "joint_q_tan" and, on the record before the call, "p_start_tan", "p_final_tan" ([n,12]) - each [n, ...] for one direction or
    [K, n, ...] for K, all agreeing on K; a missing one is zero, at least one given.  `want`: any of "swing_pos_tan", "swing_vel_tan"
    [K,n,4,3], "p_start_next_tan", "p_final_next_tan" [K,n,12] (on the record after the call) and "flags" int32 [n].  A replanned leg's
    end points follow the state (the foothold's z has tangent 0), any other leg's pass the record's tangents through; a swing leg with
    a trajectory after the call gets the sextic's linear map of the two, every other leg exact zeros.  flags bit l: leg l is replanned
    at an x_z that is not finite and > 0 - NaN in every row of the robot, in every direction.  Returns the dict of device tensors,
    squeezed to [n, ...] where the tangents came that way; `out`: a dict of tensors to write into (the aliasing contract:
    plan_swing_reference_tangent()).  Nothing of `batch` or `state_before` is written.  Asynchronous on `stream`, no synchronisation.
    ValueError with the library's message for a call it refuses.  Not covered: tangents of the phase, of gait_dt, of the gait's
    periods, of swing_height, of planner_k and of the kinematic constants."""
    launch, res, squeeze = plan_swing_reference_tangent(ctl, batch, state_before, tangents, want, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


_ROLLOUT_GAIT_REFUSED = {"stance": "the gait clock makes the contact mask from gait_phase", "swing_pos": "the references are made per step",
                         "swing_vel": "the references are made per step", "gait_dt": "the clock's step is this call's gait_dt argument",
                         "feet": "the tick reads joint_q (rollout_tangent() steps the bare rigid body on `feet`)"}
_ROLLOUT_GAIT_NEEDED = ("joint_q", "joint_qdot", "gait_phase", "swing_state")


def _gait_rollout_refusals(who, batch, lean):
    """what the rollouts through the planner refuse before anything is planned"""
    if lean is not None:
        raise ValueError(f"{who}: lean has no forward mode - lean must be None (the com reference has no forward mode)")
    for name, why in _ROLLOUT_GAIT_REFUSED.items():
        if batch.get(name) is not None:
            raise ValueError(f"{who}: batch['{name}'] must be None - {why}")
    missing = [name for name in _ROLLOUT_GAIT_NEEDED if batch.get(name) is None]
    if missing:
        raise ValueError(f"{who}: the batch carries joint_q, joint_qdot, gait_phase and swing_state - missing {missing}")


def _gait_clock(gait_dt, n, dev):
    """the clock's step of a gait rollout as a float64 [n] tensor (a tensor is copied: the caller's is not kept)"""
    import torch

    if isinstance(gait_dt, torch.Tensor):
        if gait_dt.numel() != n:
            raise ValueError(f"gait_dt: a number or a tensor of {n} values")
        return gait_dt.detach().to(dtype=torch.float64, device=dev).reshape(n).clone()
    return torch.full((n,), float(gait_dt), dtype=torch.float64, device=dev)


def rollout_gait_tangent(ctl, batch, steps, dt, leg_inertia, gait_dt, tangents, act_tol=1e-7, warm=True, stream=None, lean=None, params_tan=None):
    """The forward-mode twin of ctl.rollout_tick(batch, None, ...) for a batch with swing_state and a running clock - of
    rollout_gait_autograd() -: forward mode through the planner.  Per step: a copy of the records, swing_reference_batch() with
    `gait_dt` (a number or a float64 [n] tensor; the phases and the records advance IN PLACE), swing_reference_tangent() (the record's
    two tangents in place, swing_pos_tan / swing_vel_tan written), control_batch(want_torques=True) on the returned references and
    the phases left, tangent_batch(), torque_tangent(), swing_torque_tangent() in place on joint_tau_tan, leg_plant_step_tangent() (it
    reads the state before the step) and leg_plant_step() with those same phases - everything planned once, on one stream and without
    a host round trip.  `batch`, its gait_phase and its swing_state are advanced IN PLACE and end bit for bit where ctl.rollout_tick()
    leaves them with a gait_dt of `dt`.  `tangents`: rollout_tick_tangent()'s - the start state's "Rwb_rot_tan", "x_tan", "xdot_tan",
    "w_tan" [n,3], "joint_q_tan", "joint_qdot_tan" [n,12] and the held "x_d_tan", "xdot_d_tan" (it enters the planner too), "w_d_tan",
    "Rwb_d_rot_tan" - plus "p_start_tan", "p_final_tan" [n,12] on the start record; each [n, ...] or [K, n, ...], all agreeing; none is
    written.  The references' tangents are computed, not taken.  Returns (state, res) as rollout_swing_tangent() does; `res` adds the
    final "p_start_tan", "p_final_tan" [K,n,12] and the last "swing_pos_tan", "swing_vel_tan" [K,n,4,3].  res["flags"] int32 [n], OR-ed
    over the steps on the device, is rollout_swing_tangent()'s word with swing_reference_tangent()'s bits shifted left by
    REFERENCE_FLAGS_SHIFT = 20: bit 20 + l, leg l was replanned at an x_z that is not finite and > 0 at some step.  The clock, the
    contact mask and the plan decisions are held, as in rollout_gait_autograd(); the derivative is the one on the active face of
    every solve at `act_tol` and at every tick's clamp masks.  Tangent memory is one set of buffers whatever `steps` is.  ValueError
    for `lean` (rollout_lean_tangent() is this rollout with the lean; rollout_commander_tangent() takes a `command`), a `stance` mask,
    swing_pos / swing_vel, a gait_dt inside the batch, `feet`, and a batch without joint_q, joint_qdot, gait_phase or swing_state.
    `params_tan` ([211] or [K, 211]): directions in the handle's parameters, held over the rollout, as rollout_tick_tangent() takes them."""
    import torch

    who = "rollout_gait_tangent"
    _gait_rollout_refusals(who, batch, lean)
    unknown = [k for k in tangents if k not in ROLLOUT_GAIT_TANGENTS]
    if unknown:  # (swing_pos_tan / swing_vel_tan among them: the references' tangents are computed; refused before anything touches the device)
        raise ValueError(f"{who}: unknown tangent(s) {unknown}; the tangents are {tuple(ROLLOUT_GAIT_TANGENTS)}")
    clock = _gait_clock(gait_dt, batch["x"].shape[0], torch.device("cuda", ctl.device))
    return _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, tangents, ROLLOUT_GAIT_TANGENTS, act_tol, warm, stream, True, clock, params_tan=params_tan)


def rollout_gait_transition(ctl, batch, steps, dt, leg_inertia, gait_dt, act_tol=1e-7, warm=True, chunk=None, stream=None):
    """The 60 x 60 state-transition matrix of `steps` closed-loop steps through the planner in minimal coordinates -
    TICK_TRANSITION_COLUMNS (the rotation tangent, x, xdot, w, joint_q[12], joint_qdot[12]), then the record's p_start[12] and
    p_final[12] -: rollout_gait_tangent() on the 60 unit seeds, `chunk` seeds per rollout (None: all in one; the state, the phases and
    the records are restored between the chunks).  `batch`, its gait_phase and its swing_state are advanced in place, as by
    rollout_gait_tangent().  Returns dict(phi [n,60,60], columns, flags int32 [n]: rollout_gait_tangent()'s, OR-ed over the chunks).
    Column c equals rollout_gait_tangent() on seed c bit for bit, however the columns are chunked; steps = 0 gives the identity.
    ValueError as rollout_gait_tangent()."""
    who = "rollout_gait_transition"
    _gait_rollout_refusals(who, batch, None)

    def rollout(ctl, batch, steps, dt, leg_inertia, seeds, act_tol, warm, stream):
        return rollout_gait_tangent(ctl, batch, steps, dt, leg_inertia, gait_dt, seeds, act_tol, warm, stream)

    return _tick_transition(who, rollout, ctl, batch, steps, dt, leg_inertia, act_tol, warm, chunk, stream, GAIT_TRANSITION_COLUMNS,
                            _TICK_STATE + _GAIT_RECORD, ("gait_phase", "swing_state"))


# ------------------------------------------------------------------ forward mode through the command and the lean
def plan_commander_step_tangent(ctl, batch, command, state_before, tangents, want=COMMANDER_STEP_TANGENT_WANT, out=None, stream=None):
    """commander_step_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_commander_step_tangent_batch
    call (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors (and "flags" int32 [n] where asked for)
    and squeeze says whether the tangents came as [n, ...].  The four desired-state outputs may be the four `_prev_` tangents and
    out["Vb_next_tan"] may be tangents["Vb_tan"] (the aliasing contract of include/qc_tangent.h).  Planning launches nothing."""
    from .balance_controller import _COMMANDER_STEP_FIELDS, _record_tensor

    _library()
    unknown = [k for k in tangents if k not in COMMANDER_STEP_TANGENTS]
    if unknown:
        raise ValueError(f"commander_step_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(COMMANDER_STEP_TANGENTS)}")
    io = QcCommanderStepTangentIo()
    ctl._lib.qc_default_commander_step_tangent(C.byref(io))
    sizing = [batch.get("x"), batch.get("Rwb")] + [t for t in tangents.values() if t is not None and t.dim() == 2]
    n, dev, bi = ctl._readonly_batch("commander_step_tangent", batch, _COMMANDER_STEP_FIELDS, io, [], sizing, "neither x nor Rwb is there to size the call")
    c = ctl._marshal_command(n, command, False)  # (the records it reads are state_before)
    if _record_tensor("state_before", state_before, n, COMMANDER_STATE_DTYPE.itemsize, dev):  # (a missing one is the library's refusal)
        io.state_before = state_before.data_ptr()
    given, K, squeeze = _directions(tangents, COMMANDER_STEP_TANGENTS, n, dev, io)
    io.n_dir = K
    rows = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("commander_step_tangent", _COMMANDER_STEP_TANGENT_OUTPUTS, rows, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _COMMANDER_STEP_TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_commander_step_tangent_batch", (n, C.byref(bi), C.byref(c), C.byref(io), ctl._stream_ptr(stream)),
                           (batch, command, state_before, given, res, bi, c, io), ValueError)
    return launch, res, squeeze


def commander_step_tangent(ctl, batch, command, state_before, tangents, want=COMMANDER_STEP_TANGENT_WANT, out=None, stream=None):
    """Forward mode of ctl.commander_step_batch() (qc_commander_step_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode
    through the command and the lean"), the map ctl.commander_step_adjoint_batch() transposes, under that call's contract: `batch`: Rwb
    and x as the forward call read them; `command`: its twist, fresh and scalars (its records are not read); `state_before`: a copy of
    the record tensor from BEFORE the forward call - the latches and branch decisions are recomputed from it and held.  `tangents`: a
    dict with any of "twist_tan", "Vb_tan" [n,6] (the command that arrives, the command that is held: `fresh` says which one a robot
    reads), "Rwb_rot_tan" (the world-frame left tangent, Rwb <- exp([d]x) Rwb), "x_tan" and, on the record's desired state before the
    call, "Rwb_d_rot_prev_tan", "x_d_prev_tan", "xdot_d_prev_tan", "w_d_prev_tan" ([n,3]) - each [n, ...] for one direction or
    [K, n, ...] for K, all agreeing on K; a missing one is zero, at least one given.  `want`: any of "Rwb_d_rot_tan", "x_d_tan",
    "xdot_d_tan", "w_d_tan" [K,n,3] - what tangent_batch() and swing_reference_tangent() take under those names -, "Vb_next_tan" [K,n,6]
    and "flags" int32 [n].  A robot whose command is not applied passes the four `_prev_` tangents through bit for bit; where one is
    applied with zero angular rate the smooth limit of the rotation's derivative is used, so a yaw-rate seed is not silently lost;
    x_d_tan's z is exactly 0 there (the stand height is a constant).  flags bit 0: a command applied at gimbal lock - NaN in every row
    of the robot, in every direction.  Returns the dict of device tensors, squeezed to [n, ...] where the tangents came that way; `out`:
    a dict of tensors to write into (the aliasing contract: plan_commander_step_tangent()).  Nothing of `batch`, `command` or
    `state_before` is written.  Asynchronous on `stream`, no synchronisation.  ValueError with the library's message for a call it
    refuses.  Not covered: tangents of stand_height, stand_tol and cmd_dt."""
    launch, res, squeeze = plan_commander_step_tangent(ctl, batch, command, state_before, tangents, want, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def plan_com_reference_tangent(ctl, batch, schedule, x_d_in, tangents, mode="replace", gain=1.0, want=("x_d_out_tan",), out=None, stream=None):
    """com_reference_tangent() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_com_reference_tangent_batch
    call (graph-capturable) on tensors that are read in place; `out` holds [K, n, ...] tensors (and "flags" int32 [n] where asked for)
    and squeeze says whether the tangents came as [n, ...].  out["x_d_out_tan"] may be tangents["x_d_in_tan"].  `x_d_in` is not read by
    the derivative (the map is affine in it) and not looked at; it is taken for the symmetry with com_reference_batch() and may be None.  Planning
    launches nothing."""
    import torch

    from .balance_controller import _SUPPORT_POLYGON_FIELDS

    _library()
    if mode not in _lib.COM_MODES:
        raise ValueError(f"com_reference_tangent: mode is one of {tuple(_lib.COM_MODES)}, not {mode!r}")
    unknown = [k for k in tangents if k not in COM_REFERENCE_TANGENTS]
    if unknown:
        raise ValueError(f"com_reference_tangent: unknown tangent(s) {unknown}; the tangents are {tuple(COM_REFERENCE_TANGENTS)}")
    io = QcComReferenceTangentIo()
    ctl._lib.qc_default_com_reference_tangent(C.byref(io))
    n, dev, bi = ctl._readonly_batch("com_reference_tangent", batch, _SUPPORT_POLYGON_FIELDS, io, [], [batch.get(k) for k in ("gait_phase", "feet", "joint_q")],
                                     "the batch holds neither gait_phase nor feet nor joint_q")
    if batch.get("swing_state") is not None:  # (handed over unchecked: the library names its refusal)
        bi.swing_state = batch["swing_state"].data_ptr()
    shared = False
    if schedule is not None:
        shared = schedule.dim() == 2
        if schedule.dtype != torch.float64 or not schedule.is_contiguous() or schedule.device != dev or tuple(schedule.shape) != ((4, 4) if shared else (n, 4, 4)):
            raise ValueError(f"schedule: need contiguous float64 [4,4] (shared) or [{n},4,4] on {dev}")
        io.schedule, io.schedule_shared = schedule.data_ptr(), int(shared)
    io.mode, io.gain = _lib.COM_MODES[mode], float(gain)
    # a shared schedule's tangent is one [4,4] block per direction: [4,4] (squeezed) or [K,4,4]
    rows = {k: t for k, t in tangents.items() if not (shared and k == "schedule_tan")}
    given, K, squeeze = _directions(rows, COM_REFERENCE_TANGENTS, n, dev, io)
    st = tangents.get("schedule_tan") if shared else None
    if st is not None:
        flat = st.dim() == 2
        if st.dtype != torch.float64 or not st.is_contiguous() or st.device != dev or tuple(st.shape[-2:]) != (4, 4) or st.dim() not in (2, 3):
            raise ValueError(f"schedule_tan: with a shared schedule, need contiguous float64 [4,4] or [K,4,4] on {dev}")
        lead = 1 if flat else st.shape[0]
        if given and (lead != K or flat != squeeze):
            raise ValueError("schedule_tan: the tangents must agree on the number of directions and on the squeezed / [K, ...] form")
        K, squeeze = lead, flat
        io.schedule_tan = st.data_ptr()
        given = dict(given, schedule_tan=st)
    io.n_dir = K
    names = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("com_reference_tangent", _COM_REFERENCE_TANGENT_OUTPUTS, names, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _COM_REFERENCE_TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_com_reference_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)),
                           (batch, schedule, x_d_in, given, res, bi, io), ValueError)
    return launch, res, squeeze


def com_reference_tangent(ctl, batch, schedule, x_d_in, tangents, mode="replace", gain=1.0, want=("x_d_out_tan",), out=None, stream=None):
    """Forward mode of ctl.com_reference_batch() (qc_com_reference_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode
    through the command and the lean"), the map ctl.com_reference_adjoint_batch() transposes.  `batch`, `schedule`, `mode`, `gain`: the
    forward call's - nothing was saved; the contact mask is held.  `tangents`: a dict with any of "x_d_in_tan" [n,3], "feet_tan" [n,4,3]
    (body frame), "joint_q_tan" [n,12] (only for a batch with joint_q; added through the leg Jacobian), "Rwb_rot_tan" (the world-frame
    left tangent), "x_tan" [n,3], "phase_tan" [n,4] and "schedule_tan" - [n,4,4], or with a shared [4,4] schedule ONE block per
    direction, [4,4] / [K,4,4] - each [n, ...] for one direction or [K, n, ...] for K, all agreeing; a missing one is zero, at least one
    given.  `want`: any of "x_d_out_tan" [K,n,3] - replace: (com_xy_tan, x_d_in_tan.z); offset: x_d_in_tan + gain (com_xy_tan - the
    centroid's tangent, 0) -, "com_xy_tan" [K,n,2] (the polygon's own tangent: support_polygon_batch(world=True)'s) and "flags" int32
    [n] (bit l: the reference's 0/0 at leg l's point - NaN in every row of the robot, in every direction).  Returns the dict of device
    tensors, squeezed where the tangents came that way; `out`: a dict of tensors to write into - x_d_out_tan may be x_d_in_tan.
    Nothing of `batch` is written.  Asynchronous on `stream`, no synchronisation.  ValueError with the library's message for a call it
    refuses.  Not covered: a tangent of `gain`, and of the phase through the clock."""
    launch, res, squeeze = plan_com_reference_tangent(ctl, batch, schedule, x_d_in, tangents, mode, gain, want, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


# ------------------------------------------------------------------ the rollouts through the command and the lean
COMMANDER_FLAGS_SHIFT = 24  # rollout_commander_tangent()'s flags: rollout_gait_tangent()'s word | commander_step_tangent()'s bit << 24
LEAN_FLAGS_SHIFT = 25       # ... | com_reference_tangent()'s four bits << 25 (rollout_lean_tangent() too)
_COMMANDER_CARRIED = {"Rwb_d_rot_tan": "Rwb_d_rot_prev_tan", "x_d_tan": "x_d_prev_tan", "xdot_d_tan": "xdot_d_prev_tan", "w_d_tan": "w_d_prev_tan"}
ROLLOUT_LEAN_TANGENTS = {**ROLLOUT_GAIT_TANGENTS, "schedule_tan": 16}
ROLLOUT_COMMANDER_TANGENTS = {**ROLLOUT_GAIT_TANGENTS, "twist_tan": 6, "Vb_tan": 6, "schedule_tan": 16}


def _lead_tangent(who, name, t, inner, n, dev):
    """A tangent the hooks take themselves - `inner`: its shape for one direction, e.g. (n, 6), (steps, n, 6) or (4, 4) - as
    ([K, *inner] contiguous view, K, squeeze), or None."""
    import torch

    if t is None:
        return None
    inner = tuple(inner)
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev or tuple(t.shape) not in (inner, tuple(t.shape[:1]) + inner):
        raise ValueError(f"{who}: {name}: need contiguous float64 {list(inner)} or [K, {', '.join(str(v) for v in inner)}] on {dev}")
    squeeze = tuple(t.shape) == inner
    return t.reshape((-1,) + inner), (1 if squeeze else t.shape[0]), squeeze


def _agree(who, leads):
    """(K, squeeze) of the tangents a hook takes itself - `leads`: (view, K, squeeze) or None each -, which must agree, or None where
    there is none: the step loop validates the others once, holds them to this form and refuses a call without any tangent"""
    forms = {(K, squeeze) for _, K, squeeze in (v for v in leads if v is not None)}
    if len(forms) > 1:
        raise ValueError(f"{who}: the tangents must agree on the number of directions and on the squeezed / [K, ...] form")
    return forms.pop() if forms else None


class _LeanHook:
    """the lean in front of a step: com_reference_batch() and com_reference_tangent() on the state and the phases as the step finds
    them, before the clock advances.  `base` / `base_tan`: the x_d that is leaned and its tangent buffer (None: zero); the leaned x_d
    goes to `x_d`, its tangent to a buffer of this hook that takes the place of the held x_d_tan."""

    def __init__(self, ctl, who, batch, n, K, dev, buf, stream, lean, schedule_tan, base, base_tan, x_d):
        import torch

        schedule, mode, gain = lean
        self.flag_word = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.x_d_tan = torch.zeros((K, n, 3), dtype=torch.float64, device=dev)
        reads = {k: batch[k] for k in ("joint_q", "Rwb", "x", "gait_phase", "gait_duty") if batch.get(k) is not None}
        self.forward = ctl.plan_com_reference(reads, schedule, base, mode, gain, out={"x_d": x_d}, stream=stream)[0]
        tans = {"joint_q_tan": buf["joint_q_tan"].view(K, n, 12), "Rwb_rot_tan": buf["Rwb_rot_tan"], "x_tan": buf["x_tan"]}
        if base_tan is not None:
            tans["x_d_in_tan"] = base_tan
        if schedule_tan is not None:
            tans["schedule_tan"] = schedule_tan
        self.tangent = plan_com_reference_tangent(ctl, reads, schedule, None, tans, mode, gain, ("x_d_out_tan", "flags"),
                                                  {"x_d_out_tan": self.x_d_tan, "flags": self.flag_word}, stream)[0]

    def step(self, k):
        self.forward()
        self.tangent()

    def flags(self, word):
        word.bitwise_or_(self.flag_word.bitwise_left_shift(LEAN_FLAGS_SHIFT))


def _lean_arguments(who, lean, default_mode, tangents, n, dev):
    """(schedule, mode, gain) of `lean` and the lead form of tangents["schedule_tan"]: [n,4,4] / [K,n,4,4], or with a shared [4,4]
    schedule one block per direction, [4,4] / [K,4,4]"""
    from .autograd import _lean

    lean = _lean(who, lean, default_mode)
    st = tangents.get("schedule_tan")
    if lean is None:
        if st is not None:
            raise ValueError(f"{who}: schedule_tan needs lean")
        return None, None
    if lean[1] not in _lib.COM_MODES:
        raise ValueError(f"{who}: lean's mode is one of {tuple(_lib.COM_MODES)}, not {lean[1]!r}")
    shared = lean[0].dim() == 2
    return lean, _lead_tangent(who, "schedule_tan", st, (4, 4) if shared else (n, 4, 4), n, dev)


def rollout_lean_tangent(ctl, batch, steps, dt, leg_inertia, gait_dt, lean, tangents, act_tol=1e-7, warm=True, stream=None, params_tan=None):
    """The forward-mode twin of ctl.rollout_tick(batch, None, ..., lean=lean) for a batch with swing_state and a running clock - of
    rollout_gait_autograd(lean=lean) -: rollout_gait_tangent()'s loop with com_reference_batch() and com_reference_tangent() in front of
    each step, on the state and the phases as the step finds them (before the clock advances); the feet's tangent comes from the
    carried joint_q_tan.  lean = dict(schedule=..., mode="replace", gain=1.0), as rollout_tick() takes it; batch["x_d"] is written IN
    PLACE from a copy taken at entry, as rollout_tick() writes it.  `tangents`: rollout_gait_tangent()'s, plus "schedule_tan" - [n,4,4] /
    [K,n,4,4], or with a shared [4,4] schedule ONE block per direction, [4,4] / [K,4,4]; a held "x_d_tan" is the tangent of the x_d that
    is leaned.  The state, the phases and the records end bit for bit where rollout_tick(..., lean=lean) leaves them with a gait_dt of
    `dt`.  Returns (state, res) as rollout_gait_tangent() does; `res` adds the last step's "x_d_tan" (the leaned x_d's tangent), and
    res["flags"] carries com_reference_tangent()'s bits shifted left by LEAN_FLAGS_SHIFT = 25: bit 25 + l, leg l's point was the
    reference's 0/0 at some step.  The contact mask of the polygon is held, as the clock is.  One set of tangent buffers whatever
    `steps` is.  ValueError as rollout_gait_tangent(), and for a batch without x_d.
    `params_tan` ([211] or [K, 211]): directions in the handle's parameters, held over the rollout, as rollout_tick_tangent() takes them."""
    import torch

    who = "rollout_lean_tangent"
    _gait_rollout_refusals(who, batch, None)
    if lean is None:
        raise ValueError(f"{who}: lean is required (rollout_gait_tangent() is this rollout without it)")
    if batch.get("x_d") is None:
        raise ValueError(f"{who}: lean needs batch['x_d'] (its z in replace mode, the base of the offset)")
    unknown = [k for k in tangents if k not in ROLLOUT_LEAN_TANGENTS]
    if unknown:
        raise ValueError(f"{who}: unknown tangent(s) {unknown}; the tangents are {tuple(ROLLOUT_LEAN_TANGENTS)}")
    n, dev = batch["x"].shape[0], torch.device("cuda", ctl.device)
    lean, st = _lean_arguments(who, lean, "replace", tangents, n, dev)
    rest = {k: v for k, v in tangents.items() if k != "schedule_tan"}
    lead = _agree(who, [st])
    if lead is None and params_tan is not None and not any(v is not None for v in rest.values()):
        lead = _param_directions(who, params_tan, dev)  # params_tan alone is a seed
    clock = _gait_clock(gait_dt, n, dev)

    def hook(ctl, who, batch, n, K, dev, buf, given, stream):
        base_tan = given["x_d_tan"].reshape(K, n, 3) if "x_d_tan" in given else None
        h = _LeanHook(ctl, who, batch, n, K, dev, buf, stream, lean, None if st is None else st[0], batch["x_d"].clone(), base_tan, batch["x_d"])
        h.held, h.desired, h.res = {"x_d_tan": h.x_d_tan}, {}, {"x_d_tan": h.x_d_tan}
        return h

    return _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, rest, ROLLOUT_GAIT_TANGENTS, act_tol, warm, stream, True, clock, hook, lead, params_tan)


class _CommanderHook:
    """the commander step in front of a step: a copy of the records, commander_step_batch() (the records advance in place),
    commander_step_tangent() with the four desired-state tangents and Vb_tan carried in place, and - with `lean` - the lean of the
    commander's x_d for the tick alone, on a buffer of its own."""

    def __init__(self, ctl, who, batch, n, K, dev, buf, given, stream, command, steps, twist_tan, Vb_tan, lean, schedule_tan):
        import contextlib

        import torch

        self.on_stream = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        self.state = command["state"]
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        with self.on_stream():
            self.before = torch.empty_like(self.state)
            self.desired = {"Rwb_d": zeros(n, 9), "x_d": zeros(n, 3), "xdot_d": zeros(n, 3), "w_d": zeros(n, 3)}
            self.held = {k: (given[k].reshape(K, n, 3).clone() if k in given else zeros(K, n, 3)) for k in _COMMANDER_CARRIED}
            self.Vb_tan = Vb_tan.clone() if Vb_tan is not None else zeros(K, n, 6)
            self.flag_word = torch.zeros((n,), dtype=torch.int32, device=dev)
        twist, fresh = command.get("twist"), command.get("fresh")
        scalars = {k: command[k] for k in ("stand_height", "stand_tol", "cmd_dt") if command.get(k) is not None}
        sequence = twist is not None and twist.dim() == 3
        if sequence:  # one command per step, fresh where it says (default: everywhere)
            if fresh is None:
                fresh = torch.ones((steps, n), dtype=torch.uint8, device=dev)
            # direction-major per step: [K, steps, n, 6] -> [steps, K, n, 6]
            per_step = None if twist_tan is None else twist_tan.permute(1, 0, 2, 3).contiguous()
            variants = [(dict(scalars, twist=twist[k], fresh=fresh[k]), None if per_step is None else per_step[k]) for k in range(steps)]
            self.pick = lambda k: k
        else:  # rollout_tick()'s rule: `fresh` holds on step 0 only
            first = dict(scalars, **({} if twist is None else {"twist": twist}), **({} if fresh is None else {"fresh": fresh}))
            variants = [(first, twist_tan if twist is not None else None), (dict(scalars), None)]
            self.pick = lambda k: 0 if k == 0 else 1
        pose = {"Rwb": batch["Rwb"], "x": batch["x"]}
        carried = dict({prev: self.held[k] for k, prev in _COMMANDER_CARRIED.items()}, Vb_tan=self.Vb_tan, Rwb_rot_tan=buf["Rwb_rot_tan"], x_tan=buf["x_tan"])
        out = dict(self.held, Vb_next_tan=self.Vb_tan, flags=self.flag_word)
        self.plans = []
        for cmd, tw in variants:
            forward = ctl.plan_commander_step(pose, dict(cmd, state=self.state), tuple(self.desired), self.desired, stream)[0]
            tans = dict(carried, **({} if tw is None else {"twist_tan": tw}))
            self.plans.append((forward, plan_commander_step_tangent(ctl, pose, cmd, self.before, tans, tuple(out), out, stream)[0]))
        self.res = dict(self.held, Vb_tan=self.Vb_tan)
        self.lean = None
        if lean is not None:
            with self.on_stream():
                x_d = zeros(n, 3)
            self.lean = _LeanHook(ctl, who, batch, n, K, dev, buf, stream, lean, schedule_tan, self.desired["x_d"], self.held["x_d_tan"], x_d)
            # (the tick alone tracks the leaned value: the record and its tangent keep the un-leaned integral)
            self.desired = dict(self.desired, x_d=x_d)
            self.held = dict(self.held, x_d_tan=self.lean.x_d_tan)
            self.res["x_d_lean_tan"] = self.lean.x_d_tan

    def step(self, k):
        with self.on_stream():
            self.before.copy_(self.state)
        forward, tangent = self.plans[self.pick(k)]
        forward()
        tangent()
        if self.lean is not None:
            self.lean.step(k)

    def flags(self, word):
        word.bitwise_or_(self.flag_word.bitwise_left_shift(COMMANDER_FLAGS_SHIFT))
        if self.lean is not None:
            self.lean.flags(word)


def rollout_commander_tangent(ctl, batch, command, steps, dt, leg_inertia, gait_dt, tangents, act_tol=1e-7, warm=True, stream=None, lean=None,
                              params_tan=None):
    """The forward-mode twin of ctl.rollout_tick(batch, command, ...) for robots that stand and run - of rollout_commander_autograd() -:
    the sensitivity of a closed-loop gait rollout to the twist command.  Per step: a copy of the commander records,
    commander_step_batch() (the records advance IN PLACE), commander_step_tangent() - the four desired-state tangents and Vb_tan carried
    in place -, with `lean` com_reference_batch() and com_reference_tangent() on a separate x_d buffer for the tick alone (default
    mode "offset"; the record keeps the un-leaned integral, as in the autograd twin), then rollout_gait_tangent()'s step with the
    commander's desired state and its tangents in place of the held ones - xdot_d_tan enters the planner's tangent too.  `batch` as
    rollout_commander_autograd() takes it: joint_q, joint_qdot, gait_phase, swing_state, no desired state of its own.  `command`:
    tick_batch()'s dict; a single twist [n,6] is applied under rollout_tick()'s rule (`fresh` holds on step 0 only), a sequence
    twist [steps,n,6] with an optional fresh [steps,n] step by step.  `tangents`: rollout_gait_tangent()'s start-state and record
    tangents; "Rwb_d_rot_tan", "x_d_tan", "xdot_d_tan", "w_d_tan" are here the tangents of the START RECORD's desired state; plus
    "twist_tan" - [n,6] / [K,n,6], for a sequence [steps,n,6] / [K,steps,n,6] -, "Vb_tan" [n,6] / [K,n,6] on the held command and, with
    `lean`, "schedule_tan" as rollout_lean_tangent() takes it.  As rollout_commander_autograd(), this call reads the latches ONCE on the
    host and refuses a batch in which not every robot stands and runs.  With lean = None the state, the phases, the swing records and
    the commander records end bit for bit where ctl.rollout_tick(batch, command, ...) leaves them with a gait_dt of `dt`; with `lean`
    they are the forward values of rollout_commander_autograd(lean=lean).  Returns (state, res) as rollout_gait_tangent() does; `res`
    adds the record's final "Rwb_d_rot_tan", "x_d_tan", "xdot_d_tan", "w_d_tan" and "Vb_tan" (with `lean`: "x_d_lean_tan", the last
    tick's), and res["flags"] carries commander_step_tangent()'s bit at COMMANDER_FLAGS_SHIFT = 24 (a command applied at gimbal lock at
    some step) and com_reference_tangent()'s at LEAN_FLAGS_SHIFT = 25 ... 28.  K unit seeds on twist_tan give the Jacobian in the
    command.  One set of tangent buffers whatever `steps` is; a command SEQUENCE is an input of `steps` commands, and with it the
    planning grows with the horizon: one commander launch and one tangent launch are planned per step, and twist_tan is copied once into
    per-step [K,n,6] blocks.
    `params_tan` ([211] or [K, 211]): directions in the handle's parameters, held over the rollout, as rollout_tick_tangent() takes them."""
    import torch

    from .autograd import _COMMANDER_DESIRED_REFUSED

    who = "rollout_commander_tangent"
    _gait_rollout_refusals(who, batch, None)
    for name, why in _COMMANDER_DESIRED_REFUSED.items():
        if batch.get(name) is not None:
            raise ValueError(f"{who}: batch['{name}'] must be None - {why}")
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"{who}: steps must be >= 0")
    if command is None or command.get("state") is None:
        raise ValueError(f"{who}: command['state'] is required (new_commander_states)")
    unknown = [k for k in tangents if k not in ROLLOUT_COMMANDER_TANGENTS]
    if unknown:
        raise ValueError(f"{who}: unknown tangent(s) {unknown}; the tangents are {tuple(ROLLOUT_COMMANDER_TANGENTS)}")
    n, dev = batch["x"].shape[0], torch.device("cuda", ctl.device)
    # standing and gait_running are latched and never reset: read ONCE, here (the rollout's one host synchronisation)
    latched = command["state"].view(torch.int32).view(n, -1)[:, :2].ne(0).all(dim=0).tolist()
    if not all(latched):
        raise ValueError(f"{who}: every robot must have standing and gait_running set (not all have {'standing' if not latched[0] else 'gait_running'}): "
                         "until then the commander ignores the twist - the tangent is identically zero - and rollout_tick() runs the stand-up")
    twist, fresh = command.get("twist"), command.get("fresh")
    sequence = twist is not None and twist.dim() == 3
    if sequence and (twist.shape[0] != steps or (fresh is not None and (fresh.dim() != 2 or fresh.shape[0] != steps))):
        raise ValueError(f"{who}: a command sequence is twist [steps,n,6] with an optional fresh [steps,n]")
    if tangents.get("twist_tan") is not None and twist is None:
        raise ValueError(f"{who}: twist_tan needs command['twist']")
    lean, st = _lean_arguments(who, lean, "offset", tangents, n, dev)
    tw = _lead_tangent(who, "twist_tan", tangents.get("twist_tan"), (steps, n, 6) if sequence else (n, 6), n, dev)
    vb = _lead_tangent(who, "Vb_tan", tangents.get("Vb_tan"), (n, 6), n, dev)
    rest = {k: v for k, v in tangents.items() if k not in ("twist_tan", "Vb_tan", "schedule_tan")}
    lead = _agree(who, [tw, vb, st])
    if lead is None and params_tan is not None and not any(v is not None for v in rest.values()):
        lead = _param_directions(who, params_tan, dev)  # params_tan alone is a seed
    clock = _gait_clock(gait_dt, n, dev)

    def hook(ctl, who, batch, n, K, dev, buf, given, stream):
        return _CommanderHook(ctl, who, batch, n, K, dev, buf, given, stream, command, steps, None if tw is None else tw[0], None if vb is None else vb[0],
                              lean, None if st is None else st[0])

    return _tick_tangent_loop(ctl, who, batch, steps, dt, leg_inertia, rest, ROLLOUT_GAIT_TANGENTS, act_tol, warm, stream, True, clock, hook, lead, params_tan)

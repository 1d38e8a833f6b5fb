"""torch.autograd for control_batch(), the fused stance tick, plant_step(), leg_plant_step() and the two closed loops:
BalanceController.control_batch_autograd(), fused_tick_autograd(), plant_step_autograd(), rollout_autograd(), leg_plant_step_autograd()
and rollout_tick_autograd().

Forward is control_batch() itself; backward is the adjoint of the balance QP on the active face of the forces it returned
(qc_sensitivity_batch) and, where a rotation requires grad, the rotation cotangents behind it (qc_sensitivity_rot_batch), and where
the `params` leaf requires grad the parameter cotangents summed over the batch (qc_sensitivity_param_batch), all
on the current stream, without host synchronisation.  The gradient is the one on the active face: valid while the working set
holds; robots with bit 0 of the sensitivity flags have a one-sided derivative, robots with bit 1 NaN gradients.

fused_tick_autograd() is control_batch(want_torques=True) on joint_q: its backward puts the reverse pass of the clamped J^T torque map
in front of the same calls and that of the forward kinematics behind them (qc_sensitivity_kin_batch, twice).

plant_step_autograd() is OUT OF PLACE - plant_step() on clones of the state - and its backward is one qc_plant_step_adjoint_batch call
on the saved pre-step tensors; rollout_autograd() alternates the two and threads new tensors through.  leg_plant_step_autograd() and
rollout_tick_autograd() are the same pair around the tick: leg_plant_step() on clones, one qc_leg_plant_step_adjoint_batch call
backward, alternated with fused_tick_autograd().

tick_autograd() is control_batch(want_torques=True) with swing references (swing_pos, swing_vel): its backward is the fused stance
tick's, then the reverse pass of the swing legs' PD torques (qc_sensitivity_swing_batch) added in place; rollout_tick_autograd() uses
it for a batch that carries the references.

swing_reference_autograd() is swing_reference_batch() - the gait clock, the contact mask, the foothold planner and the sextic swing
trajectory, the front half of the tick - on a copy of the swing record, its backward one qc_swing_reference_adjoint_batch call;
rollout_gait_autograd() chains it with tick_autograd() and leg_plant_step_autograd() and threads the record through: the twin of
rollout_tick() on a batch with swing_state and a running clock.

support_polygon_autograd() is support_polygon_batch() - the desired COM x, y from the feet and the scheduled gait - its backward one
qc_support_polygon_adjoint_batch call, and for joint_q the kinematics half of qc_sensitivity_kin_batch behind it.
com_reference_autograd() is com_reference_batch() - the x_d of a step from that polygon - in the same way; rollout_gait_autograd() and
rollout_commander_autograd() call it per step when given `lean`, so that a rollout has a gradient in the schedule of the lean."""
from __future__ import annotations

import torch

from ._lib import PARAM_COUNT
from .balance_controller import _SENSITIVITY_OUTPUTS

# the inputs a gradient is produced for, in the order backward returns them, and the sensitivity output behind each
DIFFERENTIABLE = ("Rwb", "Rwb_d", "x", "xdot", "w", "x_d", "xdot_d", "w_d", "feet")
_ROTATIONS = ("Rwb", "Rwb_d")


class _ControlBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, act_tol, flags, control_kwargs, *tensors):
        *tensors, params = tensors  # (params is never read: the solve uses the handle's own parameters)
        out = ctl.control_batch(batch, **control_kwargs)
        grf_body, status = out["grf_body"], out["status"]
        ctx.ctl, ctx.act_tol, ctx.flags = ctl, act_tol, flags
        ctx.rest = {k: v for k, v in batch.items() if k not in DIFFERENTIABLE}
        ctx.present = tuple(t is not None for t in tensors)
        ctx.save_for_backward(grf_body, *[t for t in tensors if t is not None])
        ctx.mark_non_differentiable(status)
        return grf_body, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grf_bar, _status_bar):
        grf_body, *given = ctx.saved_tensors
        given = iter(given)
        inputs = {k: (next(given) if there else None) for k, there in zip(DIFFERENTIABLE, ctx.present)}
        batch = dict(ctx.rest, **{k: v for k, v in inputs.items() if v is not None})
        need = dict(zip(DIFFERENTIABLE, ctx.needs_input_grad[5:]))
        need_params = ctx.needs_input_grad[5 + len(DIFFERENTIABLE)]
        s, param_bar = _qp_backward(ctx.ctl, batch, grf_body, grf_bar.contiguous(), ctx.act_tol, ctx.flags, need, need_params)
        grads = [s[k + "_bar"].view_as(inputs[k]) if need[k] else None for k in DIFFERENTIABLE]
        return (None, None, None, None, None, *grads, param_bar)


def _qp_backward(ctl, batch, grf_body, grf_bar, act_tol, flags, need, need_params, feet_bar=False):
    """The reverse pass of the solve that control_batch_autograd() and fused_tick_autograd() share: sensitivity_batch() asked for the
    cotangents `need` (name -> bool over DIFFERENTIABLE) names - and feet_bar if `feet_bar` -, sensitivity_rotation_batch() behind it
    where a rotation is among them, sensitivity_params_batch() in sum-only mode if need_params.  Returns (the dict of cotangents,
    param_bar or None)."""
    rot = [k for k in _ROTATIONS if need.get(k)]
    want = [k + "_bar" for k in DIFFERENTIABLE[2:] if need.get(k)]
    if feet_bar and "feet_bar" not in want:
        want.append("feet_bar")
    if rot:
        want += [k for k in ("b_bar", "feet_bar") if k not in want]
    if need_params:
        want.append("adjoint")
    out = None
    if flags is not None:  # the caller's tensor receives the flags; the other outputs are allocated as sensitivity_batch would
        shape = lambda k: (grf_body.shape[0],) + _SENSITIVITY_OUTPUTS[k][0]
        out = {k: torch.zeros(shape(k), dtype=torch.float64, device=grf_body.device) for k in want}
        out["flags"] = flags
        want.append("flags")
    s = ctl.sensitivity_batch(batch, grf_body, grf_bar, want=tuple(want), act_tol=act_tol, out=out)
    if rot:
        s.update(ctl.sensitivity_rotation_batch(batch, grf_body, grf_bar, s["b_bar"], s["feet_bar"], want=tuple(k + "_bar" for k in rot)))
    param_bar = None
    if need_params:  # sum-only: no [n,211] rows are written
        param_bar = ctl.sensitivity_params_batch(batch, grf_body, grf_bar, s["adjoint"], want=("param_bar",), act_tol=act_tol)["param_bar"]
    return s, param_bar


def control_batch_autograd(ctl, batch, act_tol=1e-7, flags=None, params=None, **control_kwargs):
    """BalanceController.control_batch_autograd (see there): (grf_body, status) of control_batch(batch, **control_kwargs), with a
    grad_fn on grf_body whenever one of DIFFERENTIABLE in `batch`, or `params`, requires grad.  `params` ([211], PARAM_LAYOUT's order,
    ctl.parameter_tensor() makes it) is never read by forward - the handle's own parameters are used -; its gradient is
    sensitivity_params_batch()'s sum over the batch."""
    if params is not None and (params.dtype != torch.float64 or params.numel() != PARAM_COUNT or params.dim() != 1):
        raise ValueError(f"params: need a float64 [{PARAM_COUNT}] tensor (BalanceController.parameter_tensor() makes one)")
    jq = batch.get("joint_q")
    if jq is not None and jq.requires_grad:
        raise ValueError("control_batch_autograd: joint_q.requires_grad is not supported - differentiate with respect to `feet`, or chain the "
                         "leg Jacobian from sensitivity_batch()'s feet_bar")
    if flags is not None and (flags.dtype != torch.int32 or not flags.is_contiguous() or flags.numel() != batch["x"].shape[0]):
        raise ValueError("flags: need a contiguous int32 [n] tensor")
    tensors = [batch.get(k) for k in DIFFERENTIABLE]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    return _ControlBatch.apply(ctl, detached, float(act_tol), flags, control_kwargs, *tensors, params)


# ------------------------------------------------------------------ the fused stance tick: joint_q -> FK -> QP -> clamped J^T -> joint_tau
TICK_DIFFERENTIABLE = DIFFERENTIABLE[:-1] + ("joint_q",)
_TICK_REFUSED = {"feet": "a batch with `feet` is control_batch_autograd()'s", "swing_pos": "the swing legs' PD torques are out of scope",
                 "swing_state": "the swing legs' PD torques are out of scope", "gait_dt": "the gait clock writes gait_phase in place"}


def _stance_backward(ctl, batch, grf_body, status, tau_bar, grf_bar, act_tol, flags, need, need_params):
    """The reverse pass of the stance legs that fused_tick_autograd() and tick_autograd() share, for cotangents tau_bar and grf_bar of
    which at least one is there: the torque half of sensitivity_kinematics_batch(), _qp_backward(), the kinematics half.  Returns (the
    dict of cotangents, param_bar or None)."""
    grf_bar = None if grf_bar is None else grf_bar.contiguous()
    q_bar = None
    if tau_bar is not None:  # the torque half: the total cotangent on grf_body, and joint_q's through the torque map
        k = ctl.sensitivity_kinematics_batch(batch, grf_body, status, joint_tau_bar=tau_bar.contiguous(), grf_bar_in=grf_bar,
                                             want=("grf_bar", "joint_q_bar") if need["joint_q"] else ("grf_bar",))
        grf_bar, q_bar = k["grf_bar"].view_as(grf_body), k.get("joint_q_bar")
    s, param_bar = _qp_backward(ctl, batch, grf_body, grf_bar, act_tol, flags, need, need_params, feet_bar=need["joint_q"])
    if need["joint_q"]:  # the kinematics half, added in place
        out = None if q_bar is None else {"joint_q_bar": q_bar}
        s["joint_q_bar"] = ctl.sensitivity_kinematics_batch(batch, feet_bar=s["feet_bar"], joint_q_bar_in=q_bar, want=("joint_q_bar",), out=out)["joint_q_bar"]
    return s, param_bar


class _FusedTick(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, act_tol, flags, control_kwargs, *tensors):
        *tensors, params = tensors  # (params is never read: the solve uses the handle's own parameters)
        out = ctl.control_batch(batch, want_torques=True, **control_kwargs)
        joint_tau, grf_body, status = out["joint_tau"], out["grf_body"], out["status"]
        ctx.ctl, ctx.act_tol, ctx.flags = ctl, act_tol, flags
        ctx.rest = {k: v for k, v in batch.items() if k not in TICK_DIFFERENTIABLE}
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        ctx.save_for_backward(grf_body, status, *tensors)
        ctx.mark_non_differentiable(status)
        return joint_tau, grf_body, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, tau_bar, grf_bar, _status_bar):
        grf_body, status, *given = ctx.saved_tensors
        inputs = dict(zip(TICK_DIFFERENTIABLE, given))
        batch = dict(ctx.rest, **inputs)
        need = dict(zip(TICK_DIFFERENTIABLE, ctx.needs_input_grad[5:]))
        need_params = ctx.needs_input_grad[5 + len(TICK_DIFFERENTIABLE)]
        if tau_bar is None and grf_bar is None:  # no output reached the loss: every gradient is zero
            grads = [torch.zeros_like(inputs[k]) if need[k] else None for k in TICK_DIFFERENTIABLE]
            return (None, None, None, None, None, *grads, torch.zeros(PARAM_COUNT, dtype=torch.float64, device=grf_body.device) if need_params else None)
        s, param_bar = _stance_backward(ctx.ctl, batch, grf_body, status, tau_bar, grf_bar, ctx.act_tol, ctx.flags, need, need_params)
        grads = [s[k + "_bar"].view_as(inputs[k]) if need[k] else None for k in TICK_DIFFERENTIABLE]
        return (None, None, None, None, None, *grads, param_bar)


def fused_tick_autograd(ctl, batch, act_tol=1e-7, flags=None, params=None, **control_kwargs):
    """BalanceController.fused_tick_autograd (see there): (joint_tau, grf_body, status) of control_batch(batch, want_torques=True,
    **control_kwargs) for a batch with joint_q and no feet, differentiable in TICK_DIFFERENTIABLE and `params` through joint_tau,
    grf_body or both."""
    if params is not None and (params.dtype != torch.float64 or params.numel() != PARAM_COUNT or params.dim() != 1):
        raise ValueError(f"params: need a float64 [{PARAM_COUNT}] tensor (BalanceController.parameter_tensor() makes one)")
    for k, why in _TICK_REFUSED.items():
        if batch.get(k) is not None:
            raise ValueError(f"fused_tick_autograd: the batch carries {k} - {why}")
    missing = [k for k in TICK_DIFFERENTIABLE if batch.get(k) is None]
    if missing:
        raise ValueError(f"fused_tick_autograd: the batch lacks {missing} (the fused stance tick reads joint_q and the eight state arrays)")
    if flags is not None and (flags.dtype != torch.int32 or not flags.is_contiguous() or flags.numel() != batch["x"].shape[0]):
        raise ValueError("flags: need a contiguous int32 [n] tensor")
    tensors = [batch[k] for k in TICK_DIFFERENTIABLE]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    return _FusedTick.apply(ctl, detached, float(act_tol), flags, control_kwargs, *tensors, params)


# ------------------------------------------------------------------ the tick through a gait: the fused stance tick and the swing legs' PD torques
TICK_SWING_DIFFERENTIABLE = TICK_DIFFERENTIABLE + ("joint_qdot", "swing_pos", "swing_vel")
_TICK_SWING_REFUSED = {"feet": "a batch with `feet` is control_batch_autograd()'s", "swing_state": "the planner's references are out of scope",
                       "gait_dt": "the gait clock writes gait_phase in place"}
_SWING_IN_PLACE = ("joint_q", "Rwb", "x")  # the cotangents the swing kernel adds to in place, through its `_in` arrays
JOINT_GAIN_COUNT = 9  # kp, kd, kff of the joint controller


class _Tick(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, act_tol, flags, control_kwargs, *tensors):
        *tensors, params, joint_gains = tensors  # (neither is ever read: the tick uses the handle's own parameters and gains)
        out = ctl.control_batch(batch, want_torques=True, **control_kwargs)
        joint_tau, grf_body, status = out["joint_tau"], out["grf_body"], out["status"]
        ctx.ctl, ctx.act_tol, ctx.flags = ctl, act_tol, flags
        ctx.rest = {k: v for k, v in batch.items() if k not in TICK_SWING_DIFFERENTIABLE}
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        ctx.save_for_backward(grf_body, status, *tensors)
        ctx.mark_non_differentiable(status)
        return joint_tau, grf_body, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, tau_bar, grf_bar, _status_bar):
        grf_body, status, *given = ctx.saved_tensors
        names = TICK_SWING_DIFFERENTIABLE
        inputs = dict(zip(names, given))
        batch = dict(ctx.rest, **inputs)
        need = dict(zip(names, ctx.needs_input_grad[5:]))
        need_params, need_gains = ctx.needs_input_grad[5 + len(names):]
        dev = grf_body.device
        zeros = lambda m: torch.zeros(m, dtype=torch.float64, device=dev)
        if tau_bar is None and grf_bar is None:  # no output reached the loss: every gradient is zero
            grads = [torch.zeros_like(inputs[k]) if need[k] else None for k in names]
            return (None, None, None, None, None, *grads, zeros(PARAM_COUNT) if need_params else None, zeros(JOINT_GAIN_COUNT) if need_gains else None)
        ctl = ctx.ctl
        s, param_bar = _stance_backward(ctl, batch, grf_body, status, tau_bar, grf_bar, ctx.act_tol, ctx.flags, need, need_params)
        n = grf_body.shape[0]
        want = [k + "_bar" for k in ("swing_pos", "swing_vel", "joint_q", "joint_qdot", "Rwb", "x") if need[k]] + (["gain_bar"] if need_gains else [])
        if tau_bar is None:  # a loss on grf_body alone never reaches a swing leg's torque
            s.update({k: zeros((n, 4, 9) if k == "gain_bar" else (n, 12)) for k in want if k not in s})
        elif want:  # the swing legs last, added in place to what the stance chain left
            in_place = {k + "_bar": s[k + "_bar"] for k in _SWING_IN_PLACE if need[k]}
            out = dict(in_place, **{k: zeros((n, 4, 9) if k == "gain_bar" else (n, 4, 3)) for k in want if k not in in_place})
            s.update(ctl.sensitivity_swing_batch(batch, tau_bar.contiguous(), want=tuple(want), out=out,
                                                 **{k + "_in": t for k, t in in_place.items()}))
        grads = [s[k + "_bar"].view_as(inputs[k]) if need[k] else None for k in names]
        return (None, None, None, None, None, *grads, param_bar, s["gain_bar"].sum(dim=(0, 1)) if need_gains else None)


def tick_autograd(ctl, batch, act_tol=1e-7, flags=None, params=None, joint_gains=None, **control_kwargs):
    """BalanceController.tick_autograd (see there): (joint_tau, grf_body, status) of control_batch(batch, want_torques=True,
    **control_kwargs) for a batch with joint_q, joint_qdot, swing_pos, swing_vel and a contact mask, differentiable in
    TICK_SWING_DIFFERENTIABLE, `params` and `joint_gains`.  `joint_gains` ([9]: kp, kd, kff) is never read by forward - the handle's
    own gains are used -; its gradient is sensitivity_swing_batch()'s gain_bar summed over robots and legs."""
    if params is not None and (params.dtype != torch.float64 or params.numel() != PARAM_COUNT or params.dim() != 1):
        raise ValueError(f"params: need a float64 [{PARAM_COUNT}] tensor (BalanceController.parameter_tensor() makes one)")
    if joint_gains is not None and (joint_gains.dtype != torch.float64 or joint_gains.numel() != JOINT_GAIN_COUNT or joint_gains.dim() != 1):
        raise ValueError(f"joint_gains: need a float64 [{JOINT_GAIN_COUNT}] tensor (kp, kd, kff of the joint controller)")
    for k, why in _TICK_SWING_REFUSED.items():
        if batch.get(k) is not None:
            raise ValueError(f"tick_autograd: the batch carries {k} - {why}")
    missing = [k for k in TICK_SWING_DIFFERENTIABLE if batch.get(k) is None]
    if missing:
        raise ValueError(f"tick_autograd: the batch lacks {missing} (the tick with swing references reads joint_q, joint_qdot, swing_pos, "
                         "swing_vel and the eight state arrays)")
    if flags is not None and (flags.dtype != torch.int32 or not flags.is_contiguous() or flags.numel() != batch["x"].shape[0]):
        raise ValueError("flags: need a contiguous int32 [n] tensor")
    tensors = [batch[k] for k in TICK_SWING_DIFFERENTIABLE]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    return _Tick.apply(ctl, detached, float(act_tol), flags, control_kwargs, *tensors, params, joint_gains)


# the inputs of a plant step a gradient is produced for, in the order backward returns them; the step's outputs, in the order forward returns them
PLANT_DIFFERENTIABLE = ("Rwb", "x", "xdot", "w", "grf_body", "foot_world")
PLANT_OUTPUTS = ("Rwb", "x", "xdot", "w", "feet")
_PLANT_BAR = {"Rwb": "Rwb_bar", "x": "x_bar", "xdot": "xdot_bar", "w": "w_bar", "grf_body": "grf_bar", "foot_world": "foot_world_bar"}


class _PlantStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, dt, Rwb, x, xdot, w, grf_body, foot_world):
        new = {"Rwb": Rwb.clone(), "x": x.clone(), "xdot": xdot.clone(), "w": w.clone()}
        feet = torch.empty_like(foot_world)
        ctl.plant_step(new, grf_body, foot_world, dt, feet=feet)
        ctx.ctl, ctx.dt = ctl, dt
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        ctx.save_for_backward(Rwb, x, xdot, w, grf_body, foot_world)
        return new["Rwb"], new["x"], new["xdot"], new["w"], feet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *bars):
        Rwb, x, xdot, w, grf_body, foot_world = ctx.saved_tensors
        need = dict(zip(PLANT_DIFFERENTIABLE, ctx.needs_input_grad[2:]))
        want = tuple(_PLANT_BAR[k] for k in PLANT_DIFFERENTIABLE if need[k])
        cot = {k: b.contiguous() for k, b in zip(PLANT_OUTPUTS, bars) if b is not None}
        if not cot:  # no output reached the loss: every gradient is zero
            grads = [torch.zeros_like(t) if need[k] else None for k, t in zip(PLANT_DIFFERENTIABLE, ctx.saved_tensors)]
            return (None, None, *grads)
        s = ctx.ctl.plant_step_adjoint({"Rwb": Rwb, "x": x, "xdot": xdot, "w": w}, grf_body, foot_world, ctx.dt, cot, want=want)
        grads = [s[_PLANT_BAR[k]].view_as(t) if need[k] else None for k, t in zip(PLANT_DIFFERENTIABLE, ctx.saved_tensors)]
        return (None, None, *grads)


def plant_step_autograd(ctl, state, grf_body, foot_world, dt):
    """BalanceController.plant_step_autograd (see there): (Rwb', x', xdot', w', feet') of one plant step as NEW tensors, `state` left as
    it is, with a grad_fn whenever one of PLANT_DIFFERENTIABLE requires grad."""
    tensors = [state[k] for k in ("Rwb", "x", "xdot", "w")] + [grf_body, foot_world]
    return _PlantStep.apply(ctl, float(dt), *tensors)


def _step_outputs(n, dev, warm, active, torques):
    """The tensors a rollout step's solve writes into, this step's own: grf_body, status, joint_tau with `torques`, and with `warm` its
    working-set word - the next solve starts from it (detached: an int32), this one from `active`.  Returns (res, the solve's keyword
    arguments, the word the next step starts from)."""
    res = {"grf_body": torch.zeros((n, 12), dtype=torch.float64, device=dev), "status": torch.full((n,), -1, dtype=torch.int32, device=dev)}
    if torques:
        res["joint_tau"] = torch.zeros((n, 12), dtype=torch.float64, device=dev)
    kwargs = dict(out=res)
    if warm:
        res["active_set"] = torch.zeros((n,), dtype=torch.int32, device=dev)
        kwargs.update(warm=active, want_active_set=True)
        active = res["active_set"]
    return res, kwargs, active


def _refuse(who, batch, table):
    """ValueError for the first array of `table` (name -> why not) the batch carries"""
    for k, why in table.items():
        if batch.get(k) is not None:
            raise ValueError(f"{who}: the batch carries {k} - {why}")


def _require(who, batch, names):
    """ValueError naming the arrays of `names` the batch lacks"""
    missing = [k for k in names if batch.get(k) is None]
    if missing:
        raise ValueError(f"{who}: the batch lacks {missing}")


def rollout_autograd(ctl, batch, foot_world, steps, dt, act_tol=1e-7, warm=True, params=None):
    """BalanceController.rollout_autograd (see there): `steps` times control_batch_autograd() then plant_step_autograd(), out of place.
    The gradient is the one on the active face of every solve along the way; memory grows with `steps`.  `params` goes to every
    solve: its gradient is that of the controller's use of the parameters, the plant's use of mass and Ib held fixed."""
    if batch.get("joint_q") is not None or batch.get("feet") is None:
        raise ValueError("rollout: the plant is a single rigid body - the batch carries `feet`, not joint_q")
    steps = int(steps)
    if steps < 0:
        raise ValueError("rollout: steps must be >= 0")
    cur = dict(batch)
    out, active = {}, None
    for _ in range(steps):
        kwargs = {}
        if warm:
            _, kwargs, active = _step_outputs(cur["x"].shape[0], cur["x"].device, True, active, torques=False)
        grf, status = control_batch_autograd(ctl, cur, act_tol, params=params, **kwargs)
        Rwb, x, xdot, w, feet = plant_step_autograd(ctl, cur, grf, foot_world, dt)
        cur = dict(cur, Rwb=Rwb, x=x, xdot=xdot, w=w, feet=feet)
        out = {"grf_body": grf, "status": status}
    if warm and active is not None:
        out["active_set"] = active
    return {k: cur[k] for k in ("Rwb", "x", "xdot", "w", "feet")}, out


# ------------------------------------------------------------------ the legged plant and the closed loop around the tick
LEG_PLANT_DIFFERENTIABLE = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "joint_tau")  # also the step's outputs, less joint_tau


class _LegPlantStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, dt, leg_inertia, contact, flags, *tensors):
        *state, joint_tau = tensors
        new = {k: t.clone() for k, t in zip(LEG_PLANT_DIFFERENTIABLE, state)}
        ctl.leg_plant_step(new, joint_tau, dt, leg_inertia, flags=flags, **contact)
        ctx.ctl, ctx.dt, ctx.leg_inertia, ctx.contact = ctl, dt, leg_inertia, contact
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        ctx.save_for_backward(*tensors)
        return tuple(new[k] for k in LEG_PLANT_DIFFERENTIABLE[:-1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *bars):
        *state, joint_tau = ctx.saved_tensors
        need = dict(zip(LEG_PLANT_DIFFERENTIABLE, ctx.needs_input_grad[5:]))
        cot = {k: b.contiguous() for k, b in zip(LEG_PLANT_DIFFERENTIABLE, bars) if b is not None}
        if not cot:  # no output reached the loss: every gradient is zero
            grads = [torch.zeros_like(t) if need[k] else None for k, t in zip(LEG_PLANT_DIFFERENTIABLE, ctx.saved_tensors)]
            return (None, None, None, None, None, *grads)
        want = tuple(k + "_bar" for k in LEG_PLANT_DIFFERENTIABLE if need[k])
        s = ctx.ctl.leg_plant_step_adjoint(dict(zip(LEG_PLANT_DIFFERENTIABLE, state)), joint_tau, ctx.dt, ctx.leg_inertia, cot, want=want, **ctx.contact)
        grads = [s[k + "_bar"].view_as(t) if need[k] else None for k, t in zip(LEG_PLANT_DIFFERENTIABLE, ctx.saved_tensors)]
        return (None, None, None, None, None, *grads)


def leg_plant_step_autograd(ctl, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, flags=None):
    """BalanceController.leg_plant_step_autograd (see there): (Rwb', x', xdot', w', joint_q', joint_qdot') of one legged plant step as
    NEW tensors, `state` left as it is, with a grad_fn whenever one of LEG_PLANT_DIFFERENTIABLE requires grad."""
    contact = {k: (v.detach() if v is not None else None) for k, v in (("stance", stance), ("gait_phase", gait_phase), ("gait_duty", gait_duty))}
    tensors = [state[k] for k in LEG_PLANT_DIFFERENTIABLE[:-1]] + [joint_tau]
    return _LegPlantStep.apply(ctl, float(dt), leg_inertia, contact, flags, *tensors)


# ------------------------------------------------------------------ the swing references: clock, contact mask, foothold planner, sextic trajectory
SWING_REFERENCE_DIFFERENTIABLE = ("Rwb", "x", "xdot", "w", "xdot_d", "joint_q", "p_start", "p_final")
_SWING_RECORD_DOUBLES = 28  # qc_swing_state as doubles: 4 hold the eight int32 words, then p_start [12] and p_final [12]


def _record_points(record):
    """the p_start / p_final columns of a swing-state tensor, as float64 views [n,12] into it"""
    d = record.view(torch.float64).view(-1, _SWING_RECORD_DOUBLES)
    return d[:, 4:16], d[:, 16:28]


class _SwingReference(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, swing_state, *tensors):
        *state, p_start, p_final = tensors
        before = swing_state.clone()
        ps, pf = _record_points(before)
        ps.copy_(p_start.reshape(ps.shape))
        pf.copy_(p_final.reshape(pf.shape))
        after = before.clone()
        res = ctl.swing_reference_batch(dict(batch, swing_state=after), want=("swing_pos", "swing_vel", "planned"))
        ctx.ctl = ctl
        ctx.rest = {k: batch[k] for k in ("stance", "gait_duty") if batch.get(k) is not None}
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        # (the phases as the call left them: a copy, the caller's tensor advances again on the next tick)
        ctx.save_for_backward(before, batch["gait_phase"].clone(), *tensors)
        ps, pf = _record_points(after)
        ctx.mark_non_differentiable(after, res["planned"])
        return res["swing_pos"], res["swing_vel"], ps.clone(), pf.clone(), after, res["planned"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, pos_bar, vel_bar, ps_bar, pf_bar, _state_bar, _planned_bar):
        before, phase, *given = ctx.saved_tensors
        names = SWING_REFERENCE_DIFFERENTIABLE
        inputs = dict(zip(names, given))
        need = dict(zip(names, ctx.needs_input_grad[3:]))
        cot = {k: b.contiguous() for k, b in (("swing_pos", pos_bar), ("swing_vel", vel_bar), ("p_start", ps_bar), ("p_final", pf_bar)) if b is not None}
        want = tuple(k + "_bar" for k in names if need[k])
        if not cot or not want:  # no output reached the loss: every gradient is zero
            return (None, None, None, *[torch.zeros_like(inputs[k]) if need[k] else None for k in names])
        batch = dict(ctx.rest, gait_phase=phase, **{k: inputs[k] for k in names[:-2] if k != "xdot_d"})
        s = ctx.ctl.swing_reference_adjoint_batch(batch, before, cot, want=want)
        return (None, None, None, *[s[k + "_bar"].view_as(inputs[k]) if need[k] else None for k in names])


def swing_reference_autograd(ctl, batch, swing_state, p_start, p_final):
    """BalanceController.swing_reference_autograd (see there): (swing_pos, swing_vel, p_start', p_final', swing_state', planned) of
    swing_reference_batch() on a copy of `swing_state` whose end points are `p_start` / `p_final`, differentiable in
    SWING_REFERENCE_DIFFERENTIABLE."""
    for k in ("swing_pos", "swing_vel"):
        if batch.get(k) is not None:
            raise ValueError(f"swing_reference_autograd: the batch carries {k} - this call makes the references")
    _require("swing_reference_autograd", batch, SWING_REFERENCE_DIFFERENTIABLE[:-2] + ("gait_phase",))
    n = batch["x"].shape[0]
    for name, t in (("p_start", p_start), ("p_final", p_final)):
        if t is None or t.dtype != torch.float64 or t.numel() != 12 * n:
            raise ValueError(f"swing_reference_autograd: {name} is a float64 [n,12] tensor")
    tensors = [batch[k] for k in SWING_REFERENCE_DIFFERENTIABLE[:-2]] + [p_start, p_final]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != "swing_state"}
    return _SwingReference.apply(ctl, detached, swing_state.detach(), *tensors)


_ROLLOUT_GAIT_REFUSED = {"stance": "the gait clock makes the contact mask from gait_phase", "swing_pos": "the references are made per step",
                         "swing_vel": "the references are made per step", "gait_dt": "the clock's step is this call's gait_dt argument",
                         "feet": "the tick reads joint_q (rollout_autograd() steps the bare rigid body on `feet`)"}


_COMMANDER_DESIRED_REFUSED = {k: "in commander mode the desired state lives in command['state']" for k in ("Rwb_d", "x_d", "xdot_d", "w_d")}
_ROLLOUT_GAIT_NEEDED = ("joint_q", "joint_qdot", "gait_phase", "swing_state")


def _gait_clock(gait_dt, n, dev):
    """the clock's step of a gait rollout as a float64 [n] tensor"""
    if isinstance(gait_dt, torch.Tensor):
        return gait_dt.detach().to(dtype=torch.float64, device=dev).contiguous()
    return torch.full((n,), float(gait_dt), dtype=torch.float64, device=dev)


def _gait_step(ctl, cur, desired, phase, duty, clock, record, p_start, p_final, warm, active, flags, dt, leg_inertia, act_tol, params, joint_gains):
    """One step of the two gait rollouts behind whatever made `desired`, the desired-state arrays that take the place of the batch's own
    for this step: swing_reference_autograd() with the clock advancing, tick_autograd() on its references and phases,
    leg_plant_step_autograd() with those phases.  Returns (the next cur, the step's out, (phase, record, p_start, p_final, planned,
    active) as the next step takes them)."""
    n, dev = cur["x"].shape[0], cur["x"].device
    phase = phase.clone()  # this step's own phases: advanced in place by the references' clock, then read by the tick and the plant
    tracked = dict(cur, **desired)
    ref_in = dict({k: tracked[k] for k in SWING_REFERENCE_DIFFERENTIABLE[:-2]}, gait_phase=phase, gait_dt=clock)
    if duty is not None:
        ref_in["gait_duty"] = duty
    pos, vel, p_start, p_final, record, planned = swing_reference_autograd(ctl, ref_in, record, p_start, p_final)
    _, kwargs, active = _step_outputs(n, dev, warm, active, torques=True)
    tick_in = dict(tracked, gait_phase=phase, swing_pos=pos, swing_vel=vel)
    tau, grf, status = tick_autograd(ctl, tick_in, act_tol, params=params, joint_gains=joint_gains, **kwargs)
    new = leg_plant_step_autograd(ctl, cur, tau, dt, leg_inertia, gait_phase=phase, gait_duty=duty, flags=flags)
    out = {"joint_tau": tau, "grf_body": grf, "status": status, "flags": flags}
    return dict(cur, **dict(zip(LEG_PLANT_DIFFERENTIABLE[:-1], new))), out, (phase, record, p_start, p_final, planned, active)


def rollout_gait_autograd(ctl, batch, steps, dt, leg_inertia, gait_dt, act_tol=1e-7, warm=True, params=None, joint_gains=None, lean=None):
    """BalanceController.rollout_gait_autograd (see there): `steps` times swing_reference_autograd() with the clock advancing,
    tick_autograd() on its references and phases, leg_plant_step_autograd() with those phases; the swing record threaded through.
    With `lean`, com_reference_autograd() in front of each step makes the x_d its tick tracks."""
    lean = _lean("rollout_gait_autograd", lean, "replace")
    if lean is not None and batch.get("x_d") is None:
        raise ValueError("rollout_gait_autograd: lean needs batch['x_d'] (its z in replace mode, the base of the offset)")
    _refuse("rollout_gait_autograd", batch, _ROLLOUT_GAIT_REFUSED)
    _require("rollout_gait_autograd", batch, _ROLLOUT_GAIT_NEEDED)
    steps = int(steps)
    if steps < 0:
        raise ValueError("rollout_gait_autograd: steps must be >= 0")
    names = LEG_PLANT_DIFFERENTIABLE[:-1]
    n, dev = batch["x"].shape[0], batch["x"].device
    clock = _gait_clock(gait_dt, n, dev)
    cur = {k: v for k, v in batch.items() if k not in ("swing_state", "gait_phase")}
    duty = batch.get("gait_duty")
    record, phase = batch["swing_state"].detach(), batch["gait_phase"].detach()
    p_start, p_final = (t.clone() for t in _record_points(record))
    out, active, planned = {}, None, None
    flags = torch.zeros((n,), dtype=torch.int32, device=dev) if steps else None
    for _ in range(steps):
        desired = {} if lean is None else {"x_d": _lean_x_d(ctl, lean, cur, phase, duty, batch["x_d"])}
        cur, out, (phase, record, p_start, p_final, planned, active) = _gait_step(
            ctl, cur, desired, phase, duty, clock, record, p_start, p_final, warm, active, flags, dt, leg_inertia, act_tol, params, joint_gains)
    if warm and active is not None:
        out["active_set"] = active
    out.update(gait_phase=phase, swing_state=record, p_start=p_start, p_final=p_final)
    if planned is not None:
        out["planned"] = planned
    return {k: cur[k] for k in names}, out


# ------------------------------------------------------------------ commander mode: the commander step and a rollout with a gradient in the command
COMMANDER_STEP_DIFFERENTIABLE = ("Rwb", "x", "twist", "Vb", "Rwb_d", "x_d", "xdot_d", "w_d")
# the reverse pass's output for each of them, and the forward call's outputs a cotangent may arrive on
_COMMANDER_STEP_BARS = ("Rwb_bar", "x_bar", "twist_bar", "Vb_bar", "Rwb_d_prev_bar", "x_d_prev_bar", "xdot_d_prev_bar", "w_d_prev_bar")
_COMMANDER_RECORD_DOUBLES = 26  # qc_commander_state as doubles: 2 hold the four int32 words, then Vb [6], Rwb_d [9], x_d, xdot_d, w_d [3]
_COMMANDER_RECORD_COLUMNS = {"Vb": (2, 8), "Rwb_d": (8, 17), "x_d": (17, 20), "xdot_d": (20, 23), "w_d": (23, 26)}


def _commander_columns(record):
    """the Vb / Rwb_d / x_d / xdot_d / w_d columns of a commander-state tensor, as float64 views into it"""
    d = record.view(torch.float64).view(-1, _COMMANDER_RECORD_DOUBLES)
    return {k: d[:, a:b] for k, (a, b) in _COMMANDER_RECORD_COLUMNS.items()}


class _CommanderStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, command, state, *tensors):
        given = dict(zip(COMMANDER_STEP_DIFFERENTIABLE, tensors))
        before = state.clone()
        for k, col in _commander_columns(before).items():
            col.copy_(given[k].reshape(col.shape))
        after = before.clone()
        cmd = dict(command, state=after, twist=given["twist"])
        res = ctl.commander_step_batch({"Rwb": given["Rwb"], "x": given["x"]}, cmd, want=("Rwb_d", "x_d", "xdot_d", "w_d", "run", "applied"))
        ctx.ctl, ctx.command = ctl, command
        ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
        ctx.save_for_backward(before, *[t for t in tensors if t is not None])
        ctx.present = [t is not None for t in tensors]
        ctx.mark_non_differentiable(after, res["run"], res["applied"])
        return res["Rwb_d"], res["x_d"], res["xdot_d"], res["w_d"], _commander_columns(after)["Vb"].clone(), after, res["run"], res["applied"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, Rd_bar, xd_bar, xdd_bar, wd_bar, vb_bar, _state_bar, _run_bar, _applied_bar):
        before, *saved = ctx.saved_tensors
        names = COMMANDER_STEP_DIFFERENTIABLE
        saved = iter(saved)
        inputs = {k: (next(saved) if there else None) for k, there in zip(names, ctx.present)}
        need = dict(zip(names, ctx.needs_input_grad[3:]))
        cot = {k: b.contiguous() for k, b in (("Rwb_d", Rd_bar), ("x_d", xd_bar), ("xdot_d", xdd_bar), ("w_d", wd_bar), ("Vb", vb_bar)) if b is not None}
        want = tuple(bar for k, bar in zip(names, _COMMANDER_STEP_BARS) if need[k])
        if not cot or not want:  # no output reached the loss: every gradient is zero
            return (None, None, None, *[torch.zeros_like(inputs[k]) if need[k] else None for k in names])
        cmd = dict(ctx.command, twist=inputs["twist"])
        s = ctx.ctl.commander_step_adjoint_batch({"Rwb": inputs["Rwb"], "x": inputs["x"]}, cmd, before, cot, want=want)
        return (None, None, None, *[s[bar].view_as(inputs[k]) if need[k] else None for k, bar in zip(names, _COMMANDER_STEP_BARS)])


def commander_step_autograd(ctl, batch, command, desired, Vb):
    """BalanceController.commander_step_autograd (see there): (Rwb_d, x_d, xdot_d, w_d, Vb', state', run, applied) of
    commander_step_batch() on a copy of command["state"] whose held command is `Vb` and whose desired state is `desired`,
    differentiable in COMMANDER_STEP_DIFFERENTIABLE."""
    _require("commander_step_autograd", batch, ("Rwb", "x"))
    if command.get("state") is None:
        raise ValueError("commander_step_autograd: command['state'] is required (new_commander_states)")
    n = batch["x"].shape[0]
    if len(desired) != 4:
        raise ValueError("commander_step_autograd: desired is the tuple (Rwb_d, x_d, xdot_d, w_d)")
    for name, t, k in (("Vb", Vb, 6), ("Rwb_d", desired[0], 9), ("x_d", desired[1], 3), ("xdot_d", desired[2], 3), ("w_d", desired[3], 3)):
        if t is None or t.dtype != torch.float64 or t.numel() != k * n:
            raise ValueError(f"commander_step_autograd: {name} is a float64 [n,{k}] tensor")
    twist = command.get("twist")
    if twist is not None and not twist.is_contiguous():
        twist = twist.contiguous()
    rest = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in command.items() if k not in ("state", "twist")}
    return _CommanderStep.apply(ctl, rest, command["state"].detach(), batch["Rwb"], batch["x"], twist, Vb, *desired)


def rollout_commander_autograd(ctl, batch, command, steps, dt, leg_inertia, gait_dt, act_tol=1e-7, warm=True, params=None, joint_gains=None,
                               lean=None):
    """BalanceController.rollout_commander_autograd (see there): `steps` times commander_step_autograd(), swing_reference_autograd()
    with the commander's xdot_d and the clock advancing, tick_autograd() on the commander's desired state, leg_plant_step_autograd();
    the held command, the records' desired state and the swing record threaded through.  With `lean`, com_reference_autograd() leans
    the commander's x_d for the tick alone."""
    who = "rollout_commander_autograd"
    lean = _lean(who, lean, "offset")
    _refuse(who, batch, _ROLLOUT_GAIT_REFUSED)
    _refuse(who, batch, _COMMANDER_DESIRED_REFUSED)
    _require(who, batch, _ROLLOUT_GAIT_NEEDED)
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"{who}: steps must be >= 0")
    if command.get("state") is None:
        raise ValueError(f"{who}: command['state'] is required (new_commander_states)")
    names = LEG_PLANT_DIFFERENTIABLE[:-1]
    n, dev = batch["x"].shape[0], batch["x"].device
    cstate = command["state"].detach()
    # standing and gait_running are latched and never reset: read ONCE, here (the rollout's one host synchronisation)
    latched = cstate.view(torch.int32).view(n, -1)[:, :2].ne(0).all(dim=0).tolist()
    if not all(latched):
        raise ValueError(f"{who}: every robot must have standing and gait_running set (not all have {'standing' if not latched[0] else 'gait_running'}): "
                         "until then the commander ignores the twist - the gradient is identically zero - and rollout_tick() runs the stand-up")
    twist, fresh = command.get("twist"), command.get("fresh")
    sequence = twist is not None and twist.dim() == 3
    if sequence and (twist.shape[0] != steps or (fresh is not None and (fresh.dim() != 2 or fresh.shape[0] != steps))):
        raise ValueError(f"{who}: a command sequence is twist [steps,n,6] with an optional fresh [steps,n]")
    if sequence and fresh is None:
        fresh = torch.ones((steps, n), dtype=torch.uint8, device=dev)
    scalars = {k: command[k] for k in ("stand_height", "stand_tol", "cmd_dt") if command.get(k) is not None}
    clock = _gait_clock(gait_dt, n, dev)
    cur = {k: v for k, v in batch.items() if k not in ("swing_state", "gait_phase")}
    duty = batch.get("gait_duty")
    record, phase = batch["swing_state"].detach(), batch["gait_phase"].detach()
    p_start, p_final = (t.clone() for t in _record_points(record))
    held = {k: t.clone() for k, t in _commander_columns(cstate).items()}
    Vb, desired = held["Vb"], (held["Rwb_d"], held["x_d"], held["xdot_d"], held["w_d"])
    out, active, planned, applied = {}, None, None, None
    flags = torch.zeros((n,), dtype=torch.int32, device=dev) if steps else None
    for k in range(steps):
        if sequence:
            cmd = dict(scalars, state=cstate, twist=twist[k], fresh=fresh[k])
        elif k == 0 and fresh is not None:  # rollout_tick's rule: `fresh` holds on step 0 only
            cmd = dict(scalars, state=cstate, twist=twist, fresh=fresh)
        else:
            cmd = dict(scalars, state=cstate)
        *desired, Vb, cstate, _run, applied = commander_step_autograd(ctl, cur, cmd, desired, Vb)
        # (the leaned value goes to the tick only: `desired` keeps the un-leaned integral, the lean never feeds back into twist tracking)
        x_d = desired[1] if lean is None else _lean_x_d(ctl, lean, cur, phase, duty, desired[1])
        tracked = dict(Rwb_d=desired[0], x_d=x_d, xdot_d=desired[2], w_d=desired[3])
        cur, out, (phase, record, p_start, p_final, planned, active) = _gait_step(
            ctl, cur, tracked, phase, duty, clock, record, p_start, p_final, warm, active, flags, dt, leg_inertia, act_tol, params, joint_gains)
    if warm and active is not None:
        out["active_set"] = active
    out.update(gait_phase=phase, swing_state=record, p_start=p_start, p_final=p_final, cmd_state=cstate)
    if planned is not None:
        out.update(planned=planned, applied=applied)
    return {k: cur[k] for k in names}, out


_ROLLOUT_TICK_REFUSED = {"gait_dt": "the gait clock writes gait_phase in place; the contact mask is held over the rollout",
                         "swing_state": "the planner's references are out of scope (swing_pos and swing_vel are held over the rollout)",
                         "feet": "the tick reads joint_q (rollout_autograd() steps the bare rigid body on `feet`)"}


def rollout_tick_autograd(ctl, batch, steps, dt, leg_inertia, act_tol=1e-7, warm=True, params=None):
    """BalanceController.rollout_tick_autograd (see there): `steps` times fused_tick_autograd() - tick_autograd() for a batch with
    swing_pos and swing_vel, both held over the rollout - then leg_plant_step_autograd(), out of place.  The gradient is the one on the active face of every solve, at every tick's clamp mask and off the plant's flagged legs;
    memory grows with `steps`."""
    _refuse("rollout_tick_autograd", batch, _ROLLOUT_TICK_REFUSED)
    if batch.get("joint_q") is None or batch.get("joint_qdot") is None:
        raise ValueError("rollout_tick_autograd: the batch carries joint_q and joint_qdot (rollout_autograd() steps the bare rigid body)")
    swings = batch.get("swing_pos") is not None
    if swings != (batch.get("swing_vel") is not None):
        raise ValueError("rollout_tick_autograd: swing_pos and swing_vel go together")
    steps = int(steps)
    if steps < 0:
        raise ValueError("rollout_tick_autograd: steps must be >= 0")
    names = LEG_PLANT_DIFFERENTIABLE[:-1]
    cur = dict(batch)
    contact = {k: batch.get(k) for k in ("stance", "gait_phase", "gait_duty")}
    out, active = {}, None
    n, dev = batch["x"].shape[0], batch["x"].device
    flags = torch.zeros((n,), dtype=torch.int32, device=dev) if steps else None
    for _ in range(steps):
        # the tick, as rollout_tick(batch, None, ...) plans it: a control_batch() without swing references takes no joint_qdot
        _, kwargs, active = _step_outputs(n, dev, warm, active, torques=True)
        if swings:  # the swing legs' PD torques read joint_qdot and the held references
            tau, grf, status = tick_autograd(ctl, cur, act_tol, params=params, **kwargs)
        else:
            tick_in = {k: v for k, v in cur.items() if k != "joint_qdot"}
            tau, grf, status = fused_tick_autograd(ctl, tick_in, act_tol, params=params, **kwargs)
        new = leg_plant_step_autograd(ctl, cur, tau, dt, leg_inertia, flags=flags, **contact)
        cur = dict(cur, **dict(zip(names, new)))
        out = {"joint_tau": tau, "grf_body": grf, "status": status, "flags": flags}
    if warm and active is not None:
        out["active_set"] = active
    return {k: cur[k] for k in names}, out


# ------------------------------------------------------------------ the virtual support polygon: gait -> desired COM x, y
# the inputs a gradient is produced for, in the order backward returns them (the feet: `feet`, or joint_q through the kinematics adjoint)
SUPPORT_POLYGON_DIFFERENTIABLE = ("feet", "joint_q", "Rwb", "x", "gait_phase", "schedule")
_SUPPORT_POLYGON_BAR = {"feet": "feet_bar", "joint_q": "feet_bar", "Rwb": "Rwb_bar", "x": "x_bar", "gait_phase": "phase_bar", "schedule": "schedule_bar"}


def _polygon_backward(ctx, names, bar, lead, adjoint):
    """What _SupportPolygon.backward and _ComReference.backward share.  `names`: forward's tensor arguments; `bar`: name -> the reverse
    pass's output that is its gradient; `lead`: the number of non-tensor arguments in front of them; adjoint(batch, schedule, want):
    the reverse pass.  With joint_q a second launch carries feet_bar on; per-robot schedule_bar rows of a shared block are summed here."""
    given = iter(ctx.saved_tensors)
    inputs = {k: (next(given) if there else None) for k, there in zip(names, ctx.present)}
    need = dict(zip(names, ctx.needs_input_grad[lead:]))
    want = tuple(dict.fromkeys(bar[k] for k in names if need[k]))
    if not want:
        return (None,) * (lead + len(names))
    batch = dict(ctx.rest, **{k: v for k, v in inputs.items() if v is not None and k not in ("schedule", "x_d")})
    schedule = inputs["schedule"]
    s = adjoint(batch, schedule, want)
    grads = {k: s[bar[k]] for k in names if need[k] and k != "joint_q"}
    if need["joint_q"]:  # J(q)^T feet_bar, leg by leg: the kinematics half of the fused tick's reverse pass (unmasked: every leg)
        grads["joint_q"] = ctx.ctl.sensitivity_kinematics_batch({"joint_q": inputs["joint_q"]}, feet_bar=s["feet_bar"], want=("joint_q_bar",))["joint_q_bar"]
    if need["schedule"] and schedule.dim() == 2 and bar["schedule"] == "schedule_bar":  # a shared block: the sum over the robots
        grads["schedule"] = grads["schedule"].sum(0)
    return (*(None,) * lead, *[grads[k].view_as(inputs[k]) if need[k] else None for k in names])


def _polygon_tensors(batch, world):
    """Of the batch of the two polygon calls: the tensors a gradient is produced for, in SUPPORT_POLYGON_DIFFERENTIABLE's order less
    the schedule (None where the forward pass does not read one), and the batch detached - `feet` dropped where joint_q takes its place."""
    kin = batch.get("joint_q") is not None
    taken = {"feet": not kin, "joint_q": kin, "Rwb": bool(world), "x": bool(world), "gait_phase": True}
    tensors = [batch.get(k) if taken[k] else None for k in SUPPORT_POLYGON_DIFFERENTIABLE[:-1]]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != "feet" or not kin}
    return tensors, detached


class _SupportPolygon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, world, *tensors):
        schedule = tensors[-1]
        res = ctl.support_polygon_batch(batch, schedule, world=world, want=("com_xy",))
        ctx.ctl, ctx.world = ctl, world
        ctx.rest = {k: batch[k] for k in ("stance", "gait_duty") if batch.get(k) is not None}
        ctx.present = tuple(t is not None for t in tensors)
        ctx.save_for_backward(*[t for t in tensors if t is not None])
        return res["com_xy"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, com_bar):
        return _polygon_backward(ctx, SUPPORT_POLYGON_DIFFERENTIABLE, _SUPPORT_POLYGON_BAR, 3, lambda batch, schedule, want:
                                 ctx.ctl.support_polygon_adjoint_batch(batch, schedule, com_bar.contiguous(), world=ctx.world, want=want))


def support_polygon_autograd(ctl, batch, schedule, world=False):
    """BalanceController.support_polygon_autograd (see there): com_xy of support_polygon_batch(), differentiable in
    SUPPORT_POLYGON_DIFFERENTIABLE - `feet` where the batch has no joint_q, which the forward pass would read in its place."""
    if batch.get("gait_phase") is None or (batch.get("feet") is None and batch.get("joint_q") is None):
        raise ValueError("support_polygon_autograd: the batch lacks gait_phase, or both feet and joint_q")
    if world and (batch.get("Rwb") is None or batch.get("x") is None):
        raise ValueError("support_polygon_autograd: world=True needs Rwb and x")
    if schedule is None or schedule.dtype != torch.float64:
        raise ValueError("support_polygon_autograd: schedule is a float64 [n,4,4] or [4,4] tensor")
    tensors, detached = _polygon_tensors(batch, world)
    return _SupportPolygon.apply(ctl, detached, bool(world), *tensors, schedule)


# ------------------------------------------------------------------ the desired COM of a step from the polygon
COM_REFERENCE_DIFFERENTIABLE = ("x_d",) + SUPPORT_POLYGON_DIFFERENTIABLE
_COM_REFERENCE_BAR = dict(_SUPPORT_POLYGON_BAR, x_d="x_d_in_bar")


class _ComReference(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, mode, gain, *tensors):
        x_d, schedule = tensors[0], tensors[-1]
        res = ctl.com_reference_batch(batch, schedule, x_d.contiguous(), mode, gain)
        ctx.ctl, ctx.mode, ctx.gain = ctl, mode, gain
        ctx.rest = {k: batch[k] for k in ("stance", "gait_duty") if batch.get(k) is not None}
        ctx.present = tuple(t is not None for t in tensors)
        ctx.save_for_backward(*[t for t in tensors if t is not None])
        return res["x_d"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, x_d_bar):
        shared = ctx.saved_tensors[-1].dim() == 2  # a shared block: the kernel's sum
        bar = dict(_COM_REFERENCE_BAR, schedule="schedule_bar_sum" if shared else "schedule_bar")
        return _polygon_backward(ctx, COM_REFERENCE_DIFFERENTIABLE, bar, 4, lambda batch, schedule, want:
                                 ctx.ctl.com_reference_adjoint_batch(batch, schedule, x_d_bar.contiguous(), ctx.mode, ctx.gain, want=want))


def com_reference_autograd(ctl, batch, schedule, x_d, mode="replace", gain=1.0):
    """BalanceController.com_reference_autograd (see there): x_d of com_reference_batch(), differentiable in
    COM_REFERENCE_DIFFERENTIABLE - `feet` where the batch has no joint_q, which the forward pass would read in its place."""
    missing = [k for k in ("gait_phase", "Rwb", "x") if batch.get(k) is None]
    if missing or (batch.get("feet") is None and batch.get("joint_q") is None):
        raise ValueError(f"com_reference_autograd: the batch lacks {missing or 'both feet and joint_q'}")
    if schedule is None or schedule.dtype != torch.float64:
        raise ValueError("com_reference_autograd: schedule is a float64 [n,4,4] or [4,4] tensor")
    if x_d is None or x_d.dtype != torch.float64 or x_d.dim() != 2 or x_d.shape[1] != 3:
        raise ValueError("com_reference_autograd: x_d is a float64 [n,3] tensor")
    tensors, detached = _polygon_tensors(batch, True)
    return _ComReference.apply(ctl, detached, mode, float(gain), x_d, *tensors, schedule)


def _lean(who, lean, default_mode):
    """the `lean` keyword of the rollouts -> (schedule, mode, gain), or None"""
    if lean is None:
        return None
    unknown = [k for k in lean if k not in ("schedule", "mode", "gain")]
    if unknown or lean.get("schedule") is None:
        raise ValueError(f"{who}: lean is dict(schedule=..., mode=..., gain=...) with a schedule{f'; unknown {unknown}' if unknown else ''}")
    mode, gain = lean.get("mode"), lean.get("gain")
    return lean["schedule"], default_mode if mode is None else mode, 1.0 if gain is None else float(gain)


def _lean_x_d(ctl, lean, cur, phase, duty, x_d):
    """x_d of this step from the polygon: the state and the phases as the step finds them (before the clock advances), the phases detached"""
    b = dict({k: cur[k] for k in ("joint_q", "Rwb", "x")}, gait_phase=phase.detach())
    if duty is not None:
        b["gait_duty"] = duty
    return com_reference_autograd(ctl, b, lean[0], x_d, lean[1], lean[2])

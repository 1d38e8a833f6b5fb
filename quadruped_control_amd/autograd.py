"""torch.autograd for control_batch(): BalanceController.control_batch_autograd().

Forward is control_batch() itself; backward is the adjoint of the balance QP on the active face of the forces it returned
(qc_sensitivity_batch) and, where a rotation requires grad, the rotation cotangents behind it (qc_sensitivity_rot_batch), both
on the current stream, without host synchronisation.  The gradient is the one on the active face: valid while the working set
holds; robots with bit 0 of the sensitivity flags have a one-sided derivative, robots with bit 1 NaN gradients."""
from __future__ import annotations

import torch

from .balance_controller import _SENSITIVITY_OUTPUTS

# the inputs a gradient is produced for, in the order backward returns them, and the sensitivity output behind each
DIFFERENTIABLE = ("Rwb", "Rwb_d", "x", "xdot", "w", "x_d", "xdot_d", "w_d", "feet")
_ROTATIONS = ("Rwb", "Rwb_d")


class _ControlBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, batch, act_tol, flags, control_kwargs, *tensors):
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
        rot = [k for k in _ROTATIONS if need[k]]
        want = [k + "_bar" for k in DIFFERENTIABLE[2:] if need[k]]
        if rot:
            want += [k for k in ("b_bar", "feet_bar") if k not in want]
        out = None
        if ctx.flags is not None:  # the caller's tensor receives the flags; the other outputs are allocated as sensitivity_batch would
            shape = lambda k: (grf_body.shape[0],) + _SENSITIVITY_OUTPUTS[k][0]
            out = {k: torch.zeros(shape(k), dtype=torch.float64, device=grf_body.device) for k in want}
            out["flags"] = ctx.flags
            want.append("flags")
        grf_bar = grf_bar.contiguous()
        s = ctx.ctl.sensitivity_batch(batch, grf_body, grf_bar, want=tuple(want), act_tol=ctx.act_tol, out=out)
        if rot:
            s.update(ctx.ctl.sensitivity_rotation_batch(batch, grf_body, grf_bar, s["b_bar"], s["feet_bar"], want=tuple(k + "_bar" for k in rot)))
        grads = [s[k + "_bar"].view_as(inputs[k]) if need[k] else None for k in DIFFERENTIABLE]
        return (None, None, None, None, None, *grads)


def control_batch_autograd(ctl, batch, act_tol=1e-7, flags=None, **control_kwargs):
    """BalanceController.control_batch_autograd (see there): (grf_body, status) of control_batch(batch, **control_kwargs), with a
    grad_fn on grf_body whenever one of DIFFERENTIABLE in `batch` requires grad."""
    jq = batch.get("joint_q")
    if jq is not None and jq.requires_grad:
        raise ValueError("control_batch_autograd: joint_q.requires_grad is not supported - differentiate with respect to `feet`, or chain the "
                         "leg Jacobian from sensitivity_batch()'s feet_bar")
    if flags is not None and (flags.dtype != torch.int32 or not flags.is_contiguous() or flags.numel() != batch["x"].shape[0]):
        raise ValueError("flags: need a contiguous int32 [n] tensor")
    tensors = [batch.get(k) for k in DIFFERENTIABLE]
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    return _ControlBatch.apply(ctl, detached, float(act_tol), flags, control_kwargs, *tensors)

"""A plant of its own (include/qc_plant_model.h, csrc/qc_plant_model.hpp): the two plant steps with a PER-ROBOT body - mass [n],
Ib [n,9] - and an external wrench [n,6] at the centre of mass, the rigid-body step's reverse pass with the cotangents of all three, and
the rollouts built on them.  ctl.plant_step() and ctl.leg_plant_step() integrate the handle's mass and Ib - the numbers the QP itself
assumes - and nothing ever pushes them; with this module the plant can disagree with the controller's model (a payload, domain
randomisation), be pushed (a push schedule, one wrench per step), and be identified (a gradient in the plant's mass and inertia).

`model` is a dict with any of
  "mass"   [n]    float64, kg;
  "Ib"     [n,9]  float64, row-major body-frame inertia;
  "wrench" [n,6]  float64, force at the centre of mass then moment about it, world frame, held over the step - in rollout() and
                  rollout_tick() also [steps,n,6], one slice per step, read in place;
  "flags"  [n]    int32, OUT: bit 0 - mass not finite or <= 0, bit 1 - Ib refused (not finite, Sylvester's minors not all positive, or
                  asymmetric beyond 1e-12 max|Ib|).  A flagged robot's state comes out NaN; the rollouts OR the bits over the steps.
At least one of mass, Ib, wrench must be there: a model that changes nothing is the base call's, and the library says so.

The functions take the controller as their first argument, as tangent.py's do.  The symbols of the library are bound here, on the CDLL
that _lib.load() returns, with this module's own ctypes records: _lib.EXPORTS, BalanceController and autograd.py are not touched.

Not covered (the header's list): the leg plant's adjoint with a model, forward-mode twins, a model inside the tick or the solve,
per-robot g / dt / leg_inertia, a wrench at a body point, batch-summed mass_bar / Ib_bar, any contact model."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .balance_controller import _PLANT_ADJOINT_OUTPUTS, _PLANT_COTANGENTS, BalanceController, _check_tensor, _known_cotangents, _launched, _outputs

MODEL_KEYS = ("mass", "Ib", "wrench", "flags")
_MODEL_BAR_OUTPUTS = {"wrench_bar": ((6,), "float64"), "mass_bar": ((), "float64"), "Ib_bar": ((9,), "float64")}
PLANT_MODEL_ADJOINT_WANT = tuple(_PLANT_ADJOINT_OUTPUTS) + tuple(_MODEL_BAR_OUTPUTS)
FLAG_BAD_MASS, FLAG_BAD_IB = 1, 2


class QcPlantModel(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in ("mass", "Ib", "wrench_world", "flags")]


class QcPlantModelBar(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(k, C.c_void_p) for k in ("wrench_bar", "mass_bar", "Ib_bar", "flags")]


_bound = None


def _library():
    """the library with this module's symbols bound"""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name in ("qc_default_plant_model", "qc_default_plant_model_bar", "qc_plant_step_model_batch", "qc_leg_plant_step_model_batch",
                     "qc_plant_step_model_adjoint_batch"):
            if not hasattr(lib, name):
                raise ImportError(f"{_lib.LIB_PATH} does not export {name}")
        lib.qc_default_plant_model.argtypes = [C.POINTER(QcPlantModel)]
        lib.qc_default_plant_model.restype = None
        lib.qc_default_plant_model_bar.argtypes = [C.POINTER(QcPlantModelBar)]
        lib.qc_default_plant_model_bar.restype = None
        lib.qc_plant_step_model_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcPlantIo), C.POINTER(QcPlantModel), C.c_void_p]
        lib.qc_plant_step_model_batch.restype = C.c_int
        lib.qc_leg_plant_step_model_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcLegPlantIo), C.POINTER(QcPlantModel), C.c_void_p]
        lib.qc_leg_plant_step_model_batch.restype = C.c_int
        lib.qc_plant_step_model_adjoint_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcPlantAdjointIo), C.POINTER(QcPlantModel),
                                                          C.POINTER(QcPlantModelBar), C.c_void_p]
        lib.qc_plant_step_model_adjoint_batch.restype = C.c_int
        _bound = lib
    return _bound


def _marshal_model(ctl, model, n, steps=None):
    """`model` validated and packed: returns (record, wrench tensor or None, scheduled).  `steps`: a rollout's, where the wrench may
    also be [steps,n,6] (scheduled: the record then points at slice 0 and the caller moves it)."""
    import torch

    lib = _library()
    dev = torch.device("cuda", ctl.device)
    if not isinstance(model, dict):
        raise ValueError(f"model: need a dict with any of {MODEL_KEYS}")
    unknown = [k for k in model if k not in MODEL_KEYS]
    if unknown:
        raise ValueError(f"model: unknown key(s) {unknown}; the keys are {MODEL_KEYS}")
    rec = QcPlantModel()
    lib.qc_default_plant_model(C.byref(rec))
    if _check_tensor("model['mass']", model.get("mass"), n, None, torch.float64, dev, False, "float64"):
        rec.mass = model["mass"].data_ptr() if n else None
    if _check_tensor("model['Ib']", model.get("Ib"), n, 9, torch.float64, dev, False, "float64"):
        rec.Ib = model["Ib"].data_ptr() if n else None
    if _check_tensor("model['flags']", model.get("flags"), n, None, torch.int32, dev, False, "int32"):
        rec.flags = model["flags"].data_ptr() if n else None
    wrench, scheduled = model.get("wrench"), False
    if wrench is not None:
        scheduled = steps is not None and wrench.dim() == 3
        if scheduled and wrench.shape[0] != steps:
            raise ValueError(f"model['wrench']: a schedule has one [n,6] slice per step - need [{steps},{n},6], got {tuple(wrench.shape)}")
        _check_tensor("model['wrench']", wrench, n * (steps if scheduled else 1), 6, torch.float64, dev, True,
                      msg=f"model['wrench']: need contiguous float64 [{n},6]" + (f" or [{steps},{n},6]" if steps is not None else "") + f" on {dev}")
        rec.wrench_world = wrench.data_ptr() if wrench.numel() else None
    return rec, wrench, scheduled


def plan_plant_step(ctl, state, grf_body, foot_world, dt, model, feet=None, stream=None):
    """plant_step() marshalled once: returns `launch`, one qc_plant_step_model_batch call on tensors that are updated in place.  A call
    the library refuses raises ValueError with its message, from launch()."""
    n, io = ctl._marshal_plant(state, grf_body, foot_world, dt, feet)
    rec, _, _ = _marshal_model(ctl, model, n)
    return ctl._launcher("qc_plant_step_model_batch", (n, C.byref(io), C.byref(rec), ctl._stream_ptr(stream)),
                         (state, grf_body, foot_world, feet, model, io, rec), ValueError)


def plant_step(ctl, state, grf_body, foot_world, dt, model, feet=None, stream=None):
    """ctl.plant_step() on the model's body (module docstring): the same arguments and contracts - `state` updated IN PLACE, `feet` an
    optional output, asynchronous on `stream` - with the robot's own mass and Ib in the step and the wrench added to the legs' net force
    and moment.  A wrench of +0.0 alone gives ctl.plant_step()'s result bit for bit.  Returns `state`."""
    plan_plant_step(ctl, state, grf_body, foot_world, dt, model, feet, stream)()
    return state


def plan_leg_plant_step(ctl, state, joint_tau, dt, leg_inertia, model, stance=None, gait_phase=None, gait_duty=None, cmd_state=None, foot_world=None,
                        flags=None, stream=None):
    """leg_plant_step() marshalled once: returns `launch`, one qc_leg_plant_step_model_batch call on tensors that are updated in place."""
    n, io = ctl._marshal_leg_plant(state, joint_tau, dt, leg_inertia, stance, gait_phase, gait_duty, cmd_state, foot_world, flags)
    rec, _, _ = _marshal_model(ctl, model, n)
    keep = (state, joint_tau, stance, gait_phase, gait_duty, cmd_state, foot_world, flags, model, io, rec)
    return ctl._launcher("qc_leg_plant_step_model_batch", (n, C.byref(io), C.byref(rec), ctl._stream_ptr(stream)), keep, ValueError)


def leg_plant_step(ctl, state, joint_tau, dt, leg_inertia, model, stance=None, gait_phase=None, gait_duty=None, cmd_state=None, foot_world=None,
                   flags=None, stream=None):
    """ctl.leg_plant_step() on the model's body: the same arguments and contracts; `flags` is the leg plant's own word (singular
    Jacobian, foot out of reach), the model's bits go to model["flags"].  Returns `state`."""
    plan_leg_plant_step(ctl, state, joint_tau, dt, leg_inertia, model, stance, gait_phase, gait_duty, cmd_state, foot_world, flags, stream)()
    return state


def plan_plant_step_adjoint(ctl, state, grf_body, foot_world, dt, model, cotangents, want=PLANT_MODEL_ADJOINT_WANT, out=None, stream=None):
    """plant_step_adjoint() marshalled once: returns (launch, out), `launch()` being one qc_plant_step_model_adjoint_batch call."""
    import torch

    lib = _library()
    io = _lib.QcPlantAdjointIo()
    ctl._lib.qc_default_plant_adjoint(C.byref(io))
    n, dev = ctl._plant_arrays(io, state, grf_body, foot_world)
    _known_cotangents("plant_step_adjoint", cotangents, _PLANT_COTANGENTS, "step")
    for name, t in cotangents.items():
        if _check_tensor(f"cotangents['{name}']", t, n, int(np.prod(_PLANT_COTANGENTS[name][0])), torch.float64, dev, False, "float64"):
            setattr(io, name + "_next_bar", t.data_ptr())
    unknown = [w for w in want if w not in PLANT_MODEL_ADJOINT_WANT and w != "flags"]
    if unknown:
        raise ValueError(f"plant_step_adjoint: unknown output(s) {unknown}; want is a subset of {PLANT_MODEL_ADJOINT_WANT + ('flags',)}")
    res = _outputs("plant_step_adjoint", _PLANT_ADJOINT_OUTPUTS, tuple(w for w in want if w in _PLANT_ADJOINT_OUTPUTS), out, n, dev, io)
    io.dt = float(dt)
    rec, _, _ = _marshal_model(ctl, {k: v for k, v in model.items() if k != "flags"}, n)
    theirs = tuple(w for w in want if w in _MODEL_BAR_OUTPUTS)
    bar = None
    if theirs or "flags" in want:
        bar = QcPlantModelBar()
        lib.qc_default_plant_model_bar(C.byref(bar))
        res.update(_outputs("plant_step_adjoint", _MODEL_BAR_OUTPUTS, theirs, out, n, dev, bar, [("flags", (n,), "int32")] if "flags" in want else []))
    args = (n, C.byref(io), C.byref(rec), C.byref(bar) if bar is not None else None, ctl._stream_ptr(stream))
    return ctl._launcher("qc_plant_step_model_adjoint_batch", args, (state, grf_body, foot_world, model, cotangents, res, io, rec, bar), ValueError), res


def plant_step_adjoint(ctl, state, grf_body, foot_world, dt, model, cotangents, want=PLANT_MODEL_ADJOINT_WANT, out=None, stream=None):
    """The reverse pass of plant_step() (qc_plant_step_model_adjoint_batch): ctl.plant_step_adjoint()'s arguments and its six outputs, on
    the model's step, and any of "wrench_bar" [n,6] (the cotangents of the net force and moment), "mass_bar" [n] and "Ib_bar" [n,9]
    (ENTRYWISE, unsymmetrised: PARAM_LAYOUT's convention for Ib), and "flags" [n] int32 (the forward call's bits, recomputed).  mass_bar
    and Ib_bar are produced whether the model or the handle supplies the quantity; for the handle's they are per-robot rows, to be
    summed by the caller.  Outputs are written, not accumulated; a flagged robot's rows are NaN.  Returns the dict of device tensors."""
    return _launched(plan_plant_step_adjoint(ctl, state, grf_body, foot_world, dt, model, cotangents, want, out, stream))


# ------------------------------------------------------------------ the rollouts
class _ModelSteps:
    """The controller as rollout() and rollout_tick() see it, with the plant's plan replaced: every attribute is the controller's own,
    plan_plant() and plan_leg_plant() return the model's step.  The twins below run BalanceController.rollout / rollout_tick - their own
    text - on it, so record_every, certify_every and lean behave as the originals'.  Each step's launch moves the record to the wrench
    slice of its step (a schedule) and ORs the model's flags of the step into the rollout's word.

    What this relies on of the two rollouts (the comments at their step loops say so too), and what happens when one of them stops
    doing it - a RuntimeError, never a silently misindexed push schedule: they plan the plant step exactly ONCE (a second plan is
    refused), they call the returned launch once per step in step order and never otherwise (a launch beyond `steps` is refused, and
    finish() refuses a rollout that made fewer), and they set no attribute on `self` (refused)."""

    def __init__(self, ctl, model, steps, stream):
        object.__setattr__(self, "_own", dict(ctl=ctl, model=model, steps=steps, stream=stream, flags=None, launched=None))

    def __getattr__(self, name):
        own = object.__getattribute__(self, "_own")
        if name in ("_ctl", "_model", "_steps", "_stream"):
            return own[name[1:]]
        return getattr(own["ctl"], name)

    def __setattr__(self, name, value):
        raise RuntimeError(f"plant_model: the rollout set `{name}` on its controller - the twins run it on a stand-in that forwards reads only")

    def finish(self):
        """after the rollout: the model's flags; refuses a rollout that did not plan the step once and launch it `steps` times"""
        own = object.__getattribute__(self, "_own")
        if own["launched"] is None or own["launched"][0] != own["steps"]:
            raise RuntimeError(f"plant_model: the rollout launched the plant step {None if own['launched'] is None else own['launched'][0]} times in "
                               f"{own['steps']} steps - the push schedule and the flags are indexed by that count")
        return own["flags"]

    def _wrap(self, n, plan):
        import torch

        own = object.__getattribute__(self, "_own")
        if own["launched"] is not None:
            raise RuntimeError("plant_model: the rollout planned the plant step a second time - the twins count the launches of ONE plan")
        dev = torch.device("cuda", self._ctl.device)
        stream, steps = self._stream, self._steps
        on_stream = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        total = self._model.get("flags")
        _check_tensor("model['flags']", total, n, None, torch.int32, dev, False, "int32")
        with on_stream():  # (the buffers are zeroed on the stream the kernels and the OR run on)
            flags = total if total is not None else torch.empty((n,), dtype=torch.int32, device=dev)
            flags.zero_()
            step_flags = torch.zeros((n,), dtype=torch.int32, device=dev)
        rec, wrench, scheduled = _marshal_model(self._ctl, dict(self._model, flags=step_flags), n, steps)
        launch = plan(rec)
        base, stride, k = rec.wrench_world, n * 6 * 8, [0]
        own["flags"], own["launched"] = flags, k

        def step(_keep=(self._model, wrench, step_flags, rec)):
            if k[0] >= steps:
                raise RuntimeError(f"plant_model: the rollout launched the plant step more than once per step ({steps} steps)")
            if scheduled and base is not None:  # (None: a schedule of no robots)
                rec.wrench_world = base + k[0] * stride
            k[0] += 1
            launch()
            with on_stream():
                flags.bitwise_or_(step_flags)

        return step

    def plan_plant(self, state, grf_body, foot_world, dt, feet=None, stream=None):
        ctl = self._ctl
        n, io = ctl._marshal_plant(state, grf_body, foot_world, dt, feet)
        return self._wrap(n, lambda rec: ctl._launcher("qc_plant_step_model_batch", (n, C.byref(io), C.byref(rec), ctl._stream_ptr(stream)),
                                                       (state, grf_body, foot_world, feet, io, rec), ValueError))

    def plan_leg_plant(self, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, cmd_state=None, foot_world=None,
                       flags=None, stream=None):
        ctl = self._ctl
        n, io = ctl._marshal_leg_plant(state, joint_tau, dt, leg_inertia, stance, gait_phase, gait_duty, cmd_state, foot_world, flags)
        keep = (state, joint_tau, stance, gait_phase, gait_duty, cmd_state, foot_world, flags, io)
        return self._wrap(n, lambda rec: ctl._launcher("qc_leg_plant_step_model_batch", (n, C.byref(io), C.byref(rec), ctl._stream_ptr(stream)),
                                                       keep + (rec,), ValueError))


def rollout(ctl, batch, foot_world, steps, dt, model, warm=True, record_every=None, stream=None, certify_every=None):
    """The twin of ctl.rollout() on the model's plant: `steps` times control_batch() - the QP keeps the handle's mass and Ib - then
    plant_step() with `model`.  model["wrench"] is [n,6], held over the rollout, or [steps,n,6], one slice per step read in place: the
    push schedule.  Everything else - in-place state, warm, record_every, certify_every, the returned (state, out) - is ctl.rollout()'s;
    out["model_flags"] [n] int32 is the model's flags OR-ed over the steps (model["flags"] itself if given).  With a +0.0 wrench and
    neither mass nor Ib the states equal ctl.rollout()'s bit for bit."""
    _library()
    proxy = _ModelSteps(ctl, model, int(steps), stream)
    state, out = BalanceController.rollout(proxy, batch, foot_world, steps, dt, warm=warm, record_every=record_every, stream=stream, certify_every=certify_every)
    out["model_flags"] = proxy.finish()
    return state, out


def rollout_tick(ctl, batch, command, steps, dt, leg_inertia, model, warm=True, record_every=None, stream=None, certify_every=None, lean=None):
    """The twin of ctl.rollout_tick() on the model's legged plant, in the same way: the tick keeps the handle's model, leg_plant_step()
    integrates `model`; model["wrench"] [n,6] or [steps,n,6]; out["model_flags"] next to the leg plant's own out["flags"]."""
    _library()
    proxy = _ModelSteps(ctl, model, int(steps), stream)
    state, out = BalanceController.rollout_tick(proxy, batch, command, steps, dt, leg_inertia, warm=warm, record_every=record_every, stream=stream,
                                                certify_every=certify_every, lean=lean)
    out["model_flags"] = proxy.finish()
    return state, out


# ------------------------------------------------------------------ torch.autograd
PLANT_DIFFERENTIABLE = ("Rwb", "x", "xdot", "w", "grf_body", "foot_world", "wrench", "mass", "Ib")
PLANT_OUTPUTS = ("Rwb", "x", "xdot", "w", "feet")
_PLANT_BAR = {"Rwb": "Rwb_bar", "x": "x_bar", "xdot": "xdot_bar", "w": "w_bar", "grf_body": "grf_bar", "foot_world": "foot_world_bar",
              "wrench": "wrench_bar", "mass": "mass_bar", "Ib": "Ib_bar"}
_autograd_function = None


def _plant_step_function():
    """the torch.autograd.Function of plant_step_autograd(), made on first use (torch is imported lazily, as everywhere in the package)"""
    global _autograd_function
    if _autograd_function is not None:
        return _autograd_function
    import torch

    class _PlantStepModel(torch.autograd.Function):
        @staticmethod
        def forward(ctx, ctl, dt, flags, *tensors):
            Rwb, x, xdot, w, grf_body, foot_world, wrench, mass, Ib = tensors
            new = {"Rwb": Rwb.clone(), "x": x.clone(), "xdot": xdot.clone(), "w": w.clone()}
            feet = torch.empty_like(foot_world)
            model = {k: v for k, v in (("wrench", wrench), ("mass", mass), ("Ib", Ib), ("flags", flags)) if v is not None}
            plant_step(ctl, new, grf_body, foot_world, dt, model, feet=feet)
            ctx.ctl, ctx.dt = ctl, dt
            ctx.present = tuple(t is not None for t in tensors)
            ctx.set_materialize_grads(False)  # an output the loss never reached arrives as None: a NULL cotangent, not an array of zeros
            ctx.save_for_backward(*[t for t in tensors if t is not None])
            return new["Rwb"], new["x"], new["xdot"], new["w"], feet

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, *bars):
            saved = iter(ctx.saved_tensors)
            inputs = {k: (next(saved) if there else None) for k, there in zip(PLANT_DIFFERENTIABLE, ctx.present)}
            need = dict(zip(PLANT_DIFFERENTIABLE, ctx.needs_input_grad[3:]))
            cot = {k: b.contiguous() for k, b in zip(PLANT_OUTPUTS, bars) if b is not None}
            if not cot:  # no output reached the loss: every gradient is zero
                return (None, None, None, *[torch.zeros_like(inputs[k]) if need[k] else None for k in PLANT_DIFFERENTIABLE])
            model = {k: inputs[k] for k in ("wrench", "mass", "Ib") if inputs[k] is not None}
            s = plant_step_adjoint(ctx.ctl, {k: inputs[k] for k in ("Rwb", "x", "xdot", "w")}, inputs["grf_body"], inputs["foot_world"], ctx.dt, model, cot,
                                   want=tuple(_PLANT_BAR[k] for k in PLANT_DIFFERENTIABLE if need[k]))
            return (None, None, None, *[s[_PLANT_BAR[k]].view_as(inputs[k]) if need[k] else None for k in PLANT_DIFFERENTIABLE])

    _autograd_function = _PlantStepModel
    return _autograd_function


def plant_step_autograd(ctl, state, grf_body, foot_world, dt, model):
    """plant_step() with a gradient, OUT OF PLACE: returns (Rwb', x', xdot', w', feet') as new tensors and leaves `state` as it is.  The
    gradient covers ctl.plant_step_autograd()'s six inputs AND model["wrench"], model["mass"] and model["Ib"] (entrywise), each where it
    requires grad; backward is one plant_step_adjoint() call on the saved pre-step tensors, on the current stream, without host
    synchronisation.  model["flags"], if given, receives the forward call's bits.  No double backward, no gradient in dt."""
    _marshal_model(ctl, model, state["x"].shape[0])  # (refuses unknown keys and wrong tensors before anything is cloned)
    detach = lambda t: None if t is None else t.detach()
    tensors = [state[k] for k in ("Rwb", "x", "xdot", "w")] + [grf_body, foot_world] + [model.get(k) for k in ("wrench", "mass", "Ib")]
    return _plant_step_function().apply(ctl, float(dt), detach(model.get("flags")), *tensors)


def rollout_autograd(ctl, batch, foot_world, steps, dt, model, act_tol=1e-7, warm=True, params=None):
    """The functional twin of rollout(): `steps` times ctl.control_batch_autograd() then plant_step_autograd() with `model`, new tensors
    threaded through - `batch` is not modified.  model["wrench"] is [n,6], held, or [steps,n,6], step k reading slice k: a loss on the state
    after the rollout has a gradient in the plant's mass and Ib and in every step's push, besides everything ctl.rollout_autograd()
    differentiates.  `params` goes to every solve, as there: params.grad is the gradient in the CONTROLLER's own parameters - its mass
    and Ib among them -, separate from the plant's model["mass"].grad and model["Ib"].grad.  The gradient is the one on the active
    face of every solve (ctl.rollout_autograd()'s caveats); memory grows with `steps`.  model["flags"], if given, receives the bits
    OR-ed over the steps.  Returns (state, out) as ctl.rollout_autograd() does."""
    import torch

    if batch.get("joint_q") is not None or batch.get("feet") is None:
        raise ValueError("rollout: the plant is a single rigid body - the batch carries `feet`, not joint_q")
    steps = int(steps)
    if steps < 0:
        raise ValueError("rollout: steps must be >= 0")
    n, dev = batch["x"].shape[0], batch["x"].device
    _, wrench, scheduled = _marshal_model(ctl, model, n, steps)
    total = model.get("flags")
    step_flags = None if total is None else torch.zeros_like(total)
    if total is not None:
        total.zero_()  # (on the current stream, where every launch of this function runs: it takes no `stream`)
    cur = dict(batch)
    out, active = {}, None
    for k in range(steps):
        kwargs = {}
        if warm:
            res = {"grf_body": torch.zeros((n, 12), dtype=torch.float64, device=dev), "status": torch.full((n,), -1, dtype=torch.int32, device=dev),
                   "active_set": torch.zeros((n,), dtype=torch.int32, device=dev)}
            kwargs = dict(out=res, warm=active, want_active_set=True)
            active = res["active_set"]
        grf, status = ctl.control_batch_autograd(cur, act_tol, params=params, **kwargs)
        m = {key: v for key, v in model.items() if key != "flags"}
        if scheduled:
            m["wrench"] = wrench[k]
        if step_flags is not None:
            m["flags"] = step_flags
        Rwb, x, xdot, w, feet = plant_step_autograd(ctl, cur, grf, foot_world, dt, m)
        if step_flags is not None:
            total.bitwise_or_(step_flags)
        cur = dict(cur, Rwb=Rwb, x=x, xdot=xdot, w=w, feet=feet)
        out = {"grf_body": grf, "status": status}
    if warm and active is not None:
        out["active_set"] = active
    return {k: cur[k] for k in ("Rwb", "x", "xdot", "w", "feet")}, out

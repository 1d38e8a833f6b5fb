"""GPU: qc_leg_plant_step_adjoint_batch (csrc/qc_leg_plant_adjoint.hpp), leg_plant_step_autograd and rollout_tick_autograd against the
50-digit reverse pass (tests/leg_plant_adjoint_restatement.py), against central differences of the forward kernels themselves, and
against the direct calls.

The bar of test 1: |device - 50 digits| <= K EPS condsum per output entry, condsum the condition sum the 50-digit pass returns with the
value, K = 4 c_np with c_np the float64 restatement's own distance from the 50-digit pass in the same units, measured on the CPU on the
same pool (tests/test_leg_plant_adjoint_cpu.py, which asserts it):
    c_np   Rwb_bar 6.6   x_bar 0.2   xdot_bar 8.0   w_bar 1.0   joint_q_bar 0.9   joint_qdot_bar 0.7   joint_tau_bar 1.3
The factor 4 is the siblings' allowance for another order of operations and FMA contraction; it is not a measured device number."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from tests import leg_plant_adjoint_restatement as LA
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, ctl, q  # noqa: F401
from tests.solved_batch_support import assert_raw_refusals

pytestmark = pytest.mark.gpu
EPS = LA.EPS
SIZES = (1, 63, 64, 65, 257, 4097)
STATE = LA.INPUTS[:-1]
K = {k: 4.0 * v for k, v in LA.C_NP.items()}  # c_np is measured on the CPU, never taken from the device
# an output and the input cotangent of its layout it may be written over
ALIASES = (("Rwb_bar", "Rwb"), ("x_bar", "x"), ("xdot_bar", "xdot"), ("w_bar", "w"), ("joint_q_bar", "joint_q"), ("joint_qdot_bar", "joint_qdot"),
           ("joint_tau_bar", "joint_qdot"), ("joint_tau_bar", "joint_q"), ("x_bar", "w"))
DT, INERTIA = LA.DT, LA.INERTIA


@pytest.fixture(scope="module")
def odd_ctl(q, P):
    """a handle of this module's own at ODD_KIN (the shared `ctl` keeps the library's model)"""
    from tests.device_math_reference import ODD_KIN

    c = q.BalanceController.from_params(P, device=0)
    c.set_kinematics(**ODD_KIN.handle_arguments())
    yield c
    c.close()


def _adjoint(ctl, s, mask, bars, n, want=LA.OUTPUTS, given=None, alias=None, zeros=False, way="stance"):
    """One adjoint call over n robots (the pool tiled), every array with sentinel rows behind row n - 1.  given: the cotangents that
    are handed over (default all; the others are NULL); zeros: arrays of zeros in their place; alias = (output, cotangent): that
    output is written over that cotangent; way: how the contact mask is given (LA.WAYS).  Returns ({output: host [n + 2, k], "flags"},
    {input or cotangent: host [n + 2, k] after the call})."""
    import torch

    given = tuple(LA.COTANGENTS) if given is None else given
    d = _device_arrays(s, n)
    contact = _device_arrays(LA.contact_inputs(_tile(mask, n), way), n)
    host_bars = {k: (np.zeros_like(bars[k]) if (zeros and k not in given) else bars[k]) for k in (tuple(LA.COTANGENTS) if zeros else given)}
    b = _device_arrays(host_bars, n)
    outs = _device_arrays({k: np.full((1, LA._SIZES[k]), SENTINEL) for k in want}, n)
    out = {k: v[1] for k, v in outs.items()}
    if alias is not None:
        out[alias[0]] = b[alias[1]][1]
    flags = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    ctl.leg_plant_step_adjoint({k: d[k][1] for k in STATE}, d["joint_tau"][1], DT, INERTIA, {k: v[1] for k, v in b.items()}, want=tuple(want), out=out,
                               flags=flags[:n], **{k: v[1] for k, v in contact.items()})
    torch.cuda.synchronize()
    res = {k: (b[alias[1]][0] if alias is not None and k == alias[0] else outs[k][0]).cpu().numpy() for k in want}
    res["flags"] = flags.cpu().numpy()
    after = {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{"bar_" + k: v[0].cpu().numpy() for k, v in b.items()},
             **{"contact_" + k: v[0].cpu().numpy() for k, v in contact.items()}}
    return res, after


# ------------------------------------------------------------------ 1. against 50 digits
@pytest.mark.parametrize("way", LA.WAYS)
def test_every_output_against_50_digits(ctl, way):
    """Every output entry within K EPS condsum (module docstring) of the 50-digit reverse pass on the same doubles, at every batch
    size and with the contact mask given in each of the four ways; no robot of the pool is flagged."""
    _every_output_against_50_digits(ctl, way, "default", SIZES)


@pytest.mark.parametrize("way", LA.WAYS)
def test_every_output_against_50_digits_at_the_odd_model(odd_ctl, way):
    """The same body on a handle at ODD_KIN, the pool rebuilt under the model (all 16 contact masks), K = 4 C_NP_ODD; the sizes with
    a tail, one full wave and more than one workgroup."""
    _every_output_against_50_digits(odd_ctl, way, "odd", (1, 65, 257))


def _every_output_against_50_digits(ctl, way, model, sizes):
    from tests.device_math_reference import KINS

    K = {k: 4.0 * v for k, v in LA.C_NP_OF[model].items()}
    s, mask, bars = LA.pool(KINS[model])
    ref, _ = LA.pool_reference(KINS[model])
    for n in sizes:
        got, _ = _adjoint(ctl, s, mask, bars, n, way=way)
        assert not got["flags"][:n].any() and (got["flags"][n:] == -77).all()
        worst = {}
        for k in LA.OUTPUTS:
            val, cond = _tile(ref[k][0], n), _tile(ref[k][1], n)
            live = cond > 0  # (a stance leg's joint_qdot_bar: an exact 0)
            assert np.array_equal(got[k][:n][~live], val[~live]), k
            worst[k] = float((np.abs(got[k][:n] - val)[live] / (EPS * cond[live])).max(initial=0.0))
            assert (got[k][n:] == SENTINEL).all(), k
        print(f"{model} {way} n {n}: worst error / (EPS condsum) {worst}")
        for k in LA.OUTPUTS:
            assert worst[k] <= K[k], (n, k, worst[k], K[k])


def test_flagged_rows_are_nan_with_the_expected_bits(ctl):
    """The stretched leg, the leg with d < -1 and the singular J(q): exactly the expected bits, NaN in every output row - and the
    unflagged robots of the same call keep their values."""
    _flagged_rows(ctl, "default")


def test_flagged_rows_are_nan_with_the_expected_bits_at_the_odd_model(odd_ctl):
    """The same body at ODD_KIN: the stretched, folded and singular legs rebuilt from the model's hip and links."""
    _flagged_rows(odd_ctl, "odd")


def _flagged_rows(ctl, model):
    from tests.device_math_reference import KINS

    s, mask, bars = LA.pool(KINS[model])
    fs, fmask, fbars, expected = LA.flagged_pool(KINS[model])
    m = len(expected)
    both = lambda a, b: np.concatenate([a, b[:5]], 0)
    got, _ = _adjoint(ctl, {k: both(fs[k], s[k]) for k in s}, both(fmask, mask), {k: both(fbars[k], bars[k]) for k in bars}, m + 5)
    alone, _ = _adjoint(ctl, {k: v[:5] for k, v in s.items()}, mask[:5], {k: v[:5] for k, v in bars.items()}, 5)
    assert np.array_equal(got["flags"][:m], expected) and not got["flags"][m:m + 5].any()
    for k in LA.OUTPUTS:
        assert np.isnan(got[k][:m]).all(), k
        assert np.array_equal(got[k][m:m + 5], alone[k][:5]), k


# ------------------------------------------------------------------ 2. exact cases
def test_zero_and_null_cotangents_and_subsets_of_want(ctl):
    """All input cotangents zero: every output exactly zero.  A NULL cotangent: bit for bit what an array of zeros gives.  Every
    `want` subset of one output, and one pair: bit for bit the full call's."""
    n = 257
    s, mask, bars = LA.pool()
    zero, _ = _adjoint(ctl, s, mask, {k: np.zeros_like(v) for k, v in bars.items()}, n)
    for k in LA.OUTPUTS:
        assert not zero[k][:n].any(), k
    full, _ = _adjoint(ctl, s, mask, bars, n)
    assert all(np.abs(full[k][:n]).max() > 0 for k in LA.OUTPUTS)
    for given in [(k,) for k in LA.COTANGENTS] + [("x", "joint_q"), ("Rwb", "joint_qdot")]:
        null, _ = _adjoint(ctl, s, mask, bars, n, given=given)
        zeros, _ = _adjoint(ctl, s, mask, bars, n, given=given, zeros=True)
        for k in LA.OUTPUTS:
            assert np.array_equal(null[k], zeros[k]), (given, k)
        assert any(not np.array_equal(null[k], full[k]) for k in LA.OUTPUTS), given
    for want in [(k,) for k in LA.OUTPUTS] + [("Rwb_bar", "joint_tau_bar")]:
        part, _ = _adjoint(ctl, s, mask, bars, n, want=want)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)


# ------------------------------------------------------------------ 3. in place, own rows only
@pytest.mark.parametrize("n", (1, 65, 257, 4097))
def test_in_place_and_only_its_own_rows(ctl, n):
    """An output written over an input cotangent of its layout (ALIASES) is bit for bit what a separate array gets, and so is every
    other output of that call; the rows behind row n - 1 keep their sentinels in every array; no input array is written, and no
    cotangent array but the aliased one."""
    s, mask, bars = LA.pool()
    own, after = _adjoint(ctl, s, mask, bars, n)
    for k, a in list(own.items()) + list(after.items()):
        assert (a[n:] == (SENTINEL if a.dtype == np.float64 else (0x5A if a.dtype == np.uint8 else -77))).all(), k
    for k in LA.INPUTS:
        assert np.array_equal(after[k][:n], _tile(s[k], n)), k
    for k in LA.COTANGENTS:
        assert np.array_equal(after["bar_" + k][:n], _tile(bars[k], n)), k
    assert np.array_equal(after["contact_stance"][:n], _tile(mask, n).astype(np.uint8))
    assert all((own[k][:n] != SENTINEL).all() for k in LA.OUTPUTS)
    for alias in ALIASES:
        got, after = _adjoint(ctl, s, mask, bars, n, alias=alias)
        for k in LA.OUTPUTS:
            assert np.array_equal(got[k], own[k]), (alias, k)
        for k in LA.INPUTS:
            assert np.array_equal(after[k][:n], _tile(s[k], n)), (alias, k)
        for k in LA.COTANGENTS:
            if k != alias[1]:
                assert np.array_equal(after["bar_" + k][:n], _tile(bars[k], n)) and (after["bar_" + k][n:] == SENTINEL).all(), (alias, k)


# ------------------------------------------------------------------ 4. consistency with the forward kernel
def test_consistent_with_differences_of_leg_plant_step(ctl, P):
    """<y_bar, J v> from central differences of ctl.leg_plant_step itself at the committed h along the committed directions (all seven
    inputs, entrywise for Rwb) against <x_bar, v> of the adjoint kernel, on the first 65 robots of the pool - unflagged by
    construction (tests/test_leg_plant_adjoint_cpu.py::test_pool_covers_what_it_says), none left out - with the CPU test's bar
    (leg_plant_adjoint_restatement.fd_bar, fd_support.fd_bar's construction)."""
    import torch

    h, n = LA.FD_H, LA.FD_N
    s, mask, bars = ({k: a[:n] for k, a in d.items()} if isinstance(d, dict) else d[:n] for d in LA.pool())
    v = LA.fd_directions()
    stance = torch.from_numpy(np.ascontiguousarray(mask.astype(np.uint8))).cuda()

    def step(inputs):
        dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in inputs.items()}
        flags = torch.zeros((n,), dtype=torch.int32, device="cuda")
        ctl.leg_plant_step({k: dev[k] for k in STATE}, dev["joint_tau"], DT, INERTIA, stance=stance, flags=flags)
        torch.cuda.synchronize()
        assert not flags.any()
        return {k: dev[k].cpu().numpy() for k in STATE}

    fd1, fd2 = LA.fd_of(step, s, bars, v, h)
    got, _ = _adjoint(ctl, s, mask, bars, n)
    assert not got["flags"][:n].any()
    dd = sum((got[LA.BAR_OF[k]][:n] * v[k]).sum(axis=1) for k in LA.INPUTS)
    cond = {k: c[:n] for k, (_, c) in LA.pool_reference()[0].items()}
    bar = LA.fd_bar(P, s, mask, bars, v, cond, fd1, fd2, h)
    err = np.abs(fd1 - dd)
    print("worst error / bar", float((err / bar).max()), "worst relative bar", float((bar / np.maximum(np.abs(dd), 1e-300)).max()))
    assert np.all(err <= bar), float((err / bar).max())


# ------------------------------------------------------------------ 5. the autograd wrapper of one step
def test_autograd_equals_the_direct_calls_bit_for_bit(ctl):
    """leg_plant_step_autograd returns what leg_plant_step writes into clones, bit for bit, and leaves its inputs as they are; its
    .grads are the direct leg_plant_step_adjoint call's, bit for bit; inputs that do not require grad get None, and a backward that
    reaches only some outputs hands the others over as NULL."""
    import torch

    n = 130
    s, mask, bars = LA.pool()
    stance = torch.from_numpy(np.ascontiguousarray(mask[:n].astype(np.uint8))).cuda()
    leaves = lambda req: {k: torch.from_numpy(np.array(s[k][:n])).cuda().requires_grad_(k in req) for k in LA.INPUTS}
    dev = leaves(LA.INPUTS)
    cot = {k: torch.from_numpy(np.array(bars[k][:n])).cuda() for k in LA.COTANGENTS}
    before = {k: t.detach().clone() for k, t in dev.items()}
    fl = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out = ctl.leg_plant_step_autograd(dev, dev["joint_tau"], DT, INERTIA, stance=stance, flags=fl)
    direct = {k: before[k].clone() for k in STATE}
    ctl.leg_plant_step(direct, before["joint_tau"], DT, INERTIA, stance=stance)
    for k, t in zip(STATE, out):
        assert torch.equal(t.detach(), direct[k]), k
    assert all(torch.equal(dev[k].detach(), before[k]) for k in dev) and not fl.any()
    sum((t * cot[k]).sum() for k, t in zip(STATE, out)).backward()
    ref = ctl.leg_plant_step_adjoint({k: before[k] for k in STATE}, before["joint_tau"], DT, INERTIA, cot, stance=stance)
    for k in LA.INPUTS:
        assert torch.equal(dev[k].grad, ref[k + "_bar"].view_as(dev[k])), k
    # only x' and joint_q' reach the loss, only joint_q and joint_tau require grad
    dev = leaves(("joint_q", "joint_tau"))
    out = ctl.leg_plant_step_autograd(dev, dev["joint_tau"], DT, INERTIA, stance=stance)
    ((out[1] * cot["x"]).sum() + (out[4] * cot["joint_q"]).sum()).backward()
    ref = ctl.leg_plant_step_adjoint({k: before[k] for k in STATE}, before["joint_tau"], DT, INERTIA, {"x": cot["x"], "joint_q": cot["joint_q"]},
                                     want=("joint_q_bar", "joint_tau_bar"), stance=stance)
    assert torch.equal(dev["joint_q"].grad, ref["joint_q_bar"]) and torch.equal(dev["joint_tau"].grad, ref["joint_tau_bar"])
    assert all(dev[k].grad is None for k in ("Rwb", "x", "xdot", "w", "joint_qdot"))


# ------------------------------------------------------------------ 6. backpropagation through the closed loop around the tick
def test_backpropagation_through_a_rollout_of_the_tick(q, P):
    """rollout_tick_autograd on leg_plant_adjoint_restatement.rollout_case - stand_start(65): all stance, from a standing start -, H = 3
    at dt = 1/300, loss <c, final {Rwb, x, xdot, w, joint_q, joint_qdot}> with committed c.  Forward: bit for bit ctl.rollout_tick's on
    a copy, and `batch` is not modified.  The directional derivative in (joint_q, x, xdot, w) per robot, and in `params` through kp_p
    (the robots are independent, so the loss sums the KEPT robots and params.grad is their sum), along committed directions against
    central differences of ctl.rollout_tick at 0, +-h, +-2h, h = 1e-4.  Kept: the rule of test_backpropagation_through_a_rollout -
    solved at every step and every point, sensitivity flags 0 at every step of the base point, the working-set word of every step the
    same at all points - plus an unchanged torque clamp mask and zero plant flags at every step and point; at least 0.5 of the
    robots.  The CPU loop alone - the C oracle's tick and leg_plant_restatement's step - keeps 0.815 of them under this rule
    (tests/test_leg_plant_adjoint_cpu.py::test_cpu_loop_meets_the_rollout_tests_keep_rule).  Bar per robot:
    |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|; for the gains the same terms summed over the kept robots."""
    import torch

    n, H, h = LA.ROLLOUT_N, LA.ROLLOUT_STEPS, LA.ROLLOUT_H
    b, c, v, vp = LA.rollout_case(P)
    lo, hi = LA.tau_limits()

    def rollout(k, gains=False):
        """ctl.rollout_tick from the start (or, gains: the handle's kp_p) moved by k h: the final loss per robot, and per step the
        working-set word, the status, the clamp mask of the torques and the plant's flags"""
        ck = q.BalanceController.from_params(dict(P, kp_p=np.asarray(P["kp_p"], float) + (k * h * vp if gains else 0.0)), device=0)
        ck.set_tuning(race=0)
        start = b if gains else dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status, clamp, flags = [], [], [], []
        for steps in range(1, H + 1):  # (the last tick of an s-step rollout is step s - 1's)
            state, out = ck.rollout_tick(q.to_device(start), None, steps, LA.DT, LA.STAND_INERTIA)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            tau = out["joint_tau"].cpu().numpy()
            clamp.append((tau <= lo) | (tau >= hi))
            flags.append(out["flags"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in STATE}
        ck.close()
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags), final

    L0, w0, st0, cl0, fl0, final0 = rollout(0)
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)
    # the keep rule: the base point's sensitivity flags at every step, then every point of both sweeps
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0)
    _, rec = ctl.rollout_tick(q.to_device(b), None, H, LA.DT, LA.STAND_INERTIA, record_every=1)
    for _, hist in rec["history"]:
        bk = {name: t for name, t in dict(q.to_device(b), **{name: hist[name] for name in STATE}).items() if name != "joint_qdot"}
        o = ctl.control_batch(bk, want_torques=True)
        fl = ctl.sensitivity_batch(bk, o["grf_body"], torch.ones_like(o["grf_body"]), want=("flags",))["flags"]
        keep &= fl.cpu().numpy() == 0
    print("kept after the base point's statuses, plant flags and sensitivity flags:", keep.mean(), "words at the base point:", sorted(set(w0.ravel().tolist())))
    pts = {(k, gains): rollout(k, gains) for k in (-2, -1, 1, 2) for gains in (False, True)}
    for Lk, wk, stk, clk, flk, _ in pts.values():
        print("  point: solved", (stk == 0).all(axis=0).mean(), "same words", (wk == w0).all(axis=0).mean(), "same clamp mask",
              (clk == cl0).all(axis=(0, 2)).mean(), "no plant flag", (flk == 0).all(axis=0).mean())
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0)
    print("kept", keep.mean(), "entries at the clamp at the base point:", int(cl0.sum()))

    dev = q.to_device(b)
    for name in v:
        dev[name].requires_grad_(True)
    params = ctl.parameter_tensor().requires_grad_(True)
    before = {name: t.detach().clone() for name, t in dev.items()}
    state, out = ctl.rollout_tick_autograd(dev, H, LA.DT, LA.STAND_INERTIA, params=params)
    for name in STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name  # forward: ctl.rollout_tick's bits
    assert torch.equal(out["active_set"], torch.from_numpy(w0[-1]).cuda()) and np.array_equal(out["flags"].cpu().numpy(), fl0[-1])
    assert all(torch.equal(dev[name].detach(), before[name]) for name in dev)  # `batch` is not modified
    assert keep.mean() >= 0.5, keep.mean()
    kept = torch.from_numpy(keep.astype(np.float64)).cuda()[:, None]
    sum((state[name] * torch.from_numpy(c[name]).cuda() * kept).sum() for name in STATE).backward()
    torch.cuda.synchronize()
    g = {name: dev[name].grad.cpu().numpy() for name in v}
    gp = params.grad.cpu().numpy()[q.balance_controller.PARAM_LAYOUT["kp_p"][0]]
    fd = lambda gains: ((pts[1, gains][0] - pts[-1, gains][0]) / (2 * h), (pts[2, gains][0] - pts[-2, gains][0]) / (4 * h))
    fd1, fd2 = fd(False)
    an = sum((g[name] * v[name]).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda a: float((a[keep] / scale[keep]).max())
    print("state: worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    assert (scale[keep] > 0).all()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    assert not any(g[name][~keep].any() for name in v)  # a robot left out of the loss has no gradient: the robots are independent
    fd1, fd2 = fd(True)
    anp, fdp, tp = float(gp @ vp), float(fd1[keep].sum()), float(np.abs(fd1 - fd2)[keep].sum())
    scale_p = float(np.linalg.norm(gp) * np.linalg.norm(vp))
    print("gains: analytic", anp, "FD", fdp, "t", tp, "relative error", abs(fdp - anp) / scale_p)
    assert scale_p > 0 and abs(fdp - anp) <= tp + 1e-5 * scale_p
    for key in ("gait_dt", "swing_state", "feet"):
        with pytest.raises(ValueError, match=f"rollout_tick_autograd: the batch carries {key}"):
            ctl.rollout_tick_autograd(dict(dev, **{key: dev["x"]}), H, LA.DT, LA.STAND_INERTIA)
    with pytest.raises(ValueError, match="rollout_tick_autograd: the batch carries joint_q and joint_qdot"):
        ctl.rollout_tick_autograd({k: t for k, t in dev.items() if k != "joint_qdot"}, H, LA.DT, LA.STAND_INERTIA)
    ctl.close()


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_launch_nothing(q, ctl):
    """Each rejected call returns QC_ERR_INVALID with a message of qc_leg_plant_step_adjoint_batch's own and leaves every output at its
    sentinel.  Every pointer that is handed over is a valid device array of the right size.  The same call with everything in order
    then does run."""
    import torch

    from quadruped_control_amd import _lib

    lib, n = _lib.load(), 65
    s, mask, bars = LA.pool()
    d = _device_arrays(s, n)
    bd = _device_arrays(bars, n)
    outs = {k: torch.full((n, m), SENTINEL, dtype=torch.float64, device="cuda") for k, m in LA._SIZES.items()}
    before = {k: t[0].clone() for k, t in list(d.items()) + [("bar_" + k, t) for k, t in bd.items()]}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def io(**kw):
        a = _lib.QcLegPlantAdjointIo()
        lib.qc_default_leg_plant_adjoint(ctypes.byref(a))
        for k in LA.INPUTS:
            setattr(a, k, d[k][1].data_ptr())
        for k in LA.COTANGENTS:
            setattr(a, k + "_next_bar", bd[k][1].data_ptr())
        for k, t in outs.items():
            setattr(a, k, t.data_ptr())
        for k in range(3):
            a.leg_inertia[k] = INERTIA[k]
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def untouched(what="the valid call"):
        for k, t in list(d.items()) + [("bar_" + k, t) for k, t in bd.items()]:
            assert torch.equal(t[0], before[k]), (what, k)

    def refused(handle, a, what):
        rc = lib.qc_leg_plant_step_adjoint_batch(handle, n, ctypes.byref(a), stream)
        assert rc == -1 and _lib.last_error().startswith("qc_leg_plant_step_adjoint_batch:"), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in outs.values()), what
        untouched(what)

    refused(ctl._h, io(struct_size=0), "struct_size not set")
    for k in LA.INPUTS:
        refused(ctl._h, io(**{k: None}), f"{k} = NULL")
    refused(ctl._h, io(**{k + "_next_bar": None for k in LA.COTANGENTS}), "no cotangent")
    refused(ctl._h, io(**{k: None for k in outs}), "no output")
    for bad in (0.0, -1.0 / 300.0, float("nan"), float("inf")):
        refused(ctl._h, io(dt=bad), f"dt = {bad}")
        refused(ctl._h, io(leg_inertia=(ctypes.c_double * 3)(0.02, bad, 0.02)), f"leg_inertia = {bad}")
    Podd = dict(q.cheetah_params())
    Podd["Ib"] = np.diag([0.011253, -0.036203, 0.042673])
    odd = q.BalanceController.from_params(Podd, device=0)
    refused(odd._h, io(), "Ib not positive definite")
    assert "positive definite" in _lib.last_error()
    state = {k: d[k][1] for k in STATE}
    with pytest.raises(ValueError, match="^qc_leg_plant_step_adjoint_batch:"):
        odd.leg_plant_step_adjoint(state, d["joint_tau"][1], DT, INERTIA, {"x": bd["x"][1]}, want=("x_bar",))
    odd.close()
    # the Python wrapper checks shapes, dtypes and names before it calls
    with pytest.raises(ValueError, match="joint_tau"):
        ctl.leg_plant_step_adjoint(state, d["joint_tau"][1][:, :6].contiguous(), DT, INERTIA, {"x": bd["x"][1]})
    with pytest.raises(ValueError, match=r"cotangents\['x'\]"):
        ctl.leg_plant_step_adjoint(state, d["joint_tau"][1], DT, INERTIA, {"x": bd["x"][1].float()})
    with pytest.raises(ValueError, match="unknown cotangent"):
        ctl.leg_plant_step_adjoint(state, d["joint_tau"][1], DT, INERTIA, {"joint_tau": bd["joint_q"][1]})
    with pytest.raises(ValueError, match="unknown output"):
        ctl.leg_plant_step_adjoint(state, d["joint_tau"][1], DT, INERTIA, {"x": bd["x"][1]}, want=("foot_world_bar",))
    with pytest.raises(ValueError, match="^qc_leg_plant_step_adjoint_batch: no input cotangent"):
        ctl.leg_plant_step_adjoint(state, d["joint_tau"][1], DT, INERTIA, {}, want=("x_bar",), out={"x_bar": outs["x_bar"]})
    # no handle, no io, n beyond one launch, the struct_size of another struct; n == 0 launches nothing; the same structs, valid, do
    assert_raw_refusals(lib.qc_leg_plant_step_adjoint_batch, lambda: (ctl._h, n, None, io()), "qc_leg_plant_adjoint_io",
                        ctypes.sizeof(_lib.QcLegPlantAdjointIo), 72, [(t, SENTINEL, True) for t in outs.values()], beyond=0xFFFFFF * 256 + 1,
                        stream=stream, untouched=untouched, launched=untouched)

"""GPU: qc_plant_step_adjoint_batch (csrc/qc_plant_adjoint.hpp), plant_step_autograd and rollout_autograd against the 50-digit reverse
pass (tests/plant_adjoint_restatement.py), against central differences of the forward kernels themselves, and against the direct calls.

Batch sizes 1, 63, 64, 65, 257 and 4097: below, at and above a wave, above a block (256) and a tail behind 16 full blocks.  Every
reference is computed once per process on pools of 257 robots (one per dt: the swept rows' w is theta / dt) that the batches tile.

The bar against 50 digits, per output entry: K EPS condsum, condsum being the 50-digit pass's condition sum (every term of the forward
and the reverse pass replaced by its absolute value) and K = 4 c_np, c_np the plain numpy restatement's own worst error in the same
units, measured on the CPU on the same pools (tests/test_plant_adjoint_cpu.py, which asserts it):
    c_np   Rwb_bar 1.4    x_bar 1.6    xdot_bar 1.0    w_bar 1.0    grf_bar 2.1    foot_world_bar 2.2     (plant_adjoint_restatement.C_NP)
    K      Rwb_bar 5.6    x_bar 6.4    xdot_bar 4.0    w_bar 4.0    grf_bar 8.4    foot_world_bar 8.8
The factor 4 covers the device's other order of operations (it applies the exponential as cross products where the restatement
multiplies matrices) and FMA contraction, not another size of error."""
import ctypes

import numpy as np
import pytest

from tests import plant_adjoint_restatement as AR
from tests import plant_restatement as PR
from tests.fd_support import BAR_OF, fd_bar
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, ctl, q  # noqa: F401
from tests.solved_batch_support import assert_raw_refusals

pytestmark = pytest.mark.gpu
EPS = AR.EPS
SIZES = (1, 63, 64, 65, 257, 4097)
STATE = ("Rwb", "x", "xdot", "w")
K = {k: 4.0 * v for k, v in AR.C_NP.items()}  # c_np is measured on the CPU, never taken from the device
# an output and the input cotangent of its layout it may be written over
ALIASES = (("Rwb_bar", "Rwb"), ("x_bar", "x"), ("xdot_bar", "xdot"), ("w_bar", "w"), ("foot_world_bar", "feet"), ("grf_bar", "feet"), ("x_bar", "w"))


def _adjoint(ctl, s, bars, n, dt, want=AR.OUTPUTS, given=None, alias=None, zeros=False):
    """One adjoint call over n robots (the pool tiled), every array with sentinel rows behind row n - 1.  given: the cotangents that
    are handed over (default all; the others are NULL); zeros: arrays of zeros in their place; alias = (output, cotangent): that
    output is written over that cotangent.  Returns ({output: host [n + 2, k]}, {input or cotangent: host [n + 2, k] after the call})."""
    import torch

    given = tuple(AR.COTANGENTS) if given is None else given
    d = _device_arrays(s, n)
    host_bars = {k: (np.zeros_like(bars[k]) if (zeros and k not in given) else bars[k]) for k in (tuple(AR.COTANGENTS) if zeros else given)}
    b = _device_arrays(host_bars, n)
    outs = _device_arrays({k: np.full((1, {"Rwb_bar": 9, "grf_bar": 12, "foot_world_bar": 12}.get(k, 3)), SENTINEL) for k in want}, n)
    out = {k: v[1] for k, v in outs.items()}
    if alias is not None:
        out[alias[0]] = b[alias[1]][1]
    ctl.plant_step_adjoint({k: d[k][1] for k in STATE}, d["grf_body"][1], d["foot_world"][1], dt, {k: v[1] for k, v in b.items()}, want=tuple(want), out=out)
    torch.cuda.synchronize()
    res = {k: (b[alias[1]][0] if alias is not None and k == alias[0] else outs[k][0]).cpu().numpy() for k in want}
    return res, {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{"bar_" + k: v[0].cpu().numpy() for k, v in b.items()}}


# ------------------------------------------------------------------ 1. against 50 digits
@pytest.mark.parametrize("dt", AR.DTS)
def test_every_output_against_50_digits(ctl, P, dt):
    """Every output entry within K EPS condsum (module docstring) of the 50-digit reverse pass on the same doubles, at every batch
    size: the identity, a rotation by nearly pi, step angles of 0 exactly, 1e-12 ... 3 on both sides of the series threshold."""
    s, bars = AR.pool(dt)
    ref = AR.pool_reference(dt)
    theta = AR.step_angle(P, s, dt)
    assert (theta == 0).sum() >= 8 and ((theta > 0) & (theta < 3e-12)).any() and theta.max() >= 2.99
    assert ((theta > 0.98) & (theta * theta < AR.SERIES_BELOW)).any() and ((theta * theta >= AR.SERIES_BELOW) & (theta < 1.02)).any()
    for n in SIZES:
        got, _ = _adjoint(ctl, s, bars, n, dt)
        worst = {}
        for k in AR.OUTPUTS:
            val, cond = _tile(ref[k][0], n), _tile(ref[k][1], n)
            worst[k] = float((np.abs(got[k][:n] - val) / (EPS * cond)).max())
            assert (got[k][n:] == SENTINEL).all(), k
        print(f"dt {dt} n {n}: worst error / (EPS condsum) {worst}")
        for k in AR.OUTPUTS:
            assert worst[k] <= K[k], (n, k, worst[k], K[k])


# ------------------------------------------------------------------ 2. exact cases
def test_zero_and_null_cotangents_and_subsets_of_want(ctl):
    """All input cotangents zero: every output exactly zero.  A NULL cotangent: bit for bit what an array of zeros gives.  Every
    `want` subset of one output, and one pair: bit for bit the full call's."""
    dt, n = 1.0 / 300.0, 257
    s, bars = AR.pool(dt)
    zero, _ = _adjoint(ctl, s, {k: np.zeros_like(v) for k, v in bars.items()}, n, dt)
    for k in AR.OUTPUTS:
        assert not zero[k][:n].any(), k
    full, _ = _adjoint(ctl, s, bars, n, dt)
    assert all(np.abs(full[k][:n]).max() > 0 for k in AR.OUTPUTS)
    for given in [(k,) for k in AR.COTANGENTS] + [("x", "feet"), ("Rwb", "w")]:
        null, _ = _adjoint(ctl, s, bars, n, dt, given=given)
        zeros, _ = _adjoint(ctl, s, bars, n, dt, given=given, zeros=True)
        for k in AR.OUTPUTS:
            assert np.array_equal(null[k], zeros[k]), (given, k)
        assert any(not np.array_equal(null[k], full[k]) for k in AR.OUTPUTS), given
    for want in [(k,) for k in AR.OUTPUTS] + [("Rwb_bar", "grf_bar")]:
        part, _ = _adjoint(ctl, s, bars, n, dt, want=want)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)


# ------------------------------------------------------------------ 3. in place, own rows only
@pytest.mark.parametrize("n", (1, 65, 257, 4097))
def test_in_place_and_only_its_own_rows(ctl, n):
    """An output written over an input cotangent of its layout (ALIASES) is bit for bit what a separate array gets, and so is every
    other output of that call; the rows behind row n - 1 keep their sentinels in every array; no input array is written, and no
    cotangent array but the aliased one."""
    dt = 1.0 / 300.0
    s, bars = AR.pool(dt)
    own, after = _adjoint(ctl, s, bars, n, dt)
    for k, a in list(own.items()) + list(after.items()):
        assert (a[n:] == SENTINEL).all(), k
    for k in AR.INPUTS:
        assert np.array_equal(after[k][:n], _tile(s[k], n)), k
    for k in AR.COTANGENTS:
        assert np.array_equal(after["bar_" + k][:n], _tile(bars[k], n)), k
    assert all((own[k][:n] != SENTINEL).all() for k in AR.OUTPUTS)
    for alias in ALIASES:
        got, after = _adjoint(ctl, s, bars, n, dt, alias=alias)
        for k in AR.OUTPUTS:
            assert np.array_equal(got[k], own[k]), (alias, k)
        for k in AR.INPUTS:
            assert np.array_equal(after[k][:n], _tile(s[k], n)), (alias, k)
        for k in AR.COTANGENTS:
            if k != alias[1]:
                assert np.array_equal(after["bar_" + k][:n], _tile(bars[k], n)) and (after["bar_" + k][n:] == SENTINEL).all(), (alias, k)


# ------------------------------------------------------------------ 4. consistency with the forward kernel
def test_consistent_with_differences_of_plant_step(ctl, P):
    """<y_bar, J v> from central differences of ctl.plant_step itself at the committed h along the committed directions (all six inputs,
    entrywise for Rwb) against <x_bar, v> of the adjoint kernel, 65 robots, with the CPU test's bar: |FD(h) - FD(2h)| plus the
    quotient's rounding from the forward kernel's derived one-step bars (tests/test_gpu_plant.py holds the kernel to them) plus
    the analytic side's 4 EPS sum condsum |v|."""
    import torch

    dt, h, n = 1.0 / 300.0, AR.FD_H, AR.FD_N
    s, bars = ({k: a[:n] for k, a in d.items()} for d in AR.pool(dt))
    v = AR.fd_directions()

    def step(inputs):
        dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in inputs.items()}
        feet = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        ctl.plant_step({k: dev[k] for k in STATE}, dev["grf_body"], dev["foot_world"], dt, feet=feet)
        torch.cuda.synchronize()
        return dict({k: dev[k].cpu().numpy() for k in STATE}, feet=feet.cpu().numpy())

    fd1, fd2 = AR.fd_of(step, s, bars, v, h)
    got, _ = _adjoint(ctl, s, bars, n, dt)
    dd = sum((got[BAR_OF[k]][:n] * v[k]).sum(axis=1) for k in AR.INPUTS)
    cond = {k: c[:n] for k, (_, c) in AR.pool_reference(dt).items()}
    bar = fd_bar(P, s, bars, v, cond, fd1, fd2, h, dt)
    err = np.abs(fd1 - dd)
    print("worst error / bar", float((err / bar).max()), "worst relative bar", float((bar / np.maximum(np.abs(dd), 1e-300)).max()))
    assert np.all(err <= bar), float((err / bar).max())


# ------------------------------------------------------------------ 5. the autograd wrapper of one step
def _leaves(s, n, requires):
    import torch

    dev = {k: torch.from_numpy(np.array(s[k][:n])).cuda() for k in AR.INPUTS}
    for k in requires:
        dev[k].requires_grad_(True)
    return dev


def test_autograd_equals_the_direct_calls_bit_for_bit(ctl):
    """plant_step_autograd returns what plant_step writes into clones, bit for bit, and leaves its inputs as they are; its .grads are
    the direct plant_step_adjoint call's, bit for bit; inputs that do not require grad get None, and a backward that reaches only some
    outputs hands the others over as NULL."""
    import torch

    dt, n = 1.0 / 300.0, 130
    s, bars = AR.pool(dt)
    dev = _leaves(s, n, AR.INPUTS)
    cot = {k: torch.from_numpy(np.array(bars[k][:n])).cuda() for k in AR.COTANGENTS}
    out = ctl.plant_step_autograd(dev, dev["grf_body"], dev["foot_world"], dt)
    assert all(o.grad_fn is not None for o in out)
    clones = {k: dev[k].detach().clone() for k in STATE}
    feet = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
    ctl.plant_step(clones, dev["grf_body"].detach(), dev["foot_world"].detach(), dt, feet=feet)
    for o, ref in zip(out, [clones[k] for k in STATE] + [feet]):
        assert torch.equal(o.detach(), ref)
    for k in AR.INPUTS:
        assert np.array_equal(dev[k].detach().cpu().numpy(), s[k][:n]), k  # out of place
    direct = ctl.plant_step_adjoint({k: dev[k].detach() for k in STATE}, dev["grf_body"].detach(), dev["foot_world"].detach(), dt, cot)
    grads = torch.autograd.grad(out, [dev[k] for k in AR.INPUTS], [cot[k] for k in AR.COTANGENTS])
    torch.cuda.synchronize()
    for k, g in zip(AR.INPUTS, grads):
        assert g.shape == dev[k].shape and torch.equal(g, direct[BAR_OF[k]]), k
    # only x and w require grad, only feet' reaches the loss
    dev = _leaves(s, n, ("x", "w"))
    out = ctl.plant_step_autograd(dev, dev["grf_body"], dev["foot_world"], dt)
    (out[4] * cot["feet"]).sum().backward()
    part = ctl.plant_step_adjoint({k: dev[k].detach() for k in STATE}, dev["grf_body"], dev["foot_world"], dt, {"feet": cot["feet"]}, want=("x_bar", "w_bar"))
    torch.cuda.synchronize()
    assert torch.equal(dev["x"].grad, part["x_bar"]) and torch.equal(dev["w"].grad, part["w_bar"])
    assert all(dev[k].grad is None for k in AR.INPUTS if k not in ("x", "w"))
    dev = _leaves(s, n, ())
    assert all(o.grad_fn is None for o in ctl.plant_step_autograd(dev, dev["grf_body"], dev["foot_world"], dt))


# ------------------------------------------------------------------ 6. backpropagation through time
def test_backpropagation_through_a_rollout(q, P):
    """rollout_autograd on plant_restatement.rollout_start(65), H = 3 steps at dt = 1/300, loss <c, final {Rwb, x, xdot, w}> with
    committed c.  Forward: bit for bit ctl.rollout's on a copy, and `batch` is not modified.  The directional derivative in (x, xdot, w)
    along committed directions against central differences of ctl.rollout at 0, +-h, +-2h, h = 1e-4.  Kept (the rule of
    tests/test_gpu_sensitivity*.py): solved at every step and every point, sensitivity flags 0 at every step of the base point, the
    working-set word of every step the same at all five points; at least 0.75 of the robots (on the CPU, with the C oracle in the
    loop, these inputs keep 0.91).  Bar per robot: |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|, the sibling tests' rounding term
    (the forces' absolute error of ~1e-8 N over h)."""
    import torch

    n, H, dt, h = 65, 3, 1.0 / 300.0, 1e-4
    b, pw = PR.rollout_start(n)
    rng = np.random.default_rng(0xAD704)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in ("x", "xdot", "w")}
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)
    pwd = torch.from_numpy(pw).cuda()

    def rollout(k):
        """ctl.rollout from the start moved by k h v: the final loss per robot, and status and working-set word of every step"""
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status = [], []
        for steps in range(1, H + 1):  # (the last solve of an s-step rollout is step s - 1's)
            dev = q.to_device(start)
            state, out = ctl.rollout(dev, pwd.clone(), steps=steps, dt=dt)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), final, dev

    L0, w0, st0, final0, dev0 = rollout(0)
    dev = q.to_device(b)
    for name in v:
        dev[name].requires_grad_(True)
    before = {name: t.detach().clone() for name, t in dev.items()}
    state, out = ctl.rollout_autograd(dev, pwd, H, dt)
    for name in STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name  # forward: ctl.rollout's bits
    assert torch.equal(state["feet"].detach(), dev0["feet"]) and torch.equal(out["active_set"], torch.from_numpy(w0[-1]).cuda())
    assert all(torch.equal(dev[name].detach(), before[name]) for name in dev)  # `batch` is not modified
    loss = sum((state[name] * torch.from_numpy(c[name]).cuda()).sum() for name in STATE)
    loss.backward()
    torch.cuda.synchronize()
    g = {name: dev[name].grad.cpu().numpy() for name in v}
    # sensitivity flags of every step of the base point
    keep = (st0 == 0).all(axis=0)
    dev_h = q.to_device(b)
    _, rec = ctl.rollout(dev_h, pwd.clone(), steps=H, dt=dt, record_every=1)
    for _, hist in rec["history"]:
        bk = dict(q.to_device(b), **hist)
        o = ctl.control_batch(bk)
        fl = ctl.sensitivity_batch(bk, o["grf_body"], torch.ones_like(o["grf_body"]), want=("flags",))["flags"]
        keep &= fl.cpu().numpy() == 0
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    for Lk, wk, stk, _, _ in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0)
    fd1 = (pts[1][0] - pts[-1][0]) / (2 * h)
    fd2 = (pts[2][0] - pts[-2][0]) / (4 * h)
    an = sum((g[name] * v[name]).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda a: float((a[keep] / scale[keep]).max())
    print("kept", keep.mean(), "worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    print("robots with a non-zero working-set word at step 0:", int((w0[0] != 0).sum()), "of", n)
    assert keep.mean() >= 0.75, keep.mean()
    assert (scale[keep] > 0).all()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    with pytest.raises(ValueError, match="rollout: the plant is a single rigid body"):
        ctl.rollout_autograd(dict(dev, joint_q=dev["feet"]), pwd, H, dt)
    ctl.close()


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_launch_nothing(q, ctl):
    """Each rejected call returns QC_ERR_INVALID with a message of qc_plant_step_adjoint_batch's own and leaves every output at its
    sentinel.  Every pointer that is handed over is a valid device array of the right size.  The same call with everything in order
    then does run."""
    import torch

    from quadruped_control_amd import _lib

    lib, n, dt = _lib.load(), 65, 1.0 / 300.0
    s, bars = AR.pool(dt)
    d = _device_arrays(s, n)
    bd = _device_arrays(bars, n)
    outs = {k: torch.full((n, m), SENTINEL, dtype=torch.float64, device="cuda") for k, m in
            (("Rwb_bar", 9), ("x_bar", 3), ("xdot_bar", 3), ("w_bar", 3), ("grf_bar", 12), ("foot_world_bar", 12))}
    before = {k: t[0].clone() for k, t in list(d.items()) + [("bar_" + k, t) for k, t in bd.items()]}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def io(**kw):
        a = _lib.QcPlantAdjointIo()
        lib.qc_default_plant_adjoint(ctypes.byref(a))
        for k in AR.INPUTS:
            setattr(a, k, d[k][1].data_ptr())
        for k in AR.COTANGENTS:
            setattr(a, k + "_next_bar", bd[k][1].data_ptr())
        for k, t in outs.items():
            setattr(a, k, t.data_ptr())
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def untouched(what="the valid call"):
        for k, t in list(d.items()) + [("bar_" + k, t) for k, t in bd.items()]:
            assert torch.equal(t[0], before[k]), (what, k)

    def refused(handle, a, what):
        rc = lib.qc_plant_step_adjoint_batch(handle, n, ctypes.byref(a), stream)
        assert rc == -1 and _lib.last_error().startswith("qc_plant_step_adjoint_batch:"), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in outs.values()), what
        untouched(what)

    refused(ctl._h, io(struct_size=0), "struct_size not set")
    for k in AR.INPUTS:
        refused(ctl._h, io(**{k: None}), f"{k} = NULL")
    refused(ctl._h, io(**{k + "_next_bar": None for k in AR.COTANGENTS}), "no cotangent")
    refused(ctl._h, io(**{k: None for k in outs}), "no output")
    for bad in (0.0, -1.0 / 300.0, float("nan"), float("inf")):
        refused(ctl._h, io(dt=bad), f"dt = {bad}")
    Podd = dict(q.cheetah_params())
    Podd["Ib"] = np.diag([0.011253, -0.036203, 0.042673])
    odd = q.BalanceController.from_params(Podd, device=0)
    refused(odd._h, io(), "Ib not positive definite")
    assert "positive definite" in _lib.last_error()
    with pytest.raises(ValueError, match="^qc_plant_step_adjoint_batch:"):
        odd.plant_step_adjoint({k: d[k][1] for k in STATE}, d["grf_body"][1], d["foot_world"][1], dt, {"x": bd["x"][1]}, want=("x_bar",))
    odd.close()
    # the Python wrapper checks shapes, dtypes and names before it calls
    state = {k: d[k][1] for k in STATE}
    with pytest.raises(ValueError, match="grf_body"):
        ctl.plant_step_adjoint(state, d["grf_body"][1][:, :6].contiguous(), d["foot_world"][1], dt, {"x": bd["x"][1]})
    with pytest.raises(ValueError, match=r"cotangents\['x'\]"):
        ctl.plant_step_adjoint(state, d["grf_body"][1], d["foot_world"][1], dt, {"x": bd["x"][1].float()})
    with pytest.raises(ValueError, match="unknown cotangent"):
        ctl.plant_step_adjoint(state, d["grf_body"][1], d["foot_world"][1], dt, {"grf_body": bd["feet"][1]})
    with pytest.raises(ValueError, match="unknown output"):
        ctl.plant_step_adjoint(state, d["grf_body"][1], d["foot_world"][1], dt, {"x": bd["x"][1]}, want=("feet_bar",))
    with pytest.raises(ValueError, match="^qc_plant_step_adjoint_batch: no input cotangent"):
        ctl.plant_step_adjoint(state, d["grf_body"][1], d["foot_world"][1], dt, {}, want=("x_bar",), out={"x_bar": outs["x_bar"]})
    # no handle, no io, n beyond one launch, the struct_size of another struct; n == 0 launches nothing; the same structs, valid, do
    assert_raw_refusals(lib.qc_plant_step_adjoint_batch, lambda: (ctl._h, n, None, io()), "qc_plant_adjoint_io", ctypes.sizeof(_lib.QcPlantAdjointIo), 72,
                        [(t, SENTINEL, True) for t in outs.values()], beyond=0xFFFFFF * 256 + 1, stream=stream, untouched=untouched, launched=untouched)

"""GPU: the plant steps with a model (include/qc_plant_model.h, csrc/qc_plant_model.hpp, quadruped_control_amd/plant_model.py)
against the 50-digit maps of tests/plant_model_restatement.py, against the base kernels bit for bit where the model changes nothing,
against central differences of the forward kernels themselves, and through the rollouts.

Batch sizes 1, 63, 64, 65, 257 and 4097, tiling pools of 257 robots; every reference is computed once per process.  The bar against
50 digits, per output entry: 4 C_NP EPS condsum - condsum the 50-digit map's condition sum, C_NP the numpy restatement's own worst
error in that unit, measured on the CPU (tests/test_plant_model_cpu.py asserts it) and never on the device; the factor 4 is the
project's standing margin for the device's other operation order and FMA contraction.  The legged step's STANCE joints have no
condition sum: their bar is tests/leg_plant_restatement.py's, IK_BAR_MARGIN times the numpy step's largest deviation from 50 digits
over the pool's stance legs, measured on the CPU as well."""
import numpy as np
import pytest

from tests import leg_plant_restatement as LR
from tests import plant_model_restatement as MR
from tests import plant_restatement as PR
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, assert_same_bits, ctl, q  # noqa: F401

pytestmark = pytest.mark.gpu
EPS, DT = MR.EPS, MR.DT
SIZES = (1, 63, 64, 65, 257, 4097)
STATE = ("Rwb", "x", "xdot", "w")
LEG_STATE = STATE + ("joint_q", "joint_qdot")
K = {call: {k: 4.0 * v for k, v in c.items()} for call, c in MR.C_NP.items()}  # C_NP is measured on the CPU, never taken from the device
WIDTH = {"Rwb_bar": 9, "grf_bar": 12, "foot_world_bar": 12, "wrench_bar": 6, "mass_bar": 1, "Ib_bar": 9}


@pytest.fixture(scope="module")
def pm(q):
    return q.plant_model


def _model(host, n, flags=True):
    """device arrays of a model's host arrays (tiled, sentinel rows behind) and the dict the module takes"""
    d = _device_arrays({k: (v if v.ndim > 1 else v.reshape(-1, 1)) for k, v in host.items()}, n)
    model = {k: (v[1].reshape(n) if k == "mass" else v[1]) for k, v in d.items()}
    if flags:
        d["flags"] = _device_arrays({"flags": np.zeros((1, 1), np.int32)}, n)["flags"]
        model["flags"] = d["flags"][1].reshape(n)
    return d, model


def _step(pm, ctl, s, n, host_model, base=False):
    import torch

    d = _device_arrays(s, n)
    feet = _device_arrays({"feet": np.full((1, 12), SENTINEL)}, n)["feet"]
    md, model = _model(host_model, n)
    state = {k: d[k][1] for k in STATE}
    if base:
        ctl.plant_step(state, d["grf_body"][1], d["foot_world"][1], DT, feet=feet[1])
    else:
        pm.plant_step(ctl, state, d["grf_body"][1], d["foot_world"][1], DT, model, feet=feet[1])
    torch.cuda.synchronize()
    out = {k: v[0].cpu().numpy() for k, v in d.items()}
    out["feet"] = feet[0].cpu().numpy()
    return out, {k: v[0].cpu().numpy() for k, v in md.items()}


def _leg_step(pm, ctl, s, n, host_model, base=False):
    import torch

    d = _device_arrays(s, n)
    extra = _device_arrays({"foot_world": np.full((1, 12), SENTINEL), "leg_flags": np.full((1, 1), -77, np.int32)}, n)
    md, model = _model(host_model, n)
    state = {k: d[k][1] for k in LEG_STATE}
    kw = dict(gait_phase=d["gait_phase"][1], foot_world=extra["foot_world"][1], flags=extra["leg_flags"][1].reshape(n))
    if base:
        ctl.leg_plant_step(state, d["joint_tau"][1], DT, MR.LEG_INERTIA, **kw)
    else:
        pm.leg_plant_step(ctl, state, d["joint_tau"][1], DT, MR.LEG_INERTIA, model, **kw)
    torch.cuda.synchronize()
    out = {k: v[0].cpu().numpy() for k, v in list(d.items()) + list(extra.items())}
    return out, {k: v[0].cpu().numpy() for k, v in md.items()}


def _adjoint(pm, ctl, s, bars, n, host_model, want=MR.ADJOINT_OUTPUTS, alias=None, base=False):
    """One adjoint call; alias = (output, cotangent): that output is written over that cotangent.  Returns ({output: host [n + 2, k]},
    everything else after the call)."""
    import torch

    d, b = _device_arrays(s, n), _device_arrays(bars, n)
    outs = _device_arrays({k: np.full((1, WIDTH.get(k, 3)), SENTINEL) for k in want}, n)
    out = {k: (v[1].reshape(n) if k == "mass_bar" else v[1]) for k, v in outs.items()}
    if alias is not None:
        out[alias[0]] = b[alias[1]][1]
    md, model = _model(host_model, n, flags=False)
    state, cot = {k: d[k][1] for k in STATE}, {k: v[1] for k, v in b.items()}
    if base:
        ctl.plant_step_adjoint(state, d["grf_body"][1], d["foot_world"][1], DT, cot, want=tuple(want), out=out)
    else:
        pm.plant_step_adjoint(ctl, state, d["grf_body"][1], d["foot_world"][1], DT, model, cot, want=tuple(want), out=out)
    torch.cuda.synchronize()
    res = {k: (b[alias[1]][0] if alias is not None and k == alias[0] else outs[k][0]).cpu().numpy() for k in want}
    rest = {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{"bar_" + k: v[0].cpu().numpy() for k, v in b.items()},
            **{"model_" + k: v[0].cpu().numpy() for k, v in md.items()}}
    return res, rest


def _worst(got, ref, names, n):
    worst = {}
    for k in names:
        val, cond = _tile(ref[k][0].reshape(MR.POOL, -1), n), _tile(ref[k][1].reshape(MR.POOL, -1), n)
        err = np.abs(got[k][:n].reshape(n, -1) - val)
        exact, free = cond == 0, np.isnan(cond)
        assert (err[exact] == 0).all(), k
        use = ~exact & ~free
        worst[k] = float(np.max(err[use] / (EPS * cond[use]), initial=0.0))
        assert (got[k][n:] == SENTINEL).all(), k
    return worst


# ------------------------------------------------------------------ 1. against 50 digits
@pytest.mark.parametrize("combo", MR.COMBOS, ids=lambda c: "".join(n for n, t in zip("MIW", c) if t))
def test_every_output_against_50_digits(pm, ctl, P, combo):
    """Every output of the three calls within 4 C_NP EPS condsum of the 50-digit maps on the same doubles, at every batch size, for
    this combination of present and absent mass / Ib / wrench (every instantiation).  Measured on the device (worst error / (EPS
    condsum) over the sizes and the combinations): profiles/plant_model.md has the figures."""
    s, bars, model = MR.pool()
    ls, mask, lmodel = MR.leg_pool()
    ref, aref, lref = MR.step_reference(combo), MR.adjoint_reference(combo), MR.leg_reference(combo)
    host, lhost = MR.select(model, combo), MR.select(lmodel, combo)
    np_leg = MR.leg_plant_step_model_np(P, ls, mask, MR.LEG_INERTIA, DT, **lhost)
    ik_bar = LR.stance_ik_bars(np_leg, {k: lref[k][0].reshape(MR.POOL, 12) for k in ("joint_q", "joint_qdot")}, mask)
    sel = np.repeat(mask, 3, axis=1)
    for n in SIZES:
        got, after = _step(pm, ctl, s, n, host)
        w = _worst(got, ref, MR.STEP_OUTPUTS, n)
        print(f"{combo} n {n}: step, worst error / (EPS condsum) {w}")
        assert all(w[k] <= K["step"][k] for k in w), (n, w)
        assert not after["flags"][:n].any() and (after["flags"][n:] == -77).all()
        got, _ = _adjoint(pm, ctl, s, bars, n, host)
        w = _worst(got, aref, MR.ADJOINT_OUTPUTS, n)
        print(f"{combo} n {n}: adjoint, worst error / (EPS condsum) {w}")
        assert all(w[k] <= K["adjoint"][k] for k in w), (n, w)
        got, after = _leg_step(pm, ctl, ls, n, lhost)
        assert not got["leg_flags"][:n].any() and not after["flags"][:n].any()
        w = _worst(got, lref, MR.LEG_OUTPUTS, n)
        stance = {k: float(np.abs(got[k][:n] - _tile(lref[k][0].reshape(MR.POOL, 12), n))[_tile(sel, n)].max()) / ik_bar[k] for k in ik_bar}
        print(f"{combo} n {n}: leg, worst error / (EPS condsum) {w}, stance joints' error / their measured bar {stance}")
        assert all(w[k] <= K["leg"][k] for k in w), (n, w)
        assert all(v <= 1.0 for v in stance.values()), (n, stance)


# ------------------------------------------------------------------ 2. bit identities
@pytest.mark.parametrize("n", (1, 65, 257, 4097))
def test_a_zero_wrench_is_the_base_kernel_bit_for_bit(pm, ctl, n):
    """A wrench array of +0.0 alone: both plants' results, and - with bar = NULL - the base adjoint's six outputs, bit for bit."""
    s, bars, _ = MR.pool()
    ls, _, _ = MR.leg_pool()
    zero = {"wrench": np.zeros((MR.POOL, 6))}
    got, base = _step(pm, ctl, s, n, zero)[0], _step(pm, ctl, s, n, zero, base=True)[0]
    for k in got:
        assert np.array_equal(got[k].view(np.int64), base[k].view(np.int64)), k
    got, base = _leg_step(pm, ctl, ls, n, zero)[0], _leg_step(pm, ctl, ls, n, zero, base=True)[0]
    for k in got:
        assert np.array_equal(got[k].view(got[k].dtype if got[k].dtype != np.float64 else np.int64), base[k].view(got[k].dtype if got[k].dtype != np.float64 else np.int64)), k
    got, base = _adjoint(pm, ctl, s, bars, n, zero, want=MR.PA.OUTPUTS)[0], _adjoint(pm, ctl, s, bars, n, zero, want=MR.PA.OUTPUTS, base=True)[0]
    for k in got:
        assert np.array_equal(got[k].view(np.int64), base[k].view(np.int64)), k


def test_rollout_twins_equal_the_originals_bit_for_bit(pm, q, P):
    """pm.rollout / pm.rollout_tick with a +0.0 wrench and neither mass nor Ib against ctl.rollout / ctl.rollout_tick: bit-equal states
    after 3 steps, the same history; a [steps, n, 6] schedule of identical slices equals the held [n, 6]."""
    import torch

    n, H = 130, 3
    ctl = q.BalanceController.from_params(P, device=0)
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    zero = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    s0, o0 = ctl.rollout(q.to_device(b), pwd.clone(), H, DT, record_every=1, certify_every=2)
    s1, o1 = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": zero}, record_every=1, certify_every=2)
    for k in s0:
        assert_same_bits(s1[k], s0[k], k)
    assert_same_bits(o1["grf_body"], o0["grf_body"], "grf_body")
    assert torch.equal(o1["active_set"], o0["active_set"]) and not o1["model_flags"].any()
    assert len(o1["history"]) == len(o0["history"]) == H and len(o1["certificates"]) == len(o0["certificates"]) == 2
    for (k0, h0), (k1, h1) in zip(o0["history"], o1["history"]):
        assert k0 == k1 and all(torch.equal(h0[name], h1[name]) for name in h0)
    # a schedule of identical slices
    rng = np.random.default_rng(0xB0D5)
    push = torch.from_numpy(rng.uniform(-20.0, 20.0, (n, 6))).cuda()
    held, _ = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": push})
    sched, _ = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": push.unsqueeze(0).repeat(H, 1, 1).contiguous()})
    for k in held:
        assert_same_bits(sched[k], held[k], k)
        assert not torch.equal(held[k], s0[k]), k
    with pytest.raises(ValueError, match="one \\[n,6\\] slice per step"):
        pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": push.unsqueeze(0).repeat(H + 1, 1, 1).contiguous()})
    # around the tick
    start = LR.make_pool(n, 0xB0D6)
    desired = {k: b[k] for k in ("Rwb_d", "x_d", "xdot_d", "w_d")}
    tick = dict({k: start[k] for k in LEG_STATE}, **desired)
    t0, u0 = ctl.rollout_tick(q.to_device(tick), None, H, DT, MR.LEG_INERTIA)
    t1, u1 = pm.rollout_tick(ctl, q.to_device(tick), None, H, DT, MR.LEG_INERTIA, {"wrench": zero})
    for k in t0:
        assert_same_bits(t1[k], t0[k], k)
    assert torch.equal(u1["flags"], u0["flags"]) and torch.equal(u1["foot_world"], u0["foot_world"]) and not u1["model_flags"].any()
    held, _ = pm.rollout_tick(ctl, q.to_device(tick), None, H, DT, MR.LEG_INERTIA, {"wrench": push})
    sched, _ = pm.rollout_tick(ctl, q.to_device(tick), None, H, DT, MR.LEG_INERTIA, {"wrench": push.unsqueeze(0).repeat(H, 1, 1).contiguous()})
    for k in held:
        assert_same_bits(sched[k], held[k], k)
    assert not torch.equal(held["xdot"], t0["xdot"])
    ctl.close()


# ------------------------------------------------------------------ 3. rows and aliasing
@pytest.mark.parametrize("n", (1, 65, 257, 4097))
def test_only_its_own_rows_and_in_place(pm, ctl, n):
    """Sentinel rows behind row n - 1 are untouched in every array of the three calls, no input is written, and an adjoint output over
    an input cotangent of its layout equals the separate-array result bit for bit."""
    s, bars, model = MR.pool()
    ls, _, lmodel = MR.leg_pool()
    got, after = _step(pm, ctl, s, n, model)
    for k, a in list(got.items()) + list(after.items()):
        assert (a[n:] == (SENTINEL if a.dtype == np.float64 else -77)).all(), k
    for k in ("grf_body", "foot_world"):
        assert np.array_equal(got[k][:n], _tile(s[k], n)), k
    for k in ("mass", "Ib", "wrench"):
        assert np.array_equal(after[k][:n].reshape(n, -1), _tile(model[k].reshape(MR.POOL, -1), n)), k
    got, after = _leg_step(pm, ctl, ls, n, lmodel)
    for k, a in list(got.items()) + list(after.items()):
        assert (a[n:] == (SENTINEL if a.dtype == np.float64 else -77)).all(), k
    for k in ("joint_tau", "gait_phase"):
        assert np.array_equal(got[k][:n], _tile(ls[k], n)), k
    for k in ("mass", "Ib", "wrench"):
        assert np.array_equal(after[k][:n].reshape(n, -1), _tile(lmodel[k].reshape(MR.POOL, -1), n)), k
    own, after = _adjoint(pm, ctl, s, bars, n, model)
    for k, a in list(own.items()) + list(after.items()):
        assert (a[n:] == SENTINEL).all(), k
    for k in MR.PA.INPUTS:
        assert np.array_equal(after[k][:n], _tile(s[k], n)), k
    for k in MR.PA.COTANGENTS:
        assert np.array_equal(after["bar_" + k][:n], _tile(bars[k], n)), k
    for k in ("mass", "Ib", "wrench"):
        assert np.array_equal(after["model_" + k][:n].reshape(n, -1), _tile(model[k].reshape(MR.POOL, -1), n)), k
    assert all((own[k][:n] != SENTINEL).all() for k in MR.ADJOINT_OUTPUTS)
    for alias in (("Ib_bar", "Rwb"), ("Rwb_bar", "Rwb"), ("x_bar", "x"), ("w_bar", "xdot"), ("grf_bar", "feet"), ("foot_world_bar", "feet")):
        got, after = _adjoint(pm, ctl, s, bars, n, model, alias=alias)
        for k in MR.ADJOINT_OUTPUTS:
            assert np.array_equal(got[k], own[k]), (alias, k)
        for k in MR.PA.INPUTS:
            assert np.array_equal(after[k][:n], _tile(s[k], n)), (alias, k)


# ------------------------------------------------------------------ 4. flags
def test_flagged_robots_are_nan_and_their_neighbours_untouched(pm, ctl):
    """Bit 0 for a mass of 0, negative or NaN, bit 1 for an indefinite, asymmetric or NaN Ib: every state output of those robots is
    NaN in all three calls, every other robot is bit-equal to a run without them.  (Ordinary inputs with defined results.)"""
    n = 257
    s, bars, model = MR.pool()
    ls, _, lmodel = MR.leg_pool()
    nan = float("nan")
    bad_mass = {3: 0.0, 64: -1.5, 100: nan, 256: 0.0}
    bad_Ib = {5: np.diag([1.0, -1.0, 1.0]).reshape(9), 64: np.array([1, 2, 0, 2, 1, 0, 0, 0, 1.0]), 65: np.array([1, 0, 0, 0, 1, 0.25, 0, 0, 1.0]),
              200: np.array([1, 0, 0, 0, nan, 0, 0, 0, 1.0]), 255: np.zeros(9)}
    want = np.zeros(n, np.int32)
    for i in bad_mass:
        want[i] |= 1
    for i in bad_Ib:
        want[i] |= 2

    def spoiled(m):
        m = {k: np.array(v) for k, v in m.items()}
        for i, v in bad_mass.items():
            m["mass"][i] = v
        for i, v in bad_Ib.items():
            m["Ib"][i] = v
        return m

    good = want == 0
    clean, _ = _step(pm, ctl, s, n, model)
    got, after = _step(pm, ctl, s, n, spoiled(model))
    assert np.array_equal(after["flags"][:n, 0], want)
    for k in MR.STEP_OUTPUTS:
        assert np.isnan(got[k][:n][~good]).all(), k
        assert np.array_equal(got[k][:n][good], clean[k][:n][good]), k
    clean, _ = _leg_step(pm, ctl, ls, n, lmodel)
    got, after = _leg_step(pm, ctl, ls, n, spoiled(lmodel))
    assert np.array_equal(after["flags"][:n, 0], want)
    for k in LEG_STATE:
        assert np.isnan(got[k][:n][~good]).all(), k
        assert np.array_equal(got[k][:n][good], clean[k][:n][good]), k
    # the leg plant's own outputs keep their meaning: foot_world is of the state the step read, the word of a flagged robot is its IK's
    # on the NaN body
    assert np.array_equal(got["foot_world"], clean["foot_world"]) and np.array_equal(got["leg_flags"][:n][good], clean["leg_flags"][:n][good])
    want_all = MR.ADJOINT_OUTPUTS + ("flags",)
    clean, _ = _adjoint(pm, ctl, s, bars, n, model)
    import torch

    d, b = _device_arrays(s, n), _device_arrays(bars, n)
    _, m = _model(spoiled(model), n, flags=False)
    res = pm.plant_step_adjoint(ctl, {k: d[k][1] for k in STATE}, d["grf_body"][1], d["foot_world"][1], DT, m, {k: v[1] for k, v in b.items()}, want=want_all)
    torch.cuda.synchronize()
    assert np.array_equal(res["flags"].cpu().numpy(), want)
    for k in MR.ADJOINT_OUTPUTS:
        g = res[k].cpu().numpy().reshape(n, -1)
        assert np.isnan(g[~good]).all(), k
        assert np.array_equal(g[good], clean[k][:n][good]), k


# ------------------------------------------------------------------ 5. gradients against central differences
def test_step_gradient_in_wrench_mass_and_Ib(pm, ctl, P):
    """plant_step_autograd's gradient in wrench, mass and Ib (along symmetric directions, plant_model_restatement.symmetric) against central differences of pm.plant_step itself, on the
    first 65 robots; the map is smooth, so no robot is left out.  The bar is tests/fd_support.py's, with this map's own references:
    |FD(h) - FD(2h)| plus the quotient's rounding - each of its two losses is <c, y> with y within 4 C_NP EPS condsum of the exact
    step, test 1's bar - over h, plus the analytic side's 4 C_NP EPS sum condsum |v|.  The forward outputs equal pm.plant_step's bit
    for bit and the gradients equal the direct adjoint call's."""
    import torch

    n, h = 65, 1e-5
    s, bars, model = ({k: a[:n] for k, a in d.items()} for d in MR.pool())
    rng = np.random.default_rng(0xB0D7)
    v = {"wrench": rng.normal(0.0, 1.0, (n, 6)), "mass": 0.1 * rng.normal(0.0, 1.0, n), "Ib": MR.symmetric(1e-4 * rng.normal(0.0, 1.0, (n, 9)))}
    dev = {k: torch.from_numpy(np.array(a)).cuda() for k, a in s.items()}
    cot = {k: torch.from_numpy(np.array(a)).cuda() for k, a in bars.items()}

    def step(k):
        m = {name: torch.from_numpy(np.ascontiguousarray(model[name] + k * h * v[name])).cuda() for name in v}
        st = {name: dev[name].clone() for name in STATE}
        feet = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        pm.plant_step(ctl, st, dev["grf_body"], dev["foot_world"], DT, m, feet=feet)
        out = dict(st, feet=feet)
        return sum((out[name] * cot[name]).sum(dim=1) for name in cot).cpu().numpy(), out

    leaves = {name: torch.from_numpy(np.array(model[name])).cuda().requires_grad_(True) for name in v}
    out = pm.plant_step_autograd(ctl, dev, dev["grf_body"], dev["foot_world"], DT, leaves)
    _, direct_out = step(0)
    for o, name in zip(out, MR.STEP_OUTPUTS):
        assert torch.equal(o.detach(), direct_out[name]), name
    grads = torch.autograd.grad(out, [leaves[name] for name in v], [cot[name] for name in MR.STEP_OUTPUTS])
    direct = pm.plant_step_adjoint(ctl, {k: dev[k] for k in STATE}, dev["grf_body"], dev["foot_world"], DT, {k: t.detach() for k, t in leaves.items()}, cot,
                                   want=("wrench_bar", "mass_bar", "Ib_bar"))
    torch.cuda.synchronize()
    g = {}
    for name, t in zip(v, grads):
        assert t.shape == leaves[name].shape and torch.equal(t, direct[name + "_bar"].view_as(t)), name
        g[name] = t.cpu().numpy().reshape(n, -1)
    fd1 = (step(1)[0] - step(-1)[0]) / (2 * h)
    fd2 = (step(2)[0] - step(-2)[0]) / (4 * h)
    an = sum((g[name] * v[name].reshape(n, -1)).sum(axis=1) for name in v)
    ref, aref = MR.step_reference((True, True, True)), MR.adjoint_reference((True, True, True))
    rounding = sum((np.abs(bars[k]) * 4.0 * MR.C_NP["step"][k] * EPS * ref[k][1][:n].reshape(n, -1)).sum(axis=1) for k in bars)
    analytic = sum((4.0 * MR.C_NP["adjoint"][name + "_bar"] * EPS * aref[name + "_bar"][1][:n].reshape(n, -1) * np.abs(v[name].reshape(n, -1))).sum(axis=1) for name in v)
    bar = np.abs(fd1 - fd2) + 2.0 * rounding / (2 * h) + analytic
    err = np.abs(fd1 - an)
    print("worst error / bar", float((err / bar).max()), "worst relative bar", float((bar / np.maximum(np.abs(an), 1e-300)).max()))
    assert np.all(err <= bar), float((err / bar).max())


def test_rollout_gradient_in_the_plants_body_and_the_first_push(pm, q, P):
    """rollout_autograd over 3 steps: the gradient of <c, final {Rwb, x, xdot, w}> in the plant's mass, Ib and the step-0 push against
    central differences of pm.rollout itself at 0, +-h, +-2h, h = 1e-4.  Forward: pm.rollout's bits.  Kept (the existing rollout tests'
    rule): solved at every step and every point and the working-set word (want_active_set) of every step the same at all five
    points; at least 0.8 of the robots (tests/test_plant_model_cpu.py holds the C oracle's faces on these inputs to the same cap).  Bar per robot: |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|, the sibling tests' rounding
    term.  With params=, the same loss also has a gradient in the controller's own mass and Ib, separate from the plant's."""
    import torch

    n, H, h = 65, 3, 1e-4
    b, pw, model = MR.standing(n)
    v = MR.rollout_directions(n)
    rng = np.random.default_rng(0xB0DA)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)
    pwd = torch.from_numpy(pw).cuda()

    def moved(k):
        m = {name: np.ascontiguousarray(model[name] + k * h * v[name]) for name in ("mass", "Ib")}
        push = model["wrench"].copy()
        push[0] += k * h * v["wrench"]
        return {name: torch.from_numpy(a).cuda() for name, a in dict(m, wrench=push).items()}

    def rollout(k):
        words, status = [], []
        for steps in range(1, H + 1):  # (the last solve of an s-step rollout is step s - 1's)
            m = moved(k)
            m["wrench"] = m["wrench"][:steps].contiguous()
            state, out = pm.rollout(ctl, q.to_device(b), pwd.clone(), steps, DT, m)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            assert not out["model_flags"].any()
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), final

    L0, w0, st0, final0 = rollout(0)
    leaves = {name: t.requires_grad_(True) for name, t in moved(0).items()}
    params = ctl.parameter_tensor().requires_grad_(True)
    state, out = pm.rollout_autograd(ctl, q.to_device(b), pwd, H, DT, leaves, params=params)
    for name in STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name
    loss = sum((state[name] * torch.from_numpy(c[name]).cuda()).sum() for name in STATE)
    loss.backward()
    torch.cuda.synchronize()
    g = {"mass": leaves["mass"].grad.cpu().numpy(), "Ib": leaves["Ib"].grad.cpu().numpy(), "wrench": leaves["wrench"].grad[0].cpu().numpy()}
    assert all(float(leaves["wrench"].grad[k].abs().max()) > 0 for k in range(H))  # every step's push has a gradient
    layout = q.unpack_param_bar(params.grad)
    assert abs(layout["mass"]) > 0 and np.abs(layout["Ib"]).max() > 0 and bool(torch.isfinite(params.grad).all())  # the controller's own, separately
    keep = (st0 == 0).all(axis=0)
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    for _, wk, stk, _ in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0)
    fd1 = (pts[1][0] - pts[-1][0]) / (2 * h)
    fd2 = (pts[2][0] - pts[-2][0]) / (4 * h)
    an = sum((g[name].reshape(n, -1) * v[name].reshape(n, -1)).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name].reshape(n, -1) ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name].reshape(n, -1) ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda a: float((a[keep] / scale[keep]).max())
    print("kept", keep.mean(), "worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    assert keep.mean() >= 0.8, keep.mean()
    assert (scale[keep] > 0).all()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    ctl.close()


# ------------------------------------------------------------------ 6. a push is felt
def test_a_push_is_felt(pm, q, P):
    """A 3-step rollout with a lateral force on every second robot: after the first step xdot differs from the unpushed rollout's by
    dt F / m - each of the two to the 50-digit bar of xdot, 4 C_NP EPS condsum, the condition sum of xdot' = xdot + dt ((F + sum f) / m
    - g e_z) bounded by |xdot'| + dt (|F| + 4 fzmax (1 + mu)) / m + dt g with the solve's own force limits - and not at all for the
    rows with a zero wrench."""
    import torch

    n, H = 130, 3
    ctl = q.BalanceController.from_params(P, device=0)
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    F = np.zeros((n, 6))
    F[0::2, 1] = 25.0
    push = torch.from_numpy(F).cuda()
    s0, o0 = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": torch.zeros_like(push)}, record_every=1)
    s1, o1 = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"wrench": push}, record_every=1)
    v0, v1 = (o["history"][1][1]["xdot"].cpu().numpy() for o in (o0, o1))  # the state before step 1: after the first step
    got = v1 - v0
    want = DT * F[:, :3] / P["mass"]
    cond = np.maximum(np.abs(v0), np.abs(v1)) + DT * (np.abs(F[:, :3]) + 4.0 * P["fzmax"] * (1.0 + P["mu"])) / P["mass"] + DT * PR.G
    assert np.all(np.abs(got - want) <= 2 * 4.0 * MR.C_NP["step"]["xdot"] * EPS * cond), float(np.abs(got - want).max())
    assert np.array_equal(v1[1::2], v0[1::2]) and np.abs(got[0::2, 1]).min() > 0
    for k in s0:  # the unpushed robots never notice their neighbours
        assert torch.equal(s1[k][1::2], s0[k][1::2]), k
    assert not torch.equal(s1["x"][0::2], s0["x"][0::2])
    ctl.close()


# ------------------------------------------------------------------ 7. refusals through the module
def test_refusals(pm, ctl):
    import torch

    n = 4
    s, _, _ = MR.pool()
    dev = {k: torch.from_numpy(np.array(a[:n])).cuda() for k, a in s.items()}
    state = {k: dev[k] for k in STATE}
    before = {k: t.clone() for k, t in dev.items()}
    with pytest.raises(ValueError, match="qc_plant_step_model_batch: the model gives neither mass, Ib nor wrench_world - call qc_plant_step_batch"):
        pm.plant_step(ctl, state, dev["grf_body"], dev["foot_world"], DT, {})
    with pytest.raises(ValueError, match="unknown key"):
        pm.plant_step(ctl, state, dev["grf_body"], dev["foot_world"], DT, {"inertia": dev["Rwb"]})
    with pytest.raises(ValueError, match="model\\['mass'\\]"):
        pm.plant_step(ctl, state, dev["grf_body"], dev["foot_world"], DT, {"mass": dev["x"]})
    with pytest.raises(ValueError, match="qc_plant_step_model_batch: dt must be finite and > 0"):
        pm.plant_step(ctl, state, dev["grf_body"], dev["foot_world"], 0.0, {"mass": torch.ones(n, dtype=torch.float64, device="cuda")})
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], before[k]) for k in dev)  # nothing launched


# ------------------------------------------------------------------ 8. an empty batch, the stand-in's contract, a stream of the caller's
def test_an_empty_batch_returns_as_the_controllers_calls_do(pm, q, ctl):
    """n = 0 reads no array and launches nothing: pm.plant_step, pm.leg_plant_step, pm.rollout and pm.rollout_tick return on an empty
    batch with a valid model, where ctl.plant_step and ctl.rollout return too."""
    import torch

    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    state = dict(Rwb=z(0, 9), x=z(0, 3), xdot=z(0, 3), w=z(0, 3))
    model = {"mass": z(0), "Ib": z(0, 9), "wrench": z(0, 6), "flags": z(0, dtype=torch.int32)}
    ctl.plant_step(state, z(0, 12), z(0, 12), DT)
    assert pm.plant_step(ctl, state, z(0, 12), z(0, 12), DT, model, feet=z(0, 12)) is state
    leg = dict(state, joint_q=z(0, 12), joint_qdot=z(0, 12))
    assert pm.leg_plant_step(ctl, leg, z(0, 12), DT, MR.LEG_INERTIA, model) is leg
    with pytest.raises(ValueError, match="qc_plant_step_model_batch: dt must be finite and > 0"):  # the scalars are still judged
        pm.plant_step(ctl, state, z(0, 12), z(0, 12), -1.0, model)
    desired = dict(Rwb_d=z(0, 9), x_d=z(0, 3), xdot_d=z(0, 3), w_d=z(0, 3))
    batch = dict(state, feet=z(0, 12), **desired)
    # the twins do on an empty batch what the controller's own rollouts do on it
    tick = dict(leg, **desired)
    for base, twin in ((lambda: ctl.rollout(dict(batch), z(0, 12), 2, DT), lambda: pm.rollout(ctl, dict(batch), z(0, 12), 2, DT, {"wrench": z(2, 0, 6)})),
                       (lambda: ctl.rollout_tick(dict(tick), None, 2, DT, MR.LEG_INERTIA),
                        lambda: pm.rollout_tick(ctl, dict(tick), None, 2, DT, MR.LEG_INERTIA, {"wrench": z(0, 6)}))):
        try:
            s0, _ = base()
        except (ValueError, RuntimeError) as e:
            with pytest.raises(type(e)):
                twin()
            continue
        s1, o1 = twin()
        assert set(s1) == set(s0) and all(t.numel() == 0 for t in s1.values()) and o1["model_flags"].numel() == 0


def test_the_rollout_stand_in_refuses_a_rollout_that_breaks_its_contract(pm, q, P):
    """pm.rollout runs BalanceController.rollout on a stand-in that counts the launches of ONE plan of the plant step.  A rollout that
    plans twice, launches the step twice in a step, skips a launch or sets an attribute on its controller raises RuntimeError instead
    of misindexing the push schedule."""
    import torch

    n, H = 8, 2
    ctl = q.BalanceController.from_params(P, device=0)
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    push = torch.zeros((H, n, 6), dtype=torch.float64, device="cuda")

    def stand_in():
        dev = q.to_device(b)
        state = {k: dev[k] for k in STATE}
        grf = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        return pm._ModelSteps(ctl, {"wrench": push}, H, None), (state, grf, pwd.clone(), DT, dev["feet"])

    proxy, args = stand_in()
    step = proxy.plan_plant(*args)
    with pytest.raises(RuntimeError, match="planned the plant step a second time"):
        proxy.plan_plant(*args)
    step()
    with pytest.raises(RuntimeError, match="launched the plant step 1 times in 2 steps"):
        proxy.finish()
    step()
    assert proxy.finish().shape == (n,)
    with pytest.raises(RuntimeError, match="more than once per step"):
        step()
    proxy, _ = stand_in()
    with pytest.raises(RuntimeError, match="launched the plant step None times"):
        proxy.finish()
    with pytest.raises(RuntimeError, match="set `device` on its controller"):
        proxy.device = 1
    assert proxy.device == ctl.device and proxy.kernel_name == ctl.kernel_name  # reads are the controller's own
    ctl.close()


def test_a_rollout_on_a_stream_of_the_callers(pm, q, P):
    """pm.rollout on a non-default stream: the flag word is zeroed, OR-ed and the kernels run on THAT stream - a caller's stale flags
    are gone, the states equal the default stream's bit for bit, and a refused mass is reported (in a rollout of ONE step: no solve
    is fed the NaN state behind it)."""
    import torch

    n, H = 130, 3
    ctl = q.BalanceController.from_params(P, device=0)
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    mass = torch.full((n,), float(P["mass"]), dtype=torch.float64, device="cuda")
    push = torch.from_numpy(np.random.default_rng(0xB0DB).uniform(-5.0, 5.0, (H, n, 6))).cuda()
    ref, oref = pm.rollout(ctl, q.to_device(b), pwd.clone(), H, DT, {"mass": mass, "wrench": push})
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    flags = torch.full((n,), 0x7F, dtype=torch.int32, device="cuda")  # stale bits of an earlier use
    dev, feet = q.to_device(b), pwd.clone()
    torch.cuda.synchronize()
    got, out = pm.rollout(ctl, dev, feet, H, DT, {"mass": mass, "wrench": push, "flags": flags}, stream=side)
    side.synchronize()
    assert out["model_flags"] is flags and not flags.any() and not oref["model_flags"].any()
    for k in ref:
        assert_same_bits(got[k], ref[k], k)
    mass[7] = -1.0
    flags.fill_(0x7F)
    dev, feet, first = q.to_device(b), pwd.clone(), push[:1].contiguous()
    torch.cuda.synchronize()  # (what the default stream prepared is there before the side stream reads it)
    got, out = pm.rollout(ctl, dev, feet, 1, DT, {"mass": mass, "wrench": first, "flags": flags}, stream=side)
    side.synchronize()
    want = torch.zeros((n,), dtype=torch.int32, device="cuda")
    want[7] = 1
    assert torch.equal(flags, want) and bool(torch.isnan(got["x"][7]).all()) and bool(torch.isfinite(got["x"][:7]).all())
    ctl.close()

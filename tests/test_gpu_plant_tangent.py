"""GPU: qc_plant_step_tangent_batch against the numpy restatement (tests/plant_tangent_restatement.py), in place, with optional
outputs and NULL tangents, past its block cap, against the device's own reverse pass, and the closed loop built on it -
rollout_tangent and rollout_transition (quadruped_control_amd/tangent.py).

The device's bar is 4 x the CPU-measured constants of the restatement module: every entry within 4 C_PT EPS x condition sum of
plant_tangent_np (an entry whose condition sum is 0 is exact), the dot-product identity within 4 C_PDOT EPS x the magnitudes of its
terms.  The printed worst ratios are recorded in profiles/plant_tangent.md."""
import numpy as np
import pytest

from tests import plant_adjoint_restatement as AR
from tests import plant_restatement as PR
from tests import plant_tangent_restatement as TR
from tests import tangent_restatement as QR
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, assert_same_bits, ctl, q  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = TR.EPS
DT = 1.0 / 300.0
STATE = ("Rwb", "x", "xdot", "w")
SHAPES = tuple((n, K) for n in (1, 63, 64, 65, 130) for K in (1, 3))
CAP_PAIRS = 4096 * 64  # PLANT_TANGENT_MAX_BLOCKS x PLANT_TANGENT_BLOCK (csrc/qc_plant_tangent.hpp)
# an output and the input tangent of its layout it may be written over
ALIASES = (("Rwb_rot_next_tan", "Rwb_rot_tan"), ("x_next_tan", "x_tan"), ("xdot_next_tan", "xdot_tan"), ("w_next_tan", "w_tan"),
           ("feet_next_tan", "grf_tan"), ("feet_next_tan", "foot_world_tan"))


def _flat(t, K, n):
    """{name: [K * n, m]} host arrays of direction-major tangents"""
    return {k: np.ascontiguousarray(v.reshape(K * n, -1)) for k, v in t.items()}


def _tangent(ctl, s, tans, n, K, dt, want=tuple(TR.OUTPUTS), given=None, alias=(), zeros=False):
    """One call over n robots (s tiled) and K directions (tans: {name: [K, n, m]}), every array with sentinel rows behind its last
    row - robot n - 1 of the inputs, direction K - 1 of the tangents and outputs.  given: the tangents handed over (default all; the
    others NULL, or arrays of zeros with zeros=True); alias: (output, tangent) pairs written in place.  Returns ({output: host
    [K * n + 2, m]}, {array: host after the call})."""
    import torch

    from quadruped_control_amd import tangent as T

    given = tuple(tans) if given is None else given
    d = _device_arrays(s, n)
    host = {k: (v if k in given else np.zeros_like(v)) for k, v in _flat(tans, K, n).items() if k in given or zeros}
    td = _device_arrays(host, K * n)
    outs = _device_arrays({k: np.full((1, TR.OUTPUTS[k]), SENTINEL) for k in want}, K * n)
    over = dict(alias)
    out = {k: (td[over[k]][1] if k in over else outs[k][1]) for k in want}
    T.plant_step_tangent(ctl, {k: d[k][1] for k in STATE}, d["grf_body"][1], d["foot_world"][1], dt,
                         {k: v[1].reshape(K, n, -1) for k, v in td.items()}, want=tuple(want), out=out)
    torch.cuda.synchronize()
    res = {k: (td[over[k]][0] if k in over else outs[k][0]).cpu().numpy() for k in want}
    return res, {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}


def _worst(got, ref, K, n):
    worst = {}
    for k in TR.OUTPUTS:
        val, cond = ref[k][0].reshape(K * n, -1), ref[k][1].reshape(K * n, -1)
        g = got[k][:K * n]
        exact = cond == 0
        assert np.array_equal(g[exact], val[exact]) and (got[k][K * n:] == SENTINEL).all(), k
        worst[k] = float(np.where(exact, 0.0, np.abs(g - val) / np.where(exact, 1.0, EPS * cond)).max())
    return worst


# ------------------------------------------------------------------ 1. against the restatement
def test_every_output_against_the_restatement(ctl, P):
    """Every entry within 4 C_PT EPS x condition sum of plant_tangent_np: n in {1, 63, 64, 65, 130} with K in {1, 3} (the pool of
    dt = 1/300 tiled, seeded tangents; with K = 3 the pair index leaves the wave at another place than n does) and the 257-robot pool
    at each of its dt with the committed tangents."""
    cases = [(n, K, DT, {k: _tile(a, n) for k, a in AR.pool(DT)[0].items()}, TR.random_tangents(n, K, 0xAD720 + 16 * n + K)) for n, K in SHAPES]
    cases += [(AR.POOL, TR.REF_K, dt, AR.pool(dt)[0], TR.pool_tangents(dt)) for dt in AR.DTS]
    overall = {k: 0.0 for k in TR.OUTPUTS}
    for n, K, dt, s, tans in cases:
        ref = TR.plant_tangent_np(P["mass"], P["Ib"], *(s[k] for k in TR.INPUTS), dt, tans)
        got, _ = _tangent(ctl, s, tans, n, K, dt)
        worst = _worst(got, ref, K, n)
        print(f"n {n} K {K} dt {dt}: worst error / (EPS condsum) {worst}")
        for k in TR.OUTPUTS:
            overall[k] = max(overall[k], worst[k])
            assert worst[k] <= 4 * TR.C_PT[k], (n, K, dt, k, worst[k])
    print("worst over all shapes", overall)


# ------------------------------------------------------------------ 2. in place, own rows only
@pytest.mark.parametrize("n,K", ((1, 1), (65, 3), (130, 2)))
def test_in_place_and_only_its_own_rows(ctl, n, K):
    """Every allowed aliasing (ALIASES, one at a time and the rollout's five at once) gives bit for bit what separate arrays get, in
    every output; the rows behind robot n - 1 and direction K - 1 keep their sentinels; no input array is written, and no tangent but
    the aliased ones."""
    s = {k: _tile(a, n) for k, a in AR.pool(DT)[0].items()}
    tans = TR.random_tangents(n, K, 0xAD730 + n)
    flat = _flat(tans, K, n)
    own, after = _tangent(ctl, s, tans, n, K, DT)
    for k in TR.INPUTS:
        assert np.array_equal(after[k][:n], s[k]) and (after[k][n:] == SENTINEL).all(), k
    for k in TR.TANGENTS:
        assert np.array_equal(after[k][:K * n], flat[k]) and (after[k][K * n:] == SENTINEL).all(), k
    assert all((own[k][:K * n] != SENTINEL).all() and (own[k][K * n:] == SENTINEL).all() for k in TR.OUTPUTS)
    for alias in [(a,) for a in ALIASES] + [ALIASES[:5]]:
        got, after = _tangent(ctl, s, tans, n, K, DT, alias=alias)
        for k in TR.OUTPUTS:
            assert np.array_equal(got[k], own[k]), (alias, k)
        for k in TR.INPUTS:
            assert np.array_equal(after[k][:n], s[k]), (alias, k)
        for k in TR.TANGENTS:
            if k not in dict(alias).values():
                assert np.array_equal(after[k][:K * n], flat[k]) and (after[k][K * n:] == SENTINEL).all(), (alias, k)


# ------------------------------------------------------------------ 3. optional outputs, NULL tangents
def test_subsets_of_outputs_and_null_tangents(ctl):
    """Any subset of the outputs: the full call's bits.  A NULL tangent: bit for bit what an array of zeros gives, and not the full call's."""
    n, K = 65, 3
    s = {k: _tile(a, n) for k, a in AR.pool(DT)[0].items()}
    tans = TR.random_tangents(n, K, 0xAD740)
    full, _ = _tangent(ctl, s, tans, n, K, DT)
    for want in [(k,) for k in TR.OUTPUTS] + [("Rwb_rot_next_tan", "feet_next_tan"), ("x_next_tan", "xdot_next_tan", "w_next_tan")]:
        part, _ = _tangent(ctl, s, tans, n, K, DT, want=want)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)
    for given in [(k,) for k in TR.TANGENTS] + [("x_tan", "grf_tan"), ("Rwb_rot_tan", "w_tan", "foot_world_tan")]:
        null, _ = _tangent(ctl, s, tans, n, K, DT, given=given)
        zeros, _ = _tangent(ctl, s, tans, n, K, DT, given=given, zeros=True)
        for k in TR.OUTPUTS:
            assert np.array_equal(null[k], zeros[k]), (given, k)
        assert any(not np.array_equal(null[k], full[k]) for k in TR.OUTPUTS), given


# ------------------------------------------------------------------ 4. past the block cap
def test_past_the_block_cap(ctl):
    """One launch of n K = 4096 x 64 + 2 pairs (K = 3, n = 87382: the smallest n at K = 3 beyond the cap of 4096 one-wave workgroups, so
    the grid strides) equals bit for bit the same robots run one direction per launch, each below the cap."""
    import torch

    from quadruped_control_amd import tangent as T

    K, n = 3, CAP_PAIRS // 3 + 1
    assert (n - 1) * K <= CAP_PAIRS < n * K and n <= CAP_PAIRS
    s = {k: torch.from_numpy(_tile(a, n)).cuda() for k, a in AR.pool(DT)[0].items()}
    g = torch.Generator(device="cuda").manual_seed(0xAD750)
    tans = {k: torch.randn((K, n, m), generator=g, dtype=torch.float64, device="cuda") for k, m in TR.TANGENTS.items()}
    state = {k: s[k] for k in STATE}
    big = T.plant_step_tangent(ctl, state, s["grf_body"], s["foot_world"], DT, tans)
    for d in range(K):
        one = T.plant_step_tangent(ctl, state, s["grf_body"], s["foot_world"], DT, {k: v[d:d + 1].contiguous() for k, v in tans.items()})
        for k in TR.OUTPUTS:
            assert_same_bits(big[k][d], one[k][0], f"{k}, direction {d}")
    assert all(bool(torch.isfinite(v).all()) and bool((v != 0).any()) for v in big.values())


# ------------------------------------------------------------------ 5. against the device's own reverse pass
@pytest.mark.parametrize("dt", AR.DTS)
def test_dot_product_against_the_device_adjoint(ctl, P, dt):
    """sum <out_bar, out_tan> = sum <in_bar, in_tan> between this kernel and ctl.plant_step_adjoint on the pool, with the pool's
    cotangents: the gap within 4 C_PDOT EPS x the sum of the magnitudes of all terms, the CPU measure's scale."""
    import torch

    from quadruped_control_amd import tangent as T

    s, bars = AR.pool(dt)
    tans = TR.pool_tangents(dt)
    d = {k: torch.from_numpy(np.array(a)).cuda() for k, a in s.items()}
    state = {k: d[k] for k in STATE}
    out = T.plant_step_tangent(ctl, state, d["grf_body"], d["foot_world"], dt, {k: torch.from_numpy(np.array(v)).cuda() for k, v in tans.items()})
    adj = ctl.plant_step_adjoint(state, d["grf_body"], d["foot_world"], dt, {k: torch.from_numpy(np.array(v)).cuda() for k, v in bars.items()})
    nxt = {k: v.clone() for k, v in state.items()}
    ctl.plant_step(nxt, d["grf_body"], d["foot_world"], dt)
    torch.cuda.synchronize()
    out, adj = {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in adj.items()}
    worst = 0.0
    for k in range(TR.REF_K):
        lhs, rhs, mag = TR.dot_sides(s, nxt["Rwb"].cpu().numpy(), bars, adj, tans, out, k)
        worst = max(worst, float((np.abs(lhs - rhs) / (EPS * mag)).max()))
    print(f"dt {dt}: worst dot-product gap / (EPS magnitudes) {worst}")
    assert worst <= 4 * TR.C_PDOT, worst


# ------------------------------------------------------------------ 6. rollout_tangent
def test_rollout_tangent_state_is_the_rollouts(q, ctl):
    """(a) n = 65, H = 8: the state rollout_tangent leaves equals ctl.rollout's bit for bit, feet included, and so do the last forces."""
    import torch

    from quadruped_control_amd import tangent as T

    n, H = 65, 8
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    ref, mine = q.to_device(b), q.to_device(b)
    _, out = ctl.rollout(ref, pwd, steps=H, dt=DT)
    tans = {k: torch.from_numpy(v).cuda() for k, v in TR.random_tangents(n, 2, 0xAD760, names=("x_tan", "w_tan", "Rwb_rot_tan")).items()}
    before = {k: v.clone() for k, v in tans.items()}
    state, res = T.rollout_tangent(ctl, mine, pwd, H, DT, tans)
    for k in STATE + ("feet",):
        assert_same_bits(mine[k], ref[k], k)
    assert all(state[k] is mine[k] for k in STATE) and all(torch.equal(tans[k], before[k]) for k in tans)
    assert res["x_tan"].shape == (2, n, 3) and res["feet_tan"].shape == (2, n, 4, 3) and res["flags"].shape == (n,) and res["flags"].dtype == torch.int32
    assert all(bool(torch.isfinite(res[k]).all()) and bool((res[k] != 0).any()) for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "feet_tan", "grf_tan"))
    with pytest.raises(ValueError, match="rollout: the plant is a single rigid body"):
        T.rollout_tangent(ctl, dict(mine, joint_q=mine["feet"]), pwd, H, DT, tans)


def _reduced_cond(ctl, b, state):
    """the reduced condition number of the solve at `state` (device tensors) of the host batch b, per robot, on the CPU"""
    import quadruped_control_amd as qq

    held = dict(qq.to_device(b), **state)
    grf = ctl.control_batch(held)["grf_body"].cpu().numpy()
    host = dict(b, **{k: t.cpu().numpy() for k, t in state.items()})
    return QR.tangent(qq.cheetah_params(), host, grf, {"x_tan": np.zeros((1, b["x"].shape[0], 3))})["cond"]


def _closed_loop_step_sums(ctl, b, state, pw, tans, sums):
    """One closed-loop step's forward mode restated on the CPU at `state` (device tensors) of the host batch b: tangent_restatement
    for the solve, plant_tangent_np for the plant.  tans / sums: {Rwb_rot_tan, x_tan, xdot_tan, w_tan, feet_tan: [K, n, m]} the input
    tangents and the condition sums they come with.  Returns {the same names: (values, condition sums)} after the step; the solve's
    condition sum is tangent_restatement's grf_sum evaluated on `sums` (it takes magnitudes only)."""
    import quadruped_control_amd as qq

    P = qq.cheetah_params()
    n = b["x"].shape[0]
    held = dict(qq.to_device(b), **state)
    grf = ctl.control_batch(held)["grf_body"].cpu().numpy()
    host = dict(b, **{k: t.cpu().numpy() for k, t in state.items()})
    K = tans["x_tan"].shape[0]
    flat = lambda d: {k: np.ascontiguousarray(np.asarray(v).reshape(K, n, -1)) for k, v in d.items()}
    tans, sums = flat(tans), flat(sums)
    grf_tan = QR.tangent(P, host, grf, tans)["grf_tan"].reshape(K, n, 12)
    grf_sum = QR.tangent(P, host, grf, sums)["grf_sum"].reshape(K, n, 12)
    keys = ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan")
    out = TR.plant_tangent_np(P["mass"], P["Ib"], *(host[k] for k in STATE), grf, pw, DT, dict({k: tans[k] for k in keys}, grf_tan=grf_tan),
                              tan_sums=dict({k: sums[k] for k in keys}, grf_tan=grf_sum))
    return {k[:-9] + "_tan": out[k] for k in TR.OUTPUTS}


def _pair(bars, R, tan):
    """(sum, sum of magnitudes) per robot of <bars, tangents> at one interface of the rollout: bars {Rwb (entrywise), x, xdot, w, feet}
    numpy or None, R [n, 9] the state's rotation, tan {Rwb_rot_tan, x_tan, xdot_tan, w_tan, feet_tan} numpy [n, m]"""
    n = R.shape[0]
    dR = (TR.hat(tan["Rwb_rot_tan"].reshape(n, 3)) @ R.reshape(n, 3, 3)).reshape(n, 9)
    total, mag = np.zeros(n), np.zeros(n)
    for name, t in (("Rwb", dR), ("x", tan["x_tan"]), ("xdot", tan["xdot_tan"]), ("w", tan["w_tan"]), ("feet", tan["feet_tan"])):
        if bars.get(name) is not None:
            prod = bars[name].reshape(n, -1) * t.reshape(n, -1)
            total += prod.sum(axis=1)
            mag += np.abs(prod).sum(axis=1)
    return total, mag


def test_rollout_tangent_against_reverse_mode_and_differences(q, P):
    """(b), (c) on the inputs of tests/test_gpu_plant_adjoint.py's rollout test: rollout_start(65), H = 3, dt = 1/300, the loss
    <c, final {Rwb, x, xdot, w}> and the start directions v in (x, xdot, w) from seed 0xAD704, race = 0.
    (b) Dot product against rollout_autograd: sum <c, final tangents> (the entrywise c on Rwb paired with [delta_H]x Rwb_H) against
    sum <.grad, v>, per robot whose tangent flags are 0 over all steps.  Accumulation of the bar: the identity holds step by step
    between the interfaces s and s + 1 (s = 0 ... H - 1: the state and feet before step s), each step adding a gap of its solve and
    its plant step in units of the magnitudes on both of its sides, so
        bar = 4 C_DOT C_PDOT EPS sum_{s < H} cond_s (mag_s + mag_{s+1}),
    mag_s = sum |bar_s o tan_s| over Rwb (entrywise bar with [delta_s]x Rwb_s), x, xdot, w and feet at interface s - bar_s from
    rollout_autograd run from the recorded state s over the remaining H - s steps, tan_s from rollout_tangent over s steps - and
    cond_s the reduced condition number of solve s (tangent_restatement.tangent on the CPU), the scale of tangent_restatement.dot_gap.
    (c) Central differences of ctl.rollout along v with the existing test's kept rule (solved at every step and point, flags 0, the
    working-set word of every step the same at all five points; at least 0.75 kept) and bar: |FD(h) - FD(2h)| + 1e-5 |gradient| |v|."""
    import torch

    from quadruped_control_amd import tangent as T

    n, H, dt, h = 65, 3, DT, 1e-4
    b, pw = PR.rollout_start(n)
    rng = np.random.default_rng(0xAD704)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in ("x", "xdot", "w")}
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)
    pwd = torch.from_numpy(pw).cuda()
    cd = {k: torch.from_numpy(a).cuda() for k, a in c.items()}
    seeds = {k + "_tan": torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in v.items()}

    def rollout(k):
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status = [], []
        for steps in range(1, H + 1):
            dev = q.to_device(start)
            state, out = ctl.rollout(dev, pwd.clone(), steps=steps, dt=dt)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status)

    # the interfaces: states, tangents (forward mode over s steps) and bars (reverse mode over the remaining H - s steps)
    _, rec = ctl.rollout(q.to_device(b), pwd.clone(), steps=H, dt=dt, record_every=1)
    states = [hist for _, hist in rec["history"]]
    tan, flags = [], None
    for s in range(H + 1):
        dev = q.to_device(b)
        _, res = T.rollout_tangent(ctl, dev, pwd, s, dt, seeds)
        tan.append({k: res[k].cpu().numpy() for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "feet_tan")})
        flags = res["flags"].cpu().numpy()
        if s == H:
            states.append({k: dev[k].clone() for k in STATE + ("feet",)})
    bars, cond = [], []
    for s in range(H):
        leaf = dict(q.to_device(b), **{k: t.clone().requires_grad_(True) for k, t in states[s].items()})
        final, _ = ctl.rollout_autograd(leaf, pwd, H - s, dt)
        sum((final[k] * cd[k]).sum() for k in STATE).backward()
        bars.append({k: leaf[k].grad.cpu().numpy() for k in STATE + ("feet",)})
        cond.append(_reduced_cond(ctl, b, states[s]))
    bars.append(dict(c, feet=None))
    torch.cuda.synchronize()
    sides = [_pair(bars[s], states[s]["Rwb"].cpu().numpy(), tan[s]) for s in range(H + 1)]
    lhs, rhs = sides[H][0], sides[0][0]
    bar = 4 * QR.C_DOT * TR.C_PDOT * EPS * sum(cond[s] * (sides[s][1] + sides[s + 1][1]) for s in range(H))
    ok = flags == 0
    ratio = np.abs(lhs - rhs)[ok] / bar[ok]
    print("dot product against reverse mode: robots with flags 0", int(ok.sum()), "of", n, "worst gap / bar", float(ratio.max()),
          "worst gap / (EPS magnitudes)", float((np.abs(lhs - rhs)[ok] / (EPS * (sides[0][1] + sides[H][1])[ok])).max()))
    assert ok.mean() >= 0.75 and (np.abs(lhs[ok]) > 0).all()
    assert (ratio <= 1.0).all(), float(ratio.max())
    # (c) central differences of ctl.rollout
    g = {k: bars[0][k] for k in v}
    L0, w0, st0 = rollout(0)
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    keep = (st0 == 0).all(axis=0) & ok
    for Lk, wk, stk in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0)
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    scale = np.sqrt(sum((g[k] ** 2).sum(axis=1) for k in v)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in v))
    err, t = np.abs(fd1 - lhs), np.abs(fd1 - fd2)
    print("central differences: kept", keep.mean(), "worst relative error", float((err[keep] / scale[keep]).max()), "worst t", float((t[keep] / scale[keep]).max()))
    assert keep.mean() >= 0.75, keep.mean()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    ctl.close()


def test_rollout_tangent_memory_does_not_grow_with_steps(q, ctl):
    """(d) torch.cuda.max_memory_allocated over rollout_tangent (through rollout_transition, K = 12) at H = 4 and H = 64: the two calls
    make the same tensors, so the peaks are EQUAL - one [n] int32 tensor kept per step would show.  Over rollout_autograd the peak
    grows with H: with x, xdot and w as leaves it keeps at least 300 B per robot and step (336 B measured; its docstring's 0.6 kB is
    with every input a leaf)."""
    import torch

    from quadruped_control_amd import tangent as T

    n, K = 256, 12
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()

    def peak(run, H):
        dev = q.to_device(b)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = run(dev, H)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del keep
        return top

    fwd = lambda dev, H: T.rollout_transition(ctl, dev, pwd, H, DT)

    def rev(dev, H):
        for k in ("x", "xdot", "w"):
            dev[k].requires_grad_(True)
        return ctl.rollout_autograd(dev, pwd, H, DT)

    peak(fwd, 1), peak(rev, 1)  # (what a first call sets up once - module loads, workspaces - is not tangent memory)
    f4, f64, r4, r64 = peak(fwd, 4), peak(fwd, 64), peak(rev, 4), peak(rev, 64)
    print(f"peak bytes, n = {n}: rollout_transition (K = {K}) H = 4: {f4}, H = 64: {f64}; rollout_autograd H = 4: {r4}, H = 64: {r64}")
    assert f64 == f4, (f4, f64)
    assert r64 - r4 >= 60 * n * 300, (r4, r64)


# ------------------------------------------------------------------ 7. rollout_transition
def test_rollout_transition(q, ctl):
    """Columns bit-equal to rollout_tangent on the unit seeds (transition_seeds), all at once, chunked by 5 and one seed at a time;
    steps = 0 gives the identity; phi over H = 2 equals the product of the two one-step matrices taken along the trajectory, every
    entry within the bar of test 1 applied twice: 4 max(C_PT, C_TAN) EPS x the condition sum of the entry, where the condition sum is
    the restatements' own taken through both steps on the CPU (_closed_loop_step_sums: step 1 starts from step 0's condition sums
    instead of from magnitudes, so an entry that is a rounding residue of large terms is measured against those terms, not against
    itself), and twice that because the product carries the same sums (a condition sum is linear in the magnitudes it starts from).
    Every solve is cold, so that the one-step solves see the forces of the two-step rollout.  An entry whose bar is 0 is exact."""
    import torch

    from quadruped_control_amd import tangent as T

    n, H = 65, 2
    b, pw = PR.rollout_start(n)
    pwd = torch.from_numpy(pw).cuda()
    whole = T.rollout_transition(ctl, q.to_device(b), pwd, H, DT)
    assert whole["phi"].shape == (n, 12, 12) and whole["columns"] == list(T.TRANSITION_COLUMNS) and whole["flags"].shape == (n,)
    for chunk in (5, 1):
        dev = q.to_device(b)
        part = T.rollout_transition(ctl, dev, pwd, H, DT, chunk=chunk)
        assert_same_bits(part["phi"], whole["phi"], f"chunk {chunk}")
        assert torch.equal(part["flags"], whole["flags"])
    end = q.to_device(b)
    ctl.rollout(end, pwd, steps=H, dt=DT)
    for k in STATE + ("feet",):
        assert_same_bits(dev[k], end[k], f"{k} after a chunked transition")
    for col in (0, 4, 11):
        dev = q.to_device(b)
        _, res = T.rollout_tangent(ctl, dev, pwd, H, DT, T.transition_seeds(dev, pwd, [T.TRANSITION_COLUMNS[col]]))
        rows = torch.cat([res[k][0] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan")], dim=-1)
        assert_same_bits(whole["phi"][:, :, col].contiguous(), rows, f"column {col}")
    eye = T.rollout_transition(ctl, q.to_device(b), pwd, 0, DT)["phi"]
    assert torch.equal(eye, torch.eye(12, dtype=torch.float64, device="cuda").expand(n, 12, 12))
    dev = q.to_device(b)
    start = {k: dev[k].clone() for k in STATE + ("feet",)}
    # (every solve cold: a warm-started solve of step 1 and a cold one of the same state agree to the solver's tolerance, not bit for bit)
    whole = T.rollout_transition(ctl, q.to_device(b), pwd, H, DT, warm=False)
    one0 = T.rollout_transition(ctl, dev, pwd, 1, DT, warm=False)
    middle = {k: dev[k].clone() for k in STATE + ("feet",)}
    one1 = T.rollout_transition(ctl, dev, pwd, 1, DT, warm=False)  # (from where the first step left the batch)
    prod = one1["phi"] @ one0["phi"]
    seeds = {k: v.cpu().numpy() for k, v in T.transition_seeds(start, pwd).items()}
    first = _closed_loop_step_sums(ctl, b, start, pw, seeds, {k: np.abs(v) for k, v in seeds.items()})
    second = _closed_loop_step_sums(ctl, b, middle, pw, {k: v for k, (v, _) in first.items()}, {k: c for k, (_, c) in first.items()})
    sums = np.concatenate([second[k][1] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan")], axis=-1)  # [12 columns, n, 12 rows]
    bar = 2 * 4 * max(max(TR.C_PT.values()), QR.C_TAN) * EPS * torch.from_numpy(np.ascontiguousarray(sums.transpose(1, 2, 0))).cuda()
    ok = ((whole["flags"] | one0["flags"] | one1["flags"]) == 0)
    err = (whole["phi"] - prod).abs()
    ratio = torch.where(bar > 0, err / bar, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))[ok]
    at = int(torch.where(bar > 0, err / bar, err * float("inf")).nan_to_num(0.0).argmax())
    print("phi(2) against phi_1 phi_0: robots", int(ok.sum()), "worst error / bar", float(ratio.max()), "at (robot, row, column)", (at // 144, at % 144 // 12, at % 12),
          "phi(2)", float(whole["phi"].reshape(-1)[at]), "product", float(prod.reshape(-1)[at]), "bar", float(bar.reshape(-1)[at]))
    assert ok.float().mean() >= 0.75 and bool((ratio <= 1.0).all())


# ------------------------------------------------------------------ 8. poisoning and refusals
def test_a_nan_poisons_its_own_robot_only(ctl):
    n, K, bad = 65, 3, 17
    s = {k: _tile(a, n).copy() for k, a in AR.pool(DT)[0].items()}
    tans = TR.random_tangents(n, K, 0xAD770)
    clean, _ = _tangent(ctl, s, tans, n, K, DT)
    s["w"][bad, 1] = np.nan
    got, _ = _tangent(ctl, s, tans, n, K, DT)
    rows = np.arange(K) * n + bad
    others = np.setdiff1d(np.arange(K * n + 2), rows)
    for k in TR.OUTPUTS:
        if k not in ("x_next_tan", "xdot_next_tan"):  # (w does not reach them: they are the clean call's)
            assert np.isnan(got[k][rows]).all(), k
        assert np.array_equal(got[k][others], clean[k][others]), k


def test_refusals_raise_with_the_librarys_message(q, ctl, P):
    import torch

    from quadruped_control_amd import tangent as T

    n = 65
    s = {k: torch.from_numpy(_tile(a, n)).cuda() for k, a in AR.pool(DT)[0].items()}
    state = {k: s[k] for k in STATE}
    tans = {"x_tan": torch.ones((2, n, 3), dtype=torch.float64, device="cuda")}
    out = {"x_next_tan": torch.full((2, n, 3), SENTINEL, dtype=torch.float64, device="cuda")}
    call = lambda **kw: T.plant_step_tangent(ctl, state, s["grf_body"], s["foot_world"], kw.pop("dt", DT), kw.pop("tangents", tans), want=kw.pop("want", ("x_next_tan",)), out=kw.pop("out", out))
    for dt in (0.0, -DT, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="^qc_plant_step_tangent_batch: dt must be finite and > 0$"):
            call(dt=dt)
    with pytest.raises(ValueError, match="^qc_plant_step_tangent_batch: no tangent given"):
        call(tangents={}, out={"x_next_tan": out["x_next_tan"][:1]})  # (without a tangent K is 1)
    with pytest.raises(ValueError, match="^qc_plant_step_tangent_batch: no output requested"):
        call(want=(), out={})
    with pytest.raises(ValueError, match="unknown tangent"):
        call(tangents={"feet_tan": tans["x_tan"]})
    with pytest.raises(ValueError, match="must agree on the number of directions"):
        call(tangents=dict(tans, w_tan=torch.ones((3, n, 3), dtype=torch.float64, device="cuda")))
    bad = q.BalanceController.from_params(dict(P, Ib=np.diag([0.01, -0.03, 0.04])), device=0)
    with pytest.raises(ValueError, match="^qc_plant_step_tangent_batch: the handle's Ib is not positive definite$"):
        T.plant_step_tangent(bad, state, s["grf_body"], s["foot_world"], DT, tans, want=("x_next_tan",), out=out)
    bad.close()
    torch.cuda.synchronize()
    assert bool((out["x_next_tan"] == SENTINEL).all())  # nothing was launched
    call()
    torch.cuda.synchronize()
    assert not bool((out["x_next_tan"] == SENTINEL).any())

"""-m gpu: erf_f64 and exp_neg_sq against 50-digit mpmath (tests/support_polygon_probe.py), qc_support_polygon_batch and
qc_support_polygon_adjoint_batch against the 50-digit restatement (tests/support_polygon_restatement.py) - both input forms, body and
world mode, shared and per-robot schedule, stance bytes and the phase rule -, the reference's own test vector, the 0/0 robot, aliasing,
the chain into the kinematics adjoint, support_polygon_autograd against central differences, and the refusals; both passes on a handle
at ODD_KIN (every combination of input form, frame and schedule sharing once), and the second round of both kernels' grid stride."""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import support_polygon_restatement as SP
from tests.device_math_reference import DPS, EPS, ODD_KIN
from tests.gpu_arrays import PERIOD, SECOND_ROUND_N, UNPLANTED, second_round, sentinel_tensor
from tests.solved_batch_support import params, q  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
K_FWD, K_REV = 4.0 * SP.C_FWD, 4.0 * SP.C_REV  # the device's bars: 4 x the float64 restatement's own worst ratio (measured on the CPU)
# (input form, world, shared schedule) -> the robots the 50-digit passes are made for: every combination up to the wave boundary, two to 257
COMBOS = {("feet", False, False): 257, ("joint_q", True, True): 257, ("feet", True, True): 65, ("joint_q", False, False): 65}
# at ODD_KIN: 4 x the constants measured there (tests/test_support_polygon_cpu.py), and every combination once - the two joint_q ones of
# COMBOS, body and world frame, to 257
K_FWD_ODD, K_REV_ODD = 4.0 * SP.C_FWD_ODD, 4.0 * SP.C_REV_ODD
ODD_COMBOS = {(form, world, shared): 257 if (form, world, shared) in (("joint_q", True, True), ("joint_q", False, False)) else 65
              for form in ("feet", "joint_q") for world in (False, True) for shared in (False, True)}


@pytest.fixture(scope="module")
def ctl(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_gait(0.3, 0.3)  # duty 0.5 exactly: the draw's trot
    yield c
    c.close()


@pytest.fixture(scope="module")
def odd_ctl(q):
    """a handle of this module's own at ODD_KIN (`ctl` keeps the library's model)"""
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_kinematics(**ODD_KIN.handle_arguments())
    c.set_gait(0.3, 0.3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def handles(ctl, odd_ctl):
    return {"default": ctl, "odd": odd_ctl}


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(b, form, world, n):
    keys = (form, "gait_phase") + (("Rwb", "x") if world else ())
    return {k: np.ascontiguousarray(b[k][:n]) for k in keys}


@pytest.fixture(scope="module")
def reference():
    """the draw of 257 robots (the last 16 of every 64 from the saturating family would move with n: the last 16 of the pool are) and
    its 50-digit forward and reverse passes with every accumulator, once per combination; never changed"""
    b, sched = SP.pool(257, seed=61, saturating=16)
    # the saturating robots where every n sees some: swap them to the front of the pool (robots 0, 16, 32, ...)
    order = np.arange(257)
    for j in range(16):
        order[[16 * j, 257 - 16 + j]] = order[[257 - 16 + j, 16 * j]]
    b, sched = {k: v[order] for k, v in b.items()}, sched[order]
    rng = np.random.default_rng(67)
    bar = rng.standard_normal((257, 2))
    ins = {k + "_in": rng.standard_normal((257, SP.SIZES[k])) for k in SP.OUTPUTS}
    out = dict(b=b, sched=sched, bar=bar, ins=ins, shared=sched[3].copy())
    for (form, world, shared), n in COMBOS.items():
        bb, s = _batch(b, form, world, n), (out["shared"] if shared else sched[:n])
        fwd, fcond = SP.reference_mp(bb, s, world)
        rev, rcond, flags = SP.reference_adjoint_mp(bb, s, bar[:n], world, **{k: v[:n] for k, v in ins.items()})
        assert not flags.any() and not fwd["flags"].any()
        out[(form, world, shared)] = dict(fwd=fwd, fcond=fcond, rev=rev, rcond=rcond)
    return out


@pytest.fixture(scope="module")
def odd_reference(reference):
    """the same draw, cotangent and accumulators (the pool's feet are drawn, not derived from its joint angles: nothing to rebuild) and
    the 50-digit passes at ODD_KIN, once per combination of ODD_COMBOS; never changed"""
    c = reference
    out = {k: c[k] for k in ("b", "sched", "bar", "ins", "shared")}
    for (form, world, shared), n in ODD_COMBOS.items():
        bb, s = _batch(c["b"], form, world, n), (c["shared"] if shared else c["sched"][:n])
        fwd, fcond = SP.reference_mp(bb, s, world, kin=ODD_KIN)
        rev, rcond, flags = SP.reference_adjoint_mp(bb, s, c["bar"][:n], world, kin=ODD_KIN, **{k: v[:n] for k, v in c["ins"].items()})
        assert not flags.any() and not fwd["flags"].any()
        out[(form, world, shared)] = dict(fwd=fwd, fcond=fcond, rev=rev, rcond=rcond)
    return out


# ------------------------------------------------------------------ the two primitives
def _points(breaks):
    rng = np.random.default_rng(71)
    mag = np.exp(rng.uniform(math.log(1e-300), math.log(30.0), 4000))
    x = np.concatenate([mag, -mag, rng.uniform(-7.0, 7.0, 2000), rng.uniform(-28.0, 28.0, 1000)])
    edge = []
    for v in breaks:
        lo = hi = float(v)
        edge.append(lo)
        for _ in range(3):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            edge += [lo, hi]
    edge = np.array(edge)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1.5e-8, 3.7e-9])
    return np.concatenate([x, edge, -edge, special])


def _rel(got, ref):
    """relative errors in EPS on the points whose 50-digit value is a normal number"""
    out = []
    for g, r in zip(got, ref):
        if abs(r) >= mp.mpf(2) ** -1022:
            out.append(float(abs((mp.mpf(float(g)) - r) / r) / EPS))
    return max(out)


def test_erf_against_50_digits():
    from tests import support_polygon_probe as probe

    breaks, _ = probe.breakpoints()
    assert breaks == (0.84375, 1.25, 1.0 / 0.35, 6.0)
    x = _points(breaks)
    got = probe.erf(x)
    fin = ~np.isnan(x)
    with mp.workdps(DPS):
        ref = [mp.erf(mp.mpf(float(v))) for v in x[fin]]
        dev, libm = _rel(got[fin], ref), _rel([math.erf(float(v)) for v in x[fin]], ref)
        bar = max(4.0 * libm, 1.0)
        print(f"erf_f64: worst relative error {dev:.3f} EPS; libm's erf on the same points {libm:.3f} EPS; bar {bar:.3f}")
        assert dev <= bar
        one = np.array([float(r) in (1.0, -1.0) for r in ref])  # the 50-digit value rounds to +-1: equality
        assert np.array_equal(got[fin][one], np.array([float(r) for r in ref])[one]) and one.sum() > 100
    assert np.isnan(got[~fin]).all()
    assert np.array_equal(np.signbit(got[fin]), np.signbit(x[fin])) and np.array_equal(probe.erf(-x[fin]), -got[fin]), "odd, signed zeros kept"
    sub = np.abs(x[fin]) < 2.0 ** -1022  # results below the normal range: within one step of the subnormal grid of 2 x / sqrt(pi)
    assert sub.sum() >= 4 and all(abs(mp.mpf(float(g)) - r) <= mp.mpf(2) ** -1074 for g, r in zip(got[fin][sub], np.array(ref, dtype=object)[sub]))


def test_exp_neg_sq_against_50_digits():
    from tests import support_polygon_probe as probe

    _, zero_from = probe.breakpoints()
    x = _points((math.sqrt(zero_from), 26.0, 27.0))
    got = probe.exp_neg_sq(x)
    fin = ~np.isnan(x)
    with mp.workdps(DPS):
        ref = [mp.exp(-mp.mpf(float(v)) ** 2) for v in x[fin]]

        def split(a):  # numpy.exp(-x * x) with the exact split of the square
            s = a * a
            if not s < 745.0:
                return 0.0
            e = float(mp.mpf(a) * mp.mpf(a) - mp.mpf(s))
            return float(np.exp(-s)) * (1.0 - e)

        dev, libm = _rel(got[fin], ref), _rel([split(float(v)) for v in x[fin]], ref)
        bar = max(4.0 * libm, 1.0)
        print(f"exp_neg_sq: worst relative error {dev:.3f} EPS; numpy.exp on the exact split {libm:.3f} EPS; bar {bar:.3f}")
        assert dev <= bar
        zero = np.array([float(r) == 0.0 for r in ref])
        assert (got[fin][zero] == 0.0).all() and zero.sum() > 10
        sub = np.array([0 < r < mp.mpf(2) ** -1022 for r in ref])  # below the normal range: within one step of the subnormal grid
        assert all(abs(mp.mpf(float(g)) - r) <= mp.mpf(2) ** -1074 for g, r in zip(got[fin][sub], np.array(ref, dtype=object)[sub]))
    assert np.isnan(got[~fin]).all() and (got[np.isinf(x)] == 0.0).all() and (got[x == 0.0] == 1.0).all()


# ------------------------------------------------------------------ forward
def _forward(q, ctl, c, combo, n, want=("com_xy", "weights", "flags"), extra=None):
    import torch

    form, world, shared = combo
    dev = {k: _cuda(v) for k, v in dict(_batch(c["b"], form, world, n), **(extra or {})).items()}
    r = ctl.support_polygon_batch(dev, _cuda(c["shared"] if shared else c["sched"][:n]), world=world, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _forward_against_50_digits(q, ctl, reference, n, combos, bar):
    for combo, most in combos.items():
        if n > most:
            continue
        got, ref = _forward(q, ctl, reference, combo, n), reference[combo]
        assert not got["flags"].any()
        r = SP.worst_ratio(got["com_xy"], ref["fwd"]["com_xy"][:n], ref["fcond"]["com_xy"][:n])
        print(f"n={n} {combo} com_xy: {r:.3f} EPS x condition sum (bar {bar})")
        assert r <= bar, (combo, r)
        assert np.abs(got["weights"] - ref["fwd"]["weights"][:n]).max() <= 4 * EPS  # weights of order one: a few EPS absolute


@pytest.mark.parametrize("n", SIZES)
def test_forward_against_50_digits(q, ctl, reference, n):
    _forward_against_50_digits(q, ctl, reference, n, COMBOS, K_FWD)


@pytest.mark.parametrize("n", (65, 257))
def test_forward_at_the_odd_model(q, odd_ctl, odd_reference, n):
    """the handle at ODD_KIN against the 50-digit restatement under ODD_KIN: at n = 65 all eight combinations of (input form, frame,
    schedule sharing), at 257 joint_q in the body frame and in the world frame"""
    _forward_against_50_digits(q, odd_ctl, odd_reference, n, ODD_COMBOS, K_FWD_ODD)


def test_stance_bytes_and_the_phase_rule(q, ctl, reference):
    """stance bytes equal to the phase rule's mask: the same bits; the opposite mask: other weights, the restatement's"""
    n, combo = 65, ("feet", False, False)
    mask = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in reference["b"]["gait_phase"][:n]], np.uint8)
    by_rule, by_bytes = _forward(q, ctl, reference, combo, n), _forward(q, ctl, reference, combo, n, extra=dict(stance=mask))
    assert all(np.array_equal(by_rule[k], by_bytes[k], equal_nan=True) for k in by_rule)
    duty = _forward(q, ctl, reference, combo, n, extra=dict(gait_duty=np.full(n, SP.TROT_DUTY)))
    assert all(np.array_equal(by_rule[k], duty[k]) for k in by_rule)
    flipped = _forward(q, ctl, reference, combo, n, extra=dict(stance=1 - mask))
    ref = SP.reference_np(dict(_batch(reference["b"], "feet", False, n), stance=1 - mask), reference["sched"][:n])
    ok = ref["flags"] == 0
    assert np.array_equal(flipped["flags"], ref["flags"]) and np.abs(flipped["weights"] - ref["weights"]).max() <= 4 * EPS
    assert np.abs(flipped["com_xy"][ok] - ref["com_xy"][ok]).max() < 1e-13 and not np.array_equal(flipped["weights"], by_rule["weights"])


def _node(n=1):
    rep = lambda a: np.ascontiguousarray(np.repeat(a[None], n, 0))
    return dict(feet=rep(SP.NODE_FEET), gait_phase=rep(SP.NODE_PHASE), stance=rep(SP.NODE_STANCE))


ZERO_ROBOT = dict(gait_phase=np.array([0.2, 0.75, 0.75, 0.75]), stance=np.array([1, 0, 0, 0], np.uint8))


def test_known_vector_and_zero_over_zero(q, ctl):
    """test_node.cpp:41-57 on the device, and the 0/0 robot (three swing legs, all widths 0) at lane 0 and at lane 63 of a batch of 65:
    NaN and bit 3 there, the other robots' bits untouched"""
    import torch

    b = _node(65)
    sched = np.ascontiguousarray(np.repeat(SP.NODE_SCHEDULE[None], 65, 0))
    run = lambda bb, ss: {k: v.cpu().numpy() for k, v in ctl.support_polygon_batch({k: _cuda(v) for k, v in bb.items()}, _cuda(ss),
                                                                                    want=("com_xy", "weights", "flags")).items()}
    clean = run(b, sched)
    hi, lo = SP.NODE_WEIGHTS
    assert np.allclose(clean["weights"], [hi, lo, lo, hi], rtol=4 * EPS, atol=0) and np.abs(clean["com_xy"]).max() <= 1e-17 and not clean["flags"].any()
    for lane in (0, 63):
        bb, ss = {k: v.copy() for k, v in b.items()}, sched.copy()
        bb["gait_phase"][lane], bb["stance"][lane], ss[lane] = ZERO_ROBOT["gait_phase"], ZERO_ROBOT["stance"], 0.0
        got = run(bb, ss)
        others = np.arange(65) != lane
        assert got["flags"][lane] == 1 << 3 and not got["flags"][others].any() and np.isnan(got["com_xy"][lane]).all()
        assert list(got["weights"][lane]) == [1.0, 0.0, 0.0, 0.0]
        assert all(np.array_equal(got[k][others], clean[k][others]) for k in got)
        bar = _cuda(np.ones((65, 2)))
        rev = ctl.support_polygon_adjoint_batch({k: _cuda(v) for k, v in bb.items()}, _cuda(ss), bar, want=SP.OUTPUTS + ("flags",))
        ref = ctl.support_polygon_adjoint_batch({k: _cuda(v) for k, v in b.items()}, _cuda(sched), bar, want=SP.OUTPUTS + ("flags",))
        torch.cuda.synchronize()
        for k in SP.OUTPUTS:
            g, r = rev[k].cpu().numpy().reshape(65, -1), ref[k].cpu().numpy().reshape(65, -1)
            assert np.isnan(g[lane]).all() and np.array_equal(g[others], r[others]), k
        assert rev["flags"].cpu().numpy()[lane] == 1 << 3 and not ref["flags"].cpu().numpy().any()


# ------------------------------------------------------------------ reverse
def _reverse(q, ctl, c, combo, n, out=None, ins=True):
    import torch

    form, world, shared = combo
    dev = {k: _cuda(v) for k, v in _batch(c["b"], form, world, n).items()}
    acc = {k: _cuda(v[:n]) for k, v in c["ins"].items()} if ins is True else (ins or {})
    r = ctl.support_polygon_adjoint_batch(dev, _cuda(c["shared"] if shared else c["sched"][:n]), _cuda(c["bar"][:n]), world=world,
                                          want=SP.OUTPUTS + ("flags",), out=out, **acc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().reshape(n, -1) for k, v in r.items()}


def _reverse_pass_against_50_digits(q, ctl, reference, n, combos, bar):
    for combo, most in combos.items():
        if n > most:
            continue
        got, ref = _reverse(q, ctl, reference, combo, n), reference[combo]
        assert not got["flags"].any()
        for k in SP.OUTPUTS:
            r = SP.worst_ratio(got[k], ref["rev"][k][:n], ref["rcond"][k][:n])
            print(f"n={n} {combo} {k}: {r:.3f} EPS x condition sum (bar {bar})")
            assert r <= bar, (combo, k, r)


@pytest.mark.parametrize("n", SIZES)
def test_reverse_pass_against_50_digits(q, ctl, reference, n):
    _reverse_pass_against_50_digits(q, ctl, reference, n, COMBOS, K_REV)


@pytest.mark.parametrize("n", (65, 257))
def test_reverse_pass_at_the_odd_model(q, odd_ctl, odd_reference, n):
    """the reverse pass on the handle at ODD_KIN with every accumulator, as test_forward_at_the_odd_model: in world mode Rwb_bar reads
    the body-frame feet of the model's forward kinematics again"""
    _reverse_pass_against_50_digits(q, odd_ctl, odd_reference, n, ODD_COMBOS, K_REV_ODD)


def test_outputs_over_their_accumulators(q, ctl, reference):
    """every output written over its `_in` array: the out-of-place bits"""
    import torch

    n, combo = 65, ("joint_q", True, True)
    apart = _reverse(q, ctl, reference, combo, n)
    acc = {k: _cuda(v[:n]) for k, v in reference["ins"].items()}
    shape = {"feet_bar": (n, 4, 3), "schedule_bar": (n, 4, 4)}
    out = {k: acc[k + "_in"].view(shape.get(k, (n, SP.SIZES[k]))) for k in SP.OUTPUTS}
    out["flags"] = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    over = _reverse(q, ctl, reference, combo, n, out=out, ins=acc)
    assert all(np.array_equal(apart[k], over[k]) for k in SP.OUTPUTS)


# ------------------------------------------------------------------ the second round of the grid stride
ZERO_AT, OUTSIDE = 77, (200, 201)  # the period's 0/0 robot; the two robots of the draw that are planted after the tiling


def _second_round_rows(c, names):
    """(the period, the outside robots) as device rows: the first PERIOD robots of the draw - joint_q, world mode, a schedule per robot,
    the cotangent and every accumulator - with ZERO_ROBOT at ZERO_AT; asserted to hold a 0/0 robot, stance and swing legs on every leg,
    and the saturating family"""
    rows = dict(_batch(c["b"], "joint_q", True, 257), schedule=c["sched"], com_xy_bar=c["bar"], **c["ins"])
    rows = {k: rows[k].copy() for k in names}
    rows["gait_phase"][ZERO_AT], rows["schedule"][ZERO_AT] = ZERO_ROBOT["gait_phase"], 0.0  # (the phase rule makes ZERO_ROBOT's stance bytes)
    mask = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in rows["gait_phase"][:PERIOD]])
    assert mask[ZERO_AT].tolist() == [bool(v) for v in ZERO_ROBOT["stance"]] and mask.any(axis=0).all() and (~mask).any(axis=0).all()
    assert all(rows["schedule"][16 * j].max() <= 1e-3 for j in range(9)) and (rows["schedule"][:PERIOD].min(axis=(1, 2)) >= 0.05).sum() > 100
    assert max(OUTSIDE) < 257 and min(OUTSIDE) >= PERIOD
    return {k: _cuda(v[:PERIOD]) for k, v in rows.items()}, {k: _cuda(v[list(OUTSIDE)]) for k, v in rows.items()}


def _second_round_forward(odd_ctl, reference):
    """support_polygon_kernel at n = 4096 x 64 + 65 = 262 209 robots on the handle at ODD_KIN: the grid is capped at 4096 one-wave
    workgroups, so workgroup 0 walks a full second round and workgroup 1 has one live lane and 63 tail lanes in its second.  The
    batch is the period of _second_round_rows tiled on the device, with robots 262 149 and n - 1 replaced by two robots from outside
    the period.  com_xy, weights and flags, each starting from its sentinel, equal the n = 130 launch tiled (the two replaced robots:
    an n = 2 launch of theirs) bit for bit - the 0/0 robot's NaN and bit 3 in every copy."""
    import torch

    def launch(rows, m, over=False):
        out = {"com_xy": sentinel_tensor((m, 2), torch.float64), "weights": sentinel_tensor((m, 4), torch.float64), "flags": sentinel_tensor((m,), torch.int32)}
        odd_ctl.support_polygon_batch({k: rows[k] for k in ("joint_q", "gait_phase", "Rwb", "x")}, rows["schedule"], world=True, want=tuple(out), out=out)
        return out

    assert UNPLANTED == (4096 * 64 + 5, SECOND_ROUND_N - 1)
    small = second_round(launch, *_second_round_rows(reference, ("joint_q", "gait_phase", "Rwb", "x", "schedule")))
    flags = small["flags"].cpu().numpy()
    assert flags[ZERO_AT] == 1 << 3 and np.flatnonzero(flags).tolist() == [ZERO_AT] and bool(torch.isnan(small["com_xy"][ZERO_AT]).all())
    torch.cuda.empty_cache()


def _second_round_reverse(odd_ctl, reference):
    """support_polygon_adjoint_kernel at the same n on the same tiled period, with every `_in` accumulator given (tiled too): every
    output and the flags against the n = 130 launch tiled, the two replaced robots against their n = 2 launch; then once more at this
    n with every output written over its `_in` array: the bits of the first run."""
    import torch

    shape = {"feet_bar": (4, 3), "schedule_bar": (4, 4)}

    def launch(rows, m, over=False):
        acc = {k: (rows[k].clone() if over else rows[k]) for k in SP.INS}
        out = {k: acc[k + "_in"].view((m,) + shape.get(k, (SP.SIZES[k],))) if over else sentinel_tensor((m, SP.SIZES[k]), torch.float64) for k in SP.OUTPUTS}
        out["flags"] = sentinel_tensor((m,), torch.int32)
        odd_ctl.support_polygon_adjoint_batch({k: rows[k] for k in ("joint_q", "gait_phase", "Rwb", "x")}, rows["schedule"], rows["com_xy_bar"], world=True,
                                              want=SP.OUTPUTS + ("flags",), out=out, **acc)
        return {k: v.reshape(m, -1) if v.dim() > 1 else v for k, v in out.items()}

    names = ("joint_q", "gait_phase", "Rwb", "x", "schedule", "com_xy_bar") + SP.INS
    small = second_round(launch, *_second_round_rows(reference, names), over=True)
    flags = small["flags"].cpu().numpy()
    assert flags[ZERO_AT] == 1 << 3 and np.flatnonzero(flags).tolist() == [ZERO_AT]
    assert all(bool(torch.isnan(small[k][ZERO_AT]).all()) and bool(torch.isfinite(small[k][:ZERO_AT]).all()) for k in SP.OUTPUTS)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", ["forward", "reverse"])
def test_second_round_of_the_grid_stride(q, odd_ctl, reference, kernel):
    """both kernels past their grid cap (SENSITIVITY_MAX_BLOCKS = 4096 workgroups of 64 robots): _second_round_forward, _second_round_reverse"""
    {"forward": _second_round_forward, "reverse": _second_round_reverse}[kernel](odd_ctl, reference)


@pytest.mark.parametrize("model", ["default", "odd"])
def test_feet_bar_chains_into_the_kinematics_adjoint(q, handles, reference, model):
    """world-mode feet_bar handed to sensitivity_kinematics_batch() = the joint_q gradient of support_polygon_autograd(), on the handle
    at the library's model and on the one at ODD_KIN"""
    import torch

    n, ctl = 65, handles[model]
    b = {k: _cuda(v) for k, v in _batch(reference["b"], "joint_q", True, n).items()}
    sched, bar = _cuda(reference["sched"][:n]), _cuda(reference["bar"][:n])
    s = ctl.support_polygon_adjoint_batch(b, sched, bar, world=True, want=("feet_bar",))
    by_hand = ctl.sensitivity_kinematics_batch({"joint_q": b["joint_q"]}, feet_bar=s["feet_bar"], want=("joint_q_bar",))["joint_q_bar"]
    leaf = b["joint_q"].clone().requires_grad_(True)
    com = ctl.support_polygon_autograd(dict(b, joint_q=leaf), sched, world=True)
    (com * bar).sum().backward()
    assert torch.equal(leaf.grad.reshape(n, 12), by_hand.reshape(n, 12)) and bool((leaf.grad != 0).any())


@pytest.mark.parametrize("model", ["default", "odd"])
def test_autograd_against_central_differences(q, handles, reference, model):
    """support_polygon_autograd at n = 8, world mode on joint_q: every gradient against central differences of the forward launch.
    h = 1e-6: truncation h^2 f''' / 6 ~ 1e-11 at third derivatives of order 50 (the ramps' widths are >= 0.05), rounding
    EPS |com| / h ~ 1e-10 - the bound 1e-7 max(1, |gradient|) holds both with two digits to spare.  The same on the handle at ODD_KIN
    (links and hips within a factor 1.25 of the library's: the same orders of magnitude), where the joint_q gradient of a kernel that
    took another leg's link is off by that link's share"""
    import torch

    n, ctl = 8, handles[model]
    b, sched = SP.pool(n, seed=73)
    base = {k: _cuda(v) for k, v in _batch(b, "joint_q", True, n).items()}
    bar = _cuda(np.random.default_rng(74).standard_normal((n, 2)))
    for shared in (False, True):
        s0 = _cuda(sched[2] if shared else sched)
        leaves = {k: v.clone().requires_grad_(True) for k, v in base.items()}
        sl = s0.clone().requires_grad_(True)
        (ctl.support_polygon_autograd(leaves, sl, world=True) * bar).sum().backward()
        loss = lambda bb, ss: (ctl.support_polygon_batch(bb, ss, world=True)["com_xy"] * bar).sum(1)
        h = 1e-6
        for name, leaf in list(leaves.items()) + [("schedule", sl)]:
            src = s0 if name == "schedule" else base[name]
            flat = src.reshape(-1) if (name == "schedule" and shared) else src.reshape(n, -1)
            fd = torch.zeros_like(flat)
            for j in range(flat.shape[-1]):
                up, dn = flat.clone(), flat.clone()
                up[..., j] += h
                dn[..., j] -= h
                shape = src.shape
                if name == "schedule":
                    d = (loss(base, up.reshape(shape).contiguous()) - loss(base, dn.reshape(shape).contiguous())) / (2 * h)
                else:
                    d = (loss(dict(base, **{name: up.reshape(shape).contiguous()}), s0) - loss(dict(base, **{name: dn.reshape(shape).contiguous()}), s0)) / (2 * h)
                fd[..., j] = d.sum() if flat.dim() == 1 else d
            g = leaf.grad.reshape(flat.shape)
            err = float((fd - g).abs().max())
            print(f"shared={shared} {name}: central differences within {err:.2e} (gradient up to {float(g.abs().max()):.2e})")
            assert err < 1e-7 * max(1.0, float(g.abs().max())), (name, err)
            assert bool((g != 0).any())


# ------------------------------------------------------------------ refusals
def test_refusals(q, ctl):
    import torch

    b = {k: _cuda(v) for k, v in _node(4).items()}
    sched = _cuda(SP.NODE_SCHEDULE)
    bar = _cuda(np.ones((4, 2)))
    ok = ctl.support_polygon_batch(b, sched)["com_xy"]
    torch.cuda.synchronize()
    assert float(ok.abs().max()) <= 1e-17
    ph = b["gait_phase"]
    for extra, text in ((dict(gait_dt=_cuda(np.full(4, 1e-3))), "gait_dt must be NULL"), (dict(swing_pos=_cuda(np.zeros((4, 12)))), "swing_pos and swing_vel must be NULL"),
                        (dict(swing_vel=_cuda(np.zeros((4, 12)))), "swing_pos and swing_vel must be NULL"),
                        (dict(swing_state=torch.zeros(4 * 224, dtype=torch.uint8, device="cuda:0")), "swing_state must be NULL")):
        with pytest.raises(ValueError, match="^qc_support_polygon_batch: " + text):
            ctl.support_polygon_batch(dict(b, **extra), sched)
        with pytest.raises(ValueError, match="^qc_support_polygon_adjoint_batch: " + text):
            ctl.support_polygon_adjoint_batch(dict(b, **extra), sched, bar)
    with pytest.raises(ValueError, match="^qc_support_polygon_batch: no output requested"):
        ctl.support_polygon_batch(b, sched, want=())
    with pytest.raises(ValueError, match="^qc_support_polygon_adjoint_batch: no output requested"):
        ctl.support_polygon_adjoint_batch(b, sched, bar, want=())
    with pytest.raises(ValueError, match="^qc_support_polygon_batch: schedule is required"):
        ctl.support_polygon_batch(b, None)
    with pytest.raises(ValueError, match="^qc_support_polygon_adjoint_batch: com_xy_bar is required"):
        ctl.support_polygon_adjoint_batch(b, sched, None)
    with pytest.raises(ValueError, match="^qc_support_polygon_batch: world needs Rwb and x"):
        ctl.support_polygon_batch(b, sched, world=True)
    with pytest.raises(ValueError, match="^qc_support_polygon_batch: feet or joint_q is required"):
        ctl.support_polygon_batch(dict(gait_phase=ph), sched)
    with pytest.raises(ValueError, match="^qc_support_polygon_batch: gait_phase is required"):
        ctl.support_polygon_batch(dict(feet=b["feet"]), sched)
    with pytest.raises(ValueError, match="schedule: need contiguous float64"):
        ctl.support_polygon_batch(b, _cuda(np.zeros((3, 4, 4))))
    with pytest.raises(ValueError, match="unknown output"):
        ctl.support_polygon_batch(b, sched, want=("com",))
    assert ph.cpu().numpy().tolist() == _node(4)["gait_phase"].tolist(), "gait_phase is never written"

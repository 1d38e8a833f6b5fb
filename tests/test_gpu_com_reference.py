"""-m gpu: qc_com_reference_batch and qc_com_reference_adjoint_batch on the device - the identities of the two modes with
qc_support_polygon_batch, both passes against the 50-digit restatement (tests/com_reference_restatement.py), schedule_bar_sum against
its documented order, aliasing, the 0/0 robot, the refusals, com_reference_autograd, and the `lean` keyword of the three rollouts; both
passes on a handle at ODD_KIN (every combination of input form, schedule sharing and mode once), and the second round of the grid
stride of the forward kernel in both modes and of the non-summing reverse pass."""
import numpy as np
import pytest

from tests import com_reference_restatement as CR
from tests import leg_plant_adjoint_restatement as LA
from tests import support_polygon_restatement as SP
from tests import swing_reference_restatement as SR
from tests.device_math_reference import ODD_KIN
from tests.gpu_arrays import PERIOD, SECOND_ROUND_N, UNPLANTED, second_round, sentinel_tensor
from tests.solved_batch_support import params, q  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
PAST_THE_CAP = 64 * CR.SUM_MAX_BLOCKS + 1  # the summing kernel takes its grid stride once: workgroup 0 owns robot 65 536 too
K_FWD, K_REV = 4.0 * CR.C_FWD, 4.0 * CR.C_REV  # the device's bars: 4 x the float64 restatement's own worst ratio (measured on the CPU)
GAIN = 0.7
# (input form, shared schedule, mode) -> the robots the 50-digit passes are made for
COMBOS = {("feet", False, "replace"): 257, ("joint_q", True, "offset"): 257, ("feet", True, "offset"): 65, ("joint_q", False, "replace"): 65}
# at ODD_KIN: 4 x the constants measured there (tests/test_com_reference_cpu.py), and every combination once - the two joint_q ones of
# COMBOS to 257
K_FWD_ODD, K_REV_ODD = 4.0 * CR.C_FWD_ODD, 4.0 * CR.C_REV_ODD
ODD_COMBOS = {(form, shared, mode): 257 if (form, shared, mode) in (("joint_q", True, "offset"), ("joint_q", False, "replace")) else 65
              for form in ("feet", "joint_q") for shared in (False, True) for mode in CR.MODES}
ROWS = CR.OUTPUTS + ("flags",)


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


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(b, form, n):
    return {k: np.ascontiguousarray(b[k][:n]) for k in (form, "gait_phase", "Rwb", "x")}


@pytest.fixture(scope="module")
def reference():
    """tests/test_gpu_support_polygon.py's draw of 257 robots (the saturating family at robots 0, 16, 32, ...), an x_d, a cotangent and
    every accumulator, and the 50-digit forward and reverse passes once per combination; never changed"""
    b, sched = SP.pool(257, seed=61, saturating=16)
    order = np.arange(257)
    for j in range(16):
        order[[16 * j, 257 - 16 + j]] = order[[257 - 16 + j, 16 * j]]
    b, sched = {k: v[order] for k, v in b.items()}, sched[order]
    rng = np.random.default_rng(79)
    bar, x_d = rng.standard_normal((257, 3)), rng.uniform(-1.0, 1.0, (257, 3))
    ins = {k + "_in": rng.standard_normal((257, SP.SIZES[k])) for k in SP.OUTPUTS}
    out = dict(b=b, sched=sched, bar=bar, x_d=x_d, ins=ins, shared=sched[3].copy())
    for (form, shared, mode), n in COMBOS.items():
        bb, s = _batch(b, form, n), (out["shared"] if shared else sched[:n])
        fwd, fcond = CR.reference_mp(bb, s, x_d[:n], mode, GAIN)
        rev, rcond, flags = CR.reference_adjoint_mp(bb, s, bar[:n], mode, GAIN, **{k: v[:n] for k, v in ins.items()})
        assert not flags.any() and not fwd["flags"].any()
        out[(form, shared, mode)] = dict(fwd=fwd, fcond=fcond, rev=rev, rcond=rcond)
    return out


@pytest.fixture(scope="module")
def odd_reference(reference):
    """the same draw, x_d, cotangent and accumulators (the pool's feet are drawn, not derived from its joint angles: nothing to rebuild)
    and the 50-digit passes at ODD_KIN, once per combination of ODD_COMBOS; never changed"""
    c = reference
    out = {k: c[k] for k in ("b", "sched", "bar", "x_d", "ins", "shared")}
    for (form, shared, mode), n in ODD_COMBOS.items():
        bb, s = _batch(c["b"], form, n), (c["shared"] if shared else c["sched"][:n])
        fwd, fcond = CR.reference_mp(bb, s, c["x_d"][:n], mode, GAIN, kin=ODD_KIN)
        rev, rcond, flags = CR.reference_adjoint_mp(bb, s, c["bar"][:n], mode, GAIN, kin=ODD_KIN, **{k: v[:n] for k, v in c["ins"].items()})
        assert not flags.any() and not fwd["flags"].any()
        out[(form, shared, mode)] = dict(fwd=fwd, fcond=fcond, rev=rev, rcond=rcond)
    return out


def _sched(c, shared, n):
    return _cuda(c["shared"] if shared else c["sched"][:n])


def _forward(ctl, c, combo, n, gain=GAIN, want=("x_d", "com_xy", "flags")):
    import torch

    form, shared, mode = combo
    dev = {k: _cuda(v) for k, v in _batch(c["b"], form, n).items()}
    r = ctl.com_reference_batch(dev, _sched(c, shared, n), _cuda(c["x_d"][:n]), mode, gain, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}, dev


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("n", SIZES)
def test_identities_with_the_polygon(ctl, reference, n):
    """REPLACE: x, y are support_polygon_batch(world=True)'s com_xy bit for bit, z is x_d's; OFFSET at gain 0: x_d itself - both input
    forms, shared and per-robot schedule"""
    for form in ("feet", "joint_q"):
        for shared in (False, True):
            got, dev = _forward(ctl, reference, (form, shared, "replace"), n)
            com = ctl.support_polygon_batch(dev, _sched(reference, shared, n), world=True)["com_xy"].cpu().numpy()
            assert not got["flags"].any() and np.isfinite(com).all()
            assert np.array_equal(got["x_d"][:, :2], com) and np.array_equal(got["com_xy"], com), (form, shared)
            assert np.array_equal(got["x_d"][:, 2], reference["x_d"][:n, 2])
            zero, _ = _forward(ctl, reference, (form, shared, "offset"), n, gain=0.0)
            assert np.array_equal(zero["x_d"], reference["x_d"][:n]) and np.array_equal(zero["com_xy"], com), (form, shared)
            lean, _ = _forward(ctl, reference, (form, shared, "offset"), n)
            assert not np.array_equal(lean["x_d"][:, :2], reference["x_d"][:n, :2]) and np.array_equal(lean["x_d"][:, 2], reference["x_d"][:n, 2])


def _forward_against_50_digits(ctl, reference, n, combos, bar):
    for combo, most in combos.items():
        if n > most:
            continue
        got, ref = _forward(ctl, reference, combo, n)[0], reference[combo]
        assert not got["flags"].any()
        r = SP.worst_ratio(got["x_d"], ref["fwd"]["x_d"][:n], ref["fcond"]["x_d"][:n])
        print(f"n={n} {combo} x_d: {r:.3f} EPS x condition sum (bar {bar})")
        assert r <= bar, (combo, r)


@pytest.mark.parametrize("n", SIZES)
def test_forward_against_50_digits(ctl, reference, n):
    _forward_against_50_digits(ctl, reference, n, COMBOS, K_FWD)


@pytest.mark.parametrize("n", (65, 257))
def test_forward_at_the_odd_model(odd_ctl, odd_reference, n):
    """the handle at ODD_KIN against the 50-digit restatement under ODD_KIN: at n = 65 all eight combinations of (input form, schedule
    sharing, mode), at 257 joint_q in both modes"""
    _forward_against_50_digits(odd_ctl, odd_reference, n, ODD_COMBOS, K_FWD_ODD)


# ------------------------------------------------------------------ reverse
def _reverse(ctl, c, combo, n, want=ROWS, out=None, ins=True, bar=None):
    import torch

    form, shared, mode = combo
    dev = {k: _cuda(v) for k, v in _batch(c["b"], form, n).items()}
    acc = {k: _cuda(v[:n]) for k, v in c["ins"].items()} if ins is True else (ins or {})
    r = ctl.com_reference_adjoint_batch(dev, _sched(c, shared, n), _cuda(c["bar"][:n]) if bar is None else bar, mode, GAIN, want=want, out=out, **acc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().reshape((n, -1) if k != "schedule_bar_sum" else (16,)) for k, v in r.items()}


def _reverse_pass_against_50_digits(ctl, reference, n, combos, bar):
    for combo, most in combos.items():
        if n > most:
            continue
        got, ref = _reverse(ctl, reference, combo, n), reference[combo]
        assert not got["flags"].any()
        for k in CR.OUTPUTS:
            r = SP.worst_ratio(got[k], ref["rev"][k][:n], ref["rcond"][k][:n])
            print(f"n={n} {combo} {k}: {r:.3f} EPS x condition sum (bar {bar})")
            assert r <= bar, (combo, k, r)


@pytest.mark.parametrize("n", SIZES)
def test_reverse_pass_against_50_digits(ctl, reference, n):
    _reverse_pass_against_50_digits(ctl, reference, n, COMBOS, K_REV)


@pytest.mark.parametrize("n", (65, 257))
def test_reverse_pass_at_the_odd_model(odd_ctl, odd_reference, n):
    """the reverse pass on the handle at ODD_KIN with every accumulator, as test_forward_at_the_odd_model: Rwb_bar reads the body-frame
    feet of the model's forward kinematics again"""
    _reverse_pass_against_50_digits(odd_ctl, odd_reference, n, ODD_COMBOS, K_REV_ODD)


def test_outputs_over_their_inputs(ctl, reference):
    """every output written over its `_in` array, x_d_in_bar over the cotangent, x_d_out over x_d_in: the out-of-place bits"""
    import torch

    n, combo = 65, ("joint_q", True, "offset")
    apart = _reverse(ctl, reference, combo, n)
    acc = {k: _cuda(v[:n]) for k, v in reference["ins"].items()}
    shape = {"feet_bar": (n, 4, 3), "schedule_bar": (n, 4, 4)}
    bar = _cuda(reference["bar"][:n])
    out = {k: acc[k + "_in"].view(shape.get(k, (n, SP.SIZES[k]))) for k in SP.OUTPUTS}
    out.update(x_d_in_bar=bar, flags=torch.zeros(n, dtype=torch.int32, device="cuda:0"))
    over = _reverse(ctl, reference, combo, n, out=out, ins=acc, bar=bar)
    assert all(np.array_equal(apart[k], over[k]) for k in CR.OUTPUTS)
    fwd, dev = _forward(ctl, reference, combo, n)
    x_d = _cuda(reference["x_d"][:n])
    ctl.com_reference_batch(dev, _sched(reference, True, n), x_d, "offset", GAIN, out={"x_d": x_d})
    assert np.array_equal(x_d.cpu().numpy(), fwd["x_d"])


FLAGGED_AT = 5  # the lane of the 0/0 robot in _replace_pool


def _replace_pool(c, shared):
    """the first 65 robots of the draw with the 0/0 robot of test_a_flagged_robot planted at FLAGGED_AT (three swing legs whose widths
    are 0: per robot its own block, shared a block whose swing widths are 0 for every robot); asserted to flag under the phase rule's
    mask and to hold stance and swing legs on every leg"""
    b = {k: v.copy() for k, v in c["b"].items()}
    b["gait_phase"][FLAGGED_AT] = [0.2, 0.75, 0.75, 0.75]
    if shared:
        sched = c["shared"].copy()
        sched[:, 2:] = 0.0
    else:
        sched = c["sched"][:65].copy()
        sched[FLAGGED_AT] = 0.0
    mask = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in b["gait_phase"][:65]])
    assert mask[FLAGGED_AT].tolist() == [True, False, False, False] and mask.any(axis=0).all() and (~mask).any(axis=0).all()
    return b, sched


@pytest.mark.parametrize("n", (1, 65))
def test_replace_mode_is_the_world_polygons_reverse_pass(ctl, reference, n):
    """com_reference_adjoint_batch(mode="replace") on x_d_bar = (a, b, c) against support_polygon_adjoint_batch(world=True) on com_xy_bar =
    (a, b), the same batch and schedule: feet_bar, Rwb_bar, x_bar, phase_bar, schedule_bar and flags equal bit for bit, NaNs at the same
    places, and x_d_in_bar = (0, 0, c) - NaN for a flagged robot, the kernel's documented rule ("a flagged robot gets NaN in every output
    row, x_d_in_bar's included", qc_com_reference.hpp) - both input forms, shared and per-robot schedule, with and without
    the five `_in` accumulators; n = 65 is one full wave and one tail robot.  The two kernels hold the same lines twice: this is what
    sharing them has to keep."""
    import torch

    bar = _cuda(reference["bar"][:n])
    for form in ("feet", "joint_q"):
        for shared in (False, True):
            b, sched = _replace_pool(reference, shared)
            dev, s = {k: _cuda(v) for k, v in _batch(b, form, n).items()}, _cuda(sched if shared else sched[:n])
            for ins in (False, True):
                acc = {k: _cuda(v[:n]) for k, v in reference["ins"].items()} if ins else {}
                com = ctl.com_reference_adjoint_batch(dev, s, bar, "replace", GAIN, want=ROWS, **acc)
                pol = ctl.support_polygon_adjoint_batch(dev, s, bar[:, :2].contiguous(), world=True, want=SP.OUTPUTS + ("flags",), **acc)
                torch.cuda.synchronize()
                com, pol = ({k: v.cpu().numpy().reshape(n, -1) for k, v in r.items()} for r in (com, pol))
                flagged = com["flags"][:, 0] != 0
                assert n == 1 or (np.flatnonzero(flagged).tolist() == [FLAGGED_AT] and com["flags"][FLAGGED_AT, 0] == 1 << 3), (form, shared)
                for k in SP.OUTPUTS + ("flags",):
                    assert np.array_equal(com[k], pol[k], equal_nan=k != "flags"), (form, shared, ins, k)
                    assert k == "flags" or (np.isnan(com[k]).all(axis=1) == flagged).all(), (form, shared, ins, k)
                want = reference["bar"][:n] * [0.0, 0.0, 1.0]
                assert np.array_equal(com["x_d_in_bar"][~flagged], want[~flagged]) and np.isnan(com["x_d_in_bar"][flagged]).all()


# ------------------------------------------------------------------ the second round of the grid stride
ZERO_AT, OUTSIDE = 77, (200, 201)  # the period's 0/0 robot; the two robots of the draw that are planted after the tiling
BATCH_KEYS = ("joint_q", "gait_phase", "Rwb", "x")


def _second_round_rows(c, names):
    """(the period, the outside robots) as device rows: the first PERIOD robots of the draw - joint_q, a schedule per robot, x_d, the
    cotangent and every accumulator - with the 0/0 robot of test_a_flagged_robot at ZERO_AT (the phase rule makes its stance bytes);
    asserted to hold it, stance and swing legs on every leg, and the saturating family"""
    rows = dict(_batch(c["b"], "joint_q", 257), schedule=c["sched"], x_d=c["x_d"], x_d_bar=c["bar"], **c["ins"])
    rows = {k: rows[k].copy() for k in names}
    rows["gait_phase"][ZERO_AT], rows["schedule"][ZERO_AT] = [0.2, 0.75, 0.75, 0.75], 0.0
    mask = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in rows["gait_phase"][:PERIOD]])
    assert mask[ZERO_AT].tolist() == [True, False, False, False] and mask.any(axis=0).all() and (~mask).any(axis=0).all()
    assert all(rows["schedule"][16 * j].max() <= 1e-3 for j in range(9)) and (rows["schedule"][:PERIOD].min(axis=(1, 2)) >= 0.05).sum() > 100
    assert max(OUTSIDE) < 257 and min(OUTSIDE) >= PERIOD
    return {k: _cuda(v[:PERIOD]) for k, v in rows.items()}, {k: _cuda(v[list(OUTSIDE)]) for k, v in rows.items()}


def _second_round_forward(odd_ctl, reference, mode):
    """com_reference_kernel at n = 4096 x 64 + 65 = 262 209 robots on the handle at ODD_KIN, replace mode and offset mode at gain 0.7:
    the grid is capped at 4096 one-wave workgroups, so workgroup 0 walks a full second round and workgroup 1 has one live lane and 63
    tail lanes in its second.  The batch is the period of _second_round_rows tiled on the device, with robots 262 149 and n - 1
    replaced by two robots from outside the period.  x_d, com_xy and flags, each starting from its sentinel, equal the n = 130 launch
    tiled (the two replaced robots: an n = 2 launch of theirs) bit for bit - the 0/0 robot's NaN x, y and bit 3 in every copy."""
    import torch

    def launch(rows, m, over=False):
        out = {"x_d": sentinel_tensor((m, 3), torch.float64), "com_xy": sentinel_tensor((m, 2), torch.float64), "flags": sentinel_tensor((m,), torch.int32)}
        odd_ctl.com_reference_batch({k: rows[k] for k in BATCH_KEYS}, rows["schedule"], rows["x_d"], mode, GAIN, want=tuple(out), out=out)
        return out

    assert UNPLANTED == (4096 * 64 + 5, SECOND_ROUND_N - 1) and GAIN != 1.0
    period, outside = _second_round_rows(reference, BATCH_KEYS + ("schedule", "x_d"))
    small = second_round(launch, period, outside)
    flags = small["flags"].cpu().numpy()
    assert flags[ZERO_AT] == 1 << 3 and np.flatnonzero(flags).tolist() == [ZERO_AT]
    assert bool(torch.isnan(small["x_d"][ZERO_AT, :2]).all()) and bool(small["x_d"][ZERO_AT, 2] == period["x_d"][ZERO_AT, 2])
    torch.cuda.empty_cache()


def _second_round_reverse(odd_ctl, reference, mode):
    """com_reference_adjoint_kernel (the instantiation that does not sum; test_schedule_bar_sum takes the summing one past its own cap of
    1024) at the same n on the same tiled period in offset mode, with every `_in` accumulator given (tiled too): every output and the
    flags against the n = 130 launch tiled, the two replaced robots against their n = 2 launch; then once more at this n with every
    output written over its `_in` array and x_d_in_bar over the cotangent: the bits of the first run."""
    import torch

    shape = {"feet_bar": (4, 3), "schedule_bar": (4, 4)}

    def launch(rows, m, over=False):
        acc = {k: (rows[k].clone() if over else rows[k]) for k in SP.INS}
        bar = rows["x_d_bar"].clone() if over else rows["x_d_bar"]
        out = {k: acc[k + "_in"].view((m,) + shape.get(k, (SP.SIZES[k],))) if over else sentinel_tensor((m, SP.SIZES[k]), torch.float64) for k in SP.OUTPUTS}
        out.update(x_d_in_bar=bar if over else sentinel_tensor((m, 3), torch.float64), flags=sentinel_tensor((m,), torch.int32))
        odd_ctl.com_reference_adjoint_batch({k: rows[k] for k in BATCH_KEYS}, rows["schedule"], bar, mode, GAIN, want=ROWS, out=out, **acc)
        return {k: v.reshape(m, -1) if v.dim() > 1 else v for k, v in out.items()}

    small = second_round(launch, *_second_round_rows(reference, BATCH_KEYS + ("schedule", "x_d_bar") + SP.INS), over=True)
    flags = small["flags"].cpu().numpy()
    assert flags[ZERO_AT] == 1 << 3 and np.flatnonzero(flags).tolist() == [ZERO_AT]
    assert all(bool(torch.isnan(small[k][ZERO_AT]).all()) and bool(torch.isfinite(small[k][:ZERO_AT]).all()) for k in CR.OUTPUTS)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel,mode", [("forward", "replace"), ("forward", "offset"), ("reverse", "offset")])
def test_second_round_of_the_grid_stride(odd_ctl, reference, kernel, mode):
    """both kernels past their grid cap (SENSITIVITY_MAX_BLOCKS = 4096 workgroups of 64 robots): _second_round_forward, _second_round_reverse"""
    {"forward": _second_round_forward, "reverse": _second_round_reverse}[kernel](odd_ctl, reference, mode)


# ------------------------------------------------------------------ the sum
def _tiled(c, n):
    idx = np.arange(n) % 257
    return {k: v[idx] for k, v in c["b"].items()}, c["sched"][idx], c["bar"][idx], {k: v[idx] for k, v in c["ins"].items()}


@pytest.mark.parametrize("n", SIZES + (PAST_THE_CAP,))
def test_schedule_bar_sum(ctl, reference, n):
    """two launches bit-equal; the same with and without the rows; equal to the documented order over the rows the launch returned;
    with a per-robot schedule it is the sum of the rows, nothing more"""
    import torch

    b, sched, bar, ins = _tiled(reference, n)
    dev = {k: _cuda(b[k]) for k in ("joint_q", "gait_phase", "Rwb", "x")}
    bar = _cuda(bar)
    for shared, acc in ((True, {}), (False, {"schedule_bar_in": _cuda(ins["schedule_bar_in"])})):
        s = _cuda(reference["shared"] if shared else sched)
        run = lambda want: {k: v.cpu().numpy() for k, v in ctl.com_reference_adjoint_batch(dev, s, bar, "offset", GAIN, want=want, **acc).items()}
        both, again, alone = run(("schedule_bar", "schedule_bar_sum")), run(("schedule_bar", "schedule_bar_sum")), run(("schedule_bar_sum",))
        rows_only = run(("schedule_bar",))
        torch.cuda.synchronize()
        assert np.isfinite(both["schedule_bar_sum"]).all() and (both["schedule_bar_sum"] != 0).any()  # (one robot fills its branches' widths only)
        assert np.array_equal(both["schedule_bar_sum"], again["schedule_bar_sum"]) and np.array_equal(both["schedule_bar_sum"], alone["schedule_bar_sum"])
        assert np.array_equal(both["schedule_bar"], rows_only["schedule_bar"])
        assert np.array_equal(both["schedule_bar_sum"].reshape(16), CR.ordered_sum(both["schedule_bar"])), (n, shared)


def test_a_flagged_robot(ctl, reference):
    """the 0/0 robot (three swing legs, all widths 0) at lane 0 and at lane 63 of 65: NaN x, y and bit 3 there, z kept, the others
    untouched; backwards NaN in every row of it and in the sum"""
    n = 65
    b = _batch(reference["b"], "feet", n)
    mask = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in b["gait_phase"]], np.uint8)
    x_d, bar = _cuda(reference["x_d"][:n]), _cuda(reference["bar"][:n])
    run = lambda bb, ss, mode: {k: v.cpu().numpy() for k, v in ctl.com_reference_batch({k: _cuda(v) for k, v in bb.items()}, _cuda(ss), x_d, mode, GAIN,
                                                                                        want=("x_d", "com_xy", "flags")).items()}
    rev = lambda bb, ss, mode: {k: v.cpu().numpy().reshape((n, -1) if k != "schedule_bar_sum" else (16,)) for k, v in ctl.com_reference_adjoint_batch(
        {k: _cuda(v) for k, v in bb.items()}, _cuda(ss), bar, mode, GAIN, want=ROWS + ("schedule_bar_sum",)).items()}
    for mode in CR.MODES:
        clean_b, sched = dict(b, stance=mask), reference["sched"][:n]
        clean, clean_rev = run(clean_b, sched, mode), rev(clean_b, sched, mode)
        assert not clean["flags"].any() and np.isfinite(clean_rev["schedule_bar_sum"]).all()
        for lane in (0, 63):
            bb, ss = {k: v.copy() for k, v in clean_b.items()}, sched.copy()
            bb["gait_phase"][lane], bb["stance"][lane], ss[lane] = [0.2, 0.75, 0.75, 0.75], [1, 0, 0, 0], 0.0
            got, others = run(bb, ss, mode), np.arange(n) != lane
            assert got["flags"][lane] == 1 << 3 and not got["flags"][others].any()
            assert np.isnan(got["x_d"][lane, :2]).all() and got["x_d"][lane, 2] == reference["x_d"][lane, 2] and np.isnan(got["com_xy"][lane]).all()
            assert all(np.array_equal(got[k][others], clean[k][others]) for k in got)
            back = rev(bb, ss, mode)
            for k in CR.OUTPUTS:
                assert np.isnan(back[k][lane]).all() and np.array_equal(back[k][others], clean_rev[k][others]), k
            assert back["flags"][lane] == 1 << 3 and np.isnan(back["schedule_bar_sum"]).all()


# ------------------------------------------------------------------ autograd
def test_autograd(ctl, reference):
    """a shared schedule's .grad is the direct schedule_bar_sum bit for bit (not a torch sum); every other gradient the direct call's
    rows, joint_q through the kinematics adjoint; a per-robot schedule gets the rows"""
    import torch

    n = 65
    for mode in CR.MODES:
        b = {k: _cuda(v) for k, v in _batch(reference["b"], "joint_q", n).items()}
        bar, x_d = _cuda(reference["bar"][:n]), _cuda(reference["x_d"][:n])
        for shared in (True, False):
            sched = _sched(reference, shared, n)
            direct = ctl.com_reference_adjoint_batch(b, sched, bar, mode, GAIN, want=CR.OUTPUTS + ("schedule_bar_sum",))
            q_bar = ctl.sensitivity_kinematics_batch({"joint_q": b["joint_q"]}, feet_bar=direct["feet_bar"], want=("joint_q_bar",))["joint_q_bar"]
            leaves = {k: v.clone().requires_grad_(True) for k, v in b.items()}
            sl, xl = sched.clone().requires_grad_(True), x_d.clone().requires_grad_(True)
            out = ctl.com_reference_autograd(leaves, sl, xl, mode, GAIN)
            assert torch.equal(out, ctl.com_reference_batch(b, sched, x_d, mode, GAIN)["x_d"])
            (out * bar).sum().backward()
            assert torch.equal(sl.grad, direct["schedule_bar_sum"] if shared else direct["schedule_bar"]) and bool((sl.grad != 0).all() if shared else (sl.grad != 0).any())
            assert torch.equal(xl.grad, direct["x_d_in_bar"]) and torch.equal(leaves["joint_q"].grad.reshape(n, 12), q_bar.reshape(n, 12))
            for k, name in (("Rwb", "Rwb_bar"), ("x", "x_bar"), ("gait_phase", "phase_bar")):
                assert torch.equal(leaves[k].grad, direct[name]) and bool((leaves[k].grad != 0).any()), k


# ------------------------------------------------------------------ refusals
def test_refusals(ctl, reference):
    """ValueError with the library's message, nothing launched: the outputs keep their sentinel"""
    import torch

    n = 4
    b = {k: _cuda(v) for k, v in _batch(reference["b"], "feet", n).items()}
    sched, x_d, bar = _cuda(reference["shared"]), _cuda(reference["x_d"][:n]), _cuda(reference["bar"][:n])
    sentinel = lambda *shape: torch.full(shape, -77.0, dtype=torch.float64, device="cuda:0")
    fout = {"x_d": sentinel(n, 3), "com_xy": sentinel(n, 2)}
    rout = {"x_d_in_bar": sentinel(n, 3), "feet_bar": sentinel(n, 4, 3), "schedule_bar_sum": sentinel(4, 4)}
    fwd = lambda bb, ss=sched, xx=x_d, **kw: ctl.com_reference_batch(bb, ss, xx, out=fout, want=tuple(fout), **kw)
    rev = lambda bb, ss=sched, xx=bar, **kw: ctl.com_reference_adjoint_batch(bb, ss, xx, out=rout, want=tuple(rout), **kw)
    cases = [(dict(gait_dt=_cuda(np.full(n, 1e-3))), "gait_dt must be NULL"), (dict(swing_pos=_cuda(np.zeros((n, 12)))), "swing_pos and swing_vel must be NULL"),
             (dict(swing_vel=_cuda(np.zeros((n, 12)))), "swing_pos and swing_vel must be NULL"),
             (dict(swing_state=torch.zeros(n * 224, dtype=torch.uint8, device="cuda:0")), "swing_state must be NULL")]
    for call, who in ((fwd, "qc_com_reference_batch"), (rev, "qc_com_reference_adjoint_batch")):
        for extra, text in cases:
            with pytest.raises(ValueError, match=f"^{who}: {text}"):
                call(dict(b, **extra))
        with pytest.raises(ValueError, match=f"^{who}: schedule is required"):
            call(b, None)
        with pytest.raises(ValueError, match=f"^{who}: Rwb and x are required"):
            call({k: v for k, v in b.items() if k != "x"})
        with pytest.raises(ValueError, match=f"^{who}: feet or joint_q is required"):
            call({k: v for k, v in b.items() if k != "feet"})
        with pytest.raises(ValueError, match=f"^{who}: gait_phase is required"):
            call({k: v for k, v in b.items() if k != "gait_phase"})
        with pytest.raises(ValueError, match=f"^{who}: gain must be finite"):
            call(b, mode="offset", gain=float("inf"))
        with pytest.raises(ValueError, match="mode is one of"):
            call(b, mode="lean")
    with pytest.raises(ValueError, match="^qc_com_reference_batch: x_d_in is required"):
        fwd(b, xx=None)
    with pytest.raises(ValueError, match="^qc_com_reference_adjoint_batch: x_d_out_bar is required"):
        rev(b, xx=None)
    with pytest.raises(ValueError, match="^qc_com_reference_adjoint_batch: no output requested"):
        ctl.com_reference_adjoint_batch(b, sched, bar, want=())
    with pytest.raises(ValueError, match="unknown output"):
        ctl.com_reference_batch(b, sched, x_d, want=("weights",))
    torch.cuda.synchronize()
    assert all(bool((t == -77.0).all()) for t in list(fout.values()) + list(rout.values())), "nothing was launched"
    fwd(b)
    rev(b)
    torch.cuda.synchronize()
    assert not any(bool((t == -77.0).any()) for t in list(fout.values()) + list(rout.values()))


# ------------------------------------------------------------------ the rollouts
ROLLOUT_N, ROLLOUT_STEPS, ROLLOUT_H = 65, 4, 1e-4
STATE = LA.INPUTS[:-1]
DESIRED = ("Rwb_d", "x_d", "xdot_d", "w_d")
WIDTH = 0.2  # every ramp of the lean's shared schedule at the base point


def _handle(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_tuning(race=0)  # deterministic: `iterations` cannot differ between the two paths
    c.set_kinematics(**SR.DEFAULT_MODEL.handle_arguments())
    c.set_gait(SR.DEFAULT_MODEL.t_swing, SR.DEFAULT_MODEL.t_stance)
    return c


def _gait_start(n):
    """tests/test_gpu_swing_reference.py's placement: LA.stand_start's generic standing robots on a trot whose diagonal 1, 2 crosses its
    stance -> swing edge at the SECOND tick of a clock stepping LA.DT"""
    model = SR.DEFAULT_MODEL
    b = {k: v for k, v in LA.stand_start(n).items() if k != "stance"}
    step = LA.DT / (model.t_swing + model.t_stance)
    b["gait_phase"] = np.ascontiguousarray(np.tile([0.3 * model.duty, model.duty - 1.5 * step, model.duty - 1.5 * step, 0.3 * model.duty], (n, 1)))
    return b


def _fresh(q, start, n):
    from quadruped_control_amd.balance_controller import new_swing_states

    dev = q.to_device(start)
    st = new_swing_states(n)
    dev["swing_state"] = _cuda(st.view(np.uint8).reshape(n, -1))
    return dev


def _running(n, b):
    from tests import commander_adjoint_restatement as CA

    st = np.zeros(n, CA.STATE_DTYPE)
    st["standing"], st["gait_running"] = 1, 1
    for k in DESIRED:
        st[k] = b[k].reshape(n, -1)
    twist = np.zeros((n, 6))
    twist[:, 0:2] = np.random.default_rng(0xC0DE).uniform(-0.2, 0.2, (n, 2))
    return st, twist


def test_lean_none_changes_nothing(q):
    """each of the three rollouts with lean=None: the bits of a call without the keyword"""
    import torch

    ctl, n, H = _handle(q), 33, 3
    b = _gait_start(n)
    same = lambda a, c: all(torch.equal(a[k].detach(), c[k].detach()) for k in a if isinstance(a[k], torch.Tensor))
    runs = []
    for kw in ({}, {"lean": None}):
        dev = dict(_fresh(q, b, n), gait_dt=torch.zeros(n, dtype=torch.float64, device="cuda"))
        state, out = ctl.rollout_tick(dev, None, H, LA.DT, LA.STAND_INERTIA, **kw)
        runs.append((dict(state), {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}, dev))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1]) and same(runs[0][2], runs[1][2])
    runs = [ctl.rollout_gait_autograd(_fresh(q, b, n), H, LA.DT, LA.STAND_INERTIA, LA.DT, **kw) for kw in ({}, {"lean": None})]
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])
    st, twist = _running(n, b)
    bc = {k: v for k, v in b.items() if k not in DESIRED}
    runs = []
    for kw in ({}, {"lean": None}):
        cmd = {"state": _cuda(st.view(np.uint8).reshape(n, -1)), "twist": _cuda(twist), "fresh": _cuda(np.ones(n, np.uint8))}
        runs.append(ctl.rollout_commander_autograd(_fresh(q, bc, n), cmd, H, LA.DT, LA.STAND_INERTIA, LA.DT, **kw))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])
    cmd = {"state": _cuda(st.view(np.uint8).reshape(n, -1)), "twist": _cuda(twist), "fresh": _cuda(np.ones(n, np.uint8))}
    with pytest.raises(ValueError, match="rollout_tick: lean needs command=None .* rollout_commander_autograd"):
        ctl.rollout_tick(_fresh(q, bc, n), cmd, H, LA.DT, LA.STAND_INERTIA, lean=dict(schedule=_cuda(np.full((4, 4), WIDTH))))
    with pytest.raises(ValueError, match="lean is dict"):
        ctl.rollout_gait_autograd(_fresh(q, b, n), H, LA.DT, LA.STAND_INERTIA, LA.DT, lean=dict(mode="offset"))
    ctl.close()


def _fd_check(keep, pts, an, scale, h, share):
    """the rule of tests/test_gpu_swing_reference.py::test_gait_rollout_has_a_gradient on the kept robots: |FD(h) - gradient . direction|
    within |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|; prints the worst figures"""
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda a: float((a[keep] / scale[keep]).max())
    print("kept", keep.mean(), "worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    assert keep.mean() >= share, keep.mean()
    assert (scale[keep] > 0).all() and np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])


def test_gait_rollout_leans_and_has_a_gradient_in_the_schedule(q):
    """rollout_gait_autograd(lean=replace) over H = 4 ticks of the trot of test_gait_rollout_has_a_gradient: the forward state is
    rollout_tick(batch, None, ..., lean=...)'s bit for bit (gait_dt = dt) and differs from the un-leaned rollout; the gradient in the
    shared schedule, in x, xdot, w, joint_q and in x_d against central differences of that rollout_tick under that test's rule - kept =
    solved, unflagged, the working set, the clamp mask and the replan bits of every step unchanged at +-h, +-2h of the state's AND of
    the schedule's direction; the bar |FD(h) - FD(2h)| + 1e-5 |gradient| |direction| - with the kept share at least 0.75.  The
    schedule is one [4,4] block shared by robots that do not interact, and the loss is summed over the kept robots: its .grad (the
    kernel's sum) is compared with the kept robots' summed differences.
    Measured on the MI355X: kept 0.877; worst relative error 3.6e-8 next to a worst |FD(h) - FD(2h)| of 1.1e-7, beyond it by at most
    3.1e-9 (the allowance is 1e-5); the schedule 8.3e-9 next to 5.0e-8.  No CPU restatement of the whole rollout exists to take a
    4 x bar from: the bar is that test's, built from the differences alone."""
    import torch

    ctl = _handle(q)
    n, H, h = ROLLOUT_N, ROLLOUT_STEPS, ROLLOUT_H
    b = _gait_start(n)
    rng = np.random.default_rng(0x1EA7)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in ("x", "xdot", "w", "joint_q", "x_d")}
    vs = rng.normal(0.0, 1.0, (4, 4))
    s0 = np.full((4, 4), WIDTH)
    lo, hi = LA.tau_limits()

    def rollout(k, ks=0):
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        lean = dict(schedule=_cuda(s0 + ks * h * vs), mode="replace")
        words, status, clamp, flags, plans = [], [], [], [], []
        for steps in range(1, H + 1):  # (the last tick of an s-step rollout is step s - 1's)
            dev = dict(_fresh(q, start, n), gait_dt=torch.zeros(n, dtype=torch.float64, device="cuda"))
            state, out = ctl.rollout_tick(dev, None, steps, LA.DT, LA.STAND_INERTIA, lean=lean)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            tau = out["joint_tau"].cpu().numpy()
            clamp.append((tau <= lo) | (tau >= hi))
            flags.append(out["flags"].cpu().numpy())
            rec = dev["swing_state"].cpu().numpy().reshape(-1).view(SR.STATE_DTYPE)
            plans.append(np.c_[rec["leg_state"], rec["has_traj"]])
        final = {name: state[name].cpu().numpy() for name in STATE}
        final["x_d"] = dev["x_d"].cpu().numpy()
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags), final, np.array(plans)

    base = rollout(0)
    L0, w0, st0, cl0, fl0, final0, pl0 = base
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0)
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    spts = {k: rollout(0, k) for k in (-2, -1, 1, 2)}
    for Lk, wk, stk, clk, flk, _, plk in list(pts.values()) + list(spts.values()):
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0) & (plk == pl0).all(axis=(0, 2))
    assert not np.array_equal(final0["x_d"][:, :2], b["x_d"][:, :2]) and np.array_equal(final0["x_d"][:, 2], b["x_d"][:, 2]), "x_d was written in place"

    dev = _fresh(q, b, n)
    plain, _ = ctl.rollout_gait_autograd(dev, H, LA.DT, LA.STAND_INERTIA, LA.DT)
    for name in v:
        dev[name].requires_grad_(True)
    sl = _cuda(s0).requires_grad_(True)
    state, out = ctl.rollout_gait_autograd(dev, H, LA.DT, LA.STAND_INERTIA, LA.DT, lean=dict(schedule=sl))  # the default mode: replace
    for name in STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name  # forward: rollout_tick(lean=...)'s bits
    assert torch.equal(out["active_set"], torch.from_numpy(w0[-1]).cuda())
    assert not torch.equal(state["x"].detach(), plain["x"].detach()), "the lean moves the rollout"
    kept = torch.from_numpy(keep.astype(np.float64)).cuda()[:, None]
    sum((state[name] * torch.from_numpy(c[name]).cuda() * kept).sum() for name in STATE).backward()
    torch.cuda.synchronize()
    g = {name: dev[name].grad.cpu().numpy() for name in v}
    an = sum((g[name] * v[name]).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    print("start state and x_d:")
    _fd_check(keep, pts, an, scale, h, 0.75)
    assert bool((np.abs(g["x_d"][keep]).sum(axis=1) > 0).all()) and not any(g[name][~keep].any() for name in v)
    # the schedule: the summed gradient against the kept robots' summed differences
    gs = sl.grad.cpu().numpy()
    assert np.isfinite(gs).all() and (gs != 0).any()
    fd1 = ((spts[1][0] - spts[-1][0]) / (2 * h))[keep].sum()
    fd2 = ((spts[2][0] - spts[-2][0]) / (4 * h))[keep].sum()
    an_s, scale_s = float((gs * vs).sum()), float(np.sqrt((gs ** 2).sum()) * np.sqrt((vs ** 2).sum()))
    print("schedule: relative error", abs(fd1 - an_s) / scale_s, "t", abs(fd1 - fd2) / scale_s)
    assert abs(fd1 - an_s) <= abs(fd1 - fd2) + 1e-5 * scale_s
    ctl.close()


def test_commander_rollout_leans_by_an_offset(q):
    """rollout_commander_autograd(lean=offset, the default mode) over H = 4 ticks: the commander records are the un-leaned rollout's
    bit for bit at step 1 - the lean goes to the tick only - while the state differs; the gradient in the twist and in the shared
    schedule against central differences of its own forward pass under the rule above (rollout_tick refuses a command with a lean).
    Measured on the MI355X: kept 0.985; the twist's worst relative error 4.9e-8 next to a worst |FD(h) - FD(2h)| of 4.6e-8, beyond it
    by at most 6.7e-9; the schedule 1.8e-8 next to 8.3e-9 (within the 1e-5 allowance)."""
    import torch

    ctl = _handle(q)
    n, H, h = ROLLOUT_N, ROLLOUT_STEPS, ROLLOUT_H
    b = _gait_start(n)
    st, twist = _running(n, b)
    bc = {k: v for k, v in b.items() if k not in DESIRED}
    rng = np.random.default_rng(0x0FF5)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    vt, vs, s0 = rng.normal(0.0, 1.0, (n, 6)), rng.normal(0.0, 1.0, (4, 4)), np.full((4, 4), WIDTH)
    lo, hi = LA.tau_limits()
    ones = np.ones(n, np.uint8)

    def run(tw, sched, steps, lean=True):
        cmd = {"state": _cuda(st.view(np.uint8).reshape(n, -1)), "twist": tw, "fresh": _cuda(ones)}
        return ctl.rollout_commander_autograd(_fresh(q, bc, n), cmd, steps, LA.DT, LA.STAND_INERTIA, LA.DT, lean=dict(schedule=sched, gain=2.0) if lean else None)

    def rollout(k, ks=0):
        words, status, clamp, flags, plans = [], [], [], [], []
        with torch.no_grad():
            for steps in range(1, H + 1):
                state, out = run(_cuda(twist + k * h * vt), _cuda(s0 + ks * h * vs), steps)
                words.append(out["active_set"].cpu().numpy())
                status.append(out["status"].cpu().numpy())
                tau = out["joint_tau"].cpu().numpy()
                clamp.append((tau <= lo) | (tau >= hi))
                flags.append(out["flags"].cpu().numpy())
                rec = out["swing_state"].cpu().numpy().reshape(-1).view(SR.STATE_DTYPE)
                plans.append(np.c_[rec["leg_state"], rec["has_traj"]])
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags), final, np.array(plans)

    L0, w0, st0, cl0, fl0, final0, pl0 = rollout(0)
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0)
    pts, spts = {k: rollout(k) for k in (-2, -1, 1, 2)}, {k: rollout(0, k) for k in (-2, -1, 1, 2)}
    for Lk, wk, stk, clk, flk, _, plk in list(pts.values()) + list(spts.values()):
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0) & (plk == pl0).all(axis=(0, 2))

    tw, sl = _cuda(twist).requires_grad_(True), _cuda(s0).requires_grad_(True)
    with torch.no_grad():
        plain1, leaned1 = run(_cuda(twist), _cuda(s0), 1, lean=False), run(_cuda(twist), _cuda(s0), 1)
    assert torch.equal(plain1[1]["cmd_state"], leaned1[1]["cmd_state"]) and not torch.equal(plain1[0]["x"], leaned1[0]["x"]), "the lean goes to the tick only"
    state, out = run(tw, sl, H)
    for name in STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name
    kept = torch.from_numpy(keep.astype(np.float64)).cuda()[:, None]
    sum((state[name] * torch.from_numpy(c[name]).cuda() * kept).sum() for name in STATE).backward()
    torch.cuda.synchronize()
    gt, gs = tw.grad.cpu().numpy(), sl.grad.cpu().numpy()
    an = (gt * vt).sum(axis=1)
    scale = np.sqrt((gt ** 2).sum(axis=1)) * np.sqrt((vt ** 2).sum(axis=1))
    print("twist:")
    _fd_check(keep, pts, an, scale, h, 0.75)
    assert not gt[~keep].any() and np.isfinite(gs).all() and (gs != 0).any()
    fd1 = ((spts[1][0] - spts[-1][0]) / (2 * h))[keep].sum()
    fd2 = ((spts[2][0] - spts[-2][0]) / (4 * h))[keep].sum()
    an_s, scale_s = float((gs * vs).sum()), float(np.sqrt((gs ** 2).sum()) * np.sqrt((vs ** 2).sum()))
    print("schedule: relative error", abs(fd1 - an_s) / scale_s, "t", abs(fd1 - fd2) / scale_s)
    assert abs(fd1 - an_s) <= abs(fd1 - fd2) + 1e-5 * scale_s
    ctl.close()

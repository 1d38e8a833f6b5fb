"""GPU: qc_com_reference_tangent_batch (csrc/qc_command_tangent.hpp) against the restatement
(tests/com_reference_tangent_restatement.py): both modes, shared and per-robot schedules, `feet` and joint_q, the contact mask given
each way, NULL tangents, output subsets, the in-place form, the grid cap, the pairing with the device's adjoint (schedule_bar_sum for a
shared schedule), a flagged robot and the refusals.

n in {1, 63, 64, 65, 130} x K in {1, 3}: tail lanes, whole waves and a direction boundary inside a wave.  Robots are the first n of
support_polygon_restatement's 130-robot pool, whose last 6 are the saturating family.  The bar against the restatement, per output
and entry: 4 x C_MT x EPS x condition sum - C_MT measured on the CPU against 50 digits (tests/test_com_reference_tangent_cpu.py), never
on the device; the factor 4 is the siblings' allowance for operation order and FMA contraction."""
import os
import re

import numpy as np
import pytest

from tests import com_reference_tangent_restatement as MT
from tests import support_polygon_restatement as SP
from tests.gpu_arrays import q  # noqa: F401
from tests.solved_batch_support import EPS, params

pytestmark = pytest.mark.gpu
N_REF, K_REF, GAIN = 130, 3, 0.7
SHAPES = tuple((n, K) for n in (1, 63, 64, 65, 130) for K in (1, 3))
ALL = tuple(MT.OUTPUTS) + ("flags",)
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _header_constant(name):
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped_control_amd", "csrc", "qc_command_tangent.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


CAP_PAIRS = _header_constant("COMMAND_TANGENT_MAX_BLOCKS") * _header_constant("COMMAND_TANGENT_BLOCK")


@pytest.fixture(scope="module")
def ctl(q):
    """a handle of this module's own: the phase rule reads the handle's duty"""
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_gait(0.3, 0.3)  # duty 0.5 exactly: the draw's trot
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """per (form, shared, mode), once and never changed: the pool, K_REF directions, tangent_np and the 50-digit condition sums"""
    class Lazy(dict):
        def __missing__(self, key):
            form, shared, mode = key
            b, sched = SP.pool(N_REF, saturating=6)
            b = {k: a for k, a in b.items() if k != ("joint_q" if form == "feet" else "feet")}
            sched = sched[0] if shared else sched
            tans = MT.random_tangents(N_REF, K_REF, joint_q=form == "joint_q", shared=shared)
            val, flags = MT.tangent_np(b, sched, tans, mode, GAIN)
            cond = MT.tangent_mp(b, sched, tans, mode, GAIN)[1]
            assert not flags.any()
            self[key] = dict(b=b, sched=sched, tans=tans, val=val, cond=cond, mode=mode, shared=shared)
            return self[key]

    return Lazy()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cut(c, name, n, K):
    t = c["tans"][name]
    return t[:K].reshape(K, 4, 4) if (c["shared"] and name == "schedule_tan") else t[:K, :n]  # one [4,4] block per direction


def _batch(c, n, way=None):
    b = {k: np.ascontiguousarray(v[:n]) for k, v in c["b"].items()}
    if way == "stance":
        b["stance"] = np.array([SP.contact_mask(b, i, SP.TROT_DUTY) for i in range(n)], np.uint8)
    if way == "gait_duty":  # the handle's duty, handed over per robot
        b["gait_duty"] = np.full(n, SP.TROT_DUTY)
    return {k: _cuda(v) for k, v in b.items()}


def _call(ctl, c, n, K, given=None, want=ALL, in_place=False, way=None, tans=None, gain=GAIN):
    import torch

    from quadruped_control_amd import tangent as T

    src = dict(c, tans=c["tans"] if tans is None else tans)
    dev = {k: _cuda(_cut(src, k, n, K)) for k in src["tans"] if given is None or k in given}
    sched = _cuda(c["sched"] if c["shared"] else c["sched"][:n])
    out = {"x_d_out_tan": dev["x_d_in_tan"]} if in_place else None
    res = T.com_reference_tangent(ctl, _batch(c, n, way), sched, None, dev, c["mode"], gain, want=want, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}, dev


@pytest.mark.parametrize("n,K", SHAPES)
@pytest.mark.parametrize("form,shared,mode", (("feet", False, "replace"), ("feet", True, "offset"), ("joint_q", False, "offset"), ("joint_q", True, "replace")))
def test_against_the_restatement(ctl, refs, form, shared, mode, n, K):
    c = refs[(form, shared, mode)]
    way = (None, "stance", "gait_duty")[(n + K) % 3]  # the contact mask given each way over the shapes
    got, _ = _call(ctl, c, n, K, way=way)
    assert not got["flags"].any()
    for name in MT.OUTPUTS:
        val, cond = c["val"][name][:K, :n], c["cond"][name][:K, :n]
        exact = cond == 0.0
        assert np.array_equal(bits(got[name][exact]), bits(val[exact])), name  # z: a copy
        worst = float((np.abs(got[name] - val)[~exact] / (EPS * cond[~exact] + SP.TINY)).max())
        print(f"{form} shared={shared} {mode} n={n} K={K} {name}: {worst:.2f} of {4 * MT.C_MT[name]:.1f} EPS x condition sum")
        assert worst <= 4 * MT.C_MT[name], (name, worst)


@pytest.mark.parametrize("key", (("feet", False, "offset"), ("joint_q", True, "replace")))
def test_subsets_null_tangents_and_the_in_place_form_are_bit_equal(ctl, refs, key):
    c = refs[key]
    n, K = 65, 3
    full, _ = _call(ctl, c, n, K)
    for name in ALL:
        one, _ = _call(ctl, c, n, K, want=(name,))
        assert list(one) == [name] and np.array_equal(one[name].view(np.uint8), full[name].view(np.uint8)), name
    for name in c["tans"]:
        null, _ = _call(ctl, c, n, K, given=[k for k in c["tans"] if k != name])
        zeros, _ = _call(ctl, c, n, K, tans=dict(c["tans"], **{name: np.zeros_like(c["tans"][name])}))
        for out in ALL:
            assert np.array_equal(null[out].view(np.uint8), zeros[out].view(np.uint8)), (name, out)
    _, dev = _call(ctl, c, n, K, in_place=True, want=("x_d_out_tan",))
    assert np.array_equal(bits(dev["x_d_in_tan"].cpu().numpy()), bits(full["x_d_out_tan"]))


def test_constructed_cases_on_the_device(ctl, refs):
    n, K = 65, 3
    c = refs[("feet", False, "replace")]
    got, _ = _call(ctl, c, n, K)
    assert np.array_equal(bits(got["x_d_out_tan"][..., 2]), bits(c["tans"]["x_d_in_tan"][:K, :n, 2]))
    assert np.array_equal(bits(got["x_d_out_tan"][..., :2]), bits(got["com_xy_tan"]))
    c = refs[("joint_q", False, "offset")]
    got, _ = _call(ctl, c, n, K, gain=0.0)
    assert np.array_equal(bits(got["x_d_out_tan"]), bits(c["tans"]["x_d_in_tan"][:K, :n]))
    # a shared schedule_tan against the same block broadcast per robot
    c = refs[("feet", True, "offset")]
    got, _ = _call(ctl, c, n, K)
    per = dict(c, shared=False, sched=np.ascontiguousarray(np.broadcast_to(c["sched"], (N_REF, 4, 4))),
               tans=dict(c["tans"], schedule_tan=np.ascontiguousarray(np.broadcast_to(c["tans"]["schedule_tan"][:, None, :], (K_REF, N_REF, 16)))))
    other, _ = _call(ctl, per, n, K)
    for name in ALL:
        assert np.array_equal(other[name].view(np.uint8), got[name].view(np.uint8)), name


def test_one_launch_just_past_the_block_cap(ctl, refs):
    """n K = cap + 130 pairs at K = 2 on the 130 robots tiled: every row must equal the small call's row of the same robot, in the
    first round of the grid stride and in the second."""
    import torch

    from quadruped_control_amd import tangent as T

    c = refs[("feet", True, "offset")]
    K = 2
    n = (CAP_PAIRS + 130) // K
    reps = -(-n // N_REF)
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps, axis=0)[:n])
    tans = {k: (v[:K].reshape(K, 4, 4) if k == "schedule_tan" else np.ascontiguousarray(np.concatenate([v[:K]] * reps, axis=1)[:, :n])) for k, v in c["tans"].items()}
    batch = {k: _cuda(tile(v)) for k, v in c["b"].items()}
    res = T.com_reference_tangent(ctl, batch, _cuda(c["sched"]), None, {k: _cuda(v) for k, v in tans.items()}, c["mode"], GAIN, want=ALL)
    torch.cuda.synchronize()
    small, _ = _call(ctl, c, N_REF, K)
    assert n * K > CAP_PAIRS and not res["flags"].any().item()
    for name in MT.OUTPUTS:
        want = np.concatenate([small[name]] * reps, axis=1)[:, :n]
        assert np.array_equal(bits(res[name].cpu().numpy()), bits(want)), name


@pytest.mark.parametrize("key", (("feet", False, "replace"), ("joint_q", False, "offset"), ("feet", True, "offset"), ("joint_q", True, "replace")))
def test_pairing_with_the_device_adjoint(ctl, refs, key):
    """<x_d_out_bar, the device's x_d_out_tan> against <the device adjoint's outputs, the tangents> in EPS x the magnitudes of all terms
    (a shared schedule_tan against schedule_bar_sum, over the batch): the bar is 4 x C_MDOT, measured on the CPU."""
    import torch

    c = refs[key]
    n, K = N_REF, K_REF
    got, _ = _call(ctl, c, n, K)
    bar = np.random.default_rng(5).uniform(-1, 1, (n, 3))
    want = ("x_d_in_bar", "feet_bar", "Rwb_bar", "x_bar", "phase_bar", "schedule_bar") + (("schedule_bar_sum",) if c["shared"] else ())
    adj = ctl.com_reference_adjoint_batch(_batch(c, n), _cuda(c["sched"]), _cuda(bar), c["mode"], GAIN, want=want)
    torch.cuda.synchronize()
    adj = {k: v.cpu().numpy() for k, v in adj.items()}
    lhs, rhs, terms = MT.pairing(bar, got["x_d_out_tan"], c["tans"], adj, c["b"], shared_sum=adj["schedule_bar_sum"] if c["shared"] else None)
    gap = float(np.max(np.abs(lhs - rhs) / (EPS * terms)))
    print(f"{key}: pairing with com_reference_adjoint_batch {gap:.3f} of {4 * MT.C_MDOT:.1f} EPS x terms")
    assert gap <= 4 * MT.C_MDOT


def test_a_zero_over_zero_robot_is_flagged_and_nan_in_every_direction(ctl, refs):
    c = refs[("feet", False, "replace")]
    n, K, i = 65, 3, 5
    b = {k: v.copy() for k, v in c["b"].items()}
    b["stance"] = np.array([SP.contact_mask(b, r, SP.TROT_DUTY) for r in range(N_REF)], np.uint8)
    sched = c["sched"].copy()
    b["stance"][i], b["gait_phase"][i], sched[i] = 0, 0.5, 1e-3
    bad = dict(c, b=b, sched=sched)
    got, _ = _call(ctl, bad, n, K)
    clean, _ = _call(ctl, dict(c, b=dict(c["b"], stance=np.array([SP.contact_mask(c["b"], r, SP.TROT_DUTY) for r in range(N_REF)], np.uint8))), n, K)
    assert got["flags"][i] == 15 and not np.delete(got["flags"], i).any()
    for name in MT.OUTPUTS:
        assert np.isnan(got[name][:, i]).all() and np.array_equal(bits(np.delete(got[name], i, axis=1)), bits(np.delete(clean[name], i, axis=1))), name


def test_refusals_launch_nothing_and_carry_the_library_messages(ctl, refs):
    import torch

    from quadruped_control_amd import tangent as T

    c = refs[("feet", False, "replace")]
    n = 8
    b, sched = _batch(c, n), _cuda(c["sched"][:n])
    tans = {"x_tan": _cuda(c["tans"]["x_tan"][0, :n])}
    out = {"x_d_out_tan": torch.full((n, 3), -7.5, dtype=torch.float64, device="cuda")}
    who = "qc_com_reference_tangent_batch: "
    cases = [(dict(batch={k: v for k, v in b.items() if k != "Rwb"}, schedule=sched, tangents=tans), "Rwb and x are required"),
             (dict(batch=b, schedule=None, tangents=tans), "schedule is required"),
             (dict(batch=dict(b, gait_dt=_cuda(np.full(n, 0.01))), schedule=sched, tangents=tans), "gait_dt must be NULL"),
             (dict(batch=b, schedule=sched, tangents={"joint_q_tan": _cuda(np.zeros((n, 12)))}), "joint_q_tan needs in->joint_q"),
             (dict(batch=b, schedule=sched, tangents=tans, gain=float("inf")), "gain must be finite"),
             (dict(batch=b, schedule=sched, tangents={}), "no tangent given")]
    for kw, text in cases:
        with pytest.raises(ValueError, match=who + text):
            T.com_reference_tangent(ctl, x_d_in=None, want=("x_d_out_tan",), out=out, **kw)
    with pytest.raises(ValueError, match=who + "no output requested"):
        T.com_reference_tangent(ctl, b, sched, None, tans, want=())
    torch.cuda.synchronize()
    assert bool((out["x_d_out_tan"] == -7.5).all())

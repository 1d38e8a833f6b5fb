"""GPU: qc_swing_reference_tangent_batch (csrc/qc_swing_reference_tangent.hpp) against the restatement
(tests/swing_reference_tangent_restatement.py), its held decisions, NULL tangents, output subsets and in-place forms, the grid cap, the
pairing with the device's adjoint, flagged robots, rollout_gait_tangent() and rollout_gait_transition() through a replanned trot, and
the refusals.

A lane is one (direction, robot) pair and a workgroup one wave: n in {1, 63, 64, 65, 130} x K in {1, 3} puts tail lanes, whole waves
and a direction boundary inside a wave on the grid.  Robots are the first n of a 130-robot pool of swing_reference_restatement's six
kinds (first, edge1, edge2, carried, cleared, stance).  Every array carries sentinel rows behind its last row.  Two handles of this
module's own: the default model and gait, and the ODD one (set_kinematics, set_gait).

The bar against the restatement, per output and entry: 4 x C_RT x EPS x condition sum - C_RT the float64 restatement's own worst
distance from 50 digits, measured on the CPU (tests/test_swing_reference_tangent_cpu.py) and never on the device; the factor 4 is the
siblings' allowance for operation order and FMA contraction."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_tangent_restatement as LT
from tests import swing_reference_restatement as RR
from tests import swing_reference_tangent_restatement as RT
from tests import swing_tangent_restatement as ST
from tests import tangent_restatement as QR
from tests.gpu_arrays import SENTINEL, _device_arrays, _tile, assert_same_bits
from tests.solved_batch_support import EPS, assert_raw_refusals, batch_in, params, q  # noqa: F401

pytestmark = pytest.mark.gpu
N_REF, K_REF = 130, 3
SHAPES = tuple((n, K) for n in (1, 63, 64, 65, 130) for K in (1, 3))
IN_KEYS = ("Rwb", "x", "xdot", "w", "joint_q", "gait_phase")
ROWS = RT.OUTPUTS
ALL = ROWS + ("flags",)
STATE = LA.INPUTS[:-1]
DT = LA.DT


def _header_constant(name):
    """`constexpr int name = value;` of csrc/qc_swing_reference_tangent.hpp"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped_control_amd", "csrc", "qc_swing_reference_tangent.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


CAP_PAIRS = _header_constant("SWING_REFERENCE_TANGENT_MAX_BLOCKS") * _header_constant("SWING_REFERENCE_TANGENT_BLOCK")


def _handle(q, model):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_tuning(race=0)
    c.set_kinematics(**model.handle_arguments())
    c.set_gait(model.t_swing, model.t_stance)
    return c


@pytest.fixture(scope="module")
def handles(q):
    """the default model, and a module-owned ODD handle (never set_kinematics on a shared one)"""
    out = {name: _handle(q, M) for name, M in RR.MODELS.items()}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def references():
    """per model, once and never changed: the pool after the clock's step, K_REF seeded directions, reference_tangent_np and the
    condition sums of the 50-digit pass"""
    class Lazy(dict):
        def __missing__(self, model):
            M = RR.MODELS[model]
            b, before, after, planned, kinds = RT.pool_after(M, N_REF)
            start, _, gait_dt = RR.pool(M, N_REF)
            tans = RT.random_tangents(N_REF, K_REF)
            val, flags = RT.reference_tangent_np(M, b, before, tans)
            cond = RT.reference_tangent_mp(M, b, before, tans)[1]
            assert not flags.any() and set(kinds[:63]) == set(RR.KINDS)
            self[model] = dict(M=M, b=b, start=start, gait_dt=gait_dt, before=before, after=after, planned=planned, tans=tans, val=val, cond=cond)
            return self[model]

    return Lazy()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(state):
    return np.ascontiguousarray(state).view(np.uint8).reshape(state.shape[0], -1)


def _cut(c, n, K):
    """the first n robots and K directions of a reference: (batch, records before, records after, tangents, values, condition sums)"""
    b = {k: np.ascontiguousarray(v[:n]) for k, v in c["b"].items()}
    tans = {k: np.ascontiguousarray(v[:K, :n]) for k, v in c["tans"].items()}
    val = {k: v[:K, :n].reshape(K * n, 12) for k, v in c["val"].items()}
    cond = {k: v[:K, :n].reshape(K * n, 12) for k, v in c["cond"].items()}
    return b, c["before"][:n], c["after"][:n], tans, val, cond


def _contact(b, after, M, way):
    """the batch with the contact mask given in one of the three ways (the phases are always there: the trajectory time reads them)"""
    if way == "stance":
        return dict(b, stance=(after["leg_state"] == 1).astype(np.uint8))
    if way == "gait_duty":  # another duty than the handle's that decides every phase of the pool the same way (its margins are 5 %)
        return dict(b, gait_duty=np.full(b["x"].shape[0], 0.97 * M.duty))
    return b


def _call(ctl, b, before, tans, n, K, given=None, zeros=False, alias=None, want=ALL):
    """One call over n robots and K directions (b: host arrays of n rows; before: the records; tans: {name: [K, n, m]}), every array
    with sentinel rows behind its last row.  given: the tangents handed over (default all; the others NULL, or zeros with zeros=True);
    alias: {output: the input tangent it is written over}.  Returns ({output: host [K n + 2, 12]}, flags [n + 2], {array: host after
    the call}, {array: host before})."""
    import torch

    from quadruped_control_amd import tangent as T

    given = tuple(tans) if given is None else given
    alias = alias or {}
    d = _device_arrays({k: v for k, v in b.items() if k in IN_KEYS + ("stance", "gait_duty", "xdot_d")}, n)
    d["state_before"] = _device_arrays({"r": _bytes(before)}, n)["r"]
    flat = {k: np.ascontiguousarray(np.asarray(v).reshape(K * n, -1)) for k, v in tans.items()}
    host = {k: (v if k in given else np.zeros_like(v)) for k, v in flat.items() if k in given or zeros}
    td = _device_arrays(host, K * n)
    snap = lambda: {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}
    start = snap()
    targets, out = {}, {}
    for name in want:
        if name == "flags":
            continue
        targets[name] = td[alias[name]] if name in alias else _device_arrays({name: np.full((1, 12), SENTINEL)}, K * n)[name]
        out[name] = targets[name][1]
    flags = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    if "flags" in want:
        out["flags"] = flags[:n]
    batch = {k: v[1] for k, v in d.items() if k != "state_before"}
    T.swing_reference_tangent(ctl, batch, d["state_before"][1], {k: v[1].reshape((K, n, -1)) for k, v in td.items()}, want=want, out=out)
    torch.cuda.synchronize()
    return {k: t[0].cpu().numpy() for k, t in targets.items()}, flags.cpu().numpy(), snap(), start


def _worst(got, val, cond, rows):
    worst = {}
    for k in got:
        assert (got[k][rows:] == SENTINEL).all(), k
        worst[k] = RR.worst_ratio(got[k][:rows], val[k], cond[k])
    return worst


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("model", ("default", "odd"))
def test_against_the_restatement(handles, references, model):
    """Every output within 4 C_RT EPS x condition sum of reference_tangent_np, zero-condition entries bit-equal, over n in {1, 63, 64,
    65, 130} x K in {1, 3}; `in`, the records and every sentinel stay.  Worst ratios on the MI355X (profiles/swing_reference_tangent.md), pos / vel /
    p_start / p_final: 4.571 / 25.341 / 1.334 / 0.941 at the default model, 1.455 / 10.386 / 1.311 / 1.000 at the odd one."""
    c = references[model]
    total = {k: 0.0 for k in ROWS}
    for n, K in SHAPES:
        b, before, _, tans, val, cond = _cut(c, n, K)
        got, flags, after, start = _call(handles[model], b, before, tans, n, K)
        assert not flags[:n].any() and flags[n:].tolist() == [-77, -77]
        assert all(np.array_equal(after[k], start[k]) for k in after)  # the inputs, the records and their sentinels stay intact
        w = _worst(got, val, cond, K * n)
        print(f"{model} n={n} K={K}: " + ", ".join(f"{k} {v:.4f} (bar {4.0 * RT.C_RT[k]})" for k, v in w.items()))
        for k, v in w.items():
            assert v <= 4.0 * RT.C_RT[k], (n, K, k, v)
            total[k] = max(total[k], v)
    print(f"{model}: worst over the shapes " + ", ".join(f"{k} {v:.4f}" for k, v in total.items()))


@pytest.mark.parametrize("way", ("stance", "gait_phase", "gait_duty"))
def test_the_contact_mask_given_in_every_way(handles, references, way):
    """The pool with the mask from stance bytes, from the phases at the handle's duty and from the phases at a per-robot duty: the
    same bar - and, the decisions being the same, the same bits."""
    c, n, K = references["odd"], N_REF, K_REF
    b, before, after, tans, val, cond = _cut(c, n, K)
    got, flags, _, _ = _call(handles["odd"], _contact(b, after, c["M"], way), before, tans, n, K)
    base, _, _, _ = _call(handles["odd"], b, before, tans, n, K)
    assert not flags[:n].any()
    w = _worst(got, val, cond, K * n)
    print(f"mask by {way}: " + ", ".join(f"{k} {v:.4f}" for k, v in w.items()))
    assert all(v <= 4.0 * RT.C_RT[k] for k, v in w.items()), w
    assert all(_same(got[k], base[k]) for k in ROWS)


# ------------------------------------------------------------------ 2. held decisions
@pytest.mark.parametrize("model", ("default", "odd"))
def test_held_decisions_from_the_records_before(q, handles, references, model):
    """The device's own forward call advances the phases and OVERWRITES the live records; the tangent call then gets the advanced
    phases, the live record in `in` (not read) and a copy of the records from before: the decisions are recomputed from that copy -
    the rows of legs that do not track are +0 bit for bit, the rows of legs that are not replanned are the input's bits, and all of it
    equals the call on the restatement's phases."""
    import torch

    from quadruped_control_amd import tangent as T

    c, ctl, n, K = references[model], handles[model], N_REF, K_REF
    b, before, after, tans, _, _ = _cut(c, n, K)
    dev = q.to_device({k: c["start"][k] for k in IN_KEYS + ("xdot_d",)})
    dev["swing_state"] = _cuda(_bytes(before))
    kept = dev["swing_state"].clone()
    ctl.swing_reference_batch(dict(dev, gait_dt=_cuda(c["gait_dt"])), want=("planned",))
    torch.cuda.synchronize()
    assert not torch.equal(kept, dev["swing_state"]) and np.array_equal(dev["gait_phase"].cpu().numpy(), b["gait_phase"])
    live = dev["swing_state"].cpu().numpy().reshape(-1).view(RR.STATE_DTYPE)
    assert np.array_equal(live["leg_state"], after["leg_state"]) and np.array_equal(live["has_traj"], after["has_traj"])
    res = T.swing_reference_tangent(ctl, dev, kept, {k: _cuda(v) for k, v in tans.items()}, want=ALL)
    torch.cuda.synchronize()
    base, _, _, _ = _call(ctl, b, before, tans, n, K)
    got = {k: res[k].cpu().numpy().reshape(K, n, 4, 3) for k in ROWS}
    assert all(_same(got[k].reshape(K * n, 12), base[k][:K * n]) for k in ROWS) and not res["flags"].cpu().numpy().any()
    stance = after["leg_state"] == 1
    tracks = ~stance & (after["has_traj"] == 1)
    plan = ((c["planned"][:n, None] >> np.arange(4)) & 1).astype(bool)
    assert stance.any() and (~stance & ~tracks).any() and (tracks & ~plan).any() and plan.any()
    for name in ("swing_pos_tan", "swing_vel_tan"):
        assert not np.ascontiguousarray(got[name][:, ~tracks]).view(np.int64).any(), name
        assert (got[name][:, tracks] != 0).any(axis=-1).all(), name
    for name, tan in (("p_start_next_tan", "p_start_tan"), ("p_final_next_tan", "p_final_tan")):
        assert _same(got[name][:, ~plan], tans[tan].reshape(K, n, 4, 3)[:, ~plan]), name
    assert not np.ascontiguousarray(got["p_final_next_tan"][:, plan][..., 2]).view(np.int64).any()  # dpf_z = +0


# ------------------------------------------------------------------ 3. NULL tangents, subsets of the outputs
@pytest.mark.parametrize("n,K", ((17, 3), (64, 1)))
def test_null_tangents_and_output_subsets(handles, references, n, K):
    """Each input tangent alone with the others NULL equals the same call with explicit zeros, bit for bit; each output asked for alone
    (and the flags alone) gives the bits of the call that asks for everything."""
    c, ctl = references["odd"], handles["odd"]
    b, before, _, tans, _, _ = _cut(c, n, K)
    base, base_flags, _, _ = _call(ctl, b, before, tans, n, K)
    for name in RT.TANGENTS:
        alone, _, after, start = _call(ctl, b, before, tans, n, K, given=(name,))
        zeros, _, _, _ = _call(ctl, b, before, tans, n, K, given=(name,), zeros=True)
        assert all(_same(alone[k], zeros[k]) for k in ROWS), name
        assert all(np.array_equal(after[k], start[k]) for k in after), name
        assert all(np.isfinite(alone[k][:K * n]).all() for k in ROWS) and any(not _same(alone[k], base[k]) for k in ROWS), name
    for name in ALL:
        one, flags, after, start = _call(ctl, b, before, tans, n, K, want=(name,))
        assert set(one) == ({name} - {"flags"}) and all(_same(one[k], base[k]) for k in one), name
        assert np.array_equal(flags, base_flags if name == "flags" else np.full(n + 2, -77)), name
        assert all(np.array_equal(after[k], start[k]) for k in after), name


# ------------------------------------------------------------------ 4. in place
@pytest.mark.parametrize("n,K", ((17, 3), (65, 2)))
def test_in_place_forms(handles, references, n, K):
    """The forms the header lists: p_start_next_tan over p_start_tan and p_final_next_tan over p_final_tan (a rollout's), swing_pos_tan /
    swing_vel_tan over [K][n][12] input tangents (joint_q_tan, p_start_tan, p_final_tan) - each equals the call beside its inputs, the
    sentinel rows included; `in`, state_before and every tangent that is not written over stay."""
    c, ctl = references["default"], handles["default"]
    b, before, _, tans, _, _ = _cut(c, n, K)
    base, _, _, _ = _call(ctl, b, before, tans, n, K)
    for alias in ({"p_start_next_tan": "p_start_tan", "p_final_next_tan": "p_final_tan"},
                  {"swing_pos_tan": "joint_q_tan", "swing_vel_tan": "p_start_tan"},
                  {"swing_pos_tan": "p_final_tan", "swing_vel_tan": "joint_q_tan", "p_start_next_tan": "p_start_tan"}):
        over, flags, after, start = _call(ctl, b, before, tans, n, K, alias=alias)
        assert all(_same(over[k], base[k]) for k in ROWS), alias  # (the sentinel rows behind the last row included)
        assert not flags[:n].any() and all(np.array_equal(after[k], start[k]) for k in after if k not in alias.values()), alias


# ------------------------------------------------------------------ 5. past the grid cap
def test_past_the_block_cap(handles, references):
    """The smallest n at K = 3 whose n K pairs exceed SWING_REFERENCE_TANGENT_MAX_BLOCKS x SWING_REFERENCE_TANGENT_BLOCK - by less than a
    wave -, so the grid strides and the second round's only wave is mostly idle lanes: one launch equals, row for row and bit for bit,
    the same robots run one direction per launch (calls below the cap)."""
    import torch

    from quadruped_control_amd import tangent as T

    K = 3
    n = CAP_PAIRS // K + 1
    assert (n - 1) * K <= CAP_PAIRS < n * K < CAP_PAIRS + 64 and n <= CAP_PAIRS
    c, ctl = references["default"], handles["default"]
    dev = {k: _cuda(_tile(c["b"][k], n)) for k in IN_KEYS}
    rec = _cuda(_tile(_bytes(c["before"]), n))
    g = torch.Generator(device="cuda").manual_seed(0x5EF7)
    tans = {k: torch.randn((K, n, m), generator=g, dtype=torch.float64, device="cuda") for k, m in RT.TANGENTS.items()}
    big = T.swing_reference_tangent(ctl, dev, rec, tans, want=ALL)
    for d in range(K):
        one = T.swing_reference_tangent(ctl, dev, rec, {k: v[d:d + 1].contiguous() for k, v in tans.items()}, want=ALL)
        for k in ROWS:
            assert_same_bits(big[k][d], one[k][0], f"{k}, direction {d}")
        assert torch.equal(big["flags"], one["flags"])
    assert all(bool(torch.isfinite(big[k]).all()) and bool((big[k][:, -1] != 0).any()) for k in ("p_start_next_tan", "p_final_next_tan"))
    assert not bool(big["flags"].any())


# ------------------------------------------------------------------ 6. the pairing with the device's adjoint
@pytest.mark.parametrize("model", ("default", "odd"))
def test_pairing_with_the_device_adjoint(q, handles, references, model):
    """<swing_pos_bar, dpos> + <swing_vel_bar, dvel> + <p_start_next_bar, dps'> + <p_final_next_bar, dpf'> = <the outputs of
    ctl.swing_reference_adjoint_batch (no `_in` arrays), the input tangents>, Rwb_bar with [delta]x Rwb, within 4 C_RDOT EPS x the
    magnitudes of all terms on both sides."""
    import torch

    c, ctl, n, K = references[model], handles[model], N_REF, K_REF
    b, before, _, tans, _, _ = _cut(c, n, K)
    bars = RR.cotangents(n)
    got, _, _, _ = _call(ctl, b, before, tans, n, K)
    adj = ctl.swing_reference_adjoint_batch(q.to_device({k: b[k] for k in IN_KEYS}), _cuda(_bytes(before)), {k: _cuda(v) for k, v in bars.items()},
                                            want=RR.OUTPUTS + ("flags",))
    torch.cuda.synchronize()
    assert not adj["flags"].cpu().numpy().any()
    adj = {k: v.cpu().numpy() for k, v in adj.items()}
    lhs, rhs, terms = RT.pairing(bars, {k: got[k][:K * n].reshape(K, n, 12) for k in ROWS}, tans, adj, b["Rwb"])
    assert (terms > 0).all() and (np.abs(lhs) > 0).all()
    worst = float(np.max(np.abs(lhs - rhs) / (EPS * terms)))
    print(f"{model}: pairing, worst {worst:.4f} EPS x term magnitudes (bar {4.0 * RT.C_RDOT})")
    assert worst <= 4.0 * RT.C_RDOT, worst


# ------------------------------------------------------------------ 7. flagged robots
def test_flagged_robots(handles, references):
    """x_z = 0, < 0, NaN, +inf, -inf on every fifth robot: a robot that replans carries its plan bits and NaN in every row of every
    direction; one that replans nothing carries no bit; every other robot's rows are the unflagged call's, bit for bit."""
    c, ctl, n, K = references["default"], handles["default"], 65, 3
    b, before, _, tans, _, _ = _cut(c, n, K)
    base, _, _, _ = _call(ctl, b, before, tans, n, K)
    bad = np.arange(n) % 5 == 2
    x = b["x"].copy()
    x[bad, 2] = np.resize([0.0, -0.3, np.nan, np.inf, -np.inf], bad.sum())
    got, flags, _, _ = _call(ctl, dict(b, x=x), before, tans, n, K)
    planned = c["planned"][:n].astype(np.int32)
    expect = np.where(bad, planned, 0)
    assert np.array_equal(flags[:n], expect) and (expect != 0).sum() >= 5 and (bad & (planned == 0)).any()
    hit = expect != 0
    for k in ROWS:
        rows, ref = got[k][:K * n].reshape(K, n, 12), base[k][:K * n].reshape(K, n, 12)
        assert np.isnan(rows[:, hit]).all() and _same(rows[:, ~bad], ref[:, ~bad]) and (got[k][K * n:] == SENTINEL).all(), k
        quiet = bad & ~hit  # nothing replanned: the LIP term is not evaluated, the rows do not depend on x
        assert _same(rows[:, quiet], ref[:, quiet]), k


# ------------------------------------------------------------------ 8. the gait rollout
ROLLOUT_N, ROLLOUT_STEPS = 33, 3
SEEDED = ("x", "xdot", "w", "joint_q", "joint_qdot")


def _fresh(q, start, n):
    from quadruped_control_amd.balance_controller import new_swing_states

    dev = q.to_device(start)
    dev["swing_state"] = _cuda(_bytes(new_swing_states(n)))
    return dev


def _rollout_start(model, n):
    """LA.stand_start's generic standing placement on a trot (the start of tests/test_gpu_swing_reference.py's gait rollout): all four
    legs start in stance on the first call (nothing is planned); on the even robots legs 1 and 2 are one and a half clock steps of DT
    below the duty, so they cross their stance -> swing edge at the SECOND tick - replanned inside the horizon - and swing along those
    trajectories at the third; the odd robots stay in stance over the horizon (all phases deep in stance)"""
    b = {k: v for k, v in LA.stand_start(n).items() if k != "stance"}
    step = DT / (model.t_swing + model.t_stance)
    b["gait_phase"] = np.ascontiguousarray(np.tile([0.3 * model.duty, model.duty - 1.5 * step, model.duty - 1.5 * step, 0.3 * model.duty], (n, 1)))
    b["gait_phase"][1::2] = 0.3 * model.duty
    return b


def _pair(bars, R, tan):
    """(sum, sum of magnitudes) per robot of <bars, tangents> at one interface of the rollout: the six state arrays (Rwb_bar with
    [delta]x Rwb), the held xdot_d and the record's two end points"""
    n = R.shape[0]
    dR = ST.skew_times(tan["Rwb_rot_tan"].reshape(n, 3), R.reshape(n, 9))
    total, mag = np.zeros(n), np.zeros(n)
    for bar, t in ((bars["Rwb"], dR),) + tuple((bars[k], tan[k + "_tan"]) for k in STATE[1:] + ("xdot_d", "p_start", "p_final")):
        prod = bar.reshape(n, -1) * t.reshape(n, -1)
        total += prod.sum(axis=1)
        mag += np.abs(prod).sum(axis=1)
    return total, mag


def test_rollout_gait_tangent_through_a_replanned_trot(q):
    """rollout_gait_tangent over 3 steps of a trot whose diagonal is replanned at the second tick for the even robots, race = 0.  The
    state, the phases and the records end bit for bit where ctl.rollout_tick(batch, None, ...) leaves them with gait_dt = dt; the flags
    are 0.  <loss cotangent, final tangents> against the gradient of the gait rollout's reverse mode paired with the seeds (the state,
    the held xdot_d): the bar accumulated interface by interface as tests/test_gpu_swing_tangent.py accumulates its own -
    4 C_DOT C_LDOT max(C_TDOT, C_SDOT, C_RDOT) EPS sum_s cond_s (mag_s + mag_{s+1}), mag_s the magnitudes of the pairing at interface s
    (state, held xdot_d and the record's end points, whose cotangents come from the reverse pass of the remaining steps), cond_s the
    reduced condition number of step s's solve.  Worst ratio on the MI355X (profiles/swing_reference_tangent.md): 0.0028 of the bar."""
    import torch

    from quadruped_control_amd import autograd as AG
    from quadruped_control_amd import tangent as T

    model = RR.DEFAULT_MODEL
    P = params(q, "uniform")
    ctl = _handle(q, model)
    n, H = ROLLOUT_N, ROLLOUT_STEPS
    b = _rollout_start(model, n)
    rng = np.random.default_rng(0x6A17C)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in SEEDED + ("xdot_d",)}
    seeds = {k + "_tan": _cuda(a) for k, a in v.items()}
    cd = {k: _cuda(a) for k, a in c.items()}
    # the plain rollout: ctl.rollout_tick with the clock running
    plain = dict(_fresh(q, b, n), gait_dt=torch.zeros(n, dtype=torch.float64, device="cuda"))
    final, _ = ctl.rollout_tick(plain, None, H, DT, LA.STAND_INERTIA)
    tan, states = [], []
    for s in range(H + 1):
        dev = _fresh(q, b, n)
        state, res = T.rollout_gait_tangent(ctl, dev, s, DT, LA.STAND_INERTIA, DT, seeds)
        torch.cuda.synchronize()
        tan.append(dict({k: res[k].cpu().numpy() for k in T._TICK_STATE + T._GAIT_RECORD}, xdot_d_tan=v["xdot_d"]))
        states.append({k: t.clone() for k, t in dev.items()})
        assert not res["flags"].cpu().numpy().any(), (s, res["flags"])
    for k in STATE + ("gait_phase", "swing_state"):
        assert_same_bits(states[H][k], plain[k], k)  # ctl.rollout_tick's bits
    rec = states[2]["swing_state"].cpu().numpy().reshape(-1).view(RR.STATE_DTYPE)
    assert (rec["has_traj"][0::2] == [0, 1, 1, 0]).all() and not rec["has_traj"][1::2].any(), "the even robots replan at the second tick"
    assert bool((res["swing_pos_tan"][0::2][:, 1:3] != 0).any(dim=-1).all()) and not bool(res["swing_pos_tan"][1::2].any())
    assert np.abs(tan[H]["p_final_tan"][0::2]).sum() > 0 and not tan[1]["p_final_tan"].any()
    # reverse mode from every interface: the remaining steps with the state, xdot_d and the record's end points as leaves
    bars, cond = [], []
    clock = torch.full((n,), DT, dtype=torch.float64, device="cuda")
    for s in range(H):
        leaf = {k: states[s][k].clone().requires_grad_(True) for k in STATE + ("xdot_d",)}
        cur = dict({k: t for k, t in states[s].items() if k not in ("swing_state", "gait_phase")}, **leaf)
        record, phase = states[s]["swing_state"], states[s]["gait_phase"]
        ps, pf = (t.clone().requires_grad_(True) for t in AG._record_points(record))
        run, p0, p1, active, flags = cur, ps, pf, None, torch.zeros((n,), dtype=torch.int32, device="cuda")
        for _ in range(H - s):
            run, out, (phase, record, p0, p1, _, active) = AG._gait_step(ctl, run, {}, phase, None, clock, record, p0, p1, True, active, flags, DT,
                                                                         LA.STAND_INERTIA, 1e-7, None, None)
        sum((run[k] * cd[k]).sum() for k in STATE).backward()
        grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).cpu().numpy()
        bars.append(dict({k: grad(leaf[k]) for k in leaf}, p_start=grad(ps), p_final=grad(pf)))
        # the solve of step s, for its condition number: on the references and the phases of that step
        nxt = states[s + 1]
        mask = (nxt["swing_state"].cpu().numpy().reshape(-1).view(RR.STATE_DTYPE)["leg_state"] == 1).astype(np.uint8)
        host = {k: t.cpu().numpy() for k, t in states[s].items() if k not in ("joint_qdot", "swing_state", "gait_phase")}
        now = dict({k: t for k, t in states[s].items() if k not in ("swing_state", "gait_phase")}, stance=_cuda(mask))
        grf = ctl.control_batch({k: t for k, t in now.items() if k != "joint_qdot"})["grf_body"].cpu().numpy()
        cond.append(QR.tangent(P, dict(host, stance=mask), grf, {"x_tan": np.zeros((1, n, 3))})["cond"])
    zero = np.zeros((n, 12))
    bars.append(dict(c, xdot_d=np.zeros((n, 3)), p_start=zero, p_final=zero))
    torch.cuda.synchronize()
    sides = [_pair(bars[s], states[s]["Rwb"].cpu().numpy(), tan[s]) for s in range(H + 1)]
    # the held xdot_d's cotangent at interface 0 is the whole rollout's; the loss side has none
    lhs, rhs = sides[H][0], sides[0][0]
    bar = 4 * QR.C_DOT * LT.C_LDOT * max(LT.C_TDOT, ST.C_SDOT["default"], RT.C_RDOT) * EPS * sum(cond[s] * (sides[s][1] + sides[s + 1][1]) for s in range(H))
    assert np.isfinite(lhs).all() and np.isfinite(rhs).all() and (np.abs(lhs) > 0).all()
    assert np.abs(bars[0]["xdot_d"][0::2]).sum() > 0 and np.abs(bars[1]["p_final"]).sum() == 0 and np.abs(bars[2]["p_final"][0::2]).sum() > 0
    ratio = np.abs(lhs - rhs) / bar
    print("dot product against reverse mode: worst gap / bar", float(ratio.max()), "worst gap / (EPS magnitudes)",
          float((np.abs(lhs - rhs) / (EPS * (sides[0][1] + sides[H][1]))).max()))
    assert (ratio <= 1.0).all(), float(ratio.max())
    ctl.close()


def test_rollout_gait_tangent_memory_and_transition(q, handles):
    """torch.cuda.max_memory_allocated over rollout_gait_tangent (K = 12 seeded directions) at steps = 1 and 3: the peaks are EQUAL.
    rollout_gait_transition: steps = 0 gives the identity; the chunked matrix (chunk = 7: state, phases and records restored between
    the chunks) equals the unchunked one bit for bit, and a column equals the single-seed rollout bit for bit."""
    import torch

    from quadruped_control_amd import tangent as T

    ctl, model = handles["default"], RR.DEFAULT_MODEL
    n, K, H = 64, 12, 3
    b = _rollout_start(model, n)
    rng = np.random.default_rng(0x5EF7A)
    tans = {k: _cuda(rng.normal(0.0, 0.01, (K, n, m))) for k, m in T.ROLLOUT_GAIT_TANGENTS.items()}

    def peak(steps):
        dev = _fresh(q, b, n)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = T.rollout_gait_tangent(ctl, dev, steps, DT, LA.STAND_INERTIA, DT, tans)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del keep
        return top

    peak(1)  # (what a first call sets up once is not tangent memory)
    p1, p3 = peak(1), peak(3)
    print(f"peak bytes, n = {n}, K = {K}: steps = 1: {p1}, steps = 3: {p3}")
    assert p1 == p3, (p1, p3)
    n = 17
    b = _rollout_start(model, n)
    ident = T.rollout_gait_transition(ctl, _fresh(q, b, n), 0, DT, LA.STAND_INERTIA, DT)
    assert torch.equal(ident["phi"], torch.eye(60, dtype=torch.float64, device="cuda").expand(n, 60, 60)) and not bool(ident["flags"].any())
    dev_full, dev_chunked = _fresh(q, b, n), _fresh(q, b, n)
    full = T.rollout_gait_transition(ctl, dev_full, H, DT, LA.STAND_INERTIA, DT)
    chunked = T.rollout_gait_transition(ctl, dev_chunked, H, DT, LA.STAND_INERTIA, DT, chunk=7)
    assert full["columns"] == list(T.GAIT_TRANSITION_COLUMNS) and torch.equal(full["flags"], chunked["flags"]) and not bool(full["flags"].any())
    assert_same_bits(chunked["phi"], full["phi"], "phi at chunk = 7")
    for k in STATE + ("gait_phase", "swing_state"):
        assert_same_bits(dev_chunked[k], dev_full[k], k)
    assert bool(torch.isfinite(full["phi"]).all())
    coordinates = T._TICK_STATE + T._GAIT_RECORD
    for col in (1, 4, 13, 30, 40, 55):
        name, comp = T.GAIT_TRANSITION_COLUMNS[col]
        seed = torch.zeros((n, T.ROLLOUT_GAIT_TANGENTS[name + "_tan"]), dtype=torch.float64, device="cuda")
        seed[:, comp] = 1.0
        _, res = T.rollout_gait_tangent(ctl, _fresh(q, b, n), H, DT, LA.STAND_INERTIA, DT, {name + "_tan": seed})
        rows = torch.cat([res[k].reshape(n, -1) for k in coordinates], dim=-1)
        assert_same_bits(full["phi"][:, :, col].contiguous(), rows, f"column {col}")
    # the even robots replan legs 1 and 2 at the second tick: their end points forget the start record, the others' pass through
    record = full["phi"][:, 36:, 36:]
    assert torch.equal(record[1::2], torch.eye(24, dtype=torch.float64, device="cuda").expand(record[1::2].shape))
    assert not bool(record[0::2][:, 3:9, 3:9].any()) and bool(full["phi"][0::2][:, 36 + 3:36 + 9, :36].any())


# ------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing(q, handles, references):
    """Every refusal of qc_swing_reference_tangent_batch returns -1 with its prefix and leaves the guarded outputs as they were; n == 0
    launches nothing; the same structs, valid, do launch.  The Python entry points raise ValueError with the library's message, and
    the two rollouts refuse what they document before anything is launched."""
    import torch

    from quadruped_control_amd import _lib
    from quadruped_control_amd import tangent as T

    c, ctl, n, K = references["default"], handles["default"], 17, 2
    lib = T._library()
    b, before, _, tans, _, _ = _cut(c, n, K)
    dev = q.to_device({k: b[k] for k in IN_KEYS})
    rec = _cuda(_bytes(before))
    td = {k: _cuda(a) for k, a in tans.items()}
    outs = {k: torch.full((K, n, 12), SENTINEL, dtype=torch.float64, device="cuda") for k in ROWS}
    flags = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    guards = [(t, SENTINEL, True) for t in outs.values()] + [(flags, 77, True)]

    def io():
        s = T.QcSwingReferenceTangentIo()
        lib.qc_default_swing_reference_tangent(ctypes.byref(s))
        s.n_dir, s.state_before = K, rec.data_ptr()
        for k, t in list(td.items()) + list(outs.items()):
            setattr(s, k, t.data_ptr())
        s.flags = flags.data_ptr()
        return s

    def refused(what, bi, s, text):
        rc = lib.qc_swing_reference_tangent_batch(ctl._h, n, ctypes.byref(bi), ctypes.byref(s), None)
        assert rc == -1 and _lib.last_error().startswith("qc_swing_reference_tangent_batch:") and text in _lib.last_error(), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert all(bool((t == sentinel).all()) for t, sentinel, _ in guards), what

    for missing in IN_KEYS:
        refused("no " + missing, batch_in(dev, [k for k in IN_KEYS if k != missing]), io(), "are required")
    for name, text in (("gait_dt", "gait_dt must be NULL"), ("swing_pos", "swing_pos and swing_vel must be NULL"), ("swing_vel", "swing_pos and swing_vel must be NULL")):
        extra = batch_in(dev, IN_KEYS)
        setattr(extra, name, dev["x"].data_ptr())
        refused(name, extra, io(), text)
    extra = batch_in(dev, [k for k in IN_KEYS if k != "joint_q"])
    extra.feet = dev["joint_q"].data_ptr()
    refused("feet without joint_q", extra, io(), "feet without joint_q")
    s = io()
    s.state_before = None
    refused("no state_before", batch_in(dev, IN_KEYS), s, "state_before is required")
    s = io()
    s.n_dir = 0
    refused("n_dir", batch_in(dev, IN_KEYS), s, "n_dir must be >= 1")
    s = io()
    for k in ROWS + ("flags",):
        setattr(s, k, None)
    refused("no output", batch_in(dev, IN_KEYS), s, "no output requested")
    s = io()
    for k in td:
        setattr(s, k, None)
    refused("no tangent", batch_in(dev, IN_KEYS), s, "no tangent given")
    s = io()
    s.n_dir = 0xFFFFFF * 64 // n + 1
    refused("beyond one launch", batch_in(dev, IN_KEYS), s, "n * n_dir is beyond one launch")
    assert_raw_refusals(lib.qc_swing_reference_tangent_batch, lambda: (ctl._h, n, batch_in(dev, IN_KEYS), io()), "qc_swing_reference_tangent_io",
                        ctypes.sizeof(T.QcSwingReferenceTangentIo), ctypes.sizeof(T.QcSwingTangentIo), guards)
    # the Python entry points: the library's words, and nothing written
    for t in outs.values():
        t.fill_(SENTINEL)
    with pytest.raises(ValueError, match="^qc_swing_reference_tangent_batch: gait_dt must be NULL"):
        T.swing_reference_tangent(ctl, dict(dev, gait_dt=dev["x"][:, 0].contiguous()), rec, td, out=outs)
    with pytest.raises(ValueError, match="^qc_swing_reference_tangent_batch: no tangent given"):
        T.swing_reference_tangent(ctl, dev, rec, {}, out={k: t[0] for k, t in outs.items()})  # (no tangent: one direction)
    with pytest.raises(ValueError, match="^qc_swing_reference_tangent_batch: state_before is required"):
        T.swing_reference_tangent(ctl, dev, None, td, out=outs)
    with pytest.raises(ValueError, match="^qc_swing_reference_tangent_batch: Rwb, x, xdot, w, joint_q and gait_phase are required"):
        T.swing_reference_tangent(ctl, {k: t for k, t in dev.items() if k != "w"}, rec, td, out=outs)
    with pytest.raises(ValueError, match="swing_reference_tangent: unknown tangent"):
        T.swing_reference_tangent(ctl, dev, rec, {"swing_pos_tan": td["joint_q_tan"]})
    with pytest.raises(ValueError, match="unknown output"):
        T.swing_reference_tangent(ctl, dev, rec, td, want=("joint_tau_tan",))
    model = RR.DEFAULT_MODEL
    start = _rollout_start(model, n)
    held = {k: t.clone() for k, t in _fresh(q, start, n).items()}
    seeds = {"x_tan": td["x_tan"]}
    for fn, extra_args in ((T.rollout_gait_tangent, (seeds,)), (T.rollout_gait_transition, ())):
        who = fn.__name__
        for name in ("stance", "swing_pos", "swing_vel", "gait_dt", "feet"):
            with pytest.raises(ValueError, match=f"^{who}: batch\\['{name}'\\] must be None"):
                fn(ctl, dict(held, **{name: held["x"]}), 2, DT, LA.STAND_INERTIA, DT, *extra_args)
        for name in ("joint_q", "joint_qdot", "gait_phase", "swing_state"):
            with pytest.raises(ValueError, match=f"^{who}: the batch carries joint_q, joint_qdot, gait_phase and swing_state"):
                fn(ctl, {k: t for k, t in held.items() if k != name}, 2, DT, LA.STAND_INERTIA, DT, *extra_args)
    with pytest.raises(ValueError, match="^rollout_gait_tangent: lean has no forward mode"):
        T.rollout_gait_tangent(ctl, held, 2, DT, LA.STAND_INERTIA, DT, seeds, lean={})
    for name in ("swing_pos_tan", "swing_vel_tan", "feet_tan"):
        with pytest.raises(ValueError, match="^rollout_gait_tangent: unknown tangent"):
            T.rollout_gait_tangent(ctl, held, 2, DT, LA.STAND_INERTIA, DT, {name: td["joint_q_tan"]})
    with pytest.raises(ValueError, match="^rollout_gait_tangent: no tangent given"):
        T.rollout_gait_tangent(ctl, held, 2, DT, LA.STAND_INERTIA, DT, {})
    with pytest.raises(ValueError, match="^rollout_gait_transition: chunk must be >= 1"):
        T.rollout_gait_transition(ctl, held, 2, DT, LA.STAND_INERTIA, DT, chunk=0)
    # the entry points that were there refuse a batch with the planner's record as they did
    with pytest.raises(ValueError, match="^rollout_tick_tangent: batch\\['swing_state'\\] must be None - the swing planner has no forward mode"):
        T.rollout_tick_tangent(ctl, held, 2, DT, LA.STAND_INERTIA, seeds)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs.values())
    again = _fresh(q, start, n)
    assert all(torch.equal(held[k], again[k]) for k in again)  # nothing was stepped

"""GPU: qc_torque_tangent_batch and qc_leg_plant_step_tangent_batch against the float64 restatements
(tests/leg_plant_tangent_restatement.py), in place, with optional outputs and NULL tangents, past their block caps, against the
device's own reverse passes, on the flagged pool, and the closed loop built on them - rollout_tick_tangent and
rollout_tick_transition (quadruped_control_amd/tangent.py).

The device's bar is 4 x the CPU-measured constants of the restatement module: every entry within 4 C_LT / 4 C_TT EPS x condition sum
(an entry whose condition sum is 0 is exact), the dot-product identities within 4 C_LDOT / 4 C_TDOT EPS x the magnitudes of their
terms.  The printed worst ratios are recorded in profiles/leg_plant_tangent.md."""
import numpy as np
import pytest

from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_tangent_restatement as LT
from tests import sensitivity_kinematics_restatement as SK
from tests import tangent_restatement as QR
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, assert_same_bits, ctl, q  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = LT.EPS
DT, INERTIA = LT.DT, LT.INERTIA
STATE = LA.INPUTS[:-1]
SHAPES = tuple((n, K) for n in (1, 63, 64, 65, 130) for K in (1, 3))


def _header_constant(header, name):
    """`constexpr int name = value;` of a header of quadruped_control_amd/csrc"""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped_control_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


# lanes of one capped launch: TORQUE_TANGENT_MAX_BLOCKS x TORQUE_TANGENT_BLOCK (csrc/qc_torque_tangent.hpp) and
# LEG_PLANT_TANGENT_MAX_BLOCKS x LEG_PLANT_TANGENT_BLOCK (csrc/qc_leg_plant_tangent.hpp), read from the headers: the two kernels share it
CAP_LANES = _header_constant("qc_torque_tangent.hpp", "TORQUE_TANGENT_MAX_BLOCKS") * _header_constant("qc_torque_tangent.hpp", "TORQUE_TANGENT_BLOCK")
assert CAP_LANES == _header_constant("qc_leg_plant_tangent.hpp", "LEG_PLANT_TANGENT_MAX_BLOCKS") * _header_constant("qc_leg_plant_tangent.hpp", "LEG_PLANT_TANGENT_BLOCK")
# an output and the input tangent it may be written over
ALIASES = tuple((o, t) for t, o in LT.NEXT_OF.items()) + (("joint_qdot_next_tan", "joint_tau_tan"),)
TORQUE_N = 65


def _flat(t, K, n):
    return {k: np.ascontiguousarray(np.asarray(v).reshape(K * n, -1)) for k, v in t.items()}


def _tangent(ctl, s, mask, tans, n, K, want=tuple(LT.OUTPUTS), given=None, alias=(), zeros=False, way="stance"):
    """One leg-plant tangent call over n robots and K directions (tans: {name: [K, n, m]}), every array with sentinel rows behind its
    last row.  given: the tangents handed over (default all; the others NULL, or zeros with zeros=True); alias: (output, tangent)
    pairs written in place; way: how the contact mask is given (LA.WAYS).  Returns ({output: host [K n + 2, m], "flags" [n + 2]},
    {array: host after the call})."""
    import torch

    from quadruped_control_amd import tangent as T

    given = tuple(tans) if given is None else given
    d = _device_arrays(s, n)
    contact = _device_arrays(LA.contact_inputs(mask, way), n)
    host = {k: (v if k in given else np.zeros_like(v)) for k, v in _flat(tans, K, n).items() if k in given or zeros}
    td = _device_arrays(host, K * n)
    outs = _device_arrays({k: np.full((1, LT.OUTPUTS[k]), SENTINEL) for k in want}, K * n)
    over = dict(alias)
    out = {k: (td[over[k]][1] if k in over else outs[k][1]) for k in want}
    flags = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    out["flags"] = flags[:n]
    T.leg_plant_step_tangent(ctl, {k: d[k][1] for k in STATE}, d["joint_tau"][1], DT, INERTIA, {k: v[1].reshape(K, n, -1) for k, v in td.items()},
                             want=tuple(want) + ("flags",), out=out, **{k: v[1] for k, v in contact.items()})
    torch.cuda.synchronize()
    res = {k: (td[over[k]][0] if k in over else outs[k][0]).cpu().numpy() for k in want}
    res["flags"] = flags.cpu().numpy()
    return res, {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}


def _np(P, s, mask, tans):
    return LT.leg_plant_tangent_np(P["mass"], P["Ib"], *(s[k] for k in LT.INPUTS), mask, INERTIA, DT, tans)


def _worst(got, ref, K, n):
    worst = {}
    for k in LT.OUTPUTS:
        val, cond = ref[k][0].reshape(K * n, -1), ref[k][1].reshape(K * n, -1)
        g = got[k][:K * n]
        exact = cond == 0
        assert np.array_equal(g[exact], val[exact]) and (got[k][K * n:] == SENTINEL).all(), k
        worst[k] = float(np.where(exact, 0.0, np.abs(g - val) / np.where(exact, 1.0, EPS * cond)).max())
    return worst


def _torque(ctl, b, grf, status, tans, n, K, given=None, alias=None, zeros=False):
    """One torque-tangent call on a handle at the tests' torque limits; the arrays of b, grf, status and the tangents carry sentinel rows"""
    import torch

    from quadruped_control_amd import tangent as T

    given = tuple(tans) if given is None else given
    d = _device_arrays({k: v for k, v in dict(b, grf_body=grf, status=status).items() if v is not None}, n)
    host = {k: (v if k in given else np.zeros_like(v)) for k, v in _flat(tans, K, n).items() if k in given or zeros}
    td = _device_arrays(host, K * n)
    out = _device_arrays({"joint_tau_tan": np.full((1, 12), SENTINEL)}, K * n)["joint_tau_tan"]
    target = td[alias] if alias else out
    T.torque_tangent(ctl, {k: d[k][1] for k in b}, d["grf_body"][1], d["status"][1].reshape(n), {k: v[1].reshape(K, n, 12) for k, v in td.items()},
                     out={"joint_tau_tan": target[1]})
    torch.cuda.synchronize()
    return target[0].cpu().numpy(), {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}


@pytest.fixture(scope="module")
def clamp_ctl(q, P):
    """a handle of this module's own at the kinematics tests' torque limits (about half of the stance torques clamp)"""
    c = q.BalanceController.from_params(P, device=0)
    c.set_kinematics(tau_min=SK.TAU_MIN, tau_max=SK.TAU_MAX)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. against the restatements
def test_leg_plant_tangent_against_the_restatement(ctl, P):
    """Every entry within 4 C_LT EPS x condition sum of leg_plant_tangent_np: n in {1, 63, 64, 65, 130} x K in {1, 3} (the pool tiled,
    seeded tangents) and the 257 pool with the contact mask given in every way (LA.WAYS)."""
    s0, mask0, _ = LA.pool()
    cases = [(n, K, "stance", {k: _tile(a, n) for k, a in s0.items()}, _tile(mask0, n), LT.random_tangents(n, K, 0x7A4700 + 16 * n + K)) for n, K in SHAPES]
    pool_ref = _np(P, s0, mask0, LT.pool_tangents())
    overall = {k: 0.0 for k in LT.OUTPUTS}
    for n, K, way, s, mask, tans in cases + [(LA.POOL, LT.REF_K, way, s0, mask0, LT.pool_tangents()) for way in LA.WAYS]:
        ref = pool_ref if n == LA.POOL else _np(P, s, mask, tans)
        got, _ = _tangent(ctl, s, mask, tans, n, K, way=way)
        assert not got["flags"][:n].any() and (got["flags"][n:] == -77).all()
        worst = _worst(got, ref, K, n)
        print(f"leg plant n {n} K {K} {way}: worst error / (EPS condsum) {worst}")
        for k in LT.OUTPUTS:
            overall[k] = max(overall[k], worst[k])
            assert worst[k] <= 4 * LT.C_LT[k], (n, K, way, k, worst[k])
    print("leg plant: worst over all shapes", overall)


def test_torque_tangent_against_the_restatement(clamp_ctl):
    """Every entry within 4 C_TT EPS x terms of torque_tangent_np, a masked entry exactly 0: case(n, ...) at n in {1, 63, 64, 65, 130}
    x K in {1, 3} from the stance bytes, and n = 65 from the phase rule."""
    overall = 0.0
    for n, K, source in [(n, K, "stance") for n, K in SHAPES] + [(TORQUE_N, 3, "phase")]:
        b, grf, status, _ = SK.case(n, source)
        b = {k: b[k] for k in ("joint_q", "stance", "gait_phase", "gait_duty") if b.get(k) is not None}
        t = LT.random_torque_tangents(n, K, 0x7A4800 + 16 * n + K)
        ref = LT.torque_tangent_np(b, grf, status, SK.TAU_MIN, SK.TAU_MAX, t["grf_tan"], t["joint_q_tan"])
        got, _ = _torque(clamp_ctl, b, grf, status, t, n, K)
        val, terms = ref["joint_tau_tan"].reshape(K * n, 12), ref["terms"].reshape(K * n, 12)
        exact = terms == 0
        assert np.array_equal(got[:K * n][exact], val[exact]) and (got[K * n:] == SENTINEL).all()
        worst = float(np.where(exact, 0.0, np.abs(got[:K * n] - val) / np.where(exact, 1.0, EPS * terms)).max())
        print(f"torque n {n} K {K} {source}: worst error / (EPS terms) {worst}, masked share {exact.mean():.2f}")
        overall = max(overall, worst)
        assert worst <= 4 * LT.C_TT, (n, K, source, worst)
    print("torque: worst over all shapes", overall)


@pytest.mark.parametrize("way", LT.TORQUE_WAYS)
def test_torque_tangent_with_the_contact_mask_given_in_every_way(clamp_ctl, way):
    """case(257, "stance")'s contact pattern given as the stance bytes, as gait_phase under the handle's duty, as gait_phase under a
    per-robot gait_duty (0.5 everywhere; and 0.35 / 0.65 alternating, where a duty read at another robot's index changes the mask)
    and not at all (every leg in stance): every entry within 4 C_TT EPS x terms of torque_tangent_np, a masked entry exactly 0."""
    n, K = LA.POOL, 3
    b, grf, status, _ = SK.case(n, "stance")
    contact, resolved = LT.torque_contact_inputs(b["stance"] != 0, way)
    b = dict(contact, joint_q=b["joint_q"])
    t = LT.random_torque_tangents(n, K, 0x7A4850)
    ref = LT.torque_tangent_np(b, grf, status, SK.TAU_MIN, SK.TAU_MAX, t["grf_tan"], t["joint_q_tan"])
    assert np.array_equal(ref["emit"], resolved & (status == 0)[:, None]) and 0.05 < ref["mask"].mean() < 0.95
    got, _ = _torque(clamp_ctl, b, grf, status, t, n, K)
    val, terms = ref["joint_tau_tan"].reshape(K * n, 12), ref["terms"].reshape(K * n, 12)
    exact = terms == 0
    assert np.array_equal(got[:K * n][exact], val[exact]) and (got[K * n:] == SENTINEL).all()
    worst = float(np.where(exact, 0.0, np.abs(got[:K * n] - val) / np.where(exact, 1.0, EPS * terms)).max())
    print(f"torque n {n} K {K} {way}: worst error / (EPS terms) {worst}, masked share {exact.mean():.2f}")
    assert worst <= 4 * LT.C_TT, (way, worst)


# ------------------------------------------------------------------ 2. in place, subsets, NULL tangents
@pytest.mark.parametrize("n,K", ((1, 1), (65, 3), (130, 2)))
def test_in_place_and_only_its_own_rows(ctl, clamp_ctl, n, K):
    """Every allowed aliasing, one at a time and the rollout's six at once, gives bit for bit what separate arrays get; the rows behind
    the last robot and direction keep their sentinels; no input array is written, and no tangent but the aliased ones."""
    s0, mask0, _ = LA.pool()
    s, mask = {k: _tile(a, n) for k, a in s0.items()}, _tile(mask0, n)
    tans = LT.random_tangents(n, K, 0x7A4730 + n)
    flat = _flat(tans, K, n)
    own, after = _tangent(ctl, s, mask, tans, n, K)
    for k in LT.INPUTS:
        assert np.array_equal(after[k][:n], s[k]) and (after[k][n:] == SENTINEL).all(), k
    for k in LT.TANGENTS:
        assert np.array_equal(after[k][:K * n], flat[k]) and (after[k][K * n:] == SENTINEL).all(), k
    assert all(not (own[k][:K * n] == SENTINEL).any() and (own[k][K * n:] == SENTINEL).all() for k in LT.OUTPUTS)
    for alias in [(a,) for a in ALIASES] + [ALIASES[:6]]:
        got, after = _tangent(ctl, s, mask, tans, n, K, alias=alias)
        for k in LT.OUTPUTS:
            assert np.array_equal(got[k], own[k]), (alias, k)
        for k in LT.INPUTS:
            assert np.array_equal(after[k][:n], s[k]), (alias, k)
        for k in LT.TANGENTS:
            if k not in dict(alias).values():
                assert np.array_equal(after[k][:K * n], flat[k]) and (after[k][K * n:] == SENTINEL).all(), (alias, k)
    # the torque map: joint_tau_tan over grf_tan and over joint_q_tan
    b, grf, status, _ = SK.case(n, "stance")
    b = {k: b[k] for k in ("joint_q", "stance")}
    t = LT.random_torque_tangents(n, K, 0x7A4830 + n)
    own, after = _torque(clamp_ctl, b, grf, status, t, n, K)
    assert np.array_equal(after["joint_q"][:n], b["joint_q"]) and np.array_equal(after["grf_body"][:n], grf) and all(np.array_equal(after[k][:K * n], _flat(t, K, n)[k]) for k in t)
    for alias in t:
        got, after = _torque(clamp_ctl, b, grf, status, t, n, K, alias=alias)
        other = [k for k in t if k != alias][0]
        assert np.array_equal(got, own) and np.array_equal(after[other][:K * n], _flat(t, K, n)[other]), alias


def test_subsets_of_outputs_and_null_tangents(ctl, clamp_ctl):
    """Any subset of the outputs: the full call's bits.  A NULL tangent: bit for bit what an array of zeros gives."""
    n, K = 65, 3
    s0, mask0, _ = LA.pool()
    s, mask = {k: _tile(a, n) for k, a in s0.items()}, _tile(mask0, n)
    tans = LT.random_tangents(n, K, 0x7A4740)
    full, _ = _tangent(ctl, s, mask, tans, n, K)
    for want in [(k,) for k in LT.OUTPUTS] + [("Rwb_rot_next_tan", "joint_q_next_tan"), ("x_next_tan", "xdot_next_tan", "w_next_tan", "joint_qdot_next_tan")]:
        part, _ = _tangent(ctl, s, mask, tans, n, K, want=want)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)
    for given in [(k,) for k in LT.TANGENTS] + [("x_tan", "joint_tau_tan"), ("Rwb_rot_tan", "w_tan", "joint_q_tan")]:
        null, _ = _tangent(ctl, s, mask, tans, n, K, given=given)
        zeros, _ = _tangent(ctl, s, mask, tans, n, K, given=given, zeros=True)
        for k in LT.OUTPUTS:
            assert np.array_equal(null[k], zeros[k]), (given, k)
        assert any(not np.array_equal(null[k], full[k]) for k in LT.OUTPUTS), given
    b, grf, status, _ = SK.case(n, "stance")
    b = {k: b[k] for k in ("joint_q", "stance")}
    t = LT.random_torque_tangents(n, K, 0x7A4840)
    full, _ = _torque(clamp_ctl, b, grf, status, t, n, K)
    for given in (("grf_tan",), ("joint_q_tan",)):
        null, _ = _torque(clamp_ctl, b, grf, status, t, n, K, given=given)
        zeros, _ = _torque(clamp_ctl, b, grf, status, t, n, K, given=given, zeros=True)
        assert np.array_equal(null, zeros) and not np.array_equal(null, full), given


# ------------------------------------------------------------------ 3. past the block caps
def test_past_the_block_caps(ctl, clamp_ctl):
    """The smallest n at K = 3 beyond each kernel's cap of 4096 one-wave workgroups (leg plant: n K > 4096 x 64; torque: 4 n K > 4096 x
    64), so the grid strides: one launch equals bit for bit the same robots run one direction per launch."""
    import torch

    from quadruped_control_amd import tangent as T

    K = 3
    n = CAP_LANES // K + 1
    assert (n - 1) * K <= CAP_LANES < n * K
    s0, mask0, _ = LA.pool()
    s = {k: torch.from_numpy(_tile(a, n)).cuda() for k, a in s0.items()}
    stance = torch.from_numpy(_tile(mask0.astype(np.uint8), n)).cuda()
    g = torch.Generator(device="cuda").manual_seed(0x7A4750)
    tans = {k: torch.randn((K, n, m), generator=g, dtype=torch.float64, device="cuda") for k, m in LT.TANGENTS.items()}
    state = {k: s[k] for k in STATE}
    big = T.leg_plant_step_tangent(ctl, state, s["joint_tau"], DT, INERTIA, tans, stance=stance)
    for d in range(K):
        one = T.leg_plant_step_tangent(ctl, state, s["joint_tau"], DT, INERTIA, {k: v[d:d + 1].contiguous() for k, v in tans.items()}, stance=stance)
        for k in LT.OUTPUTS:
            assert_same_bits(big[k][d], one[k][0], f"{k}, direction {d}")
    assert all(bool(torch.isfinite(v).all()) and bool((v != 0).any()) for v in big.values())
    n = CAP_LANES // (4 * K) + 1
    assert 4 * (n - 1) * K <= CAP_LANES < 4 * n * K
    b, grf, status, _ = SK.case(n, "stance")
    dev = {k: torch.from_numpy(b[k]).cuda() for k in ("joint_q", "stance")}
    grf, status = torch.from_numpy(grf).cuda(), torch.from_numpy(status).cuda()
    t = {k: torch.randn((K, n, 12), generator=g, dtype=torch.float64, device="cuda") for k in ("grf_tan", "joint_q_tan")}
    big = T.torque_tangent(clamp_ctl, dev, grf, status, t)["joint_tau_tan"]
    for d in range(K):
        one = T.torque_tangent(clamp_ctl, dev, grf, status, {k: v[d:d + 1].contiguous() for k, v in t.items()})["joint_tau_tan"]
        assert_same_bits(big[d], one[0], f"joint_tau_tan, direction {d}")
    assert bool(torch.isfinite(big).all()) and bool((big != 0).any())


# ------------------------------------------------------------------ 4. against the device's own reverse passes
def test_dot_products_against_the_device_adjoints(ctl, clamp_ctl, P):
    """sum <out_bar, out_tan> = sum <in_bar, in_tan> between the leg-plant kernel and ctl.leg_plant_step_adjoint on the pool within
    4 C_LDOT EPS x magnitudes, and between the torque kernel and ctl.sensitivity_kinematics_batch's torque half within 4 C_TDOT."""
    import torch

    from quadruped_control_amd import tangent as T

    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    s, mask, bars = LA.pool()
    tans = LT.pool_tangents()
    d = {k: cu(a) for k, a in s.items()}
    state = {k: d[k] for k in STATE}
    stance = cu(mask.astype(np.uint8))
    out = T.leg_plant_step_tangent(ctl, state, d["joint_tau"], DT, INERTIA, {k: cu(v) for k, v in tans.items()}, stance=stance)
    adj = ctl.leg_plant_step_adjoint(state, d["joint_tau"], DT, INERTIA, {k: cu(v) for k, v in bars.items()}, stance=stance)
    nxt = {k: v.clone() for k, v in state.items()}
    ctl.leg_plant_step(nxt, d["joint_tau"], DT, INERTIA, stance=stance)
    torch.cuda.synchronize()
    out, adj = {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in adj.items()}
    worst = 0.0
    for k in range(LT.REF_K):
        lhs, rhs, mag = LT.dot_sides(s, nxt["Rwb"].cpu().numpy(), bars, adj, tans, out, k)
        worst = max(worst, float((np.abs(lhs - rhs) / (EPS * mag)).max()))
    print(f"leg plant: worst dot-product gap / (EPS magnitudes) {worst}")
    assert worst <= 4 * LT.C_LDOT, worst
    b, grf, status, cot = SK.case(TORQUE_N, "stance")
    t = LT.random_torque_tangents(TORQUE_N, 2, 0x7A46E8)
    dev = {k: cu(b[k]) for k in ("joint_q", "stance")}
    got = T.torque_tangent(clamp_ctl, dev, cu(grf), cu(status), {k: cu(v) for k, v in t.items()})["joint_tau_tan"].cpu().numpy()
    adj = clamp_ctl.sensitivity_kinematics_batch(dev, cu(grf), cu(status), joint_tau_bar=cu(cot["joint_tau_bar"]), want=("grf_bar", "joint_q_bar"))
    worst = 0.0
    for k in range(2):
        lhs, rhs, mag = LT.torque_dot_sides(cot["joint_tau_bar"], got[k], adj["grf_bar"].cpu().numpy(), adj["joint_q_bar"].cpu().numpy(), t["grf_tan"][k], t["joint_q_tan"][k])
        live = mag > 0
        assert np.array_equal(lhs[~live], rhs[~live])
        worst = max(worst, float((np.abs(lhs - rhs)[live] / (EPS * mag[live])).max()))
    print(f"torque: worst dot-product gap / (EPS magnitudes) {worst}")
    assert worst <= 4 * LT.C_TDOT, worst


# ------------------------------------------------------------------ 5. the flagged pool, poisoning
def test_flagged_rows_are_nan_with_the_expected_bits(ctl):
    """The stretched leg, the leg with d < -1 and the singular J(q): exactly the expected bits, NaN in all K directions for the flagged
    robots only; the neighbours equal the clean call's bits.  A NaN in one robot's w poisons that robot's rows only."""
    s, mask, _ = LA.pool()
    fs, fmask, _, expected = LA.flagged_pool()
    m, K = len(expected), 3
    both = lambda a, b: np.concatenate([a, b[:5]], 0)
    tans = LT.random_tangents(m + 5, K, 0x7A4760)
    got, _ = _tangent(ctl, {k: both(fs[k], s[k]) for k in s}, both(fmask, mask), tans, m + 5, K)
    alone, _ = _tangent(ctl, {k: v[:5] for k, v in s.items()}, mask[:5], {k: np.ascontiguousarray(v[:, m:]) for k, v in tans.items()}, 5, K)
    assert np.array_equal(got["flags"][:m], expected) and not got["flags"][m:m + 5].any()
    for k in LT.OUTPUTS:
        g = got[k][:K * (m + 5)].reshape(K, m + 5, -1)
        assert np.isnan(g[:, :m]).all(), k
        assert np.array_equal(g[:, m:], alone[k][:K * 5].reshape(K, 5, -1)), k
    n, bad = 65, 16  # (robot 16 of the pool is all stance: every joint row depends on the rotation)
    s2, mask2 = {k: _tile(a, n).copy() for k, a in s.items()}, _tile(mask, n)
    assert mask2[bad].all()
    tans = LT.random_tangents(n, K, 0x7A4770)
    clean, _ = _tangent(ctl, s2, mask2, tans, n, K)
    s2["w"][bad, 1] = np.nan
    got, _ = _tangent(ctl, s2, mask2, tans, n, K)
    rows = np.arange(K) * n + bad
    others = np.setdiff1d(np.arange(K * n + 2), rows)
    for k in LT.OUTPUTS:
        if k not in ("x_next_tan", "xdot_next_tan"):  # (w does not reach them)
            assert np.isnan(got[k][rows]).all(), k
        assert np.array_equal(got[k][others], clean[k][others]), k


# ------------------------------------------------------------------ 6. rollout_tick_tangent
def test_rollout_tick_tangent_state_is_the_rollouts(q, ctl):
    """n = 65, H = 8: the six state arrays rollout_tick_tangent leaves equal ctl.rollout_tick(batch, None, ...)'s bit for bit."""
    import torch

    from quadruped_control_amd import tangent as T

    n, H = 65, 8
    b = LA.stand_start(n)
    ref, mine = q.to_device(b), q.to_device(b)
    _, out = ctl.rollout_tick(ref, None, H, DT, LA.STAND_INERTIA)
    tans = {k: torch.from_numpy(v).cuda() for k, v in LT.random_tangents(n, 2, 0x7A4780, names=("x_tan", "w_tan", "joint_q_tan")).items()}
    before = {k: v.clone() for k, v in tans.items()}
    state, res = T.rollout_tick_tangent(ctl, mine, H, DT, LA.STAND_INERTIA, tans)
    for k in STATE:
        assert_same_bits(mine[k], ref[k], k)
    assert all(state[k] is mine[k] for k in STATE) and all(torch.equal(tans[k], before[k]) for k in tans)
    assert res["x_tan"].shape == (2, n, 3) and res["joint_q_tan"].shape == (2, n, 4, 3) and res["joint_tau_tan"].shape == (2, n, 4, 3)
    assert res["flags"].shape == (n,) and res["flags"].dtype == torch.int32
    ok = res["flags"] == 0
    assert float(ok.double().mean()) >= 0.5
    assert all(bool(torch.isfinite(res[k][:, ok]).all()) and bool((res[k] != 0).any()) for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan", "grf_tan", "joint_tau_tan"))


def _pair(bars, R, tan):
    """(sum, sum of magnitudes) per robot of <bars, tangents> at one interface of the rollout: bars {Rwb (entrywise), x, xdot, w,
    joint_q, joint_qdot}, R [n, 9] the state's rotation, tan the six state tangents, numpy [n, m]"""
    n = R.shape[0]
    dR = (LT.PT.hat(tan["Rwb_rot_tan"].reshape(n, 3)) @ R.reshape(n, 3, 3)).reshape(n, 9)
    total, mag = np.zeros(n), np.zeros(n)
    for name, t in (("Rwb", dR),) + tuple((k, tan[k + "_tan"]) for k in STATE[1:]):
        prod = bars[name].reshape(n, -1) * t.reshape(n, -1)
        total += prod.sum(axis=1)
        mag += np.abs(prod).sum(axis=1)
    return total, mag


def test_rollout_tick_tangent_against_reverse_mode_and_differences(q, P):
    """On LA.rollout_case (stand_start(65), H = 3, all stance, STAND_INERTIA), race = 0, loss <c, final six state arrays>.
    Dot product against rollout_tick_autograd: sum <c, final tangents> (the entrywise c on Rwb paired with [delta_H]x Rwb_H) against
    sum <.grad, v>, on the robots whose flags are 0 over all steps, at least 0.5 of them (the CPU loop keeps 0.815:
    LA.cpu_rollout_kept).  The bar is accumulated interface by interface as in tests/test_gpu_plant_tangent.py (b): the identity holds
    step by step between the interfaces s and s + 1, each step adding the gaps of its solve, its torque map and its plant step in
    units of the magnitudes on both of its sides,
        bar = 4 C_DOT C_LDOT C_TDOT EPS sum_{s < H} cond_s (mag_s + mag_{s+1}),
    mag_s = sum |bar_s o tan_s| at interface s - bar_s from rollout_tick_autograd run from the recorded state s over the remaining
    H - s steps, tan_s from rollout_tick_tangent over s steps -, cond_s the reduced condition number of solve s.
    Central differences of ctl.rollout_tick along LA.rollout_case's directions with the existing kept rule (statuses, flags,
    working-set words and clamp masks equal at all five points; kept >= 0.5) and bar |FD(h) - FD(2h)| + 1e-5 |gradient| |v|."""
    import torch

    import quadruped_control_amd as qq
    from quadruped_control_amd import tangent as T

    n, H, h = LA.ROLLOUT_N, LA.ROLLOUT_STEPS, LA.ROLLOUT_H
    b, c, v, _ = LA.rollout_case(P)
    lo, hi = LA.tau_limits()
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)
    cd = {k: torch.from_numpy(a).cuda() for k, a in c.items()}
    seeds = {k + "_tan": torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in v.items()}

    def rollout(k):
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status, clamp, flags = [], [], [], []
        for steps in range(1, H + 1):
            state, out = ctl.rollout_tick(q.to_device(start), None, steps, DT, LA.STAND_INERTIA)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            tau = out["joint_tau"].cpu().numpy()
            clamp.append((tau <= lo) | (tau >= hi))
            flags.append(out["flags"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags)

    _, rec = ctl.rollout_tick(q.to_device(b), None, H, DT, LA.STAND_INERTIA, record_every=1)
    states = [{k: hist[k] for k in STATE} for _, hist in rec["history"]]
    tan, flags = [], None
    for s in range(H + 1):
        dev = q.to_device(b)
        _, res = T.rollout_tick_tangent(ctl, dev, s, DT, LA.STAND_INERTIA, seeds)
        tan.append({k: res[k].cpu().numpy() for k in T._TICK_STATE})
        flags = res["flags"].cpu().numpy()
        if s == H:
            states.append({k: dev[k].clone() for k in STATE})
    bars, cond = [], []
    for s in range(H):
        leaf = dict(q.to_device(b), **{k: t.clone().requires_grad_(True) for k, t in states[s].items()})
        final, _ = ctl.rollout_tick_autograd(leaf, H - s, DT, LA.STAND_INERTIA)
        sum((final[k] * cd[k]).sum() for k in STATE).backward()
        bars.append({k: leaf[k].grad.cpu().numpy() for k in STATE})
        held = {k: t for k, t in dict(q.to_device(b), **states[s]).items() if k != "joint_qdot"}
        grf = ctl.control_batch(held)["grf_body"].cpu().numpy()
        host = {k: t for k, t in dict(b, **{k: t.cpu().numpy() for k, t in states[s].items()}).items() if k != "joint_qdot"}
        cond.append(QR.tangent(qq.cheetah_params(), host, grf, {"x_tan": np.zeros((1, n, 3))})["cond"])
    bars.append(c)
    torch.cuda.synchronize()
    sides = [_pair(bars[s], states[s]["Rwb"].cpu().numpy(), tan[s]) for s in range(H + 1)]
    lhs, rhs = sides[H][0], sides[0][0]
    bar = 4 * QR.C_DOT * LT.C_LDOT * LT.C_TDOT * EPS * sum(cond[s] * (sides[s][1] + sides[s + 1][1]) for s in range(H))
    ok = flags == 0
    assert np.isfinite(rhs[ok]).all() and np.isfinite(lhs[ok]).all()  # (forward flags 0 and a NaN from reverse mode is a disagreement)
    ratio = np.abs(lhs - rhs)[ok] / bar[ok]
    print("dot product against reverse mode: robots with flags 0", int(ok.sum()), "of", n, "worst gap / bar", float(ratio.max()),
          "worst gap / (EPS magnitudes)", float((np.abs(lhs - rhs)[ok] / (EPS * (sides[0][1] + sides[H][1])[ok])).max()))
    assert ok.mean() >= 0.5 and (np.abs(lhs[ok]) > 0).all()
    assert (ratio <= 1.0).all(), float(ratio.max())
    # central differences of ctl.rollout_tick
    g = {k: bars[0][k] for k in v}
    L0, w0, st0, cl0, fl0 = rollout(0)
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0) & ok
    for Lk, wk, stk, clk, flk in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0)
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    scale = np.sqrt(sum((g[k] ** 2).sum(axis=1) for k in v)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in v))
    err, t = np.abs(fd1 - lhs), np.abs(fd1 - fd2)
    print("central differences: kept", keep.mean(), "worst relative error", float((err[keep] / scale[keep]).max()), "worst t", float((t[keep] / scale[keep]).max()))
    assert keep.mean() >= 0.5, keep.mean()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    ctl.close()


def test_rollout_tick_tangent_memory_does_not_grow_with_steps(q, ctl):
    """torch.cuda.max_memory_allocated over rollout_tick_tangent (K = 12 seeded directions) at H = 4 and H = 64: the peaks are EQUAL."""
    import torch

    from quadruped_control_amd import tangent as T

    n, K = 256, 12
    b = LA.stand_start(n)
    tans = {k: torch.from_numpy(v).cuda() for k, v in LT.random_tangents(n, K, 0x7A4790, names=T._TICK_STATE).items()}

    def peak(H):
        dev = q.to_device(b)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = T.rollout_tick_tangent(ctl, dev, H, DT, LA.STAND_INERTIA, tans)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del keep
        return top

    peak(1)  # (what a first call sets up once is not tangent memory)
    p4, p64 = peak(4), peak(64)
    print(f"peak bytes, n = {n}, K = {K}: H = 4: {p4}, H = 64: {p64}")
    assert p64 == p4, (p4, p64)


# ------------------------------------------------------------------ 7. rollout_tick_transition
def test_rollout_tick_transition(q, ctl):
    """n = 65, H = 2: [n, 36, 36]; columns bit-equal to rollout_tick_tangent on unit seeds, whole, chunked by 7 and one at a time;
    steps = 0 gives the identity; the joint_qdot columns of an all-stance robot are exactly 0."""
    import torch

    from quadruped_control_amd import tangent as T

    n, H = 65, 2
    b = LA.stand_start(n)
    whole = T.rollout_tick_transition(ctl, q.to_device(b), H, DT, LA.STAND_INERTIA)
    assert whole["phi"].shape == (n, 36, 36) and whole["columns"] == list(T.TICK_TRANSITION_COLUMNS) and whole["flags"].shape == (n,)
    assert [name for name, _ in whole["columns"][::3][:4]] == ["Rwb_rot", "x", "xdot", "w"] and whole["columns"][12] == ("joint_q", 0) and whole["columns"][24] == ("joint_qdot", 0)
    for chunk in (7, 1):
        dev = q.to_device(b)
        part = T.rollout_tick_transition(ctl, dev, H, DT, LA.STAND_INERTIA, chunk=chunk)
        assert_same_bits(part["phi"], whole["phi"], f"chunk {chunk}")
        assert torch.equal(part["flags"], whole["flags"])
    end = q.to_device(b)
    ctl.rollout_tick(end, None, H, DT, LA.STAND_INERTIA)
    for k in STATE:
        assert_same_bits(dev[k], end[k], f"{k} after a chunked transition")
    for col in (0, 4, 11, 17, 35):
        dev = q.to_device(b)
        _, res = T.rollout_tick_tangent(ctl, dev, H, DT, LA.STAND_INERTIA, T.tick_transition_seeds(n, dev["x"].device, [T.TICK_TRANSITION_COLUMNS[col]]))
        rows = torch.cat([res[k][0].reshape(n, -1) for k in T._TICK_STATE], dim=-1)
        assert_same_bits(whole["phi"][:, :, col].contiguous(), rows, f"column {col}")
    eye = T.rollout_tick_transition(ctl, q.to_device(b), 0, DT, LA.STAND_INERTIA)["phi"]
    assert torch.equal(eye, torch.eye(36, dtype=torch.float64, device="cuda").expand(n, 36, 36))
    ok = whole["flags"] == 0
    assert float(ok.double().mean()) >= 0.5
    assert not bool(whole["phi"][ok][:, :, 24:].any()) and bool(torch.isfinite(whole["phi"][ok]).all()) and bool(whole["phi"][ok][:, :, :24].any())


# ------------------------------------------------------------------ 8. refusals
def test_refusals_raise_with_the_librarys_message(q, ctl, P):
    """Every refusal arrives with the library's message and nothing is launched (sentinels intact)."""
    import torch

    from quadruped_control_amd import tangent as T

    n = 65
    s0, _, _ = LA.pool()
    s = {k: torch.from_numpy(_tile(a, n)).cuda() for k, a in s0.items()}
    state = {k: s[k] for k in STATE}
    tans = {"x_tan": torch.ones((2, n, 3), dtype=torch.float64, device="cuda")}
    out = {"x_next_tan": torch.full((2, n, 3), SENTINEL, dtype=torch.float64, device="cuda")}
    call = lambda **kw: T.leg_plant_step_tangent(ctl, kw.pop("state", state), s["joint_tau"], kw.pop("dt", DT), kw.pop("inertia", INERTIA), kw.pop("tangents", tans),
                                                 want=kw.pop("want", ("x_next_tan",)), out=kw.pop("out", out))
    who = "qc_leg_plant_step_tangent_batch"
    for dt in (0.0, -DT, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=f"^{who}: dt must be finite and > 0$"):
            call(dt=dt)
    for inertia in (0.0, (0.02, -0.03, 0.025), float("nan")):
        with pytest.raises(ValueError, match=f"^{who}: leg_inertia"):
            call(inertia=inertia)
    with pytest.raises(ValueError, match=f"^{who}: no tangent given"):
        call(tangents={}, out={"x_next_tan": out["x_next_tan"][:1]})  # (without a tangent K is 1)
    with pytest.raises(ValueError, match=f"^{who}: no output requested"):
        call(want=(), out={})
    with pytest.raises(ValueError, match=f"^{who}: joint_q, joint_qdot and joint_tau are required$"):
        call(state={k: v for k, v in state.items() if k != "joint_q"})
    with pytest.raises(ValueError, match="unknown tangent"):
        call(tangents={"grf_tan": tans["x_tan"]})
    with pytest.raises(ValueError, match="must agree on the number of directions"):
        call(tangents=dict(tans, w_tan=torch.ones((3, n, 3), dtype=torch.float64, device="cuda")))
    # the torque map
    b, grf, status, _ = SK.case(n, "stance")
    dev = {k: torch.from_numpy(b[k]).cuda() for k in ("joint_q", "stance")}
    grf, status = torch.from_numpy(grf).cuda(), torch.from_numpy(status).cuda()
    tt = {"grf_tan": torch.ones((2, n, 12), dtype=torch.float64, device="cuda")}
    tout = {"joint_tau_tan": torch.full((2, n, 12), SENTINEL, dtype=torch.float64, device="cuda")}
    who = "qc_torque_tangent_batch"
    with pytest.raises(ValueError, match=f"^{who}: no tangent given"):
        T.torque_tangent(ctl, dev, grf, status, {}, out={"joint_tau_tan": tout["joint_tau_tan"][:1]})
    with pytest.raises(ValueError, match=f"^{who}: joint_tau_tan needs grf_body and status$"):
        T.torque_tangent(ctl, dev, None, status, tt, out=tout)
    with pytest.raises(ValueError, match=f"^{who}: joint_tau_tan needs grf_body and status$"):
        T.torque_tangent(ctl, dev, grf, None, tt, out=tout)
    with pytest.raises(ValueError, match=f"^{who}: joint_q is required$"):
        T.torque_tangent(ctl, {"stance": dev["stance"]}, grf, status, tt, out=tout)
    with pytest.raises(ValueError, match="must agree on the number of directions"):
        T.torque_tangent(ctl, dev, grf, status, dict(tt, joint_q_tan=torch.ones((3, n, 12), dtype=torch.float64, device="cuda")), out=tout)
    # the closed loop
    start = q.to_device(LA.stand_start(n))
    seeds = {"x_tan": tans["x_tan"]}
    for key in ("swing_state", "swing_pos", "swing_vel", "gait_dt"):
        with pytest.raises(ValueError, match=f"^rollout_tick_tangent: batch\\['{key}'\\] must be None"):
            T.rollout_tick_tangent(ctl, dict(start, **{key: start["x"]}), 2, DT, LA.STAND_INERTIA, seeds)
    with pytest.raises(ValueError, match="^rollout_tick_tangent: commander mode has no forward mode"):
        T.rollout_tick_tangent(ctl, start, 2, DT, LA.STAND_INERTIA, seeds, command={})
    with pytest.raises(ValueError, match="^rollout_tick_tangent: lean has no forward mode"):
        T.rollout_tick_tangent(ctl, start, 2, DT, LA.STAND_INERTIA, seeds, lean={})
    with pytest.raises(ValueError, match="^rollout_tick_tangent: no tangent given$"):
        T.rollout_tick_tangent(ctl, start, 2, DT, LA.STAND_INERTIA, {})
    with pytest.raises(ValueError, match="must agree on the number of directions"):
        T.rollout_tick_tangent(ctl, start, 2, DT, LA.STAND_INERTIA, dict(seeds, w_tan=torch.ones((3, n, 3), dtype=torch.float64, device="cuda")))
    torch.cuda.synchronize()
    assert bool((out["x_next_tan"] == SENTINEL).all()) and bool((tout["joint_tau_tan"] == SENTINEL).all())  # nothing was launched
    assert all(torch.equal(start[k], t) for k, t in q.to_device(LA.stand_start(n)).items())
    call()
    T.torque_tangent(ctl, dev, grf, status, tt, out=tout)
    torch.cuda.synchronize()
    assert not bool((out["x_next_tan"] == SENTINEL).any()) and not bool((tout["joint_tau_tan"] == SENTINEL).any())

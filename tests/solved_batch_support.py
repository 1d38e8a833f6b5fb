"""What the GPU tests of the entry points that read a solved batch share (certify, sensitivity, rotation, parameters; the refusal
driver serves the plant family too): the three parameter sets and their handles, the placed-force batches, the cotangent draws, the
upload-run-synchronise-download helper and the raw-ABI tail of the "refusals launch nothing" tests.  A plain module: the fixtures
are imported by name into the test modules that use them (`from tests.solved_batch_support import q, ctls  # noqa: F401`), and
every assert carries its message, since pytest does not rewrite the asserts of a module that holds no tests."""
import ctypes
import functools

import numpy as np
import pytest

from tests.gpu_arrays import SENTINEL, q  # noqa: F401 - the one sentinel of every guarded output, the one `q` fixture

EPS = 2.0 ** -52
STATE_KEYS = ("Rwb", "Rwb_d", "x", "xdot", "w", "x_d", "xdot_d", "w_d")
FORMS = {"uniform": "diagW-6x6-uniform", "per-axis": "diagW-6x6", "dense": "dense-12x12"}  # params(q, kind) -> kernel_name
BEYOND_ONE_LAUNCH = 0xFFFFFF * 64 + 1  # robots: one more than 2^24 - 1 workgroups of one wave hold


def params(q, kind):
    P = q.cheetah_params(mu=0.6)
    if kind == "uniform":
        return P
    rng = np.random.default_rng(5)
    if kind == "per-axis":
        return dict(P, W=np.diag(1e-5 * rng.uniform(0.5, 2.0, 12)))
    M = rng.normal(size=(12, 12))
    N = rng.normal(size=(6, 6))
    return dict(P, W=1e-5 * (np.eye(12) + 0.05 * (M @ M.T) / 12.0), S=np.asarray(P["S"]) + 0.2 * (N @ N.T) / 6.0)  # dense S and W


@functools.lru_cache(maxsize=None)
def _odd_law(kind):
    import quadruped_control_amd as q

    P = params(q, kind)
    rng = np.random.default_rng(77)
    N = rng.normal(size=(3, 3))
    kff = np.array([0.11, 0.23, 0.15, 0.31, 0.17, 0.29])
    ratio = lambda k, r: np.asarray(P[k], float) * np.array(r)
    odd = dict(P, mass=9.3, Ib=np.asarray(P["Ib"], float) + 0.004 * (N @ N.T) / 3.0, kff=kff, kp_p=ratio("kp_p", (0.8, 1.3, 1.0)),
               kd_p=ratio("kd_p", (0.7, 1.0, 1.3)), kp_w=ratio("kp_w", (0.6, 1.0, 0.84)), kd_w=ratio("kd_w", (1.0, 0.64, 0.82)))
    if kind == "uniform":  # (the uniform form asks for a diagonal S: six distinct weights; a dense S is the "dense" kind's)
        odd["S"] = np.asarray(P["S"], float) * np.diag([0.9, 1.0, 1.1, 0.8, 1.2, 1.05])
    Ib = odd["Ib"]
    assert np.array_equal(Ib, Ib.T) and np.linalg.eigvalsh(Ib).min() > 0 and 1e-3 < np.abs(Ib[np.triu_indices(3, 1)]).min() < 1e-2, Ib
    for k in ("kp_p", "kd_p", "kp_w", "kd_w"):
        r = odd[k] / np.asarray(P[k], float)
        assert len(set(odd[k])) == 3 and 0.6 <= r.min() and r.max() <= 1.3, (k, odd[k])
    assert len(set(kff)) == 6 and 0.1 <= kff.min() and kff.max() <= 0.35, kff
    assert all(odd[k] == P[k] for k in ("mu", "fzmin", "fzmax")) and odd["mass"] != P["mass"]
    return odd


def odd_law(kind="uniform"):
    """params(q, kind) off the cheetah's control law, so that every index of the PD law b(state; gains) is visible: mass 9.3; Ib dense
    symmetric positive definite (the cheetah's diagonal + 0.004 N N^T / 3: off-diagonals of a few 1e-3); kp_p, kd_p, kp_w, kd_w
    three distinct values each, 0.6 ... 1.3 of the cheetah's; six distinct non-zero kff in 0.1 ... 0.35; for "uniform" six distinct
    weights on the diagonal of S (qc_create keeps the uniform form only for a diagonal S, and the kernel name must stay FORMS[kind];
    the "dense" kind carries a dense S).  mu, fzmin, fzmax as they were: the forces
    inputs() places stay exactly on their faces.  Fixed seed, cached: callers copy before they write."""
    return dict(_odd_law(kind))


@functools.lru_cache(maxsize=None)
def _odd_states(n, seed):
    from scipy.spatial.transform import Rotation

    r = np.random.default_rng(seed)
    axis = r.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    turn = Rotation.from_rotvec(axis * r.uniform(0.1, 0.6, (n, 1))).as_matrix()
    return r.uniform(-0.3, 0.3, (n, 3)), r.uniform(-0.3, 0.3, (n, 3)), r.uniform(-0.2, 0.2, (n, 3)), turn


def odd_states(b, seed):
    """a copy of the batch `b` off config3's states: w_d and xdot_d uniform in (-0.3, 0.3)^3 (config3: w_d = (0, 0, +-0.05),
    xdot_d[2] = 0), w moved by up to 0.2 per component, Rwb_d = a general-axis rotation of 0.1 ... 0.6 rad times Rwb.  Rwb itself is
    untouched: the level robots carry the on-face forces of inputs().  Fixed by (n, seed); the draws are cached."""
    n = b["x"].shape[0]
    w_d, xdot_d, dw, turn = _odd_states(n, seed)
    out = {k: v.copy() for k, v in b.items()}
    out["w_d"], out["xdot_d"], out["w"] = w_d.copy(), xdot_d.copy(), np.ascontiguousarray(b["w"] + dw)
    out["Rwb_d"] = np.ascontiguousarray((turn @ b["Rwb"].reshape(n, 3, 3)).reshape(n, 9))
    return out


def assert_tangent_close(got, ref, what, rows=None, c=None):
    """qc_tangent_batch's outputs against tangent_restatement.tangent(): flags exactly, every entry of grf_tan and b_tan within
    4 x c x EPS x its condition sum (c: tangent_restatement.C_TAN unless given); prints and returns the worst error / bar"""
    from tests.tangent_restatement import C_TAN

    c = C_TAN if c is None else c
    rows = range(ref["flags"].shape[0]) if rows is None else rows
    assert np.array_equal(got["flags"], ref["flags"]), what
    worst = 0.0
    rows = list(rows)
    for name, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
        err, bar = np.abs(got[name][:, rows] - ref[name][:, rows]), 4 * c * EPS * ref[sums][:, rows]
        worst = max(worst, float((err / np.where(bar > 0, bar, 1.0))[bar > 0].max()) if (bar > 0).any() else 0.0)
        bad = np.argwhere(~(err <= bar))
        assert not len(bad), (what, name, bad[0].tolist(), float(err[tuple(bad[0])]), float(bar[tuple(bad[0])]))
    print(what, "worst error / bar", worst)
    return worst


@pytest.fixture(scope="module")
def ctls(q):
    """one handle per formulation, keyed as FORMS"""
    out = {k: q.BalanceController.from_params(params(q, k), device=0) for k in FORMS}
    assert [c.kernel_name for c in out.values()] == list(FORMS.values()), [c.kernel_name for c in out.values()]
    yield out
    for c in out.values():
        c.close()


def odd_handle(q, kind="uniform"):
    """a NEW handle at params(q, kind) with ODD_KIN's hip and links (the caller's fixture owns and closes it; never set_kinematics on
    a shared one)"""
    from tests.device_math_reference import ODD_KIN

    c = q.BalanceController.from_params(params(q, kind), device=0)
    c.set_kinematics(hip=ODD_KIN.hip.reshape(12), links=ODD_KIN.links.reshape(12))
    return c


def odd_inputs(n):
    """inputs(n, "joint_q") for a handle at ODD_KIN: (the batch the device reads - joint_q and gait_phase, no feet -, the same batch
    with `feet` = ODD_KIN's forward kinematics of joint_q for the numpy restatements, the forces, kin = (hip [12], links [12]) for the
    50-digit passes)"""
    from tests import kkt_certificate_restatement as KR
    from tests.device_math_reference import ODD_KIN

    b, grf = inputs(n, "joint_q")
    return b, KR.with_feet(b, ODD_KIN), grf, (ODD_KIN.hip.reshape(-1), ODD_KIN.links.reshape(-1))


@functools.lru_cache(maxsize=None)
def inputs(n, source):
    """(batch, world forces): contact pattern i % 16; even robots level (Rwb = I).  source: 'feet' with stance bytes, 'joint_q' with
    gait_phase (0.3 stance / 0.9 swing against the handle's duty 0.816), 'duty' = joint_q, gait_phase 0.3 / 0.7 and gait_duty 0.5.
    Every force component is exactly on a face (fx ASSIGNED as mu * fz, fz as fzmin / fzmax) or well inside, and the on-face ones sit
    on the level robots, so the device and numpy classify alike.  Cached: callers copy before they write."""
    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = dict(workloads.config3(n=n))
    b["Rwb"] = b["Rwb"].copy()
    b["Rwb"][0::2] = np.eye(3).reshape(9)
    st = ((np.arange(n)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    if source == "feet":
        b["stance"] = st
    else:
        b = workloads.with_joint_angles(b)
        b.pop("feet", None)
        b.pop("stance", None)
        b["gait_phase"] = np.where(st != 0, 0.3, 0.9 if source == "joint_q" else 0.7)
        if source == "duty":
            b["gait_duty"] = np.full(n, 0.5)
    rng = np.random.default_rng(1000 + n)
    mu, fzmin, fzmax = P["mu"], P["fzmin"], P["fzmax"]
    level = (np.arange(n) % 2 == 0)[:, None]
    pick = rng.integers(0, 3, (n, 4))
    fz = np.where(level & (pick == 0), fzmin, np.where(level & (pick == 1), fzmax, rng.uniform(fzmin + 1.0, fzmax - 1.0, (n, 4))))
    fw = np.zeros((n, 4, 3))
    fw[..., 2] = fz
    for k in range(2):
        side = rng.integers(-1, 2, (n, 4))
        inside = rng.uniform(-0.9, 0.9, (n, 4)) * (mu * fz)
        fw[..., k] = np.where(level & (side == 1), mu * fz, np.where(level & (side == -1), -(mu * fz), inside))
    fw[st == 0] = 0.0
    R = b["Rwb"].reshape(n, 3, 3)
    grf = -np.einsum("nji,nkj->nki", R, fw).reshape(n, 12)  # grf_body = -Rwb^T f_w
    grf[0::2] = -fw[0::2].reshape(-1, 12)  # exactly, where Rwb = I
    grf += 0.0  # (no -0.0)
    return {k: np.ascontiguousarray(v) for k, v in b.items()}, np.ascontiguousarray(grf)


def gbar(base, n, seed=0):
    """the force cotangent [n, 12] of a test: `base` is its module's own (4000 sensitivity, 5000 rotation, 7000 parameters)"""
    return np.random.default_rng(base + n + seed).normal(0.0, 1.0, (n, 12))


def to_cuda(*arrays):
    import torch

    return tuple(torch.from_numpy(a).cuda() for a in arrays)


def run(q, call, b, *arrays, **kw):
    """Upload the batch and the arrays, call(dev batch, *device arrays, **kw), synchronise; returns (outputs as numpy, the device's)"""
    import torch

    out = call(q.to_device(b), *to_cuda(*arrays), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, out


def batch_in(dev, keys):
    """a qc_batch_in pointing at the device tensors dev[k], k in keys"""
    from quadruped_control_amd import _lib

    bi = _lib.QcBatchIn()
    for k in keys:
        setattr(bi, k, dev[k].data_ptr())
    return bi


def assert_raw_refusals(fn, valid, record, size, wrong_size, guards, beyond=BEYOND_ONE_LAUNCH, stream=None, untouched=None, launched=None):
    """The raw-ABI tail of a "refusals launch nothing" test, for the entry point `fn` (a ctypes function of the library; its name is
    the prefix of every message).  valid() returns a freshly filled valid (handle, n, batch or None, io): the plant family's entry
    points take no batch, fn(handle, n, io, stream), the others fn(handle, n, batch, io, stream).  Checked:
      * no handle, no batch, no io and n = `beyond` (None: the entry point sets no such limit) each return -1 with the prefix;
      * valid() set io.struct_size = `size`; with wrong_size the call returns -1 and the message names `record`.struct_size;
      * after each of them and after n == 0, which returns QC_OK, every guard keeps its sentinel;
      * the same structs, valid, return QC_OK and the sentinels are gone.
    guards: (tensor, sentinel, every) - after the valid call `every` element differs from the sentinel, or (every = False, a record
    of bytes) not all are equal to it.  untouched(what) / launched(): further checks of the caller's, made after the synchronize that
    follows each refused call (and n == 0) / the valid call."""
    import torch
    from quadruped_control_amd import _lib

    prefix = fn.__name__ + ":"
    h, n, bi, io = valid()
    ref = lambda s: ctypes.byref(s) if s is not None else None
    call = (lambda h, n, bi, io: fn(h, n, ref(bi), ref(io), stream)) if bi is not None else (lambda h, n, bi, io: fn(h, n, ref(io), stream))

    def intact(what):
        torch.cuda.synchronize()
        for i, (t, sentinel, _) in enumerate(guards):
            assert bool((t == sentinel).all()), (prefix, what, "guard", i)
        if untouched is not None:
            untouched(what)

    def refused(what, h, n, bi, io, message=prefix):
        rc = call(h, n, bi, io)
        assert rc == -1 and _lib.last_error().startswith(message), (what, rc, _lib.last_error())
        intact(what)

    refused("no handle", None, n, bi, io)
    if bi is not None:
        refused("no batch", h, n, None, io)
    refused("no io", h, n, bi, None)
    if beyond is not None:
        refused("n beyond one launch", h, beyond, bi, io)
    assert io.struct_size == size != wrong_size, (prefix, io.struct_size, size, wrong_size)
    io.struct_size = wrong_size
    refused("struct_size of another revision", h, n, bi, io, f"{prefix} {record}.struct_size")
    io.struct_size = size
    rc = call(h, 0, bi, io)
    assert rc == 0, (prefix, "n == 0 is QC_OK and launches nothing", rc, _lib.last_error())
    intact("n == 0")
    rc = call(h, n, bi, io)
    assert rc == 0, (prefix, "the same structs, valid, do launch", rc, _lib.last_error())
    torch.cuda.synchronize()
    for i, (t, sentinel, every) in enumerate(guards):
        gone = bool((t != sentinel).all()) if every else not bool((t == sentinel).all())
        assert gone, (prefix, "the valid call left a sentinel", "guard", i)
    if launched is not None:
        launched()

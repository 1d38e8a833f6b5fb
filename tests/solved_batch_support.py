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

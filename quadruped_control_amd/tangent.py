"""Forward mode of the balance QP (include/qc_tangent.h, csrc/qc_tangent.hpp): tangents of the inputs of a solved batch pushed
through the QP on its active face, and the Jacobian d grf_body / d inputs as the tangent call on unit seeds.

The functions take the controller as their first argument, as autograd.py's do.  The two symbols of the library are bound here, on
the CDLL that _lib.load() returns, with this module's own ctypes record: _lib.EXPORTS and BalanceController are not touched."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .balance_controller import _READONLY_FIELDS, _outputs

# name -> values per robot; the names are the record's fields
TANGENTS = {"x_tan": 3, "xdot_tan": 3, "w_tan": 3, "x_d_tan": 3, "xdot_d_tan": 3, "w_d_tan": 3, "Rwb_rot_tan": 3, "Rwb_d_rot_tan": 3,
            "feet_tan": 12, "joint_q_tan": 12}
_TANGENT_OUTPUTS = {"grf_tan": ((4, 3), "float64"), "b_tan": ((6,), "float64")}
JACOBIAN_WRT = ("x", "xdot", "w", "x_d", "xdot_d", "w_d", "Rwb_rot", "Rwb_d_rot")  # jacobian_batch's default; "feet" and "joint_q" are allowed too


class QcTangentIo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("grf_body", C.c_void_p), ("act_tol", C.c_double), ("n_dir", C.c_size_t)] + \
               [(k, C.c_void_p) for k in tuple(TANGENTS) + ("grf_tan", "b_tan", "flags")]


_bound = None


def _library():
    """the library with this module's two symbols bound"""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name in ("qc_default_tangent", "qc_tangent_batch"):
            if not hasattr(lib, name):
                raise ImportError(f"{_lib.LIB_PATH} does not export {name}")
        lib.qc_default_tangent.argtypes = [C.POINTER(QcTangentIo)]
        lib.qc_default_tangent.restype = None
        lib.qc_tangent_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.QcBatchIn), C.POINTER(QcTangentIo), C.c_void_p]
        lib.qc_tangent_batch.restype = C.c_int
        _bound = lib
    return _bound


def plan_tangent(ctl, batch, grf_body, tangents, want=("grf_tan",), act_tol=1e-7, out=None, stream=None):
    """tangent_batch() marshalled once: returns (launch, out, squeeze), `launch()` being one qc_tangent_batch call (graph-capturable)
    on tensors that are read in place; `out` holds [K, n, ...] tensors and squeeze says whether the tangents came as [n, ...].
    Planning launches nothing."""
    import torch

    _library()
    unknown = [k for k in tangents if k not in TANGENTS]
    if unknown:
        raise ValueError(f"tangent: unknown tangent(s) {unknown}; the tangents are {tuple(TANGENTS)}")
    io = QcTangentIo()
    ctl._lib.qc_default_tangent(C.byref(io))
    n, dev, bi = ctl._readonly_batch("tangent", batch, _READONLY_FIELDS, io, [("grf_body", grf_body, 12)])
    given = {k: t for k, t in tangents.items() if t is not None}
    K, squeeze = None, False
    for k, t in given.items():
        m = TANGENTS[k]
        bad = ValueError(f"{k}: need contiguous float64 [{n},{m}] or [K,{n},{m}] on {dev}")
        if t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev or t.dim() < 1 or t.numel() == 0:
            raise bad
        stacked = t.dim() >= 2 and t.shape[1] == n and t.shape[0] * n * m == t.numel()  # [K, n, ...]
        flat = not stacked and t.shape[0] == n and t.numel() == n * m                   # [n, ...]: K = 1, squeezed
        if not stacked and not flat:
            raise bad
        lead = t.shape[0] if stacked else 1
        if K is None:
            K, squeeze = lead, flat
        elif K != lead or squeeze != flat:
            raise ValueError(f"{k}: the tangents must agree on the number of directions and on the [n, ...] / [K, n, ...] form")
        setattr(io, k, t.data_ptr())
    K = 1 if K is None else K  # (no tangent at all is the library's refusal)
    io.n_dir = K
    io.act_tol = float(act_tol)
    wanted = tuple(w for w in want if w != "flags")
    extra = [("flags", (n,), "int32")] if "flags" in want else []
    res = _outputs("tangent", _TANGENT_OUTPUTS, wanted, out, K * n, dev, io, extra)
    res = {k: (v if k == "flags" else v.view((K, n) + _TANGENT_OUTPUTS[k][0])) for k, v in res.items()}
    launch = ctl._launcher("qc_tangent_batch", (n, C.byref(bi), C.byref(io), ctl._stream_ptr(stream)), (batch, grf_body, given, res, bi, io), ValueError)
    return launch, res, squeeze


def tangent_batch(ctl, batch, grf_body, tangents, want=("grf_tan",), act_tol=1e-7, out=None, stream=None):
    """Forward mode of the balance QP on the active face of `grf_body` [n,12] (as control_batch() wrote it) for the batch the solve
    read (qc_tangent_batch, include/qc_tangent.h; INTEGRATION.md "Forward mode: tangents and the Jacobian").  `tangents`: a dict of
    device tensors named as the record's fields - "x_tan", "xdot_tan", "w_tan", "x_d_tan", "xdot_d_tan", "w_d_tan", "Rwb_rot_tan",
    "Rwb_d_rot_tan" ([n,3]; the rotation tangents are world-frame left tangents, R <- exp([d]x) R), "feet_tan" [n,4,3] (body frame)
    and "joint_q_tan" [n,12] (only for a batch with joint_q) - each [n, ...] for one direction or [K, n, ...] for K, all agreeing on
    K; a missing one is zero.  `want`: any of "grf_tan" [K,n,4,3] (body frame), "b_tan" [K,n,6] and "flags" int32 [n] (bit 0: a foot
    on both rows of an axis, the derivative is one-sided; bit 1: a bad pivot, the robot's outputs are NaN in every direction).
    The reduced system is factorised once per robot and substituted K times in one launch.  Nothing of `batch` is written.
    Asynchronous on `stream`, no synchronisation.  Returns the dict of device tensors, [K, n, ...] - squeezed to [n, ...] where the
    tangents came that way; `out`: a dict of tensors with K * n rows to write into.  ValueError with the library's message for a
    call it refuses.  Not covered: entrywise rotation tangents, tangents of the handle's parameters, of the torque map, the plants
    and the swing pipeline."""
    launch, res, squeeze = plan_tangent(ctl, batch, grf_body, tangents, want, act_tol, out, stream)
    launch()
    return {k: (v[0] if squeeze and k != "flags" else v) for k, v in res.items()}


def jacobian_columns(wrt=JACOBIAN_WRT):
    """the columns of jacobian_batch(): the list of (name, component)"""
    unknown = [w for w in wrt if w + "_tan" not in TANGENTS]
    if unknown:
        raise ValueError(f"jacobian: unknown input(s) {unknown}; wrt is a subset of {tuple(k[:-4] for k in TANGENTS)}")
    return [(w, c) for w in wrt for c in range(TANGENTS[w + "_tan"])]


def jacobian_batch(ctl, batch, grf_body, wrt=JACOBIAN_WRT, act_tol=1e-7, chunk=None, stream=None):
    """The Jacobian d grf_body / d inputs of a solved batch on its active face: tangent_batch() on unit seeds built on the device,
    `chunk` directions per launch (None: all in one).  `wrt`: any of "x", "xdot", "w", "x_d", "xdot_d", "w_d", "Rwb_rot", "Rwb_d_rot"
    (3 columns each) and "feet", "joint_q" (12 each; "joint_q" only for a batch with joint_q).  Returns dict(jac [n, 12, C] - column c
    is d grf_body / d (columns[c]) -, columns: the list of (name, component), flags int32 [n]).  Column c equals tangent_batch() on
    the unit seed of columns[c] bit for bit, however the columns are chunked.  ValueError as tangent_batch()."""
    import torch

    cols = jacobian_columns(wrt)
    n = grf_body.shape[0]
    dev = grf_body.device
    total = len(cols)
    step = total if chunk is None else int(chunk)
    if step < 1:
        raise ValueError("jacobian: chunk must be >= 1")
    jac = torch.empty((n, 12, total), dtype=torch.float64, device=dev)
    flags = None
    for c0 in range(0, total, step):
        part = cols[c0:c0 + step]
        seeds = {}
        for j, (name, comp) in enumerate(part):
            key = name + "_tan"
            if key not in seeds:
                seeds[key] = torch.zeros((len(part), n, TANGENTS[key]), dtype=torch.float64, device=dev)
            seeds[key][j, :, comp] = 1.0
        res = tangent_batch(ctl, batch, grf_body, seeds, want=("grf_tan", "flags"), act_tol=act_tol, stream=stream)
        jac[:, :, c0:c0 + len(part)] = res["grf_tan"].reshape(len(part), n, 12).permute(1, 2, 0)
        flags = res["flags"]
    return dict(jac=jac, columns=cols, flags=flags)

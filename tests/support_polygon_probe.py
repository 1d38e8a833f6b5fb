"""ctypes view of tests/hip/libqc_support_polygon_probe.so (tests/hip/support_polygon_probe.hip): erf_f64 and exp_neg_sq of
qc_device.hpp, one value per thread, over torch tensors on cuda:0.  Built by __graft_entry__.build_support_polygon_probe(); a missing
library is an error."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "libqc_support_polygon_probe.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is not built (__graft_entry__.build_support_polygon_probe())")
        _lib = C.CDLL(LIB_PATH)
        _lib.qcs_erf.restype = _lib.qcs_exp_neg_sq.restype = C.c_int
        _lib.qcs_breakpoints.restype = None
    return _lib


def breakpoints():
    """-> (the four |x| at which erf_f64 changes form, the a^2 from which exp_neg_sq returns 0)"""
    out = (C.c_double * 5)()
    lib().qcs_breakpoints(out)
    return tuple(out[:4]), float(out[4])


def _apply(name, x):
    x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0")
    y = torch.full_like(x, 12345.0)
    st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    err = getattr(lib(), name)(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_int(x.numel()), st)
    if err != 0:
        raise RuntimeError(f"{name}: hipError_t {err}")
    torch.cuda.synchronize(0)
    return y.cpu().numpy()


def erf(x):
    return _apply("qcs_erf", x)


def exp_neg_sq(x):
    return _apply("qcs_exp_neg_sq", x)

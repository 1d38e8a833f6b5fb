"""What the GPU tests share (a plain module; test modules import its fixtures by name, `from tests.gpu_arrays import q  # noqa: F401`):
the package fixture `q`, the plant steps' default-parameter handle, pools tiled to a batch size, device copies with sentinel rows
behind the batch, and the comparison of an output against (value, bar) references."""
import numpy as np
import pytest

SENTINEL = -7777.25


@pytest.fixture(scope="module")
def q(built):
    import quadruped_control_amd as q

    return q


@pytest.fixture(scope="module")
def P(q):
    return q.cheetah_params()


@pytest.fixture(scope="module")
def ctl(q, P):
    """one handle at cheetah_params(): the plant family's (the solved-batch tests build theirs at mu = 0.6)"""
    c = q.BalanceController.from_params(P, device=0)
    yield c
    c.close()


def _sentinel(dtype):
    return SENTINEL if dtype == np.float64 else (0x5A if dtype == np.uint8 else -77)


def _tile(a, n):
    return np.ascontiguousarray(np.concatenate([a] * -(-n // a.shape[0]), 0)[:n])


def _device_arrays(host, n, pad=2):
    """{name: (whole tensor [n + pad, k], view of its first n rows)}: the rows behind row n - 1 hold a sentinel"""
    import torch

    out = {}
    for k, a in host.items():
        a2 = a.reshape(a.shape[0], -1)
        full = np.full((n + pad, a2.shape[1]), _sentinel(a2.dtype), dtype=a2.dtype)
        full[:n] = _tile(a2, n)
        t = torch.from_numpy(full).cuda()
        out[k] = (t, t[:n] if a.ndim > 1 else t[:n].reshape(n))
    return out


def _worst_over_bar(got, ref, names, n, what):
    """{name: largest error / bar} of got[name][:n] against ref[name] = (values, bars) of a pool, tiled to n; where the bar is 0
    the output is asserted to be exact."""
    worst = {}
    for k in names:
        val, bar = _tile(ref[k][0], n), _tile(ref[k][1], n)
        err = np.abs(got[k][:n] - val)
        exact = bar == 0
        assert np.array_equal(got[k][:n][exact], val[exact]), (what, k)
        worst[k] = float(np.where(exact, 0.0, err / np.where(exact, 1.0, bar)).max())
    return worst

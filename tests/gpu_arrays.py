"""What the GPU tests share (a plain module; test modules import its fixtures by name, `from tests.gpu_arrays import q  # noqa: F401`):
the package fixture `q`, the plant steps' default-parameter handle, pools tiled to a batch size, device copies with sentinel rows
behind the batch, the second-round test of a per-robot kernel on a capped grid, and the comparison of an output against (value, bar)
references."""
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


# ------------------------------------------------------------------ the second round of a capped grid
# A per-robot kernel on capped_blocks(n, 64, 4096) one-wave workgroups walks its grid stride twice from n = 4096 x 64 + 1 on.  At
# SECOND_ROUND_N workgroup 0 walks a full second round and workgroup 1 a wave of one live lane and 63 tail lanes.  PERIOD is no
# multiple of 64, so a robot of the period lands in many lanes.  UNPLANTED: a robot of the second round and robot n - 1, whose inputs
# are replaced after the tiling - a kernel that re-read round one's robot in round two would return the tile's rows there.
SECOND_ROUND_N, PERIOD = 4096 * 64 + 65, 130
UNPLANTED = (4096 * 64 + 5, SECOND_ROUND_N - 1)


def sentinel_tensor(shape, dtype):
    """a device tensor no kernel has written: SENTINEL (float64), 0x5A (uint8), -77 (int32)"""
    import torch

    return torch.full(shape, {torch.float64: SENTINEL, torch.uint8: 0x5A, torch.int32: -77}[dtype], dtype=dtype, device="cuda")


def unwritten(t):
    """whether any entry of `t` still holds its dtype's sentinel"""
    import torch

    return bool((t == {torch.float64: SENTINEL, torch.uint8: 0x5A, torch.int32: -77}[t.dtype]).any())


def assert_same_bits(got, want, what):
    """two device tensors of one shape and dtype, equal bit for bit (a NaN equals the NaN of the same bits)"""
    import torch

    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = lambda t: (t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()).reshape(t.shape[0], -1)
    g, w = bits(got), bits(want)
    if not torch.equal(g, w):
        rows = (g != w).any(dim=1).nonzero().reshape(-1)
        raise AssertionError(f"{what}: {rows.numel()} rows differ, the first at {int(rows[0])}, the last at {int(rows[-1])}: "
                             f"{got[int(rows[0])].reshape(-1).tolist()} for {want[int(rows[0])].reshape(-1).tolist()}")


def second_round(launch, period, outside, over=False, in_place=(), n=SECOND_ROUND_N, at=UNPLANTED):
    """The second-round test of one per-robot kernel.  `launch(rows, m, over=False)` runs it on m robots - `rows` a dict of device
    tensors with m rows each, which it must not modify (what the kernel updates in place it copies first) - with every output starting
    from its sentinel, and returns the dict of everything the kernel wrote; over=True: the same with every output written over its
    input array (a copy).  `in_place`: the returned names that are such updated copies (phases, state records) and never held a
    sentinel.  `period`: the rows of the period's robots; `outside`: the rows of len(at) robots that are not in it.
    Asserted: the launches of the period and of the outside robots leave no sentinel; the launch of n robots - the period tiled on
    the device, robots `at` overwritten with the outside ones - equals, in every output and bit for bit, the period's launch tiled
    with the outside launch's rows at `at`; with over=True the n-robot launch over its inputs equals the n-robot launch beside them.
    Returns the period's outputs, for the caller's assertions about what the period holds."""
    import torch

    p = next(iter(period.values())).shape[0]
    assert set(period) == set(outside) and all(v.shape[0] == p for v in period.values()) and all(v.shape[0] == len(at) for v in outside.values())
    assert n > 4096 * 64 and p % 64 and all(0 <= i < n for i in at)
    small, pair = launch(period, p), launch(outside, len(at))
    for k in small:
        assert k in in_place or not (unwritten(small[k]) or unwritten(pair[k])), k
    index = list(at)

    def tiled(rows, two):
        out = {}
        for k, v in rows.items():
            t = v.repeat((-(-n // p),) + (1,) * (v.dim() - 1))[:n].contiguous()
            t[index] = two[k]
            out[k] = t
        return out

    big_in = tiled(period, outside)
    big = launch(big_in, n)
    want = tiled(small, pair)
    assert set(big) == set(want)
    for j, i in enumerate(index):  # the outside robots are no robots of the tile: their outputs differ from the tile's rows
        assert any(not torch.equal(pair[k][j], small[k][i % p]) for k in small), i
    for k in want:
        assert_same_bits(big[k], want[k], f"{k} at n = {n}")
    if over:
        del want
        again = launch(big_in, n, over=True)
        for k in big:
            assert_same_bits(again[k], big[k], f"{k} at n = {n}, written over its input")
    return small


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

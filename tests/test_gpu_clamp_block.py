"""-m gpu: the clamp recalculations of the racing 4-lane kernel and the loop around its recalculations (DESIGN 7 entry 28: the
running robots as the wave's lane mask, the stop test of the race as one compare; tests/test_clamp_block_cpu.py restates them
without a GPU).  Batches of the config-2 distribution at n = 1 (one robot), 4 (one full racing wave), 5 (a ragged second wave),
16 (one XCD-aligned group of waves) and 67 (a ragged last group past the XCD map's `full` boundary), cold, and n = 67 warm-started
too.

The robots are the ones tests/test_gpu_decision_block.py screens out of a 2 048-robot config-2 batch: every decision of all four
strategies' walks has a margin in the traced strategy model (oracle/prototypes: QP.eqp, the clamp of
proto_race_strategies_lib; `_walk` there), so the device must take the model's walks.  On them `iterations` is asserted EQUAL
to the model's count of the first strategy to arrive, and `active_set` EQUAL to the word of the lowest-numbered strategy among
the first - one pass too many or too few in the loop, a wrong vote or a wrong winner shows.  The wins of strategies 2 and 3 - two
and three clamp recalculations - are decided by the clamp recalculations: the robots they win come first in the order, so every
size holds one (asserted on the model, not on the device).  The 56 screened robots do not fill the batch of 67; its other 11 are
unscreened config-2 robots, spread over the waves, and held against the oracle only.

Against the C oracle, every robot: status, and forces at tests/test_gpu_ratio_block.py's bar; every face in the returned word is
a face the oracle's forces lie on.  Everything is bit-equal across two launches.

Warm: from the model's own KKT words (the device must confirm each in ONE recalculation and hand the word back, exactly), and
from the words of a slightly different previous tick (the model has no walk from a foreign set: oracle checks only).
"""
import numpy as np
import pytest

from tests.gpu_arrays import q  # noqa: F401
from tests.test_gpu_decision_block import MARGIN, STRATEGIES, _pinned_robots, _word
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

SIZES = (1, 4, 5, 16, 67)
QC_MAX_ITER, QC_NOT_PD = 1, 3

_cache = {}


def _pool(q):
    """the screened robots, those won by strategy 2 or 3 first; their model counts [k, 4] and words [k, 4]; 11 fillers"""
    if "pool" not in _cache:
        from quadruped_control_amd import workloads as W

        pin = _pinned_robots()["plain"]
        walks = pin["walks"]
        full = np.array([min(x[3] for x in w) > MARGIN for w in walks])
        counts = np.array([[x[0] for x in w] for w in walks])
        words = np.array([[_word(x[1]) for x in w] for w in walks], dtype=np.uint32)
        late = counts[:, 2:].min(axis=1) < counts[:, :2].min(axis=1)  # strategy 2 or 3 arrives strictly first
        order = np.concatenate([np.flatnonzero(full & late), np.flatnonzero(full & ~late)])
        assert len(order) >= 56 and int((full & late).sum()) >= 4, (len(order), int((full & late).sum()))
        b = {k: np.ascontiguousarray(v[order]) for k, v in pin["b"].items()}
        _cache["pool"] = (b, counts[order], words[order], W.config2(11, seed=0xC1A30043))
    return _cache["pool"]


def _batch(q, n):
    """(P, batch, oracle forces, oracle status, screened [n] bool, model counts, model words)"""
    if n not in _cache:
        from oracle import c_oracle as O

        pool, counts, words, fill = _pool(q)
        k = min(n, len(counts))
        b = {key: v[:k] for key, v in pool.items()}
        screened = np.ones(n, bool)
        src = np.arange(k)
        if n > k:  # the fillers go to every sixth place: they share their waves with screened robots
            at = np.arange(n - k) * 6 + 3
            screened[at] = False
            src = np.full(n, -1)
            src[screened] = np.arange(k)
            merged = {}
            for key, v in b.items():
                m = np.empty((n,) + v.shape[1:], v.dtype)
                m[screened] = v
                m[at] = fill[key][:n - k]
                merged[key] = np.ascontiguousarray(m)
            b = merged
        b = {key: np.ascontiguousarray(v) for key, v in b.items()}
        P = q.cheetah_params(0.6)
        ref, st, _ = O.control_batch(P, b, threads=8)
        cm = np.zeros((n, 4), int); wm = np.zeros((n, 4), np.uint32)
        cm[screened], wm[screened] = counts[:k], words[:k]
        _cache[n] = (P, b, ref, st, screened, cm, wm)
    return _cache[n]


def _model_first(cm, wm):
    """the model's race: the count of the first strategy to arrive and the word of the lowest-numbered one among the first"""
    best = cm.min(axis=1)
    win = np.argmax(cm == best[:, None], axis=1)
    return best, wm[np.arange(len(cm)), win], win


def _relerr(a, ref):
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    return float(np.max(np.abs(a - ref) / scale)) if a.size else 0.0


def _fields(words):
    """[n, 4 feet, 3 axes] fields of the working-set words: 0 free, 1 upper face, 3 lower face"""
    w = np.asarray(words).astype(np.uint32)
    return np.stack([np.stack([(w >> np.uint32(6 * k + 2 * a)) & np.uint32(3) for a in range(3)], axis=1) for k in range(4)], axis=1)


def _check(o, P, b, ref, ref_st, what):
    ok = ref_st == 0
    assert np.array_equal(o["status"], ref_st), (what, o["status"], ref_st)
    assert _relerr(o["grf_body"][ok], ref[ok]) < RTOL, what
    assert np.all(o["grf_body"][~ok] == 0.0), what
    assert np.all(o["grf_body"][np.repeat(b["stance"] == 0, 3, axis=1)] == 0.0), what
    # the working set against the faces the oracle's forces lie on (world frame: the frusta are the world's)
    words = np.asarray(o["active_set"]).astype(np.uint32)
    assert ((words[ok] >> np.uint32(31)) == 1).all(), what
    fld = _fields(words)
    assert np.isin(fld, (0, 1, 3)).all(), what
    assert np.all(fld[b["stance"] == 0] == 0), what
    Rwb = b["Rwb"].reshape(-1, 3, 3)
    fw = -np.einsum("nij,nkj->nki", Rwb, ref.reshape(-1, 4, 3))  # grf_body = -Rwb^T f
    bar = RTOL * np.maximum(1.0, np.abs(ref).max(axis=1))[:, None]
    mu, lo, hi = P["mu"], P["fzmin"], P["fzmax"]
    m = mu * fw[:, :, 2]
    for a in (0, 1):
        up, dn = fld[:, :, a] == 1, fld[:, :, a] == 3
        assert np.all(np.abs(m - fw[:, :, a])[up & ok[:, None]] <= (1.0 + mu) * bar.repeat(4, 1)[up & ok[:, None]]), (what, a)
        assert np.all(np.abs(m + fw[:, :, a])[dn & ok[:, None]] <= (1.0 + mu) * bar.repeat(4, 1)[dn & ok[:, None]]), (what, a)
    up, dn = fld[:, :, 2] == 1, fld[:, :, 2] == 3
    assert np.all(np.abs(hi - fw[:, :, 2])[up & ok[:, None]] <= bar.repeat(4, 1)[up & ok[:, None]]), what
    assert np.all(np.abs(fw[:, :, 2] - lo)[dn & ok[:, None]] <= bar.repeat(4, 1)[dn & ok[:, None]]), what


def _racing(q, P, n, warm=False):
    ctl = q.BalanceController.from_params(P)
    if warm:
        ctl = ctl.set_tuning(race=4)
    info = ctl.query_launch(n, warm=warm)
    assert info["lanes_per_robot"] == 4 and info["strategies"] == 4, info
    return ctl


@pytest.mark.parametrize("n", SIZES)
def test_cold_racing_batches_walk_the_model_and_match_the_oracle(q, n):
    P, b, ref, ref_st, scr, cm, wm = _batch(q, n)
    best, word, win = _model_first(cm[scr], wm[scr])
    # conditions of the fixture, on the model: a robot whose race is won by two or three clamp steps, at every size
    assert (win >= 2).any() and (ref_st[scr] == 0).all(), (n, win)
    if n == 67:
        assert int(scr.sum()) == 56 and set(win.tolist()) >= {0, 2, 3}
    ctl = _racing(q, P, n)
    o = ctl.control_batch_host(b, want_iterations=True, want_active_set=True)
    _check(o, P, b, ref, ref_st, n)
    it, ws = np.asarray(o["iterations"]), np.asarray(o["active_set"]).astype(np.uint32)
    print(f"n={n} iterations {it.tolist()} model {best.tolist()} winner {win.tolist()}")
    assert np.array_equal(it[scr], best), (n, np.flatnonzero(it[scr] != best), it[scr], best)
    assert np.array_equal(ws[scr], word), (n, np.flatnonzero(ws[scr] != word))
    again = ctl.control_batch_host(b, want_iterations=True, want_active_set=True)
    for k in ("grf_body", "status", "iterations", "active_set"):
        assert np.array_equal(np.asarray(o[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), (n, k)
    # the unscreened robots: no later than the one-strategy kernel, which is strategy 0 of the race
    solo = q.BalanceController.from_params(P).set_tuning(group=4, one_fill=1, race=0, clamp_steps=1).control_batch_host(b, want_iterations=True)
    assert np.array_equal(solo["status"], ref_st), n
    assert np.array_equal(np.asarray(solo["iterations"])[scr], cm[scr][:, 0]), n
    assert (it >= 1).all() and (it <= np.asarray(solo["iterations"])).all(), n


def _kkt_point_is_clear_of_every_free_face(P, b, k, word):
    """the model's f^ on the set `word`: no free coordinate within MARGIN of a bound the warm start's clamp compares it with"""
    from oracle import numpy_restatement as R
    from oracle.prototypes.prototype_as import QP

    d = R.assemble(R.cheetah_params(mu=0.6), b["Rwb"][k].reshape(3, 3), b["Rwb_d"][k].reshape(3, 3), b["x"][k], b["xdot"][k], b["w"][k],
                   b["x_d"][k], b["xdot_d"][k], b["w_d"][k], b["feet"][k], b["stance"][k])
    qp = QP(d["H"], d["g"], b["stance"][k], P["mu"], P["fzmin"], P["fzmax"])
    dec = lambda v: -1 if v == 3 else int(v)
    S = [np.array([dec((int(word) >> (6 * i + 2 * a)) & 3) for i in range(4)]) for a in range(3)]
    fh = qp.eqp(S)[0]
    scale = max(1.0, float(np.max(np.abs(fh))))
    for i in range(4):
        if not qp.st[i]:
            continue
        fz = fh[3 * i + 2]
        if S[2][i] == 0 and min(abs(fz - qp.hi), abs(fz - qp.lo)) <= MARGIN * scale:
            return False
        for a in (0, 1):
            if S[a][i] == 0 and min(abs(fh[3 * i + a] - qp.mu * fz), abs(fh[3 * i + a] + qp.mu * fz)) <= MARGIN * scale:
                return False
    return True


def test_warm_start_from_the_models_words_is_confirmed_in_one_recalculation(q):
    n = 67
    P, b, ref, ref_st, scr, cm, wm = _batch(q, n)
    _, word, _ = _model_first(cm, wm)
    sure = scr & np.array([bool(scr[k]) and _kkt_point_is_clear_of_every_free_face(P, b, k, word[k]) for k in range(n)])
    assert int(sure.sum()) >= 40, int(sure.sum())
    warm = np.where(scr, word, np.uint32(0)).astype(np.uint32)  # (the unscreened robots start cold: bit 31 clear)
    ctl = _racing(q, P, n, warm=True)
    o = ctl.control_batch_host(b, warm=warm, want_iterations=True, want_active_set=True)
    _check(o, P, b, ref, ref_st, "warm, model words")
    it, ws = np.asarray(o["iterations"]), np.asarray(o["active_set"]).astype(np.uint32)
    assert (it[sure] == 1).all(), (np.flatnonzero(it[sure] != 1), it[sure])
    assert np.array_equal(ws[sure], word[sure]), np.flatnonzero(ws[sure] != word[sure])
    again = ctl.control_batch_host(b, warm=warm, want_iterations=True, want_active_set=True)
    for k in ("grf_body", "status", "iterations", "active_set"):
        assert np.array_equal(np.asarray(o[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k


def test_warm_started_racing_batch_matches_the_oracle(q):
    n = 67
    P, b, ref, ref_st = _batch(q, n)[:4]
    prev = dict(b)
    prev["xdot_d"] = b["xdot_d"] * 0.9
    prev["x"] = b["x"] + 1e-3
    words = q.BalanceController.from_params(P).control_batch_host(prev, want_active_set=True)["active_set"]
    ctl = _racing(q, P, n, warm=True)
    o = ctl.control_batch_host(b, warm=words, want_iterations=True, want_active_set=True)
    _check(o, P, b, ref, ref_st, "warm")
    again = ctl.control_batch_host(b, warm=words, want_iterations=True, want_active_set=True)
    for k in ("grf_body", "status", "iterations", "active_set"):
        assert np.array_equal(np.asarray(o[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
    assert (np.asarray(o["iterations"]) >= 1).all()


@pytest.mark.parametrize("cap", (2, 3, 5))
def test_nan_robot_and_iteration_cap_report_as_across_the_widths(q, cap):
    """what tests/test_gpu_matrix.py::test_iteration_cap_and_bad_inputs_agree_across_widths expects of the race: bad inputs come
    back QC_NOT_PD with zero forces, a capped robot QC_MAX_ITER with zero forces and at most `cap` recalculations, and every robot
    the one-strategy kernel solves under the cap is solved, in at most as many recalculations.  Caps 2 and 3 end the race inside
    its clamp recalculations."""
    n = 67
    P, b, ref, ref_st = _batch(q, n)[:4]
    b = {k: v.copy() for k, v in b.items()}
    bad = np.array([3, 16, 66])
    b["x"][bad[::2], 1] = np.nan
    b["Rwb"][bad[1::2], 4] = np.inf
    solo = q.BalanceController.from_params(P, max_iter=cap).set_tuning(group=4, one_fill=1, race=0, clamp_steps=1).control_batch_host(b, want_iterations=True)
    ctl = q.BalanceController.from_params(P, max_iter=cap)
    info = ctl.query_launch(n)
    assert info["lanes_per_robot"] == 4 and info["strategies"] == 4, info
    r = ctl.control_batch_host(b, want_iterations=True)
    assert (solo["status"][bad] == QC_NOT_PD).all() and (r["status"][bad] == QC_NOT_PD).all()
    assert np.all(r["grf_body"][bad] == 0.0)
    assert (solo["status"] == QC_MAX_ITER).any()
    ok = solo["status"] == 0
    assert (r["status"][ok] == 0).all() and (r["iterations"][ok] <= solo["iterations"][ok]).all()
    assert np.isin(r["status"], (0, QC_MAX_ITER, QC_NOT_PD)).all()
    capped = r["status"] == QC_MAX_ITER
    assert (r["iterations"][capped] == cap).all() and (r["iterations"] <= cap).all()
    assert np.all(r["grf_body"][r["status"] != 0] == 0.0)
    good = (r["status"] == 0) & (ref_st == 0)
    good[bad] = False
    assert _relerr(r["grf_body"][good], ref[good]) < RTOL

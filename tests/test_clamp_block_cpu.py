"""No GPU: what DESIGN 7 entry 28 rewrote around the recalculations of the racing 4-lane kernel, restated on integers and held
against the forms it replaces - and the clamp block the pass read and left as it is, pinned against the prototype's clamp.

* The race's stop test: `busy & !done & (solved_mask == 0)` against the one compare `((busy & !done) ? solved_mask : 1) == 0`,
  and the vote `(busy & kkt) ? 1 << sid : 0` against `kkt ? 1 << sid : 0` with kkt = live & solved and live = busy - every
  combination of the operands.
* The loops: per-lane `busy` flags tested by a ballot at the top of `for (k ...)`, `for (it = 2; it <= 3 && ...)` and `while`
  against the wave's lane mask `running`, tested as an integer and handed to the recalculation as `live`.  A wave of four robots
  with four strategies each is walked through both drivers for EVERY combination of the recalculation in which each strategy
  arrives (1 ... 5, or never before the cap) and every cap 1 ... 6, on every robot slot: the phase of each recalculation (FIRST /
  MIXED / STEADY), `fresh` = `iters <= nclamp` for iters 1 ... 4 against nclamp 1, 2, 3, the counts, the race's masks and the
  winner are the same.
* The clamp block (clamp_foot + encode_foot, the word the clamp recalculation writes): all 27 working-set states of a foot, both
  contact states, f^ inside, on and outside every face, +-0 and NaN included - every combination, against
  oracle/prototypes/proto_race_strategies_lib.clamp_keep.  The pass weighed writing that word from the packed word's fields and
  did not take it; this holds what any later rewrite has to reproduce.
"""
import itertools

import numpy as np

from oracle.prototypes.proto_race_strategies_lib import clamp_keep

NCLAMP = (1, 1, 2, 3)  # strategies 0 ... 3 of the racing kernel (qc_balance.hip)
FIRST, MIXED, STEADY = "FIRST", "MIXED", "STEADY"


# ------------------------------------------------------------------------------------------------ the stop test and the vote
def test_stop_test_as_one_compare_and_the_vote_without_busy():
    for busy, done, mask in itertools.product((False, True), (False, True), range(16)):
        old = busy and (not done) and mask == 0
        stop = mask if (busy and not done) else 1
        assert (stop == 0) == old, (busy, done, mask)
    for busy, solved, sid in itertools.product((False, True), (False, True), range(4)):
        live = busy
        kkt = live and solved
        assert ((1 << sid) if (busy and kkt) else 0) == ((1 << sid) if kkt else 0)


# ---------------------------------------------------------------------------------------------------------------- the loops
class _Wave:
    """a racing wave: ROB = 4 robots x 4 strategies; group grp = sid * 4 + slot solves robot `slot` with strategy sid.  A
    strategy arrives (reaches the KKT point) in recalculation arrive[slot][sid]; `cap` is max_iter."""

    def __init__(self, arrive, cap, stock_n):
        self.arrive, self.cap, self.stock_n = arrive, cap, stock_n
        self.iters = [0] * 16
        self.status = [1] * 16  # QC_MAX_ITER
        self.kkt = [False] * 16
        self.mask = [0] * 16  # solved_mask per group (the same in the four groups of a robot after race_or)
        self.log = []

    def iterate(self, phase, live):
        """Lane::iterate as far as the loops see it: the count, `fresh`, the status, kkt, and the return value"""
        done, fresh = [], []
        for grp in range(16):
            slot, sid = grp % 4, grp // 4
            self.iters[grp] += 1 if live[grp] else 0
            fresh.append(True if phase == FIRST else (False if phase == STEADY else self.iters[grp] <= NCLAMP[sid]))
            solved = self.iters[grp] == self.arrive[slot][sid]
            self.kkt[grp] = live[grp] and solved
            if live[grp] and solved:
                self.status[grp] = 0
            done.append(solved or self.iters[grp] >= self.cap)
        self.log.append((phase, tuple(live), tuple(fresh)))
        return done

    def race_or(self, mine):
        return [mine[g % 4] | mine[g % 4 + 4] | mine[g % 4 + 8] | mine[g % 4 + 12] for g in range(16)]

    def result(self):
        win = [(self.mask[g] & -self.mask[g]).bit_length() - 1 if self.mask[g] else 0 for g in range(16)]
        pushed = {g % 4: (self.status[g], self.iters[g]) for g in range(16) if g % 4 < self.stock_n and g // 4 == win[g]}
        return self.log, tuple(self.mask), pushed


def _drive_flags(w):
    """the parent: per-lane `busy`, a ballot at the top of every loop"""
    busy = [g % 4 < w.stock_n for g in range(16)]

    def after(done):
        mine = [(1 << (g // 4)) if (busy[g] and w.kkt[g]) else 0 for g in range(16)]
        m = w.race_or(mine)
        for g in range(16):
            w.mask[g] |= m[g]
            busy[g] = busy[g] and (not done[g]) and w.mask[g] == 0

    k = 0
    while k < 1 and (k == 0 or any(busy)):
        after(w.iterate(FIRST, list(busy)))
        k += 1
    it = 2
    while it <= 3 and any(busy):
        after(w.iterate(MIXED, list(busy)))
        it += 1
    while any(busy):
        after(w.iterate(STEADY, list(busy)))
    return w.result()


def _drive_mask(w):
    """the result: the running robots as the wave's lane mask"""
    running = sum(1 << g for g in range(16) if g % 4 < w.stock_n)

    def after(live, done):
        mine = [(1 << (g // 4)) if w.kkt[g] else 0 for g in range(16)]
        m = w.race_or(mine)
        r = 0
        for g in range(16):
            w.mask[g] |= m[g]
            stop = w.mask[g] if (live[g] and not done[g]) else 1
            r |= (1 << g) if stop == 0 else 0
        return r

    k = 0
    while k < 1 and (k == 0 or running != 0):
        live = [bool(running >> g & 1) for g in range(16)]
        running = after(live, w.iterate(FIRST, live))
        k += 1
    it = 2
    while it <= 3 and running != 0:
        live = [bool(running >> g & 1) for g in range(16)]
        running = after(live, w.iterate(MIXED, live))
        it += 1
    while running != 0:
        live = [bool(running >> g & 1) for g in range(16)]
        running = after(live, w.iterate(STEADY, live))
    return w.result()


def test_lane_mask_loops_walk_every_race_as_the_flag_loops_did():
    never = 99
    arrivals = list(itertools.product((1, 2, 3, 4, 5, never), repeat=4))  # one robot's four strategies: 1 296 races
    fresh_seen, phases_seen, winners = set(), set(), set()
    for cap in range(1, 7):
        for k, a in enumerate(arrivals):
            # the robot under test in slot k % 4, next to three robots with other races (the wave's loops run to its slowest robot)
            arrive = [arrivals[(k * 7 + 13 * s) % len(arrivals)] for s in range(4)]
            arrive[k % 4] = a
            stock_n = 4 if k % 5 else 1 + k % 4
            old, new = _drive_flags(_Wave(arrive, cap, stock_n)), _drive_mask(_Wave(arrive, cap, stock_n))
            assert old == new, (cap, arrive, stock_n)
            log, mask, pushed = new
            assert len(log) <= cap and set(pushed) == set(range(stock_n))
            for n, (phase, live, fresh) in enumerate(log, 1):
                assert phase == (FIRST if n == 1 else (MIXED if n <= 3 else STEADY))
                phases_seen.add(phase)
                for g in range(16):
                    if live[g]:  # a live lane's count is the recalculation's number: fresh = iters <= nclamp
                        assert fresh[g] == (n <= NCLAMP[g // 4]) or phase != MIXED
                        fresh_seen.add((min(n, 4), NCLAMP[g // 4], fresh[g]))
            for slot, (status, iters) in pushed.items():
                best = min(arrive[slot])
                if best <= cap:
                    assert status == 0 and iters == best and mask[slot] == sum(1 << s for s in range(4) if arrive[slot][s] == best)
                    winners.add(arrive[slot].index(best))
                else:
                    assert status == 1 and iters == cap and mask[slot] == 0
    assert phases_seen == {FIRST, MIXED, STEADY} and winners == {0, 1, 2, 3}
    assert {(i, c) for i, c, _ in fresh_seen} == set(itertools.product((1, 2, 3, 4), (1, 2, 3)))


# ---------------------------------------------------------------------------------------------------------- the clamp block
def _clamp_foot(mu, lo, hi, wx, wy, wz, fx, fy, fz):
    """qc_device.hpp clamp_foot, statement for statement (selects: a NaN compares false everywhere)"""
    with np.errstate(all="ignore"):
        zu, zl = bool(fz > hi), bool(fz < lo)
        fz = hi if zu else (lo if zl else fz)
        sz = 1 if zu else (-1 if zl else wz)
        m = np.float64(mu) * fz
        xu, xl = bool(fx > m), bool(fx < -m)
        cx = m if xu else (-m if xl else fx)
        nx = np.float64(wx) * m if wx != 0 else cx
        sx = wx if wx != 0 else int(xu) - int(xl)
        yu, yl = bool(fy > m), bool(fy < -m)
        cy = m if yu else (-m if yl else fy)
        ny = np.float64(wy) * m if wy != 0 else cy
        sy = wy if wy != 0 else int(yu) - int(yl)
        moved = zu or zl or bool(nx != fx) or bool(ny != fy)
    return (nx, ny, fz), (sx, sy, sz), moved


def _encode(sx, sy, sz):
    return (sx & 3) | ((sy & 3) << 2) | ((sz & 3) << 4)


class _OneFoot:
    def __init__(self, st, mu, lo, hi):
        self.st, self.mu, self.lo, self.hi = [st, False, False, False], mu, lo, hi


def _same(a, b):
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def test_clamp_block_writes_the_prototypes_state_for_every_state_contact_and_point():
    mu, fzmin, fzmax = 0.6, 10.0, 160.0
    seen_fields, moved_seen, n = set(), set(), 0
    for contact in (True, False):
        lo, hi = (fzmin, fzmax) if contact else (0.0, 0.0)  # FaceConst: a swing foot's bounds are folded to 0
        zs = (lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), 0.5 * (lo + hi), lo - 3.0, hi + 3.0, 0.0, -0.0, np.nan)
        for fz in zs:
            with np.errstate(all="ignore"):
                mz = mu * min(max(fz, lo), hi) if not np.isnan(fz) else np.nan
            m = 1.0 if np.isnan(mz) else mz
            ts = (m, -m, np.nextafter(m, np.inf), np.nextafter(-m, -np.inf), 0.5 * m, m + 2.0, -m - 2.0, 0.0, -0.0, np.nan)
            for fx, fy in itertools.product(ts, repeat=2):
                for wx, wy, wz in itertools.product((-1, 0, 1), repeat=3):
                    f, s, moved = _clamp_foot(mu, lo, hi, wx, wy, wz, fx, fy, fz)
                    n += 1
                    word = _encode(*s)
                    assert all(((word >> (2 * a)) & 3) in (0, 1, 3) for a in range(3))
                    seen_fields.add(word)
                    moved_seen.add(moved)
                    # a kept face stays; a free axis takes the violated face; Z takes its violated face over whatever it had
                    assert (s[0] == wx if wx else s[0] in (-1, 0, 1)) and (s[1] == wy if wy else True)
                    if contact and not (np.isnan(fx) or np.isnan(fy) or np.isnan(fz)):
                        S = [np.array([wx, 0, 0, 0]), np.array([wy, 0, 0, 0]), np.array([wz, 0, 0, 0])]
                        fh = np.zeros(12); fh[:3] = (fx, fy, fz)
                        pf, pS, pm = clamp_keep(_OneFoot(True, mu, lo, hi), fh, S)
                        assert (int(pS[0][0]), int(pS[1][0]), int(pS[2][0])) == s, (wx, wy, wz, fx, fy, fz)
                        assert bool(pm) == moved and all(_same(pf[k], f[k]) for k in range(3)), (wx, wy, wz, fx, fy, fz)
    assert n == 2 * 10 * 100 * 27 and moved_seen == {True, False} and len(seen_fields) == 27

"""The complete tick with a host-supplied desired state (qc_control_batch) against commander mode (qc_tick_batch, a fresh command
for every robot every tick: the worst case - every robot integrates its twist and stores a new desired state), config-3 inputs
with the gait clock running, as bench.py's `--tick full` builds them, in rotating input sets larger than the caches.

HIP events around K launches after >= 25 ms of untimed launches; the two variants alternate, R rounds.  Prints one JSON line per
batch size.  usage: python tools/commander_tick_bench.py [--sizes 65536,262144] [--steps 200] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(q, ctl, n, sets, fresh_frac):
    import torch

    import bench

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    plain, cmd = [], []
    keep = []
    for j in range(sets):
        b = bench.make_tick_batch(3, n, 0, "full", j)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
        d["swing_state"] = torch.from_numpy(q.new_swing_states(n).view(np.uint8).copy()).to(dev)
        out = {"grf_body": torch.empty((n, 12), dtype=torch.float64, device=dev), "status": torch.empty((n,), dtype=torch.int32, device=dev),
               "joint_tau": torch.empty((n, 12), dtype=torch.float64, device=dev)}
        plain.append(ctl.plan_batch(d, out=out)[0])
        # commander mode on the same robots: running, the desired state the host path is given, a fresh command every tick
        s = q.new_commander_states(n)
        s["standing"] = s["gait_running"] = 1
        for k in ("Rwb_d", "x_d", "xdot_d", "w_d"):
            s[k] = b[k]
        twist = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.1, 0.1, n), np.zeros(n), rng.uniform(-0.02, 0.02, n),
                          rng.uniform(-0.02, 0.02, n), rng.uniform(-0.05, 0.05, n)], axis=1)
        dc = {k: v for k, v in d.items() if k not in ("Rwb_d", "x_d", "xdot_d", "w_d")}
        dc["gait_phase"] = d["gait_phase"].clone()
        dc["swing_state"] = d["swing_state"].clone()
        command = dict(state=torch.from_numpy(s.view(np.uint8).copy()).to(dev), twist=torch.from_numpy(twist).to(dev),
                       fresh=torch.from_numpy((rng.uniform(size=n) < fresh_frac).astype(np.uint8)).to(dev))
        outc = {k: torch.empty_like(v) for k, v in out.items()}
        cmd.append(ctl.plan_tick(dc, command, out=outc)[0])
        keep.append((d, dc, command, out, outc))
    return plain, cmd, keep


def timed(launches, steps):
    import torch

    t_end = time.perf_counter() + 0.025  # >= 25 ms of untimed launches: clocks up, caches in their rotating steady state
    i = 0
    while time.perf_counter() < t_end or i < len(launches):
        launches[i % len(launches)]()
        i += 1
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(steps):
        launches[(i + k) % len(launches)]()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=512)
    ap.add_argument("--fresh", type=float, default=1.0, help="fraction of robots with a fresh command every tick (1 = worst case)")
    args = ap.parse_args()
    import quadruped_control_amd as q

    ctl = q.BalanceController.from_params(q.cheetah_params(0.6))
    for n in [int(v) for v in args.sizes.split(",")]:
        per_robot = 1005 + 208 + 56  # the plain tick's algorithmic bytes + a commander record + twist and fresh
        sets = max(2, (args.rotate_mb << 20) // (per_robot * n) + 1)
        plain, cmd, keep = build(q, ctl, n, sets, args.fresh)
        rows = {"plain": [], "commander": []}
        for r in range(args.rounds):
            order = (("plain", plain), ("commander", cmd)) if r % 2 == 0 else (("commander", cmd), ("plain", plain))
            for name, launches in order:
                rows[name].append(timed(launches, args.steps))
        med = {k: float(np.median(v)) for k, v in rows.items()}
        print(json.dumps({"n": n, "fresh": args.fresh, "sets": sets, "steps": args.steps, "rounds": args.rounds, "launch": ctl.query_launch(n, kin=True),
                          "us_per_tick_median": med, "us_per_tick_all": rows,
                          "commander_over_plain": med["commander"] / med["plain"] - 1.0}), flush=True)
        del plain, cmd, keep


if __name__ == "__main__":
    main()

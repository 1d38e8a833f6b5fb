"""Timings behind profiles/plant_step.md: the plant kernel alone, one closed-loop step (solve + plant), and control_batch alone.

  python tools/plant_bench.py --out plant.json                     # everything, on the tree's own package
  python tools/plant_bench.py --solve-only --package-root DIR      # control_batch alone on another checkout's package (an A/B
                                                                   # against the parent commit in the same session)

HIP events around `reps` back-to-back launches after at least 25 ms of warm-up; `rounds` such windows per figure, median and
minimum reported.  Bytes are the algorithm's: 336 B read and 240 B written per robot and plant step."""
import argparse
import json
import os
import statistics
import sys
import time

PLANT_BYTES = 336 + 240
HBM_PEAK = 8.0e12  # B/s, the MI355X's specified peak


def timed(torch, launch, rounds=7, window_ms=20.0, reset=None):
    """us per launch(): (median, min) over `rounds` windows of at least window_ms each"""
    t0 = time.perf_counter()
    n_warm = 0
    while (time.perf_counter() - t0) * 1e3 < 25.0 or n_warm < 10:
        launch()
        n_warm += 1
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        launch()
    b.record()
    torch.cuda.synchronize()
    reps = max(10, int(window_ms / max(a.elapsed_time(b) / 10, 1e-4)))
    out = []
    for _ in range(rounds):
        if reset is not None:
            reset()
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return dict(median_us=statistics.median(out), min_us=min(out), reps=reps, rounds=rounds)


def solve_cases(q, workloads, torch):
    """control_batch alone: config 2 (4 096 robots, cold) and config 4's second tick warm-started from the first (262 144)"""
    res = {}
    ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
    dev = q.to_device(workloads.config2(n=4096))
    launch, _ = ctl.plan_batch(dev)
    res["control_batch config2 n=4096 cold"] = timed(torch, launch)
    t0, t1 = workloads.config4(n=262144)
    first = ctl.control_batch(q.to_device(t0), want_active_set=True)
    torch.cuda.synchronize()
    launch, _ = ctl.plan_batch(q.to_device(t1), warm=first["active_set"])
    res["control_batch config4 n=262144 warm"] = timed(torch, launch)
    ctl.close()
    return res


def world_feet(np, b):
    n = b["x"].shape[0]
    R = b["Rwb"].reshape(n, 3, 3)
    return np.ascontiguousarray((b["x"][:, None, :] + np.einsum("nij,nlj->nli", R, b["feet"].reshape(n, 4, 3))).reshape(n, 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--solve-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "plant_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"package_root": args.package_root, "device": torch.cuda.get_device_name(0)}
    res.update(solve_cases(q, workloads, torch))
    if not args.solve_only:
        ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
        for n in args.sizes:  # the plant kernel alone, on the forces of a solve of that batch
            b = workloads.config2(n=n)
            dev = q.to_device(b)
            out = ctl.control_batch(dev)
            pw = torch.from_numpy(world_feet(np, b)).cuda()
            state = {k: dev[k] for k in ("Rwb", "x", "xdot", "w")}
            start = {k: t.clone() for k, t in state.items()}
            launch = ctl.plan_plant(state, out["grf_body"], pw, 1.0 / 300.0, dev["feet"])

            def reset():
                for k, t in state.items():
                    t.copy_(start[k])

            r = timed(torch, launch, reset=reset)
            r["bytes_per_robot"] = PLANT_BYTES
            r["GBps_median"] = PLANT_BYTES * n / r["median_us"] * 1e-3
            r["fraction_of_hbm_peak_median"] = PLANT_BYTES * n / (r["median_us"] * 1e-6) / HBM_PEAK
            r["fraction_of_hbm_peak_min_time"] = PLANT_BYTES * n / (r["min_us"] * 1e-6) / HBM_PEAK
            res[f"plant_step n={n}"] = r
        # one closed-loop step = one solve + one plant step, as rollout() issues them
        for name, b, warm in (("config2 n=4096 cold", workloads.config2(n=4096), False), ("config4 n=262144 warm", workloads.config4(n=262144)[0], True)):
            dev = q.to_device(b)
            pw = torch.from_numpy(world_feet(np, b)).cuda()
            start = {k: dev[k].clone() for k in ("Rwb", "x", "xdot", "w", "feet")}
            steps = 200
            box = {}

            def launch():
                for k, t in start.items():
                    dev[k].copy_(t)
                box["out"] = ctl.rollout(dev, pw, steps=steps, dt=1.0 / 300.0, warm=warm)[1]

            r = timed(torch, launch, window_ms=100.0)
            r = {k: (v / steps if k.endswith("_us") else v) for k, v in r.items()}
            r["steps_per_launch"] = steps
            r["solved_fraction_last_step"] = float((box["out"]["status"] == 0).float().mean().item())
            res[f"closed-loop step (solve + plant, {steps}-step rollouts incl. their marshalling) {name}"] = r
        ctl.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

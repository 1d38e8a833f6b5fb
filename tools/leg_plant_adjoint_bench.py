"""Timings behind profiles/leg_plant_adjoint.md: the legged plant step's reverse pass (qc_leg_plant_step_adjoint_batch) next to the
forward leg plant kernel, in one session.

  python tools/leg_plant_adjoint_bench.py --out leg_plant_adjoint.json

tools/plant_adjoint_bench.py's protocol: HIP events around back-to-back launches after a warm-up, `rounds` windows, median and
minimum, both kernels over a ROTATION of independent copies of their arrays whose footprint is at least --footprint bytes, so that
no launch finds its inputs in the last-level cache.  The forward kernel steps each copy once per rotation and is not reset; it runs
with dt = 1e-9 so that thousands of steps leave the legs where they are (dt is a kernel argument: it changes no instruction).  All
stance, stance bytes given.  Bytes are the algorithm's: the forward step reads 54 doubles and 4 bytes and writes 42 doubles and the
flags per robot; the reverse pass, with every cotangent given and every output asked for, reads 42 + 42 doubles (joint_qdot is not
read) and 4 bytes and writes 54 doubles and the flags."""
import argparse
import json
import os
import sys

FORWARD_BYTES = 54 * 8 + 4 + 42 * 8 + 4
ADJOINT_BYTES = 84 * 8 + 4 + 54 * 8 + 4
HBM_PEAK = 8.0e12  # B/s, the MI355X's specified peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--footprint", type=float, default=1.0e9, help="bytes all rotated copies together must exceed")
    ap.add_argument("--max-copies", type=int, default=512)
    args = ap.parse_args()
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from tools.plant_bench import timed

    assert torch.cuda.is_available(), "leg_plant_adjoint_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"device": torch.cuda.get_device_name(0), "footprint_bytes": args.footprint}
    ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
    dt, inertia = 1.0 / 300.0, 0.02
    names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
    sizes = (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("joint_q", 12), ("joint_qdot", 12))
    for n in args.sizes:
        dev = q.to_device(workloads.with_joint_angles(workloads.config2(n=n)))
        dev["joint_qdot"] = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        tau = ctl.control_batch({k: v for k, v in dev.items() if k != "joint_qdot"}, want_torques=True)["joint_tau"]
        stance = torch.ones((n, 4), dtype=torch.uint8, device="cuda")
        copies = int(min(args.max_copies, max(2, -(-args.footprint // (ADJOINT_BYTES * n)))))
        gen = torch.Generator(device="cuda").manual_seed(n)
        fwd, adj, flagged = [], [], 0
        for _ in range(copies):
            state = {k: dev[k].clone() for k in names}
            t, st = tau.clone(), stance.clone()
            flags = torch.zeros((n,), dtype=torch.int32, device="cuda")
            fwd.append(ctl.plan_leg_plant({k: v.clone() for k, v in state.items()}, t, 1e-9, inertia, stance=st, flags=torch.zeros_like(flags)))
            cot = {k: torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen) for k, m in sizes}
            launch, _ = ctl.plan_leg_plant_adjoint(state, t, dt, inertia, cot, stance=st, flags=flags)
            launch()
            flagged = int((flags != 0).sum().item())
            adj.append(launch)
        for name, launches, nbytes in (("leg_plant_step", fwd, FORWARD_BYTES), ("leg_plant_step_adjoint", adj, ADJOINT_BYTES)):
            turn = [0]

            def launch():
                launches[turn[0] % copies]()
                turn[0] += 1

            r = timed(torch, launch)
            r.update(copies=copies, bytes_per_robot=nbytes, GBps_median=nbytes * n / r["median_us"] * 1e-3,
                     fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK, flagged_robots=flagged)
            res[f"{name} n={n}"] = r
        res[f"ratio n={n}"] = res[f"leg_plant_step_adjoint n={n}"]["median_us"] / res[f"leg_plant_step n={n}"]["median_us"]
        del fwd, adj
        torch.cuda.empty_cache()
    ctl.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Timings behind profiles/plant_adjoint.md: the plant step's reverse pass (qc_plant_step_adjoint_batch) next to the forward plant
kernel, in one session.

  python tools/plant_adjoint_bench.py --out plant_adjoint.json

tools/plant_bench.py's protocol (HIP events around back-to-back launches after a warm-up, `rounds` windows, median and minimum), with
one addition: both kernels run over a ROTATION of independent copies of their arrays, enough of them that a launch never finds its
inputs in the 256 MB last-level cache from the launch before (the footprint of all copies is at least --footprint bytes), so the
figures are HBM figures at every batch size.  The forward kernel therefore steps each copy once per rotation and is not reset: its
states drift, which changes no instruction it executes.  Bytes are the algorithm's: the forward step reads 336 B and writes 240 B
per robot; the reverse pass, with every cotangent given and every output asked for, reads 336 + 240 B and writes 336 B.
control_batch and plant_step against another checkout: tools/plant_bench.py --package-root DIR."""
import argparse
import json
import os
import sys

FORWARD_BYTES = 336 + 240
ADJOINT_BYTES = 336 + 240 + 336
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
    import numpy as np
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from tools.plant_bench import timed, world_feet

    assert torch.cuda.is_available(), "plant_adjoint_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"device": torch.cuda.get_device_name(0), "footprint_bytes": args.footprint}
    ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
    dt = 1.0 / 300.0
    for n in args.sizes:
        b = workloads.config2(n=n)
        dev = q.to_device(b)
        grf = ctl.control_batch(dev)["grf_body"]
        pw = torch.from_numpy(world_feet(np, b)).cuda()
        copies = int(min(args.max_copies, max(2, -(-args.footprint // (ADJOINT_BYTES * n)))))
        gen = torch.Generator(device="cuda").manual_seed(n)
        fwd, adj = [], []
        for _ in range(copies):
            state = {k: dev[k].clone() for k in ("Rwb", "x", "xdot", "w")}
            g, p = grf.clone(), pw.clone()
            fwd.append(ctl.plan_plant({k: t.clone() for k, t in state.items()}, g, p, dt, torch.zeros_like(p)))
            cot = {k: torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("feet", 12))}
            adj.append(ctl.plan_plant_adjoint(state, g, p, dt, cot)[0])
        for name, launches, nbytes in (("plant_step", fwd, FORWARD_BYTES), ("plant_step_adjoint", adj, ADJOINT_BYTES)):
            turn = [0]

            def launch():
                launches[turn[0] % copies]()
                turn[0] += 1

            r = timed(torch, launch)
            r.update(copies=copies, bytes_per_robot=nbytes, GBps_median=nbytes * n / r["median_us"] * 1e-3,
                     fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                     fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
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

"""Timings behind profiles/plant_tangent.md: the plant step's forward mode (qc_plant_step_tangent_batch) at K = 1 and K = 12 next to
12 launches of its reverse pass and to the forward plant kernel, and one closed-loop step of rollout_tangent at K = 12 next to one
step of ctl.rollout and to forward plus backward of one rollout_autograd step, in one session.

  python tools/plant_tangent_bench.py --out plant_tangent.json

tools/plant_adjoint_bench.py's protocol: HIP events around back-to-back launches after a warm-up, median and minimum, every kernel
over a ROTATION of independent copies of its arrays whose footprint is at least --footprint bytes (512 MiB), so that a launch never
finds its inputs in the last-level cache.  Bytes are the algorithm's: per (robot, direction) the forward mode reads the 336 B of base
state (from L2 for all directions but the first) and 288 B of tangents and writes 144 B in place; per robot the forward step reads
336 B and writes 240 B.  The closed-loop figures time the launches of one step, planned once as the rollouts plan them, on one copy of
the batch (warm cache: the solve dominates); the reverse-mode figure is one step of rollout_autograd, forward plus backward, Python's
autograd included."""
import argparse
import json
import os
import sys

PAIR_BYTES = 336 + 288 + 144
FORWARD_BYTES = 336 + 240
HBM_PEAK = 8.0e12  # B/s, the MI355X's specified peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--footprint", type=float, default=512.0 * 2 ** 20, help="bytes all rotated copies together must exceed")
    ap.add_argument("--max-copies", type=int, default=256)
    args = ap.parse_args()
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import tangent as T
    from quadruped_control_amd import workloads
    from tools.plant_bench import timed, world_feet

    assert torch.cuda.is_available(), "plant_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"device": torch.cuda.get_device_name(0), "footprint_bytes": args.footprint}
    ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
    dt = 1.0 / 300.0
    for n in args.sizes:
        b = workloads.config2(n=n)
        dev = q.to_device(b)
        grf = ctl.control_batch(dev)["grf_body"]
        pw = torch.from_numpy(world_feet(np, b)).cuda()
        gen = torch.Generator(device="cuda").manual_seed(n)
        sets = {}
        for K in (1, 12):
            copies = int(min(args.max_copies, max(2, -(-args.footprint // (PAIR_BYTES * n * K)))))
            launches = []
            for _ in range(copies):
                state = {k: dev[k].clone() for k in ("Rwb", "x", "xdot", "w")}
                tans = {k: torch.randn((K, n, m), dtype=torch.float64, device="cuda", generator=gen) for k, m in T.PLANT_TANGENTS.items()}
                out = {"Rwb_rot_next_tan": tans["Rwb_rot_tan"], "x_next_tan": tans["x_tan"], "xdot_next_tan": tans["xdot_tan"], "w_next_tan": tans["w_tan"],
                       "feet_next_tan": tans["foot_world_tan"]}  # in place, as a rollout runs it (the values drift; no instruction changes)
                launches.append(T.plan_plant_step_tangent(ctl, state, grf.clone(), pw.clone(), dt, tans, out=out)[0])
            sets[f"plant_step_tangent K={K}"] = (launches, PAIR_BYTES * K)
        copies = int(min(args.max_copies, max(2, -(-args.footprint // (912 * n)))))
        fwd, adj = [], []
        for _ in range(copies):
            state = {k: dev[k].clone() for k in ("Rwb", "x", "xdot", "w")}
            g, p = grf.clone(), pw.clone()
            fwd.append(ctl.plan_plant({k: t.clone() for k, t in state.items()}, g, p, dt, torch.zeros_like(p)))
            cot = {k: torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("feet", 12))}
            one = ctl.plan_plant_adjoint(state, g, p, dt, cot)[0]
            adj.append(lambda one=one: [one() for _ in range(12)])
        sets["plant_step"] = (fwd, FORWARD_BYTES)
        sets["12 x plant_step_adjoint"] = (adj, 12 * 912)
        for name, (launches, nbytes) in sets.items():
            turn = [0]

            def launch():
                launches[turn[0] % len(launches)]()
                turn[0] += 1

            r = timed(torch, launch)
            r.update(copies=len(launches), bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
        del sets, fwd, adj
        torch.cuda.empty_cache()
        # one closed-loop step, the launches planned once as the rollouts plan them (cold solves; the state advances in place and
        # settles, which changes the solves' iteration counts a little and nothing else), under the same protocol
        K = 12
        d = q.to_device(b)
        state = {k: d[k] for k in ("Rwb", "x", "xdot", "w")}
        solve, out = ctl.plan_batch(d)
        step = ctl.plan_plant(state, out["grf_body"], pw, dt, d["feet"])
        seeds = T.transition_seeds(d, pw)
        grf_tan = torch.zeros((K, n, 4, 3), dtype=torch.float64, device="cuda")
        solve_tan = T.plan_tangent(ctl, d, out["grf_body"], seeds, ("grf_tan",), out={"grf_tan": grf_tan})[0]
        plant_in = dict({k: seeds[k] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan")}, grf_tan=grf_tan)
        plant_out = {"Rwb_rot_next_tan": seeds["Rwb_rot_tan"], "x_next_tan": seeds["x_tan"], "xdot_next_tan": seeds["xdot_tan"], "w_next_tan": seeds["w_tan"],
                     "feet_next_tan": seeds["feet_tan"]}
        step_tan = T.plan_plant_step_tangent(ctl, state, out["grf_body"], pw, dt, plant_in, out=plant_out)[0]

        def closed_loop():
            solve()
            step()

        def closed_loop_tangent():
            solve()
            solve_tan()
            step_tan()
            step()

        start = q.to_device(b)
        leaves = dict(start, **{k: start[k].clone().requires_grad_(True) for k in ("x", "xdot", "w")})

        def reverse():
            final, _ = ctl.rollout_autograd(leaves, pw, 1, dt, warm=False)
            sum(final[k].sum() for k in ("Rwb", "x", "xdot", "w")).backward()

        res[f"closed-loop step: control_batch + plant_step n={n}"] = timed(torch, closed_loop)
        res[f"closed-loop step with tangents K=12 (4 launches) n={n}"] = timed(torch, closed_loop_tangent)
        res[f"rollout_autograd, one step forward + backward n={n}"] = timed(torch, reverse)
    ctl.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

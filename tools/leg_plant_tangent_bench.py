"""Timings behind profiles/leg_plant_tangent.md: the forward mode around the tick - qc_torque_tangent_batch and
qc_leg_plant_step_tangent_batch at K = 1 and K = 12 next to 12 launches of qc_leg_plant_step_adjoint_batch, and one closed tick step
of rollout_tick_tangent with the 36 tangents of a transition matrix next to one step of ctl.rollout_tick and to forward plus backward
of one rollout_tick_autograd step, in one session.

  python tools/leg_plant_tangent_bench.py --out leg_plant_tangent.json

tools/plant_tangent_bench.py's protocol: HIP events around back-to-back launches after a warm-up, median and minimum, every kernel
over a ROTATION of independent copies of its arrays whose footprint is at least --footprint bytes (512 MiB), so that a launch never
finds its inputs in the last-level cache.  All stance, stance bytes given; the tangent kernels write separate output arrays, so the
values a launch reads never change.  Bytes are the algorithm's: per (robot, direction) the leg plant's forward mode reads 340 B of
base state (42 doubles and the stance bytes; from L2 for all directions but the first), 384 B of tangents and writes 288 B; the
torque map's reads 200 B of base (joint_q, grf_body, status, stance), 192 B of tangents and writes 96 B; the reverse pass reads
84 doubles and writes 54.  The closed-loop figures time the launches of one step, planned once as the rollouts plan them, on one copy
of the batch (warm cache); the reverse-mode figure is one step of rollout_tick_autograd, forward plus backward, Python's autograd
included."""
import argparse
import json
import os
import sys

LEG_PAIR_BYTES = 340 + 384 + 288
TORQUE_PAIR_BYTES = 200 + 192 + 96
ADJOINT_BYTES = 84 * 8 + 4 + 54 * 8 + 4
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
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import tangent as T
    from quadruped_control_amd import workloads
    from tools.plant_bench import timed

    assert torch.cuda.is_available(), "leg_plant_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"device": torch.cuda.get_device_name(0), "footprint_bytes": args.footprint}
    ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
    dt, inertia = 1.0 / 300.0, 0.02
    names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
    for n in args.sizes:
        host = workloads.with_joint_angles(workloads.config2(n=n))
        dev = q.to_device(host)
        dev["joint_qdot"] = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        tick_in = {k: v for k, v in dev.items() if k != "joint_qdot"}
        solved = ctl.control_batch(tick_in, want_torques=True)
        stance = torch.ones((n, 4), dtype=torch.uint8, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(n)
        rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)
        sets = {}
        for K in (1, 12):
            copies = int(min(args.max_copies, max(2, -(-args.footprint // (LEG_PAIR_BYTES * n * K)))))
            leg, torque = [], []
            for _ in range(copies):
                state = {k: dev[k].clone() for k in names}
                tans = {k: rnd(K, n, m) for k, m in T.LEG_PLANT_TANGENTS.items()}
                leg.append(T.plan_leg_plant_step_tangent(ctl, state, solved["joint_tau"].clone(), dt, inertia, tans, stance=stance.clone())[0])
            copies = int(min(args.max_copies, max(2, -(-args.footprint // (TORQUE_PAIR_BYTES * n * K)))))
            for _ in range(copies):
                b = {"joint_q": dev["joint_q"].clone(), "stance": stance.clone()}
                torque.append(T.plan_torque_tangent(ctl, b, solved["grf_body"].clone(), solved["status"].clone(), {"grf_tan": rnd(K, n, 12), "joint_q_tan": rnd(K, n, 12)})[0])
            sets[f"leg_plant_step_tangent K={K}"] = (leg, LEG_PAIR_BYTES * K)
            sets[f"torque_tangent K={K}"] = (torque, TORQUE_PAIR_BYTES * K)
        copies = int(min(args.max_copies, max(2, -(-args.footprint // (ADJOINT_BYTES * n)))))
        adj = []
        for _ in range(copies):
            state = {k: dev[k].clone() for k in names}
            cot = {k: rnd(n, m) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("joint_q", 12), ("joint_qdot", 12))}
            one = ctl.plan_leg_plant_adjoint(state, solved["joint_tau"].clone(), dt, inertia, cot, stance=stance.clone())[0]
            adj.append(lambda one=one: [one() for _ in range(12)])
        sets["12 x leg_plant_step_adjoint"] = (adj, 12 * ADJOINT_BYTES)
        for name, (launches, nbytes) in sets.items():
            turn = [0]

            def launch():
                launches[turn[0] % len(launches)]()
                turn[0] += 1

            r = timed(torch, launch)
            r.update(copies=len(launches), bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
        del sets, adj
        torch.cuda.empty_cache()
        # one closed tick step, the launches planned once as the rollouts plan them (cold solves; dt = 1e-9 for the plant so that
        # thousands of steps leave the robot where it is - dt is a kernel argument: it changes no instruction), 36 unit seeds
        K = 36
        d = q.to_device(host)
        d["joint_qdot"] = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        d["stance"] = stance
        state = {k: d[k] for k in names}
        tick = {k: v for k, v in d.items() if k != "joint_qdot"}
        solve, out = ctl.plan_batch(tick, want_torques=True)
        step = ctl.plan_leg_plant(state, out["joint_tau"], 1e-9, inertia, stance=stance)
        seeds = T.tick_transition_seeds(n, d["x"].device)
        grf_tan, tau_tan = (torch.zeros((K, n, 4, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        nxt = {k[:-4] + "_next_tan": torch.zeros_like(v) for k, v in seeds.items()}
        solve_tan = T.plan_tangent(ctl, tick, out["grf_body"], {k: seeds[k] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan")}, ("grf_tan",),
                                   out={"grf_tan": grf_tan})[0]
        torque_tan = T.plan_torque_tangent(ctl, tick, out["grf_body"], out["status"], {"grf_tan": grf_tan, "joint_q_tan": seeds["joint_q_tan"]},
                                           out={"joint_tau_tan": tau_tan})[0]
        step_tan = T.plan_leg_plant_step_tangent(ctl, state, out["joint_tau"], 1e-9, inertia, dict(seeds, joint_tau_tan=tau_tan), stance=stance, out=nxt)[0]

        def closed_loop():
            solve()
            step()

        def closed_loop_tangent():
            solve()
            solve_tan()
            torque_tan()
            step_tan()
            step()

        start = q.to_device(host)
        start["joint_qdot"] = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
        start["stance"] = stance
        leaves = dict(start, **{k: start[k].clone().requires_grad_(True) for k in ("x", "xdot", "w", "joint_q")})

        def reverse():
            final, _ = ctl.rollout_tick_autograd(leaves, 1, dt, inertia, warm=False)
            sum(final[k].sum() for k in names).backward()

        res[f"closed tick step: control_batch + leg_plant_step n={n}"] = timed(torch, closed_loop)
        res[f"closed tick step with tangents K=36 (5 launches) n={n}"] = timed(torch, closed_loop_tangent)
        res[f"rollout_tick_autograd, one step forward + backward n={n}"] = timed(torch, reverse)
        del seeds, grf_tan, tau_tan, nxt
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

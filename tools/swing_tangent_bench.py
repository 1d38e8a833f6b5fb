"""Timings behind profiles/swing_tangent.md: qc_swing_torque_tangent_batch at K = 1 and K = 12 on 4 096, 65 536 and 262 144 robots of
config 3 with joint angles and swing references inside reach (tools/sensitivity_swing_bench.py's), on a trot mask (the two diagonals
in turn) and with all four legs swinging; next to it, in the same process and under the same protocol, 12 launches of
qc_sensitivity_swing_batch; and one closed trot step with the 36 tangents of a transition matrix next to one step of
rollout_tick_autograd, forward plus backward.

  python tools/swing_tangent_bench.py --out swing_tangent.json

Cold-cache protocol (tools/sensitivity_swing_bench.py's): the launches rotate through distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache -, every set is touched once before timing; one HIP event pair per launch, so the figure
INCLUDES the launch itself.  Bytes are the algorithm's, per (direction, robot, leg) ROW, for the call rollout_swing_tangent() makes
(every tangent given, joint_tau_tan written over joint_tau_tan_in):
  base     a quarter of Rwb 72 + x 24 + stance 4 (one robot's, read by its four rows), joint_q, joint_qdot, swing_pos, swing_vel 4 x 24: 121 B -
           from L2 for every direction but the first
  tangents a quarter of Rwb_rot_tan 24 + x_tan 24, five per-leg rows 5 x 24: 132 B;  written 24 B                                277 B
A stance row reads its 24 B of joint_tau_tan_in and the mask byte and writes 24 B; the count above is the swing row's, so the
all-swing figures are the ones to read against the HBM peak.  The closed-loop figures time the launches of one step, planned once as
the rollouts plan them, on one copy of the batch (warm cache); the reverse-mode figure is one step of rollout_tick_autograd, forward
plus backward, Python's autograd included."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, timed  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402
from sensitivity_swing_bench import BYTES as ADJOINT_BYTES  # noqa: E402
from sensitivity_swing_bench import swing_references  # noqa: E402

ROW_BYTES = (72 + 24 + 4) // 4 + 4 * 24 + (24 + 24) // 4 + 5 * 24 + 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--max-sets", type=int, default=256)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import tangent as T
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "swing_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    res = {"device": torch.cuda.get_device_name(0), "row_bytes": ROW_BYTES}
    dt, inertia = 1.0 / 300.0, 0.02
    names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        host = workloads.with_joint_angles(workloads.config3(n=n))
        host.pop("feet", None)
        host["swing_pos"], host["swing_vel"] = swing_references(q, host), np.zeros((n, 12))
        host["joint_qdot"] = np.zeros((n, 12))
        stance = {"trot": np.where((np.arange(n) % 2 == 0)[:, None], [1, 0, 0, 1], [0, 1, 1, 0]).astype(np.uint8), "all-swing": np.zeros((n, 4), np.uint8)}
        base = q.to_device(host)
        swing_only = {k: base[k] for k in ("Rwb", "x", "joint_q", "joint_qdot", "swing_pos", "swing_vel")}
        plans = {}
        for m in ("trot", "all-swing"):
            for K in (1, 12):
                sets = int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (4 * n * K * ROW_BYTES)))))
                for _ in range(sets):
                    dev = dict({key: v.clone() for key, v in swing_only.items()}, stance=torch.from_numpy(stance[m]).cuda())
                    tans = {k: rnd(K, n, w) for k, w in T.SWING_TORQUE_TANGENTS.items()}
                    plans.setdefault((f"swing_torque_tangent K={K} {m}", 4 * K * ROW_BYTES), []).append(
                        T.plan_swing_torque_tangent(ctl, dev, tans, out={"joint_tau_tan": tans["joint_tau_tan_in"]})[0])
            sets = int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * ADJOINT_BYTES)))))
            for _ in range(sets):
                dev = dict({key: v.clone() for key, v in swing_only.items()}, stance=torch.from_numpy(stance[m]).cuda())
                tb, qin, rin, xin = rnd(n, 12), rnd(n, 4, 3), rnd(n, 9), rnd(n, 3)
                out = {"swing_pos_bar": rnd(n, 4, 3), "swing_vel_bar": rnd(n, 4, 3), "joint_q_bar": qin, "joint_qdot_bar": rnd(n, 4, 3), "Rwb_bar": rin, "x_bar": xin}
                one = ctl.plan_sensitivity_swing(dev, tb, out=out, joint_q_bar_in=qin, Rwb_bar_in=rin, x_bar_in=xin)[0]
                plans.setdefault((f"12 x sensitivity_swing {m}", 12 * ADJOINT_BYTES), []).append(lambda one=one: [one() for _ in range(12)])
        torch.cuda.synchronize()
        for (name, nbytes), launches in plans.items():
            r = timed_rotating(torch, launches, args.launches)
            r.update(sets=len(launches), bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
            print(json.dumps({f"{name} n={n}": r}), flush=True)
        del plans
        torch.cuda.empty_cache()
        # one closed trot step, the launches planned once as rollout_swing_tangent() plans them (cold solves; dt = 1e-9 for the plant so
        # that thousands of steps leave the robot where it is - dt is a kernel argument: it changes no instruction), 36 unit seeds
        K = 36
        d = dict(q.to_device(host), stance=torch.from_numpy(stance["trot"]).cuda())
        state = {k: d[k] for k in names}
        solve, out = ctl.plan_batch(d, want_torques=True)
        step = ctl.plan_leg_plant(state, out["joint_tau"], 1e-9, inertia, stance=d["stance"])
        seeds = T.tick_transition_seeds(n, d["x"].device)
        grf_tan, tau_tan = (torch.zeros((K, n, 4, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        nxt = {k[:-4] + "_next_tan": torch.zeros_like(v) for k, v in seeds.items()}
        solve_tan = T.plan_tangent(ctl, d, out["grf_body"], {k: seeds[k] for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan")}, ("grf_tan",),
                                   out={"grf_tan": grf_tan})[0]
        torque_tan = T.plan_torque_tangent(ctl, d, out["grf_body"], out["status"], {"grf_tan": grf_tan, "joint_q_tan": seeds["joint_q_tan"]},
                                           out={"joint_tau_tan": tau_tan})[0]
        swing_tan = T.plan_swing_torque_tangent(ctl, d, dict({k: seeds[k] for k in ("Rwb_rot_tan", "x_tan", "joint_q_tan", "joint_qdot_tan")}, joint_tau_tan_in=tau_tan),
                                                out={"joint_tau_tan": tau_tan})[0]
        step_tan = T.plan_leg_plant_step_tangent(ctl, state, out["joint_tau"], 1e-9, inertia, dict(seeds, joint_tau_tan=tau_tan), stance=d["stance"], out=nxt)[0]

        def closed_loop():
            solve()
            step()

        def closed_loop_tangent():
            solve()
            solve_tan()
            torque_tan()
            swing_tan()
            step_tan()
            step()

        start = dict(q.to_device(host), stance=torch.from_numpy(stance["trot"]).cuda())
        leaves = dict(start, **{k: start[k].clone().requires_grad_(True) for k in ("x", "xdot", "w", "joint_q", "joint_qdot")})

        def reverse():
            final, _ = ctl.rollout_tick_autograd(leaves, 1, dt, inertia, warm=False)
            sum(final[k].sum() for k in names).backward()

        for name, fn in ((f"closed trot step: control_batch + leg_plant_step n={n}", closed_loop),
                         (f"closed trot step with tangents K=36 (6 launches) n={n}", closed_loop_tangent),
                         (f"rollout_tick_autograd through a trot, one step forward + backward n={n}", reverse)):
            res[name] = timed(torch, fn)
            print(json.dumps({name: res[name]}), flush=True)
        del seeds, grf_tan, tau_tan, nxt
        torch.cuda.empty_cache()
    ctl.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

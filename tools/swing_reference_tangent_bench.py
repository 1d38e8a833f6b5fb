"""Timings behind profiles/swing_reference_tangent.md: qc_swing_reference_tangent_batch at K = 1 and K = 12 on 4 096, 65 536 and
262 144 robots of config 3 with joint angles, on a trot whose swinging diagonal is replanned by this call for every other robot and
carried for the rest; next to it, in the same process and under the same protocol, 12 launches of qc_swing_reference_adjoint_batch;
and one closed gait step with the 60 tangents of a transition matrix next to one step of rollout_gait_autograd, forward plus backward.

  python tools/swing_reference_tangent_bench.py --out swing_reference_tangent.json

Cold-cache protocol (tools/sensitivity_swing_bench.py's): the launches rotate through distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache -, every set is touched once before timing; one HIP event pair per launch, so the figure
INCLUDES the launch itself.  Bytes are the algorithm's, per (direction, robot) PAIR, for the call rollout_gait_tangent() makes (every
tangent given, the record's two tangents written in place):
  base     Rwb 72, x, xdot, w 72, joint_q 96, gait_phase 32, the record's leg_state and has_traj 32: 304 B - from L2 for every
           direction but the first
  tangents five [3] rows 120, joint_q_tan, p_start_tan, p_final_tan 288: 408 B;  written four [12] rows: 384 B            1 096 B
The adjoint's launch, per robot: the same base, four cotangents 384 B, eight outputs 456 B: 1 144 B.
The closed-loop figures are whole calls of rollout_gait_tangent() on a fresh copy of the batch, planning and buffers included, at
steps = 1 and steps = 11: a tenth of the difference is one step's launches.  The reverse-mode figure is one step of
rollout_gait_autograd, forward plus backward, Python's autograd included."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, timed  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

BASE_BYTES = 72 + 72 + 96 + 32 + 32
PAIR_BYTES = BASE_BYTES + 5 * 24 + 3 * 96 + 4 * 96
ADJOINT_BYTES = BASE_BYTES + 4 * 96 + 72 + 4 * 24 + 3 * 96


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
    from quadruped_control_amd.balance_controller import SWING_STATE_DTYPE, new_swing_states

    assert torch.cuda.is_available(), "swing_reference_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    res = {"device": torch.cuda.get_device_name(0), "pair_bytes": PAIR_BYTES, "adjoint_bytes": ADJOINT_BYTES}
    dt, inertia = 1.0 / 300.0, 0.02
    names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
    read = ("Rwb", "x", "xdot", "w", "joint_q", "gait_phase")
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        host = workloads.with_joint_angles(workloads.config3(n=n))
        host.pop("feet", None)
        host.pop("stance", None)
        host["joint_qdot"] = np.zeros((n, 12))
        # a trot as the forward call left it: the diagonal 1, 2 swings (phase 0.9), legs 0, 3 stand (0.3); the records before the call
        # make it a stance -> swing edge for the even robots (both legs replanned) and a carried trajectory for the odd ones
        host["gait_phase"] = np.ascontiguousarray(np.tile([0.3, 0.9, 0.9, 0.3], (n, 1)))
        rec = np.zeros(n, SWING_STATE_DTYPE)
        rec["leg_state"] = np.where((np.arange(n) % 2 == 0)[:, None], [1, 1, 1, 1], [1, 0, 0, 1])
        rec["has_traj"] = np.where((np.arange(n) % 2 == 0)[:, None], [0, 0, 0, 0], [0, 1, 1, 0])
        records = torch.from_numpy(rec.view(np.uint8).reshape(n, -1)).cuda()
        base = q.to_device({k: host[k] for k in read})
        plans = {}
        for K in (1, 12):
            sets = int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * K * PAIR_BYTES)))))
            for _ in range(sets):
                dev = {key: v.clone() for key, v in base.items()}
                tans = {k: rnd(K, n, w) for k, w in T.SWING_REFERENCE_TANGENTS.items()}
                out = {"swing_pos_tan": rnd(K, n, 4, 3), "swing_vel_tan": rnd(K, n, 4, 3), "p_start_next_tan": tans["p_start_tan"], "p_final_next_tan": tans["p_final_tan"]}
                plans.setdefault((f"swing_reference_tangent K={K}", K * PAIR_BYTES), []).append(
                    T.plan_swing_reference_tangent(ctl, dev, records.clone(), tans, out=out)[0])
        sets = int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * ADJOINT_BYTES)))))
        for _ in range(sets):
            dev = {key: v.clone() for key, v in base.items()}
            cot = {k: rnd(n, 12) for k in ("swing_pos", "swing_vel", "p_start", "p_final")}
            one = ctl.plan_swing_reference_adjoint(dev, records.clone(), cot, out=None)[0]
            plans.setdefault(("12 x swing_reference_adjoint", 12 * ADJOINT_BYTES), []).append(lambda one=one: [one() for _ in range(12)])
        torch.cuda.synchronize()
        for (name, nbytes), launches in plans.items():
            r = timed_rotating(torch, launches, args.launches)
            r.update(sets=len(launches), bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
            print(json.dumps({f"{name} n={n}": r}), flush=True)
        del plans
        torch.cuda.empty_cache()
        # one closed gait step: whole calls on a fresh copy of a standing batch at the start of a trot (the first call plans whatever swings)
        start = dict(q.to_device(host), swing_state=torch.from_numpy(new_swing_states(n).view(np.uint8).reshape(n, -1)).cuda())
        fresh = lambda: {k: v.clone() for k, v in start.items()}
        seeds = T.tick_transition_seeds(n, start["x"].device, T.GAIT_TRANSITION_COLUMNS, T._TICK_STATE + T._GAIT_RECORD)

        def plain(steps):
            d = dict(fresh(), gait_dt=torch.zeros(n, dtype=torch.float64, device="cuda"))
            ctl.rollout_tick(d, None, steps, dt, inertia)

        def forward(steps):
            T.rollout_gait_tangent(ctl, fresh(), steps, dt, inertia, dt, seeds)

        def reverse():
            d = fresh()
            leaves = dict(d, **{k: d[k].requires_grad_(True) for k in ("x", "xdot", "w", "joint_q", "joint_qdot")})
            final, _ = ctl.rollout_gait_autograd(leaves, 1, dt, inertia, dt, warm=False)
            sum(final[k].sum() for k in names).backward()

        for name, fn in ((f"rollout_tick, gait, steps=1 n={n}", lambda: plain(1)), (f"rollout_tick, gait, steps=11 n={n}", lambda: plain(11)),
                         (f"rollout_gait_tangent K=60 steps=1 n={n}", lambda: forward(1)), (f"rollout_gait_tangent K=60 steps=11 n={n}", lambda: forward(11)),
                         (f"rollout_gait_autograd, one step forward + backward n={n}", reverse)):
            res[name] = timed(torch, fn)
            print(json.dumps({name: res[name]}), flush=True)
        del seeds, start
        torch.cuda.empty_cache()
    ctl.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

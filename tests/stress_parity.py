"""One-off stress check: all kernel forms agree with each other on N robots (default 1,048,576: many rounds of workgroups,
paired waves on the 6x6 forms; 16,384 / 65,536 exercise the narrower one-fill layouts) and with the C oracle on a subset of
up to 65,536.
usage: python tests/stress_parity.py [N]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np, torch
import quadruped_control_amd as q
from quadruped_control_amd import workloads as W
from oracle import c_oracle as O
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
P = q.cheetah_params(0.6)
b = W.config3(n, seed=0x5EED00AA)
d = q.to_device(b)
res = {}
for name, env in (("G2/G4 default", {}), ("G1", {"group": 1}), ("G4", {"group": 4}), ("general6x6", {"force_general": 1}), ("dense12x12", {"force_dense": 1})):
    ctl = q.BalanceController.from_params(P).set_tuning(**env)
    o = ctl.control_batch(d, want_iterations=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0, name
    res[name] = o["grf_body"].cpu().numpy()
    print(name, ctl.kernel_name, "max iters", int(o["iterations"].max()), "mean %.3f" % o["iterations"].float().mean().item())
base = res["G2/G4 default"]
scale = np.maximum(1.0, np.abs(base).max(axis=1, keepdims=True))
for name, g in res.items():
    print("vs default: %-14s max rel diff %.3e" % (name, np.max(np.abs(g - base) / scale)))
idx = np.random.default_rng(0).choice(n, min(n, 65536), replace=False)
sub = {k: np.ascontiguousarray(v[idx]) for k, v in b.items()}
t = time.time(); ref, st, _ = O.control_batch(P, sub, threads=16); print("oracle (%d robots): %.1f s" % (len(idx), time.time() - t), "status ok", (st == 0).all())
print("GPU vs oracle: max rel diff %.3e" % np.max(np.abs(base[idx] - ref) / scale[idx]))

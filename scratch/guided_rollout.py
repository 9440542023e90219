"""Guided rollout at the dashboard's settings (reference plotting.py:165: 16 Heun steps, rho 2, sigma 0.01 .. 80, S_churn 0;
gym_train.py:129 samples with guidance 2): the gym net after 8 context frames, three paths run alternately in ONE process --
  unguided   guidance 1 (the graphed pair-free rollout, bench.py --mode rollout),
  pair       guidance 2, every evaluation ONE evaluation over 2B rows (Precond(_guidance=), the graphed / fused frame loop),
  two-call   guidance 2 with the pair switched off: the cached evaluation + a cacheless just_2d evaluation + a torch lerp, eager
             (what the sampler did before the pair existed).
Prints one JSON line per (path, B) with ms per evaluation (31 per frame) and frames/s.
  python scratch/guided_rollout.py [--batches 1 8] [--frames 4] [--rounds 3]
Kernels per guided evaluation: a separate run under  rocprofv3 --kernel-trace --stats -- python scratch/guided_rollout.py --frames 1
--rounds 1 --paths pair  (31 evaluations + the frame's updates per generated frame)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fork(c):
    return {k: fork(v) for k, v in c.items()} if isinstance(c, dict) else c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--paths", nargs="+", default=["unguided", "pair", "two-call"])
    args = ap.parse_args()
    import torch
    from bench import GYM_CFG
    from edm2.networks_edm2 import UNet, Precond
    from edm2.sampler import edm_sampler_with_mse
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unet = UNet(**GYM_CFG).to(dev)
    torch.nn.init.constant_(unet.out_gain, 1.0)
    net = Precond(unet, sigma_data=1.0).to(dev).eval()
    settings = dict(num_steps=16, sigma_min=0.01, sigma_max=80, rho=2)
    for B in args.batches:
        with torch.no_grad():
            ctx = torch.randn(B, 8, 8, 64, 64, device=dev)
            lab = torch.randint(0, 4, (B, 8), device=dev)
            _, cache0 = net(ctx, torch.ones(B, 8, device=dev) * 0.05, lab, update_cache=True)

        def run(path, n):
            guidance = 1 if path == "unguided" else 2
            if path == "two-call":
                net.pair_served = lambda *a, **k: False
            try:
                cache = fork(cache0)
                with torch.no_grad():
                    _, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=lab[:, :1], guidance=guidance, **settings)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        x, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=lab[:, :1], guidance=guidance, **settings)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, bool(torch.isfinite(x).all())
            finally:
                if path == "two-call":
                    del net.pair_served
        res = {p: [] for p in args.paths}
        for r in range(args.rounds):
            for p in args.paths:
                dt, ok = run(p, args.frames)
                res[p].append((dt, ok))
        for p in args.paths:
            dts = [d for d, _ in res[p]]
            best = min(dts)
            print(json.dumps({"path": p, "batch": B, "frames": args.frames, "rounds": args.rounds,
                              "ms_per_eval_best": best / (31 * args.frames) * 1e3,
                              "ms_per_eval_all": [d / (31 * args.frames) * 1e3 for d in dts],
                              "frames_per_s_best": B * args.frames / best, "finite": all(o for _, o in res[p])}), flush=True)


if __name__ == "__main__":
    main()

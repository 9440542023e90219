"""Generate fixture G17 (VAE training at the shapes G16 leaves out: group size 8, every (time, spatial) compression pair, widths
below the capacity of their kernel instantiation) by IMPORTING the reference (read-only) on CPU in the build container.  Run from
the repo root:   python tests/golden/make_golden_vae_shapes.py

  g17_vae_shapes.npz   per config (prefix "A/", "B/"):
      A  channels=[3,12,24,5], n_res_blocks=1, time_compressions=[2,2,2], spatial_compressions=[2,1,2], x (2,3,16,12,20)
      B  channels=[3,48,6,20], n_res_blocks=1, time_compressions=[1,1,2], spatial_compressions=[2,2,1], x (1,3,4,20,36)
    the reference's VAE in .train() mode and in float64.  The state dict is drawn entry by entry in its own order by
    tests/vae_stage_oracle.py seeded_state_dict from `seed` (stored with the names and shapes, so that a test regenerates it and
    nothing of it needs storing); x, t_sample and noise are stored as drawn (float32) and substituted for the reference's
    torch.rand / torch.randn_like during the call.  Outputs mean, r_mean, r_logvar are stored in float64.  The loss is G16's,
    L = sum r_mean c1 + sum r_logvar c2 + sum mean c3 with c_k = cos(0.7 i + phi_k); of each parameter gradient two float64
    scalars are stored, `gnorm/<name>` its L2 norm and `gproj/<name>` its projection sum_i grad_i cos(0.3 i + 1) over the flat
    index (the gradients themselves are 2.7 MB), and `ref32_rel/<name>`: the rel L2 of the reference's own float32 run of the same
    call against its float64 run.  The seeds are kept where that run stays within 1.0e-5 on every gradient, the basis of the GPU
    tests' bound 5e-5 (seed 1702 for B makes d logvar_multiplier, one scalar, a cancelling sum that float32 misses by 4e-4).
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refshim  # noqa: E402

edm2 = _refshim.install()
from edm2.vae import VAE  # noqa: E402
from vae_stage_oracle import seeded_state_dict  # noqa: E402

torch.set_num_threads(8)
PHI = (0.1, 1.3, 2.9)
CONFIGS = {
    "A": (dict(channels=[3, 12, 24, 5], n_res_blocks=1, time_compressions=[2, 2, 2], spatial_compressions=[2, 1, 2]),
          (2, 3, 16, 12, 20), 1701),
    "B": (dict(channels=[3, 48, 6, 20], n_res_blocks=1, time_compressions=[1, 1, 2], spatial_compressions=[2, 2, 1]),
          (1, 3, 4, 20, 36), 1703),
}


def cot(shape, phi, dtype):
    n = int(np.prod(shape))
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64) + phi).reshape(shape).to(dtype)


def proj(g):
    g = g.detach().double().reshape(-1)
    return float((g * torch.cos(0.3 * torch.arange(g.numel(), dtype=torch.float64) + 1)).sum())


def run(kw, sd, x, t_sample, noise, dtype):
    vae = VAE(**kw).train()
    vae.load_state_dict(sd, strict=True)
    vae = vae.to(dtype)
    rand, randn_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: t_sample.to(dtype)                       # times t = 1 below: t_b = t_sample exactly (vae.py:233)
    torch.randn_like = lambda m, **k: noise.to(dtype)
    try:
        r_mean, r_logvar, mean, cache = vae(x.to(dtype), t=1.0)
    finally:
        torch.rand, torch.randn_like = rand, randn_like
    L = sum((o * cot(o.shape, p, dtype)).sum() for o, p in zip((r_mean, r_logvar, mean), PHI))
    L.backward()
    outs = dict(mean=mean.detach(), r_mean=r_mean.detach(), r_logvar=r_logvar.detach())
    return outs, {n: p.grad.detach() for n, p in vae.named_parameters()}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def main():
    store = {}
    for name, (kw, xshape, seed) in CONFIGS.items():
        ref_sd = VAE(**kw).state_dict()
        names, shapes = list(ref_sd), [tuple(v.shape) for v in ref_sd.values()]
        sd = seeded_state_dict(names, shapes, seed)
        g = torch.Generator().manual_seed(seed + 100)
        x = torch.rand(xshape, generator=g) * 2 - 1
        t_sample = torch.rand(xshape[0], generator=g) * 0.1
        tc, sc = int(np.prod(kw["time_compressions"])), int(np.prod(kw["spatial_compressions"]))
        noise = torch.randn(xshape[0], kw["channels"][-1], xshape[2] // tc, xshape[3] // sc, xshape[4] // sc, generator=g)
        o64, g64 = run(kw, sd, x, t_sample, noise, torch.float64)
        o32, g32 = run(kw, sd, x, t_sample, noise, torch.float32)
        assert all(bool((v != 0).any()) for v in g64.values()), "a gradient is identically zero"
        for k in o64:
            print(f"{name}: output {k} {tuple(o64[k].shape)}: float32 run vs float64 run, rel L2 {rel(o32[k], o64[k]):.2e}")
        ref32 = {k: rel(g32[k], g64[k]) for k in g64}
        print(f"{name}: {sum(v.numel() for v in g64.values())} gradient values; float32 vs float64, worst "
              f"{max(ref32, key=ref32.get)} {max(ref32.values()):.2e}")
        p = name + "/"
        store[p + "seed"] = np.int64(seed)
        store[p + "names"] = np.array(names)
        store[p + "shapes"] = np.array([",".join(str(s) for s in sh) for sh in shapes])
        for k in ("channels", "n_res_blocks", "time_compressions", "spatial_compressions"):
            store[p + "kw_" + k] = np.asarray(kw[k], dtype=np.int64)
        store[p + "x"], store[p + "t_sample"], store[p + "noise"] = x.numpy(), t_sample.numpy(), noise.numpy()
        for k, v in o64.items():
            store[p + k] = v.numpy()
        for k, v in g64.items():
            store[p + "gnorm/" + k] = np.float64(v.double().norm().item())
            store[p + "gproj/" + k] = np.float64(proj(v))
            store[p + "ref32_rel/" + k] = np.float32(ref32[k])
    path = os.path.join(HERE, "g17_vae_shapes.npz")
    np.savez_compressed(path, **store)
    print(f"g17_vae_shapes: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

"""Generate fixture G16 (VAE training: forward and every parameter gradient) by IMPORTING the reference (read-only) on CPU in
the build container.  Run from the repo root:   python tests/golden/make_golden_vae_train.py

  g16_vae_train.npz         the VAE of G14 (channels=[3,8,16,8], n_res_blocks=2, its state dict g14_vae_sd.npz, every parameter
                            non-zero) in .train() mode and in float64, on G15's frames (2, 12, 24, 40, 3) as frames / 127.5 - 1:
                            non-square, ragged against the 16x16 tile at every level, 3 time groups at g = 4.  t_sample (2,)
                            and noise (2, 8, 3, 6, 10) come from a seeded generator and are substituted for the reference's
                            torch.rand / torch.randn_like during the call (re-seeding does not carry across dtypes).  Stores
                            t_sample, noise and the outputs mean, r_mean, r_logvar as float32.
  g16_vae_train_grads.npz   the gradient of L = sum r_mean c1 + sum r_logvar c2 + sum mean c3, c_k = cos(0.7 i + phi_k) over the
                            flat index (phi = 0.1, 1.3, 2.9: nothing of the cotangents needs storing), with respect to every
                            parameter (174 767 values, float32), and per parameter `ref32_rel/<name>`: the rel L2 of the
                            reference's own float32 run of the same call against its float64 run.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refshim  # noqa: E402

edm2 = _refshim.install()
from edm2.vae import VAE  # noqa: E402

torch.set_num_threads(8)
PHI = (0.1, 1.3, 2.9)


def cot(shape, phi, dtype):
    n = int(np.prod(shape))
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64) + phi).reshape(shape).to(dtype)


def run(sd, kw, x, t_sample, noise, dtype):
    vae = VAE(channels=[3, 8, 16, 8], n_res_blocks=2, mean=kw["mean"], std=kw["std"]).train()
    vae.load_state_dict(sd, strict=True)
    vae = vae.to(dtype)
    rand, randn_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: t_sample.to(dtype)                       # times t = 1 below: t_b = t_sample exactly (vae.py:233)
    torch.randn_like = lambda m, **k: noise.to(dtype)
    try:
        r_mean, r_logvar, mean, cache = vae(x.to(dtype), t=1.0)
    finally:
        torch.rand, torch.randn_like = rand, randn_like
    leaves = [c for blk in cache["encoder"].values() for rb in blk.values() for c in rb.values()]
    leaves += [c for blk in cache["decoder"].values() for rb in blk.values() for c in rb.values()]
    assert len(leaves) == 12 and all(c is None for c in leaves)
    L = sum((o * cot(o.shape, p, dtype)).sum() for o, p in zip((r_mean, r_logvar, mean), PHI))
    L.backward()
    outs = dict(mean=mean.detach(), r_mean=r_mean.detach(), r_logvar=r_logvar.detach())
    return outs, {n: p.grad.detach() for n, p in vae.named_parameters()}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def main():
    z = np.load(os.path.join(HERE, "g14_vae.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "g14_vae_sd.npz"), allow_pickle=False).items()}
    kw = dict(mean=z["kw_mean"].tolist(), std=z["kw_std"].tolist())
    frames = torch.from_numpy(np.load(os.path.join(HERE, "g15_vae_enc.npz"), allow_pickle=False)["frames"])
    assert frames.shape == (2, 12, 24, 40, 3)
    x = (frames / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    g = torch.Generator().manual_seed(1601)
    t_sample = torch.rand(2, generator=g) * 0.1
    noise = torch.randn(2, 8, 3, 6, 10, generator=g)
    o64, g64 = run(sd, kw, x, t_sample, noise, torch.float64)
    o32, g32 = run(sd, kw, x, t_sample, noise, torch.float32)
    assert sum(v.numel() for v in g64.values()) == 174767, sum(v.numel() for v in g64.values())
    assert all(bool((v != 0).any()) for v in g64.values())
    for k in o64:
        print(f"output {k}: float32 run vs float64 run, rel L2 {rel(o32[k], o64[k]):.2e}")
    ref32 = {k: rel(g32[k], g64[k]) for k in g64}
    for k in sorted(ref32, key=ref32.get, reverse=True)[:8]:
        print(f"ref32_rel {k}: {ref32[k]:.2e}")
    path = os.path.join(HERE, "g16_vae_train.npz")
    np.savez_compressed(path, t_sample=t_sample.numpy(), noise=noise.numpy(), **{k: v.float().numpy() for k, v in o64.items()})
    print(f"g16_vae_train: {os.path.getsize(path) / 1024:.0f} KiB")
    path = os.path.join(HERE, "g16_vae_train_grads.npz")
    np.savez_compressed(path, **{k: v.float().numpy() for k, v in g64.items()},
                        **{"ref32_rel/" + k: np.float32(v) for k, v in ref32.items()})
    print(f"g16_vae_train_grads: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

"""Generate fixture G25 (the VAE at a 512-channel block: training forward, every parameter gradient, and the eval-mode encode and
decode) by IMPORTING the reference (read-only) on CPU in the build container, in float64.  Run from the repo root:
    python tests/golden/make_golden_vae_512.py

  g25_vae_512.npz  G24's model with 512 in place of 72: channels=[3,8,512,8], n_res_blocks=1, time_compressions=[1,2,1],
                   spatial_compressions=[2,1,2], seed_params(..., 2501), .double(); the parameters are NOT stored (the tests
                   re-seed them; param_sums notices a drifting generator).  Encoder: 3 -> 8 at g = 2, 8 -> 512 at g = 2 (the wide
                   block, conv A's K = 2g 9 C = 18 432), 512 -> 8 at g = 1; decoder: 8 at g = 1, 512 at g = 2 (up by 2 in time),
                   8 at g = 2.  B = 2, 8 seeded uint8 frames of 12x20 as x = frames / 127.5 - 1; t_sample (2,) and noise
                   (2, 8, 4, 3, 5) come from a seeded generator and are substituted for the reference's torch.rand /
                   torch.randn_like during the training call.  Stores the frames, t_sample, noise, the float64 training-mode
                   outputs mean, r_mean, r_logvar, and per parameter the float64 gradient of L = sum r_mean c1 + sum r_logvar c2 +
                   sum mean c3, c_k = cos(0.7 i + phi_k) over the flat index (phi = 0.1, 1.3, 2.9) as `grad/<name>`; a gradient of
                   more than FULL elements is stored at the flat indices 0, s, 2s, ... (s = stride(numel), odd) together with
                   `norm/<name>` and `sum/<name>`, the float64 L2 norm and sum of ALL its elements, exactly as G24 does.
                   In addition, from the same model in eval mode under no_grad: `eval_mean` = encode(x)[0] and
                   (`eval_r_mean`, `eval_r_logvar`) = decode(noise, t_sample)[:2] -- the decoder on latents that no encoder made --
                   so that the inference path has a target of the reference's own too.
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
from vae_wide_oracle import seed_params, param_sums  # noqa: E402

torch.set_num_threads(8)
KW = dict(channels=[3, 8, 512, 8], n_res_blocks=1, time_compressions=[1, 2, 1], spatial_compressions=[2, 1, 2])
SEED = 2501
PHI = (0.1, 1.3, 2.9)
FULL = 8192


def stride(numel):
    """The sampling stride of a gradient of numel > FULL elements: the smallest odd number that leaves at most 4096 samples."""
    s = -(-numel // 4096)
    return s + 1 - (s & 1)


def cot(shape, phi, dtype):
    n = int(np.prod(shape))
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64) + phi).reshape(shape).to(dtype)


def main():
    torch.manual_seed(25)
    vae = seed_params(VAE(**KW), SEED).double().train()
    g = torch.Generator().manual_seed(2502)
    B, T, H, W = 2, 8, 12, 20
    frames = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    t_sample = torch.rand(B, generator=g) * 0.1
    noise = torch.randn(B, 8, 4, 3, 5, generator=g)
    x = (frames.double() / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    rand, randn_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: t_sample.double()                        # times t = 1 below: t_b = t_sample exactly
    torch.randn_like = lambda m, **k: noise.double()
    try:
        r_mean, r_logvar, mean, cache = vae(x, t=1.0)
    finally:
        torch.rand, torch.randn_like = rand, randn_like
    leaves = [c for side in cache.values() for blk in side.values() for rb in blk.values() for c in rb.values()]
    assert len(leaves) == 6 and all(c is None for c in leaves)
    assert mean.shape == (B, 8, 4, 3, 5) and r_mean.shape == (B, 3, T, H, W) and r_mean.dtype == torch.float64
    sum((o * cot(o.shape, p, torch.float64)).sum() for o, p in zip((r_mean, r_logvar, mean), PHI)).backward()
    vae.eval()
    with torch.no_grad():
        eval_mean = vae.encode(x)[0]
        eval_r_mean, eval_r_logvar = vae.decode(noise.double(), t_sample.double())[:2]
    assert eval_mean.shape == mean.shape and eval_r_mean.shape == r_mean.shape
    arrs = {"frames": frames, "t_sample": t_sample, "noise": noise, "mean": mean, "r_mean": r_mean, "r_logvar": r_logvar,
            "eval_mean": eval_mean, "eval_r_mean": eval_r_mean, "eval_r_logvar": eval_r_logvar,
            "seed": np.array(SEED), "param_sums": param_sums(vae)}
    for k, v in KW.items():
        arrs["kw_" + k] = np.array(v)
    for name, p in vae.named_parameters():
        gr = p.grad.detach().reshape(-1)
        assert bool((gr != 0).any()), name
        if gr.numel() <= FULL:
            arrs["grad/" + name] = gr.reshape(p.shape)
        else:
            arrs["grad/" + name] = gr[::stride(gr.numel())]
            arrs["norm/" + name] = gr.norm()
            arrs["sum/" + name] = gr.sum()
    path = os.path.join(HERE, "g25_vae_512.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f"g25_vae_512: {os.path.getsize(path)} bytes, {sum(1 for k in arrs if k.startswith('norm/'))} sampled")
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()

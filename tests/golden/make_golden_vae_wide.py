"""Generate fixture G22 (the VAE decoder at block widths above 64) by IMPORTING the reference (read-only) on CPU in the build
container, in float64.  Run from the repo root:   python tests/golden/make_golden_vae_wide.py

  g22_vae_wide.npz  channels=[3,72,160,8], n_res_blocks=2 (decoder blocks: 8 channels at g = 1, 160 at g = 2, 72 at g = 4: a
                    narrow block, a wide one, a wide ragged one), .double().eval(), every parameter seeded non-zero by
                    seed_params (tests/vae_wide_oracle.py) and NOT stored: the tests re-seed them, and the float64 sum and sum of
                    squares of every parameter are stored so that a drifting generator is noticed.  B = 2, 2 latent frames of
                    5x7 latents (20x28 frames, ragged tiles at every level), t = [0.1, 0.35], mean / std kwargs.  Stores z,
                    latents, decode() mean / logvar, the mean of the reference's own chunked decode (1 + 1 latent frames through
                    its cache), frames_pre = clip((mean + 1) 127.5, 0, 255) of latents_to_frames' decode (t = 0.1), and the
                    reference's state-dict keys and shapes.
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

MEAN = [0.31, -0.12, 0.05, 0.4, -0.27, 0.18, -0.06, 0.22]
STD = [1.3, 0.8, 1.1, 0.9, 1.6, 0.7, 1.2, 1.05]
CHANNELS, N_RES, SEED = [3, 72, 160, 8], 2, 2201


def main():
    torch.manual_seed(22)
    vae = seed_params(VAE(channels=CHANNELS, n_res_blocks=N_RES, mean=MEAN, std=STD), SEED).double().eval()
    g = torch.Generator().manual_seed(2202)
    B, T, h, w = 2, 2, 5, 7
    latents = torch.randn(B, T, 8, h, w, generator=g).double()
    t = torch.tensor([0.1, 0.35], dtype=torch.float64)
    z = (latents * vae.std[:, None, None] + vae.mean[:, None, None]).permute(0, 2, 1, 3, 4).contiguous()
    with torch.no_grad():
        mean, logvar, _ = vae.decode(z, t)
        m0, _, cache = vae.decode(z[:, :, :1], t)
        m1, _, _ = vae.decode(z[:, :, 1:], t, cache)
        pre = torch.clip((vae.decode(z, 0.1 * torch.ones(B, dtype=torch.float64))[0] + 1) * 127.5, 0, 255).permute(0, 2, 3, 4, 1)
    chunked = torch.cat((m0, m1), dim=2)
    assert mean.dtype == torch.float64 and mean.shape == (B, 3, 4 * T, 4 * h, 4 * w)
    print("chunked vs whole (reference):", (chunked - mean).abs().max().item())
    sd = vae.state_dict()
    arrs = {"latents": latents, "t": t, "z": z, "mean": mean, "logvar": logvar, "frames_pre": pre, "chunked_mean": chunked,
            "kw_mean": np.array(MEAN), "kw_std": np.array(STD), "kw_channels": np.array(CHANNELS), "kw_n_res_blocks": np.array(N_RES),
            "seed": np.array(SEED), "param_sums": param_sums(vae),
            "sd_keys": np.array(list(sd)), "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}
    path = os.path.join(HERE, "g22_vae_wide.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f"g22_vae_wide: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

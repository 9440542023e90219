"""Generate fixture G14 (the VAE decoder) by IMPORTING the reference (read-only) on CPU in the build container.
Run from the repo root:   python tests/golden/make_golden_vae.py

  g14_vae.npz       channels=[3,8,16,8], n_res_blocks=2 (decoder block widths 8 -> 16 -> 8 -> 6: the channel-area
                    residual goes up and down), every parameter seeded non-zero; B = 2, 3 latent frames of 6x6 latents
                    (24x24 frames, ragged tiles at every level), t = [0.1, 0.35], mean / std kwargs.  Stores decode()
                    mean / logvar, latents_to_frames() as uint8 with its pre-truncation value
                    clip((mean + 1) * 127.5, 0, 255), and the mean of the reference's own chunked decode (1 + 2 frames
                    through its cache).
  g14_vae_sd.npz    the state dict of that VAE, encoder and decoder (kept apart: each file stays under 1 MB).
  g14_vae_gym.pt    the gym VAE (channels=[3,8,8,8], n_res_blocks=2, gym_vae_train.py:32-36) with seeded non-zero
                    parameters, written in the reference's checkpoint format {"state_dict", "kwargs"} (utils.py:15-34).
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

MEAN = [0.31, -0.12, 0.05, 0.4, -0.27, 0.18, -0.06, 0.22]
STD = [1.3, 0.8, 1.1, 0.9, 1.6, 0.7, 1.2, 1.05]


def seed_params(vae, seed):
    """Every parameter non-zero (the reference initialises conv3d1, t_cond and half of the time taps to zero): conv weights
    ~ N(0, 1 / fan_in), biases ~ 0.1 N(0, 1), the t_cond linear ~ 0.5 N(0, 1 / fan_in); logvar_multiplier -1.7."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in vae.named_parameters():
            if name.endswith("logvar_multiplier"):
                p.fill_(-1.7)
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p[0].numel()
                s = 0.5 if ".t_cond." in name else 1.0
                p.copy_(s * torch.randn(p.shape, generator=g) / fan_in ** 0.5)
    return vae


def main():
    torch.manual_seed(14)
    vae = seed_params(VAE(channels=[3, 8, 16, 8], n_res_blocks=2, mean=MEAN, std=STD), 1401).eval()
    g = torch.Generator().manual_seed(1402)
    B, T, h = 2, 3, 6
    latents = torch.randn(B, T, 8, h, h, generator=g)
    t = torch.tensor([0.1, 0.35])
    z = (latents * vae.std[:, None, None] + vae.mean[:, None, None]).permute(0, 2, 1, 3, 4).contiguous()
    with torch.no_grad():
        mean, logvar, _ = vae.decode(z, t)
        m0, _, cache = vae.decode(z[:, :, :1], t)
        m1, _, _ = vae.decode(z[:, :, 1:], t, cache)
        frames = vae.latents_to_frames(latents)
        pre = torch.clip((vae.decode(z, 0.1 * torch.ones(B))[0] + 1) * 127.5, 0, 255).permute(0, 2, 3, 4, 1)
    chunked = torch.cat((m0, m1), dim=2)
    assert frames.shape == (B, 4 * T, 4 * h, 4 * h, 3) and np.array_equal(frames, pre.numpy().astype(int))
    print("chunked vs whole (reference):", (chunked - mean).abs().max().item())
    arrs = {"latents": latents, "t": t, "z": z, "mean": mean, "logvar": logvar, "frames": frames.astype(np.uint8),
            "frames_pre": pre, "chunked_mean": chunked, "kw_mean": np.array(MEAN), "kw_std": np.array(STD)}
    for name, a in (("g14_vae", arrs), ("g14_vae_sd", vae.state_dict())):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in a.items()})
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")

    torch.manual_seed(15)
    gym = seed_params(VAE(channels=[3, 8, 8, 8], n_res_blocks=2, mean=MEAN, std=STD), 1501)
    path = os.path.join(HERE, "g14_vae_gym.pt")
    torch.save({"state_dict": gym.state_dict(), "kwargs": gym.kwargs}, path)     # BetterModule.save_to_state_dict, local path
    print(f"g14_vae_gym: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

"""Generate fixture G15 (the VAE encoder) by IMPORTING the reference (read-only) on CPU in the build container.
Run from the repo root:   python tests/golden/make_golden_vae_enc.py

  g15_vae_enc.npz   the VAE of G14 (channels=[3,8,16,8], n_res_blocks=2, its state dict g14_vae_sd.npz, every parameter
                    non-zero; encoder widths 8 -> 16 -> 8: the channel-area residual goes up, 3 -> 8, and down, 64 -> 16 and
                    128 -> 8) on uint8 frames (2, 12, 24, 40, 3): a non-square size, ragged against the 16x16 tile at every
                    level, 3 latent frames.  Stores the frames, the reference's encode() mean (2, 8, 3, 6, 10) of
                    frames / 127.5 - 1 (vae.py:271), the mean of the reference's own chunked encode (4 + 8 frames through
                    its cache) and the normalised latents (mean - kw_mean) / kw_std as (B, T, C, h, w) -- the formula of
                    cs_train.py:102; the reference's frames_to_latents itself does not run (vae.py:264-284).
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


def main():
    z = np.load(os.path.join(HERE, "g14_vae.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "g14_vae_sd.npz"), allow_pickle=False).items()}
    assert all(bool((v != 0).all()) for k, v in sd.items() if k.startswith("encoder."))
    vae = VAE(channels=[3, 8, 16, 8], n_res_blocks=2, mean=z["kw_mean"].tolist(), std=z["kw_std"].tolist()).eval()
    vae.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(1501)
    frames = torch.randint(0, 256, (2, 12, 24, 40, 3), generator=g, dtype=torch.uint8)
    x = (frames / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    with torch.no_grad():
        mean, _ = vae.encode(x)
        m0, cache = vae.encode(x[:, :, :4])
        m1, _ = vae.encode(x[:, :, 4:], cache)
        x2 = x.clone()
        x2[:, :, 8:] = -x2[:, :, 8:]
        mean2, _ = vae.encode(x2)
    chunked = torch.cat((m0, m1), dim=2)
    assert mean.shape == (2, 8, 3, 6, 10)
    print("chunked vs whole (reference), rel L2:", ((chunked - mean).norm() / mean.norm()).item())
    print("latent frames 0, 1 unchanged by frames 8..11:", torch.equal(mean[:, :, :2], mean2[:, :, :2]))
    latents = ((mean - vae.mean[:, None, None, None]) / vae.std[:, None, None, None]).permute(0, 2, 1, 3, 4).contiguous()
    arrs = {"frames": frames, "mean": mean, "chunked_mean": chunked, "latents": latents}
    path = os.path.join(HERE, "g15_vae_enc.npz")
    np.savez_compressed(path, **{k: v.detach().numpy() for k, v in arrs.items()})
    print(f"g15_vae_enc: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

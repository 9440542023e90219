"""Generate fixture G23 (the VAE encoder at block widths above 64) by IMPORTING the reference (read-only) on CPU in the build
container, in float64.  Run from the repo root:   python tests/golden/make_golden_vae_wide_enc.py

  g23_vae_wide_enc.npz  the model of G22: channels=[3,72,160,8], n_res_blocks=2, G22's mean / std, seed_params(..., 2201),
                        .double().eval(); the parameters are NOT stored (the tests re-seed them; param_sums notices a drifting
                        generator).  Encoder blocks: 3 -> 72 at g = 4 (a wide block reading the raw frames, K = 3), 72 -> 160 at
                        g = 2 (K = 576), 160 -> 8 at g = 1 (K = 1280 into a narrow block).  B = 2, 8 seeded uint8 frames of 20x28
                        (ragged tiles at every level).  Stores the frames, x = frames / 127.5 - 1 as (B, 3, T, H, W), encode()
                        mean, the mean of the reference's own chunked encode (4 + 4 frames through its cache), the normalised
                        latents (mean - kw_mean) / kw_std as (B, T, C, h, w) (the formula of cs_train.py:102; the reference's
                        frames_to_latents itself does not run), param_sums, the seed and the kwargs.
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
from make_golden_vae_wide import MEAN, STD, CHANNELS, N_RES, SEED  # noqa: E402

torch.set_num_threads(8)


def main():
    torch.manual_seed(23)
    vae = seed_params(VAE(channels=CHANNELS, n_res_blocks=N_RES, mean=MEAN, std=STD), SEED).double().eval()
    g = torch.Generator().manual_seed(2301)
    B, T, H, W = 2, 8, 20, 28
    frames = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    x = (frames.double() / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    with torch.no_grad():
        mean, _ = vae.encode(x)
        m0, cache = vae.encode(x[:, :, :4])
        m1, _ = vae.encode(x[:, :, 4:], cache)
    chunked = torch.cat((m0, m1), dim=2)
    assert mean.dtype == torch.float64 and mean.shape == (B, 8, T // 4, H // 4, W // 4)
    print("chunked vs whole (reference):", (chunked - mean).abs().max().item())
    latents = ((mean - vae.mean.double()[:, None, None, None]) / vae.std.double()[:, None, None, None]).permute(0, 2, 1, 3, 4).contiguous()
    arrs = {"frames": frames, "x": x, "mean": mean, "chunked_mean": chunked, "latents": latents,
            "kw_mean": np.array(MEAN), "kw_std": np.array(STD), "kw_channels": np.array(CHANNELS), "kw_n_res_blocks": np.array(N_RES),
            "seed": np.array(SEED), "param_sums": param_sums(vae)}
    path = os.path.join(HERE, "g23_vae_wide_enc.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f"g23_vae_wide_enc: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

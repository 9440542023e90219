"""CPU restatement of the VAE decoder (reference: edm2/vae/vae.py :18-204, :288-318) in plain fp32 PyTorch, channels-first, from
a state dict and the constructor kwargs.  Written from the formulas, independently of both the reference's modules and the HIP
kernels; fixture G14 (tests/golden/make_golden_vae.py) pins it to the reference, and the GPU tests hold the kernels against it
at sizes the fixtures cannot store."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _rms(x):
    return x / torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-4)


def _area_channels(x, cout):
    """F.interpolate(mode='area') over the channel axis: output o averages input channels [floor(o cin / cout), ceil((o+1) cin / cout))."""
    cin = x.shape[1]
    outs = []
    for o in range(cout):
        s0, s1 = (o * cin) // cout, -((-(o + 1) * cin) // cout)
        outs.append(x[:, s0:s1].mean(dim=1))
    return torch.stack(outs, dim=1)


def decode(sd, kwargs, z, t, cache=None):
    """z (B, C, T, h, w), t (B,) -> (mean, logvar, cache); cache: {(block, res block): padded activated prefix (B, C, g, H+2, W+2)}."""
    channels = list(kwargs["channels"])[::-1]
    outs = channels[1:]
    outs[-1] = 2 * outs[-1]
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    groups = [int(g) for g in np.cumprod(tcs)]
    sd = {k: v.float() for k, v in sd.items()}
    x, t = z.float(), torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    cache = {} if cache is None else cache
    new_cache = {}
    for i, (C, Cout, tc, sc, g) in enumerate(zip(channels[:-1], outs, tcs, scs, groups)):
        p = f"decoder.encoder_blocks.{i}."
        x = F.conv3d(x, sd[p + "decompression_block.weight"], sd[p + "decompression_block.bias"])
        B, _, T, H, W = x.shape
        x = x.reshape(B, tc, sc, sc, C, T, H, W).permute(0, 4, 5, 1, 6, 2, 7, 3).reshape(B, C, T * tc, H * sc, W * sc)
        T, H, W = T * tc, H * sc, W * sc
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            four = torch.cos(t[:, None] * sd[q + "fourier_cond.freqs"][None] + sd[q + "fourier_cond.phases"][None]) * math.sqrt(2)
            e = four @ sd[q + "t_cond.weight"].T + sd[q + "t_cond.bias"]
            scale, shift = e[:, :C, None, None, None], e[:, C:, None, None, None]
            y = F.silu(_rms(x) * (1 + scale) + shift)
            yp = F.pad(y, (1, 1, 1, 1))
            prefix = cache.get((i, j))
            seq = torch.cat((yp[:, :, :g] if prefix is None else prefix, yp), dim=2)
            new_cache[(i, j)] = seq[:, :, -g:]
            y = F.conv3d(seq, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], stride=(g, 1, 1))
            y = y.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)     # '(c g) t -> c (t g)'
            y = F.silu(_rms(y))
            x = x + F.conv3d(y, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"], padding=(0, 1, 1))
        x = F.conv3d(x, sd[p + "final_conv.weight"], sd[p + "final_conv.bias"]) + _area_channels(x, Cout)
    mean, logvar = x.split(x.shape[1] // 2, dim=1)
    return mean, logvar * torch.exp(sd["decoder.logvar_multiplier"]), new_cache


def frames_pre(sd, kwargs, latents, t=0.1):
    """latents (B, T, C, h, w) -> clip((mean + 1) * 127.5, 0, 255) (B, 4T, H, W, 3) before truncation (vae.py:288-318)."""
    std = torch.as_tensor(kwargs["std"], dtype=torch.float32)[:, None, None]
    mean = torch.as_tensor(kwargs["mean"], dtype=torch.float32)[:, None, None]
    z = (latents.float() * std + mean).permute(0, 2, 1, 3, 4)
    m, _, _ = decode(sd, kwargs, z, t * torch.ones(latents.shape[0]))
    return torch.clip((m + 1) * 127.5, 0, 255).permute(0, 2, 3, 4, 1)

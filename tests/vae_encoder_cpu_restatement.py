"""CPU restatement of the VAE encoder (reference: edm2/vae/vae.py :18-204, :239-241, :271) in plain fp32 PyTorch, channels-first,
from a state dict and the constructor kwargs.  Written from the formulas, independently of both the reference's modules and the
HIP kernels; fixture G15 (tests/golden/make_golden_vae_enc.py) pins it to the reference, and the GPU tests hold the kernels
against it at sizes the fixtures cannot store."""
import numpy as np
import torch
import torch.nn.functional as F

from vae_cpu_restatement import _area_channels, _rms


def encode(sd, kwargs, x, cache=None):
    """x (B, 3, T, H, W) -> (mean (B, C, T / 4, H / 4, W / 4), cache); cache: {(block, res block): padded activated prefix
    (B, C, g, H + 2, W + 2)}."""
    channels = list(kwargs["channels"])
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    groups = [int(g) for g in np.cumprod(tcs)[::-1]]
    sd = {k: v.float() for k, v in sd.items()}
    x = x.float()
    cache = {} if cache is None else cache
    new_cache = {}
    for i, (Cout, tc, sc, g) in enumerate(zip(channels[1:], tcs, scs, groups)):
        p = f"encoder.encoder_blocks.{i}."
        B, C, T, H, W = x.shape
        T, H, W = T // tc, H // sc, W // sc
        x = x.reshape(B, C, T, tc, H, sc, W, sc).permute(0, 3, 5, 7, 1, 2, 4, 6).reshape(B, tc * sc * sc * C, T, H, W)
        x = F.conv3d(x, sd[p + "compression_block.weight"], sd[p + "compression_block.bias"]) + _area_channels(x, Cout)
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            yp = F.pad(F.silu(_rms(x)), (1, 1, 1, 1))
            prefix = cache.get((i, j))
            seq = torch.cat((yp[:, :, :g] if prefix is None else prefix, yp), dim=2)
            new_cache[(i, j)] = seq[:, :, -g:]
            y = F.conv3d(seq, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], stride=(g, 1, 1))
            y = y.reshape(B, Cout, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, Cout, T, H, W)   # '(c g) t -> c (t g)'
            y = F.silu(_rms(y))
            x = x + F.conv3d(y, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"], padding=(0, 1, 1))
    return x, new_cache


def frames_to_latents(sd, kwargs, frames):
    """frames (B, T, H, W, 3), values 0..255 -> (encode(frames / 127.5 - 1) - mean) / std as (B, T / 4, C, h, w)."""
    std = torch.as_tensor(kwargs["std"], dtype=torch.float32, device=frames.device)[:, None, None]
    mean = torch.as_tensor(kwargs["mean"], dtype=torch.float32, device=frames.device)[:, None, None]
    x = (frames.float() / 127.5 - 1).permute(0, 4, 1, 2, 3)
    m, _ = encode(sd, kwargs, x)
    return (m.permute(0, 2, 1, 3, 4) - mean) / std

"""Float64 evaluation of the VAE encoder (reference: edm2/vae/vae.py :96-204, :239-241), written from the formulas, channels-last
[B][T][H][W][C] like the kernels: the `down` stage here, the ResBlock stages from tests/vae_wide_oracle.py (act without FiLM: the
encoder passes t = None).  Nothing casts to fp32 and nothing launches a kernel.  Fixture G23
(tests/golden/make_golden_vae_wide_enc.py) pins `encode` to the reference in float64."""
import numpy as np
import torch

from vae_wide_oracle import F64, act, area_windows, conv_a, conv_b, sequence


def rearrange_down(x, tc, sc):
    """'b c (t tc) (h hc) (w wc) -> b (tc hc wc c) t h w' on channels-last x (B, T tc, H sc, W sc, C) -> (B, T, H, W, tc sc sc C):
    rearranged channel k = ((tq sc + hq) sc + wq) C + c."""
    B, T, H, W, C = x.shape
    y = x.reshape(B, T // tc, tc, H // sc, sc, W // sc, sc, C).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return y.reshape(B, T // tc, H // sc, W // sc, tc * sc * sc * C)


def down(x, weight, bias, tc, sc):
    """The rearrangement, the compression 1x1 conv K = C tc sc^2 -> Cout and interpolate_channels of the rearranged input (the mean
    over the window [floor(o K / Cout), ceil((o + 1) K / Cout)) of its channel axis); weight (Cout, K, ...)."""
    r = rearrange_down(x.to(F64), tc, sc)
    K, Cout = r.shape[-1], weight.shape[0]
    y = r @ weight.to(F64).reshape(Cout, K).T + bias.to(F64)
    area = torch.stack([r[..., s0:s1].mean(dim=-1) for s0, s1 in area_windows(K, Cout)], dim=-1)
    return y + area


def encode(sd, kwargs, x, cache=None):
    """x (B, 3, T, H, W) -> (mean (B, C, t, h, w) float64, cache {(block, res block): (B, g, H, W, C)})."""
    channels = list(kwargs["channels"])
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    groups = [int(g) for g in np.cumprod(tcs)][::-1]
    sd = {k: v.to(F64) for k, v in sd.items()}
    x = x.to(F64).permute(0, 2, 3, 4, 1)
    cache = {} if cache is None else cache
    new_cache = {}
    for i, (tc, sc, g) in enumerate(zip(tcs, scs, groups)):
        p = f"encoder.encoder_blocks.{i}."
        x = down(x, sd[p + "compression_block.weight"], sd[p + "compression_block.bias"], int(tc), int(sc))
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            S, new_cache[(i, j)] = sequence(act(x), g, cache.get((i, j)))
            a = conv_a(S, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], g)
            x = conv_b(act(a), x, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"])
    assert x.shape[-1] == channels[-1]
    return x.permute(0, 4, 1, 2, 3), new_cache


def frames_to_latents(sd, kwargs, frames):
    """frames (B, T, H, W, 3) with values 0..255 -> (encode(frames / 127.5 - 1) - mean) / std as (B, t, C, h, w)."""
    x = (frames.to(F64) / 127.5 - 1).permute(0, 4, 1, 2, 3)
    m, _ = encode(sd, kwargs, x)
    mean = torch.tensor(kwargs["mean"]).to(F64)[:, None, None, None]      # fp32 buffers in the reference (vae.py:221-222)
    std = torch.tensor(kwargs["std"]).to(F64)[:, None, None, None]
    return ((m - mean) / std).permute(0, 2, 1, 3, 4)

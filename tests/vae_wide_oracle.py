"""Float64 evaluation of the VAE decoder (reference: edm2/vae/vae.py :18-204, :288-318), written from the formulas, channels-last
[B][T][H][W][C] like the kernels, and stage by stage: the activation, conv A on a given sequence S, conv B, up, out.  Nothing here
casts to fp32 (tests/vae_cpu_restatement.py does, and so cannot judge an fp32 kernel at 1e-5) and nothing launches a kernel.
Fixture G22 (tests/golden/make_golden_vae_wide.py) pins `decode` to the reference in float64."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def seed_params(vae, seed):
    """tests/golden/make_golden_vae.py's seeding, restated: every parameter non-zero; conv weights ~ N(0, 1 / fan_in), biases
    ~ 0.1 N(0, 1), the t_cond linear ~ 0.5 N(0, 1 / fan_in); logvar_multiplier -1.7.  Drawn in fp32 in named_parameters order.
    Then the buffers of the state dict, which a constructor draws at random (MPFourier): freqs ~ 2 pi N(0, 1), phases ~ 2 pi
    U(0, 1), in named_buffers order."""
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
        for name, b in vae.named_buffers():
            if name.endswith(".freqs"):
                b.copy_(2 * math.pi * torch.randn(b.shape, generator=g))
            elif name.endswith(".phases"):
                b.copy_(2 * math.pi * torch.rand(b.shape, generator=g))
    return vae


def param_sums(vae):
    """(sum, sum of squares) in float64 of every entry of the state dict, in its order."""
    return np.array([[p.detach().double().sum().item(), (p.detach().double() ** 2).sum().item()] for p in vae.state_dict().values()])


def area_windows(K, N):
    return [((o * K) // N, -((-(o + 1) * K) // N)) for o in range(N)]


# ---- stages, channels-last float64

def act(x, emb=None):
    """SiLU(RMS(x) (1 + scale) + shift) over the last axis; x (B, T, H, W, C), emb (B, 2C) scale | shift or None."""
    x = x.to(F64)
    C = x.shape[-1]
    v = x / torch.sqrt((x ** 2).mean(dim=-1, keepdim=True) + 1e-4)
    if emb is not None:
        e = emb.to(F64)
        v = v * (1 + e[:, None, None, None, :C]) + e[:, None, None, None, C:]
    return v * torch.sigmoid(v)


def sequence(y, g, cache_in=None):
    """S = [prefix ++ y] (B, g + T, H, W, C) and cache_out = its last g frames; prefix = cache_in or the first g frames of y."""
    S = torch.cat((y[:, :g] if cache_in is None else cache_in.to(y.dtype), y), dim=1)
    return S, S[:, -g:]


def conv_a(S, weight, bias, g):
    """The group-causal conv on S (B, g + T, H, W, C): weight (C g, C, 2g, 3, 3), stride g in time, zero padding 1 in space,
    '(c g) t -> c (t g)'; returns a (B, T, H, W, C)."""
    B, TS, H, W, C = S.shape
    T = TS - g
    x = F.pad(S.to(F64).permute(0, 4, 1, 2, 3), (1, 1, 1, 1))
    y = F.conv3d(x, weight.to(F64), bias.to(F64), stride=(g, 1, 1))                       # (B, C g, T / g, H, W)
    y = y.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def conv_b(u, res, weight, bias):
    """res + bias + conv3x3(u); weight (C, C, 1, 3, 3)."""
    y = F.conv3d(u.to(F64).permute(0, 4, 1, 2, 3), weight.to(F64), bias.to(F64), padding=(0, 1, 1))
    return res.to(F64) + y.permute(0, 2, 3, 4, 1)


def up(x, weight, bias, tc, sc):
    """The decompression 1x1 conv C -> C tc sc^2 and 'b (tc hc wc c) t h w -> b c (t tc) (h hc) (w wc)'; weight (C tc sc^2, C)."""
    B, T, H, W, C = x.shape
    y = x.to(F64) @ weight.to(F64).reshape(-1, C).T + bias.to(F64)                        # (B, T, H, W, tc sc sc C)
    y = y.reshape(B, T, H, W, tc, sc, sc, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return y.reshape(B, T * tc, H * sc, W * sc, C).contiguous()


def out(x, weight, bias):
    """The final 1x1 conv Cin -> Cout + the channel-area residual; weight (Cout, Cin)."""
    x = x.to(F64)
    Cin, Cout = x.shape[-1], weight.shape[0]
    y = x @ weight.to(F64).reshape(Cout, Cin).T + bias.to(F64)
    area = torch.stack([x[..., s0:s1].mean(dim=-1) for s0, s1 in area_windows(Cin, Cout)], dim=-1)
    return y + area


def split(y, logvar_multiplier):
    """(mean, logvar exp(m)) of the last block's output, both (B, T, H, W, Cout / 2)."""
    half = y.shape[-1] // 2
    return y[..., :half], y[..., half:] * math.exp(float(logvar_multiplier))


def temb(sd, q, t):
    """t_cond(MPFourier(t)).  The Fourier features are fp32 by definition (utils.py:145-150 casts t, freqs and phases to fp32 in a
    model of any dtype); the linear map is float64."""
    f32 = torch.float32
    four = (torch.cos(torch.outer(t.to(f32), sd[q + "fourier_cond.freqs"].to(f32)) + sd[q + "fourier_cond.phases"].to(f32))
            * math.sqrt(2)).to(F64)
    return four @ sd[q + "t_cond.weight"].T + sd[q + "t_cond.bias"]


# ---- the whole decoder

def decode(sd, kwargs, z, t, cache=None):
    """z (B, C, T, h, w), t (B,) -> (mean, logvar (B, 3, T', H, W) float64, cache {(block, res block): (B, g, H, W, C)})."""
    channels = list(kwargs["channels"])[::-1]
    outs = channels[1:]
    outs[-1] = 2 * outs[-1]
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    groups = [int(g) for g in np.cumprod(tcs)]
    sd = {k: v.to(F64) for k, v in sd.items()}
    x = z.to(F64).permute(0, 2, 3, 4, 1)
    t = torch.as_tensor(t, dtype=F64).reshape(-1)
    if t.numel() == 1:
        t = t.expand(x.shape[0])
    cache = {} if cache is None else cache
    new_cache = {}
    for i, (C, Cout, tc, sc, g) in enumerate(zip(channels[:-1], outs, tcs, scs, groups)):
        p = f"decoder.encoder_blocks.{i}."
        x = up(x, sd[p + "decompression_block.weight"], sd[p + "decompression_block.bias"], int(tc), int(sc))
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            S, new_cache[(i, j)] = sequence(act(x, temb(sd, q, t)), g, cache.get((i, j)))
            a = conv_a(S, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], g)
            x = conv_b(act(a), x, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"])
        x = out(x, sd[p + "final_conv.weight"], sd[p + "final_conv.bias"])
    mean, logvar = split(x, sd["decoder.logvar_multiplier"])
    return mean.permute(0, 4, 1, 2, 3), logvar.permute(0, 4, 1, 2, 3), new_cache


def frames_pre(sd, kwargs, latents, t=0.1):
    """latents (B, T, C, h, w) -> clip((mean + 1) 127.5, 0, 255) (B, T', H, W, 3) before truncation (vae.py:288-318)."""
    std = torch.tensor(kwargs["std"]).to(F64)[:, None, None]               # fp32 buffers in the reference (vae.py:221-222)
    mean = torch.tensor(kwargs["mean"]).to(F64)[:, None, None]
    z = (latents.to(F64) * std + mean).permute(0, 2, 1, 3, 4)
    m, _, _ = decode(sd, kwargs, z, t * torch.ones(latents.shape[0], dtype=F64))
    return torch.clip((m + 1) * 127.5, 0, 255).permute(0, 2, 3, 4, 1)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()

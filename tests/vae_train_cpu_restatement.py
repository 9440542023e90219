"""Plain-PyTorch restatement of the VAE's training forward (reference: edm2/vae/vae.py :18-53, :56-93, :96-141, :167-204,
:228-237), channels-first, from a state dict and the constructor kwargs.  Written from the formulas, independently of both the
reference's modules and the HIP kernels.  It runs in the dtype of its inputs and is differentiable by autograd with respect to
every state-dict entry that requires grad.  Unlike the decoder / encoder restatements (inference) it uses the training-mode
prefix of the group-causal convs: the first g activated input frames, DETACHED (vae.py:43-44), so that its autograd gradients
are the reference's.  Fixture G16 (tests/golden/make_golden_vae_train.py) pins it to the reference."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _rms(x):
    return x / torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-4)


def _area_channels(x, cout):
    cin = x.shape[1]
    outs = []
    for o in range(cout):
        s0, s1 = (o * cin) // cout, -((-(o + 1) * cin) // cout)
        outs.append(x[:, s0:s1].mean(dim=1))
    return torch.stack(outs, dim=1)


def _res_block(sd, q, x, g, t, emb=None):
    """vae.py:74-93 in training mode without a cache.  emb (B, 2C): a ready scale | shift in place of the one computed from t."""
    B, C, T, H, W = x.shape
    y = _rms(x)
    if emb is not None:
        y = y * (1 + emb[:, :C, None, None, None]) + emb[:, C:, None, None, None]
    elif t is not None:
        four = torch.cos(t.float()[:, None] * sd[q + "fourier_cond.freqs"][None].float() +      # MPFourier works in fp32
                         sd[q + "fourier_cond.phases"][None].float()) * math.sqrt(2)            # whatever t is (utils.py:145-150)
        four = four.to(t.dtype)
        e = four @ sd[q + "t_cond.weight"].T + sd[q + "t_cond.bias"]
        y = y * (1 + e[:, :C, None, None, None]) + e[:, C:, None, None, None]
    yp = F.pad(F.silu(y), (1, 1, 1, 1))
    seq = torch.cat((yp[:, :, :g].detach(), yp), dim=2)
    y = F.conv3d(seq, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], stride=(g, 1, 1))
    y = y.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)         # '(c g) t -> c (t g)'
    y = F.silu(_rms(y))
    return x + F.conv3d(y, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"], padding=(0, 1, 1))


def down(x, weight, bias, tc, sc):
    """vae.py:157-161, :109-122: 'b c (t tc) (h hc) (w wc) -> b (tc hc wc c) t h w', the compression conv plus the channel-area
    residual of the rearranged input."""
    B, C, T, H, W = x.shape
    T, H, W = T // tc, H // sc, W // sc
    x = x.reshape(B, C, T, tc, H, sc, W, sc).permute(0, 3, 5, 7, 1, 2, 4, 6).reshape(B, tc * sc * sc * C, T, H, W)
    return F.conv3d(x, weight, bias) + _area_channels(x, weight.shape[0])


def up(x, weight, bias, tc, sc):
    """vae.py:96-133, :148-164: the decompression conv, then 'b (tc hc wc c) t h w -> b c (t tc) (h hc) (w wc)'."""
    C = x.shape[1]
    x = F.conv3d(x, weight, bias)
    B, _, T, H, W = x.shape
    return x.reshape(B, tc, sc, sc, C, T, H, W).permute(0, 4, 5, 1, 6, 2, 7, 3).reshape(B, C, T * tc, H * sc, W * sc)


def out(x, weight, bias):
    """vae.py:128-141: the final conv plus the channel-area residual."""
    return F.conv3d(x, weight, bias) + _area_channels(x, weight.shape[0])


def forward(sd, kwargs, x, t_sample, noise):
    """x (B, 3, T, H, W), t_sample (B,), noise (the shape of mean) -> (r_mean, r_logvar, mean) of VAE.forward in training mode
    with t_b = t_sample and randn_like(mean) = noise."""
    channels = list(kwargs["channels"])
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    n_res = kwargs["n_res_blocks"]
    # encoder
    groups = [int(g) for g in np.cumprod(tcs)[::-1]]
    for i, (Cout, tc, sc, g) in enumerate(zip(channels[1:], tcs, scs, groups)):
        p = f"encoder.encoder_blocks.{i}."
        x = down(x, sd[p + "compression_block.weight"], sd[p + "compression_block.bias"], tc, sc)
        for j in range(n_res):
            x = _res_block(sd, p + f"res_blocks.{j}.", x, g, None)
    mean = x
    # the mix (vae.py:233-234)
    t = t_sample.reshape(-1)
    tb = t[:, None, None, None, None]
    x = mean * (1 - tb) + noise * tb
    # decoder
    channels = channels[::-1]
    outs = channels[1:]
    outs[-1] = 2 * outs[-1]
    groups = [int(g) for g in np.cumprod(tcs)]
    for i, (C, Cout, tc, sc, g) in enumerate(zip(channels[:-1], outs, tcs, scs, groups)):
        p = f"decoder.encoder_blocks.{i}."
        x = up(x, sd[p + "decompression_block.weight"], sd[p + "decompression_block.bias"], tc, sc)
        for j in range(n_res):
            x = _res_block(sd, p + f"res_blocks.{j}.", x, g, t)
        x = out(x, sd[p + "final_conv.weight"], sd[p + "final_conv.bias"])
    r_mean, r_logvar = x.split(x.shape[1] // 2, dim=1)
    return r_mean, r_logvar * torch.exp(sd["decoder.logvar_multiplier"]), mean


def cotangents(shape, phi, dtype):
    """The closed-form cotangent cos(0.7 i + phi) over the flat index of an output of `shape`."""
    n = int(np.prod(shape))
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64) + phi).reshape(shape).to(dtype)


PHIS = (0.1, 1.3, 2.9)


def loss(r_mean, r_logvar, mean, phis=PHIS):
    """L = sum r_mean c1 + sum r_logvar c2 + sum mean c3 with c_k = cos(0.7 i + phi_k); phi = 0.1, 1.3, 2.9 is fixture G16's."""
    return sum((o * cotangents(o.shape, phi, o.dtype).to(o.device)).sum() for o, phi in zip((r_mean, r_logvar, mean), phis))


def grads(sd, kwargs, x, t_sample, noise, dtype=torch.float64, phis=(PHIS,)):
    """Outputs and every parameter gradient of the sum of `loss` over `phis`, in `dtype`, on the CPU."""
    leaves = {k: v.detach().cpu().to(dtype).requires_grad_("fourier_cond" not in k) for k, v in sd.items()}
    r_mean, r_logvar, mean = forward(leaves, kwargs, x.cpu().to(dtype), t_sample.cpu().to(dtype), noise.cpu().to(dtype))
    sum(loss(r_mean, r_logvar, mean, ph) for ph in phis).backward()
    outs = dict(r_mean=r_mean.detach(), r_logvar=r_logvar.detach(), mean=mean.detach())
    return outs, {k: v.grad for k, v in leaves.items() if v.requires_grad}

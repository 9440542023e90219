"""The bf16-faithful float64 oracle of VAE.bf16_inference() (autoregressive_diffusion_amd/vae.py, csrc/vae_wide_bf16.h): the float64
stage functions of tests/vae_wide_oracle.py and tests/vae_wide_encoder_oracle.py, called on operands passed through
`t.float().bfloat16().double()` (round-to-nearest-even, once) at exactly the points the contract names -- the weights and the
activated input of conv A, conv B, up, down and out -- with the bias, conv B's residual and the channel-area terms taken from the
unrounded tensors.  Whole models round only where the model launches an MFMA kernel: in blocks wider than 64 channels, and in the
`down` of a narrow block that compresses more than 512 channels (the GEMM).  Nothing here launches a kernel.

Also here: the float32 evaluation of a stage on the same rounded operands (torch's own conv / matmul in float32: what the bound of a
stage test is derived from), the judge of a stage test, and the oracle with one deliberate defect at a time (DEFECTS), which
tests/test_vae_bf16.py holds against the faithful one."""
import numpy as np
import torch
import torch.nn.functional as F

import vae_stage_oracle as S
import vae_wide_encoder_oracle as E
import vae_wide_oracle as O

F64 = torch.float64
MAX_NARROW, MAX_DOWN_K = 64, 512
FLOOR = 1e-5                        # the project's bound for these stages (tests/test_vae_512_gpu.py TOL); FACTOR is S.FACTOR
DEFECTS = ("weights_unrounded", "activations_unrounded", "truncation", "residual_rounded")
HAS_RESIDUAL = ("conv_b", "out", "down")      # the stages "residual_rounded" can touch


def rne(t):
    """fp32 -> bf16, round to nearest even, as float64."""
    return t.float().bfloat16().double()


def trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (the defect a staging conversion must not have), as float64."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def _rounders(defect):
    """(weights, activations, residual source) of the oracle with `defect` (None: the contract)."""
    assert defect is None or defect in DEFECTS, defect
    ident = lambda t: t.double()
    r = trunc if defect == "truncation" else rne
    rw = ident if defect == "weights_unrounded" else r
    ra = ident if defect == "activations_unrounded" else r
    rr = r if defect == "residual_rounded" else ident
    return rw, ra, rr


def _area(x, cout):
    """interpolate_channels of channels-last x: the mean over the window [floor(o K / cout), ceil((o + 1) K / cout))."""
    return torch.stack([x[..., s0:s1].mean(dim=-1) for s0, s1 in O.area_windows(x.shape[-1], cout)], dim=-1)


# ---- stages, channels-last; the operands arrive unrounded (fp32 values in any dtype)

def conv_a(Sq, weight, bias, g, defect=None):
    rw, ra, _ = _rounders(defect)
    return O.conv_a(ra(Sq), rw(weight), bias, g)


def conv_b(u, res, weight, bias, defect=None):
    rw, ra, rr = _rounders(defect)
    return O.conv_b(ra(u), rr(res), rw(weight), bias)


def up(x, weight, bias, tc, sc, defect=None):
    rw, ra, _ = _rounders(defect)
    return O.up(ra(x), rw(weight), bias, tc, sc)


def out(x, weight, bias, defect=None, area=True):
    """O.out with the product on rounded operands and the area term on the unrounded x (area=False: the product and bias alone)."""
    rw, ra, rr = _rounders(defect)
    Cin, Cout = x.shape[-1], weight.shape[0]
    y = ra(x) @ rw(weight).reshape(Cout, Cin).T + bias.double()
    return y + _area(rr(x), Cout) if area else y


def down(x, weight, bias, tc, sc, defect=None, area=True):
    """E.down likewise: x (B, T tc, H sc, W sc, C)."""
    rw, ra, rr = _rounders(defect)
    Cout = weight.shape[0]
    y = E.rearrange_down(ra(x), tc, sc) @ rw(weight).reshape(Cout, -1).T + bias.double()
    return y + _area(E.rearrange_down(rr(x), tc, sc), Cout) if area else y


def stage(kind, *args, defect=None):
    return dict(conv_a=conv_a, conv_b=conv_b, up=up, out=out, down=down)[kind](*args, defect=defect)


def unrounded(kind, *args):
    """The stage in float64 on the operands as they are: the oracle of the fp32 path."""
    return dict(conv_a=O.conv_a, conv_b=O.conv_b, up=O.up, out=O.out, down=E.down)[kind](*args)


# ---- the float32 evaluation of the same rounded operands: torch's conv / matmul in float32, not the code under test

def stage32(kind, *args):
    f, r = torch.float32, lambda t: t.float().bfloat16().float()
    if kind == "conv_a":
        Sq, w, b, g = args
        B, TS, H, W, C = Sq.shape
        T = TS - g
        y = F.conv3d(F.pad(r(Sq).permute(0, 4, 1, 2, 3), (1, 1, 1, 1)), r(w), b.to(f), stride=(g, 1, 1))
        y = y.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)
        return y.permute(0, 2, 3, 4, 1)
    if kind == "conv_b":
        u, res, w, b = args
        return res.to(f) + F.conv3d(r(u).permute(0, 4, 1, 2, 3), r(w), b.to(f), padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
    if kind == "up":
        x, w, b, tc, sc = args
        B, T, H, W, C = x.shape
        y = (r(x) @ r(w).reshape(-1, C).T + b.to(f)).reshape(B, T, H, W, tc, sc, sc, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
        return y.reshape(B, T * tc, H * sc, W * sc, C)
    if kind == "out":
        x, w, b = args
        return r(x) @ r(w).reshape(w.shape[0], -1).T + b.to(f) + _area(x.to(f), w.shape[0])
    x, w, b, tc, sc = args
    return E.rearrange_down(r(x), tc, sc) @ r(w).reshape(w.shape[0], -1).T + b.to(f) + _area(E.rearrange_down(x.to(f), tc, sc), w.shape[0])


def bound(kind, *args):
    """(the faithful float64 result, the bounds (rel L2, max / rms) of a Gaussian stage test, the float32 evaluation's figures):
    max(FLOOR, S.FACTOR x the distance of the float32 evaluation of the same rounded operands from float64), per metric."""
    ref = stage(kind, *args)
    f32 = S.metrics(stage32(kind, *args), ref)
    return ref, tuple(max(FLOOR, S.FACTOR * m) for m in f32), f32


def outside(got, ref, bnd):
    """The figures of `got` against `ref` and whether either exceeds its bound."""
    m = S.metrics(got, ref)
    return m, not (m[0] <= bnd[0] and m[1] <= bnd[1])


# ---- whole models: the rounding in blocks wider than MAX_NARROW only (faithful=False: the unrounded float64 oracle)

def decode(sd, kwargs, z, t, cache=None, faithful=True):
    """O.decode with the bf16 rounding of the contract in the wide blocks."""
    if not faithful:
        return O.decode(sd, kwargs, z, t, cache)
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
    for i, (C, tc, sc, g) in enumerate(zip(channels[:-1], tcs, scs, groups)):
        wide = C > MAX_NARROW
        p = f"decoder.encoder_blocks.{i}."
        x = (up if wide else O.up)(x, sd[p + "decompression_block.weight"], sd[p + "decompression_block.bias"], int(tc), int(sc))
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            Sq, new_cache[(i, j)] = O.sequence(O.act(x, O.temb(sd, q, t)), g, cache.get((i, j)))
            a = (conv_a if wide else O.conv_a)(Sq, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], g)
            x = (conv_b if wide else O.conv_b)(O.act(a), x, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"])
        x = (out if wide else O.out)(x, sd[p + "final_conv.weight"], sd[p + "final_conv.bias"])
    mean, logvar = O.split(x, sd["decoder.logvar_multiplier"])
    return mean.permute(0, 4, 1, 2, 3), logvar.permute(0, 4, 1, 2, 3), new_cache


def encode(sd, kwargs, x, cache=None, faithful=True):
    """E.encode with the bf16 rounding of the contract in the wide blocks (a block is wide by its OUTPUT width), and in the `down`
    of a narrow block that compresses more than MAX_DOWN_K = 512 channels: that one runs as the GEMM, on MFMA operands."""
    if not faithful:
        return E.encode(sd, kwargs, x, cache)
    channels = list(kwargs["channels"])
    tcs, scs = kwargs.get("time_compressions", [1, 2, 2]), kwargs.get("spatial_compressions", [1, 2, 2])
    groups = [int(g) for g in np.cumprod(tcs)][::-1]
    sd = {k: v.to(F64) for k, v in sd.items()}
    x = x.to(F64).permute(0, 2, 3, 4, 1)
    cache = {} if cache is None else cache
    new_cache = {}
    for i, (tc, sc, g) in enumerate(zip(tcs, scs, groups)):
        wide = channels[i + 1] > MAX_NARROW
        p = f"encoder.encoder_blocks.{i}."
        gemm = wide or x.shape[-1] * int(tc) * int(sc) ** 2 > MAX_DOWN_K
        x = (down if gemm else E.down)(x, sd[p + "compression_block.weight"], sd[p + "compression_block.bias"], int(tc), int(sc))
        for j in range(kwargs["n_res_blocks"]):
            q = p + f"res_blocks.{j}."
            Sq, new_cache[(i, j)] = O.sequence(O.act(x), g, cache.get((i, j)))
            a = (conv_a if wide else O.conv_a)(Sq, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], g)
            x = (conv_b if wide else O.conv_b)(O.act(a), x, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"])
    return x.permute(0, 4, 1, 2, 3), new_cache


def forward(sd, kwargs, x, t_sample, noise, faithful=True):
    """The eval-mode VAE.forward: (r_mean, r_logvar, mean), float64."""
    mean = encode(sd, kwargs, x, faithful=faithful)[0]
    tb = t_sample.double()[:, None, None, None, None]
    r_mean, r_logvar, _ = decode(sd, kwargs, mean * (1 - tb) + noise.double() * tb, t_sample, faithful=faithful)
    return r_mean, r_logvar, mean

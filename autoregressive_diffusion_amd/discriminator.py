"""The VAE's adversarial critic (reference: edm2/vae/discriminator.py) -- `from autoregressive_diffusion_amd.discriminator import
MixedDiscriminator` instead of `from edm2.vae import MixedDiscriminator`.

`Discriminator2D`, the per-frame half and by far the larger one, runs on HIP kernels (include/oniris.h: oniris_disc_*, csrc/disc.hip,
csrc/disc_conv3.h, csrc/disc_parts.h): fp32 storage and fp32 arithmetic, every convolution an implicit GEMM on the exact-f32 matrix
instruction.  One
autograd Function per block plus the stem and the head; activations travel between them channels-last [N][H][W][C].  BatchNorm and
LeakyReLU never exist as tensors: a conv emits per-tile (count, centre, S2, S1) of what it stores, a finalize launch turns them into the
per-channel scale s and shift t, and the consumer (the next conv, or the blur pool) applies lrelu(x s + t) while it stages its operand.
What stays in torch: the NCHW <-> channels-last copies at the two ends and permutations at parameter size.

`Discriminator3D`, the spatio-temporal half, runs on HIP kernels as well when model and input are on the GPU (oniris_disc3d_*,
csrc/disc3d.hip, csrc/disc_conv3d.h, the tile parts shared with the 2-D half in csrc/disc_parts.h): the same structure on
[N][T][H][W][C], a 27-tap conv being the sum over kt of 9-tap convs of neighbouring planes, GroupNorm(32) in place of BatchNorm with
scale and shift per (sample, channel), a stride-2 stem and a 3-D blur
pool; with CPU tensors it stays plain torch.nn code.  `MixedDiscriminator` joins the two as the reference does.

Gradients are summed in a fixed order into a bounded number of partial slabs and then over the slabs; nothing uses atomics, two runs
give the same bits."""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .vae import _p, _stream

_REF = "the reference's edm2.vae (this package runs the 2-D discriminator on HIP kernels only)"
_SLAB_BYTES = 64 << 20          # the most memory one launch's partial slabs may take
_MAX_SLABS = 1024               # and the most slabs: tests lower it to make the work items wrap
MAX_WIDTH = 256
_SCALE = 1.0 / math.sqrt(2.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: thin wrappers, one per entry point, on channels-last fp32 tensors of the GPU

def _nslab(work, size):
    """Partial slabs of `size` floats for `work` work items: one per item up to _MAX_SLABS, fewer when the slabs are large."""
    return int(max(1, min(work, _MAX_SLABS, max(64, _SLAB_BYTES // (4 * size)))))


def _padc(c):
    return 8 if c <= 8 else c


def pack_weight(w):
    """nn.Conv2d weight (Cout, Cin, k, k) -> the forward layout [taps][CinP][CoutP] of oniris_disc_conv."""
    Cout, Cin, kh, kw = w.shape
    out = torch.zeros(kh * kw, _padc(Cin), -(-Cout // 32) * 32, dtype=torch.float32, device=w.device)
    out[:, :Cin, :Cout] = w.detach().float().permute(2, 3, 1, 0).reshape(kh * kw, Cin, Cout)
    return out


def pack_weight_dgrad(w, scale=1.0):
    """nn.Conv2d weight -> the layout of the data gradient: the conv Cout -> Cin on w'[8 - tap][co][ci] (times `scale`)."""
    Cout, Cin, kh, kw = w.shape
    out = torch.zeros(kh * kw, _padc(Cout), -(-Cin // 32) * 32, dtype=torch.float32, device=w.device)
    out[:, :Cout, :Cin] = w.detach().float().flip(2, 3).permute(2, 3, 0, 1).reshape(kh * kw, Cout, Cin) * scale
    return out


def conv(x, wp, bias, Cout, taps, pro=None, res=None, res_scale=1.0, stats=False):
    """oniris_disc_conv: x (N, H, W, Cin), wp packed -> (out (N, H, W, Cout), per-tile statistics or None)."""
    N, H, W, Cin = x.shape
    out = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x.device)
    part = torch.empty(N * -(-H // 16) * -(-W // 16), 4, Cout, dtype=torch.float32, device=x.device) if stats else None
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc_conv(_p(x), _p(wp), _p(bias), _p(s), _p(t), _p(res), res_scale, _p(out), _p(part), N, H, W, Cin,
                                         Cout, taps, _stream()), "disc_conv")
    return out, part


def finalize(part, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """oniris_disc_stats_finalize -> stats (5, C): mean, biased var, s, t, rstd; updates the running buffers in place."""
    P, _, C = part.shape
    stats = torch.empty(5, C, dtype=torch.float32, device=part.device)
    _lib.check(_lib.lib.oniris_disc_stats_finalize(_p(part), P, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum,
                                                   eps, _p(stats), _stream()), "disc_stats_finalize")
    return stats


def blur(x, pro=None):
    N, H, W, C = x.shape
    out = torch.empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc_blur(_p(x), _p(s), _p(t), _p(out), N, H, W, C, _stream()), "disc_blur")
    return out


def blur_bwd(dy, H, W):
    N, _, _, C = dy.shape
    dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_disc_blur_bwd(_p(dy), _p(dx), N, H, W, C, _stream()), "disc_blur_bwd")
    return dx


def bn_bwd(da, z, stats, add=None, add_scale=1.0, eval_mode=False, want_dx=True):
    """BatchNorm + LeakyReLU backward at z: -> (dx or None, sums (2, C) = d beta | d gamma)."""
    C = z.shape[-1]
    npix = z.numel() // C
    P = -(-npix // 1024)
    part = torch.empty(P, 2 * C, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib.oniris_disc_bn_bwd_reduce(_p(da), _p(z), _p(stats), _p(part), npix, C, _stream()), "disc_bn_bwd_reduce")
    sums = torch.empty(2, C, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib.oniris_disc_part_sum(_p(part), P, 2 * C, _p(sums), _stream()), "disc_part_sum")
    dx = None
    if want_dx:
        dx = torch.empty_like(z)
        _lib.check(_lib.lib.oniris_disc_bn_bwd_dx(_p(da), _p(z), _p(stats), _p(sums), _p(add), add_scale, _p(dx), npix, C,
                                                  int(eval_mode), _stream()), "disc_bn_bwd_dx")
    return dx, sums


def wgrad(x, dy, taps, pro=None):
    """oniris_disc_wgrad + the slab sum -> (d weight in nn.Conv2d's layout (Cout, Cin, k, k), d bias (Cout,))."""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    n = taps * Cin * Cout + Cout
    nslab = _nslab(N * -(-H // 16) * -(-W // 16), n)
    slab = torch.empty(nslab, n, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc_wgrad(_p(x), _p(s), _p(t), _p(dy), _p(slab), nslab, N, H, W, Cin, Cout, taps, _stream()),
               "disc_wgrad")
    r = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_vae_slab_sum_bwd(_p(slab), nslab, n, _p(r), _stream()), "vae_slab_sum_bwd")
    k = 3 if taps == 9 else 1
    return r[:n - Cout].view(k, k, Cin, Cout).permute(3, 2, 0, 1), r[n - Cout:]


def _f32(t):
    return t.detach().float().contiguous()


def _norm_stats(norm, part, training):
    """The (5, C) statistics of one BatchNorm: from the producer's partials (training: running buffers move) or the buffers."""
    if training:
        st = finalize(part, _f32(norm.weight), _f32(norm.bias), norm.running_mean, norm.running_var, norm.momentum, norm.eps)
        norm.num_batches_tracked += 1
        return st
    rstd = torch.rsqrt(norm.running_var.float() + norm.eps)
    s = norm.weight.detach().float() * rstd
    return torch.stack((norm.running_mean.float(), norm.running_var.float(), s, norm.bias.detach().float() - norm.running_mean * s,
                        rstd)).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# autograd

class Stem(torch.autograd.Function):
    """conv_in / conv_out: x (N, H, W, Cin) -> (conv + bias (N, H, W, Cout), the statistics partials of it or None)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stats):
        x = x.contiguous()
        out, part = conv(x, pack_weight(weight), _f32(bias), weight.shape[0], 9, stats=stats)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(*(() if part is None else (part,)))
        return out, part

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = wgrad(x, dout, 9)
        if ctx.needs_input_grad[0]:
            dx = conv(dout, pack_weight_dgrad(weight), None, weight.shape[1], 9)[0]
        return dx, dw, db, None


class Block(torch.autograd.Function):
    """A DiscriminatorBlock2D: x (N, H, W, Cin) and the statistics partials of x -> ((conv2(..) + shortcut) / sqrt 2, partials)."""

    @staticmethod
    def forward(ctx, x, part, g1, b1, w1, c1, g2, b2, w2, c2, ws, bs, blk, stats_out):
        x = x.contiguous()
        N, H, W, Cin = x.shape
        Cout = w1.shape[0]
        train, down = blk.training, ws is not None
        if train and N * H * W < 2:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm2d)")
        st1 = _norm_stats(blk.norm1, part, train)
        h1, part1 = conv(x, pack_weight(w1), _f32(c1), Cout, 9, pro=(st1[2], st1[3]), stats=train)
        st2 = _norm_stats(blk.norm2, part1, train)
        if down:
            b0 = blur(x)
            sc = conv(b0, pack_weight(ws), _f32(bs), Cout, 1)[0]
            pooled = blur(h1, pro=(st2[2], st2[3]))
            out, part_o = conv(pooled, pack_weight(w2), _f32(c2), Cout, 9, res=sc, res_scale=_SCALE, stats=stats_out)
            ctx.save_for_backward(x, h1, st1, st2, w1, w2, pooled, b0, ws)
        else:
            out, part_o = conv(h1, pack_weight(w2), _f32(c2), Cout, 9, pro=(st2[2], st2[3]), res=x, res_scale=_SCALE,
                               stats=stats_out)
            ctx.save_for_backward(x, h1, st1, st2, w1, w2)
        ctx.train, ctx.down = train, down
        ctx.mark_non_differentiable(*(() if part_o is None else (part_o,)))
        return out, part_o

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, h1, st1, st2, w1, w2 = ctx.saved_tensors[:6]
        need = ctx.needs_input_grad
        dout = dout.contiguous()
        N, H, W, Cin = x.shape
        Cout = w1.shape[0]
        ev = not ctx.train
        dx = dg1 = db1 = dw1 = dc1 = dg2 = db2 = dw2 = dc2 = dws = dbs = None
        # conv2 and what it read
        if ctx.down:
            pooled, b0, ws = ctx.saved_tensors[6:]
            if need[8] or need[9]:
                dw2, dc2 = (g * _SCALE for g in wgrad(pooled, dout, 9))
            da2 = blur_bwd(conv(dout, pack_weight_dgrad(w2, _SCALE), None, Cout, 9)[0], H, W)
        else:
            if need[8] or need[9]:
                dw2, dc2 = (g * _SCALE for g in wgrad(h1, dout, 9, pro=(st2[2], st2[3])))
            da2 = conv(dout, pack_weight_dgrad(w2, _SCALE), None, Cout, 9)[0]
        # norm2 + LeakyReLU
        dh1, sums2 = bn_bwd(da2, h1, st2, eval_mode=ev)
        if need[6]:
            dg2 = sums2[1].clone()
        if need[7]:
            db2 = sums2[0].clone()
        # conv1
        if need[4] or (need[5] and ev):
            dw1, dc1 = wgrad(x, dh1, 9, pro=(st1[2], st1[3]))
        if need[5] and not ev:
            dc1 = torch.zeros(Cout, dtype=torch.float32, device=x.device)       # a bias in front of a BatchNorm: exactly zero
        # norm1 + LeakyReLU, plus the shortcut's share of dx
        if need[0] or need[2] or need[3]:
            da1 = conv(dh1, pack_weight_dgrad(w1), None, Cin, 9)[0]
            add, add_scale = None, 1.0
            if need[0]:
                if ctx.down:
                    add = blur_bwd(conv(dout, pack_weight_dgrad(ws, _SCALE), None, Cin, 1)[0], H, W)
                else:
                    add, add_scale = dout, _SCALE
            dx, sums1 = bn_bwd(da1, x, st1, add, add_scale, eval_mode=ev, want_dx=need[0])
            if need[2]:
                dg1 = sums1[1].clone()
            if need[3]:
                db1 = sums1[0].clone()
        if ctx.down and (need[10] or need[11]):
            dws, dbs = (g * _SCALE for g in wgrad(b0, dout, 1))
        return dx, None, dg1, db1, dw1, dc1, dg2, db2, dw2, dc2, dws, dbs, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# modules: parameter holders with the reference's names (load_state_dict(strict=True) takes a reference checkpoint)

def _blur_filter(channels, dims):
    f = torch.tensor([1.0, 2.0, 1.0])
    k = f
    for _ in range(dims - 1):
        k = k[..., None] * f
    k = k / k.sum()
    return k[None, None].repeat(channels, 1, *([1] * dims)).contiguous()


class BlurPooling2D(nn.Module):
    """The [1,2,1] x [1,2,1] / 16 filter at stride 2, padding 1, per channel (discriminator.py:154-178): the buffer `filt`."""

    def __init__(self, in_channels, out_channels=None):
        super().__init__()
        assert out_channels is None or out_channels == in_channels
        self.in_channels = self.out_channels = in_channels
        self.register_buffer("filt", _blur_filter(in_channels, 2))

    def forward(self, x):
        return F.conv2d(x, self.filt, stride=2, padding=1, groups=self.in_channels)


class BlurPooling3D(nn.Module):
    def __init__(self, in_channels, out_channels=None):
        super().__init__()
        assert out_channels is None or out_channels == in_channels
        self.in_channels = self.out_channels = in_channels
        self.register_buffer("filt", _blur_filter(in_channels, 3))

    def forward(self, x):
        return F.conv3d(x, self.filt, stride=2, padding=1, groups=self.in_channels)


class DiscriminatorBlock2D(nn.Module):
    """discriminator.py:11-67 (parameters and buffers only; the computation is `Block`)."""

    def __init__(self, in_channels, out_channels, add_downsample=True):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1)
        self.downsampler = BlurPooling2D(out_channels) if add_downsample else nn.Identity()
        self.norm2 = nn.BatchNorm2d(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1)
        self.shortcut = (nn.Sequential(BlurPooling2D(in_channels), nn.Conv2d(in_channels, out_channels, kernel_size=1))
                         if add_downsample else nn.Identity())
        self.add_downsample = add_downsample


class Discriminator2D(nn.Module):
    """The reference's Discriminator2D (discriminator.py:70-111) on HIP kernels, forward and backward.

    Domain: in_channels 1..8; every width a multiple of 32 up to 256; the last two widths equal (the final block's shortcut is the
    identity); any H, W >= 1; fp32 input (N, C, H, W) on the GPU -> logits (N, 2, H', W'), H' = H halved len(widths) - 1 times by
    (H - 1) // 2 + 1.  Anything else raises NotImplementedError.  Train mode normalises with batch statistics and moves the running
    buffers on every forward, eval mode uses the buffers, as nn.BatchNorm2d does.  `conv_norm_out` exists and is unused, as in the
    reference: its gradients stay None.

    Gradients: of the input and of every used parameter; what nobody asked for (requires_grad, needs_input_grad) is not computed --
    with the parameters frozen, a backward launches no weight-gradient kernel.  In train mode `blocks.i.conv1.bias` sits in front of
    a BatchNorm that subtracts the batch mean, so its gradient is exactly zero: zeros are returned without computing anything."""

    def __init__(self, in_channels=3, block_out_channels=(64,)):
        super().__init__()
        widths = [int(c) for c in block_out_channels]
        if not 1 <= int(in_channels) <= 8:
            raise NotImplementedError(f"Discriminator2D: in_channels {in_channels}: the HIP kernels take 1..8")
        if not widths or any(c % 32 or not 32 <= c <= MAX_WIDTH for c in widths):
            raise NotImplementedError(f"Discriminator2D: widths {widths}: the HIP kernels take multiples of 32 up to {MAX_WIDTH}")
        if len(widths) > 1 and widths[-1] != widths[-2]:
            raise NotImplementedError(f"Discriminator2D: widths {widths}: the last two must be equal (the final block's shortcut "
                                      "is the identity)")
        self.conv_in = nn.Conv2d(in_channels, widths[0], kernel_size=3, padding=1)
        self.blocks = nn.ModuleList()
        cin = widths[0]
        for i, c in enumerate(widths):
            self.blocks.append(DiscriminatorBlock2D(cin, c, add_downsample=i < len(widths) - 1))
            cin = c
        self.conv_norm_out = nn.BatchNorm2d(widths[-1])
        self.conv_out = nn.Conv2d(widths[-1], 2, kernel_size=3, padding=1)

    def forward(self, x):
        if not x.is_cuda or not self.conv_in.weight.is_cuda:
            raise NotImplementedError(f"Discriminator2D: runs on HIP kernels only (model and input on the GPU); on the CPU use {_REF}")
        if x.dim() != 4 or x.shape[1] != self.conv_in.in_channels:
            raise ValueError(f"Discriminator2D: input {tuple(x.shape)}, expected (N, {self.conv_in.in_channels}, H, W)")
        y = x.float().permute(0, 2, 3, 1)
        y, part = Stem.apply(y, self.conv_in.weight, self.conv_in.bias, self.training)
        for i, blk in enumerate(self.blocks):
            sc = blk.shortcut[1] if blk.add_downsample else None
            y, part = Block.apply(y, part, blk.norm1.weight, blk.norm1.bias, blk.conv1.weight, blk.conv1.bias, blk.norm2.weight,
                                  blk.norm2.bias, blk.conv2.weight, blk.conv2.bias, None if sc is None else sc.weight,
                                  None if sc is None else sc.bias, blk, self.training and i < len(self.blocks) - 1)
        y, _ = Stem.apply(y, self.conv_out.weight, self.conv_out.bias, False)
        return y.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the 3-D half: launches on channels-last fp32 tensors (N, T, H, W, C) of the GPU

GROUPS = 32


def _nslab3(work, size):
    """Partial slabs for a 27-tap weight gradient: as _nslab, without its floor of 64 -- one launch stays within _SLAB_BYTES."""
    return int(max(1, min(work, _MAX_SLABS, _SLAB_BYTES // (4 * size))))


def _half(n):
    return (n - 1) // 2 + 1


def pack_weight3(w):
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) -> the forward layout [27][CinP][CoutP] of oniris_disc3d_conv."""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(27, _padc(Cin), -(-Cout // 32) * 32, dtype=torch.float32, device=w.device)
    out[:, :Cin, :Cout] = w.detach().float().permute(2, 3, 4, 1, 0).reshape(27, Cin, Cout)
    return out


def pack_weight3_dgrad(w, scale=1.0):
    """nn.Conv3d weight -> the layout of the stride-1 data gradient: the conv Cout -> Cin on w'[26 - tap][co][ci] (times `scale`)."""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(27, _padc(Cout), -(-Cin // 32) * 32, dtype=torch.float32, device=w.device)
    out[:, :Cout, :Cin] = w.detach().float().flip(2, 3, 4).permute(2, 3, 4, 0, 1).reshape(27, Cout, Cin) * scale
    return out


def conv3(x, wp, bias, Cout, stride=1, pro=None, res=None, res_scale=1.0, stats=False):
    """oniris_disc3d_conv: x (N, T, H, W, Cin), wp packed -> (out (N, T', H', W', Cout), per-tile statistics (N, P, 4, Cout) or None)."""
    N, T, H, W, Cin = x.shape
    To, Ho, Wo = ((T - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1)
    out = torch.empty(N, To, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    part = torch.empty(N, To * -(-Ho // 16) * -(-Wo // 16), 4, Cout, dtype=torch.float32, device=x.device) if stats else None
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc3d_conv(_p(x), _p(wp), _p(bias), _p(s), _p(t), _p(res), res_scale, _p(out), _p(part), N, T, H, W,
                                           Cin, Cout, stride, _stream()), "disc3d_conv")
    return out, part


def stem_dgrad3(dy, wp, T, H, W, Cin):
    """oniris_disc3d_stem_dgrad: dy (N, T', H', W', Cout), wp = pack_weight3(conv_in.weight) -> dx (N, T, H, W, Cin)."""
    N, Cout = dy.shape[0], dy.shape[-1]
    dx = torch.empty(N, T, H, W, Cin, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_disc3d_stem_dgrad(_p(dy), _p(wp), _p(dx), N, T, H, W, Cin, Cout, _stream()), "disc3d_stem_dgrad")
    return dx


def wgrad3(x, dy, stride=1, pro=None):
    """oniris_disc3d_wgrad + the slab sum -> (d weight in nn.Conv3d's layout (Cout, Cin, 3, 3, 3), d bias (Cout,))."""
    N, T, H, W, Cin = x.shape
    _, To, Ho, Wo, Cout = dy.shape
    n = 27 * Cin * Cout + Cout
    nslab = _nslab3(N * To * -(-Ho // 16) * -(-Wo // 16), n)
    slab = torch.empty(nslab, n, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc3d_wgrad(_p(x), _p(s), _p(t), _p(dy), _p(slab), nslab, N, T, H, W, Cin, Cout, stride, _stream()),
               "disc3d_wgrad")
    r = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_vae_slab_sum_bwd(_p(slab), nslab, n, _p(r), _stream()), "vae_slab_sum_bwd")
    return r[:n - Cout].view(3, 3, 3, Cin, Cout).permute(4, 3, 0, 1, 2), r[n - Cout:]


def gn_finalize(part, gamma, beta, eps=1e-5):
    """oniris_disc3d_gn_finalize: partials (N, P, 4, C) -> stats (5, N, C): mean, biased var, s, t, rstd per (sample, channel)."""
    N, P, _, C = part.shape
    stats = torch.empty(5, N, C, dtype=torch.float32, device=part.device)
    _lib.check(_lib.lib.oniris_disc3d_gn_finalize(_p(part), N, P, C, _p(gamma), _p(beta), eps, _p(stats), _stream()),
               "disc3d_gn_finalize")
    return stats


def blur3(x, pro=None):
    N, T, H, W, C = x.shape
    out = torch.empty(N, _half(T), _half(H), _half(W), C, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc3d_blur(_p(x), _p(s), _p(t), _p(out), N, T, H, W, C, _stream()), "disc3d_blur")
    return out


def blur3_bwd(dy, T, H, W):
    N, C = dy.shape[0], dy.shape[-1]
    dx = torch.empty(N, T, H, W, C, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_disc3d_blur_bwd(_p(dy), _p(dx), N, T, H, W, C, _stream()), "disc3d_blur_bwd")
    return dx


def gn_bwd(da, z, stats, gamma, add=None, add_scale=1.0, want_dx=True):
    """GroupNorm + LeakyReLU backward at z (N, T, H, W, C): -> (dx or None, sums (2, C) = d beta | d gamma)."""
    N, C = z.shape[0], z.shape[-1]
    npix = z.numel() // (N * C)
    P = -(-npix // 1024)
    part = torch.empty(N, P, 2 * C, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib.oniris_disc3d_gn_bwd_reduce(_p(da), _p(z), _p(stats), _p(part), N, npix, C, _stream()), "disc3d_gn_bwd_reduce")
    nsum = torch.empty(N, 2 * C, dtype=torch.float32, device=z.device)
    mm = torch.empty(2, N, GROUPS, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib.oniris_disc3d_gn_bwd_finalize(_p(part), N, P, C, _p(gamma), npix, _p(nsum), _p(mm), _stream()),
               "disc3d_gn_bwd_finalize")
    sums = torch.empty(2, C, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib.oniris_disc_part_sum(_p(nsum), N, 2 * C, _p(sums), _stream()), "disc_part_sum")
    dx = None
    if want_dx:
        dx = torch.empty_like(z)
        _lib.check(_lib.lib.oniris_disc3d_gn_bwd_dx(_p(da), _p(z), _p(stats), _p(gamma), _p(mm), _p(add), add_scale, _p(dx), N, npix, C,
                                                    _stream()), "disc3d_gn_bwd_dx")
    return dx, sums


def _planes(x):
    """(N, T, H, W, C) -> the N T planes (N T, H, W, C) the 2-D entry points take (the 1x1x1 shortcut convs)."""
    return x.reshape(-1, *x.shape[2:])


def _gn_check(x):
    N, T, H, W, C = x.shape
    if N * (C // GROUPS) * T * H * W == 1:
        raise ValueError("Expected more than 1 value per channel when training (GroupNorm)")


class Stem3D(torch.autograd.Function):
    """conv_in: x (N, T, H, W, Cin) -> (the stride-2 conv + bias, the statistics partials of it)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        out, part = conv3(x, pack_weight3(weight), _f32(bias), weight.shape[0], stride=2, stats=True)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(part)
        return out, part

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = wgrad3(x, dout, stride=2)
        if ctx.needs_input_grad[0]:
            dx = stem_dgrad3(dout, pack_weight3(weight), *x.shape[1:])
        return dx, dw, db


class Head3D(torch.autograd.Function):
    """conv_out: x (N, T, H, W, C) -> the 27-tap conv + bias (N, T, H, W, 2), no normalisation in front (as in the reference)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        out, _ = conv3(x, pack_weight3(weight), _f32(bias), weight.shape[0])
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = wgrad3(x, dout)
        if ctx.needs_input_grad[0]:
            dx = conv3(dout, pack_weight3_dgrad(weight), None, weight.shape[1])[0]
        return dx, dw, db


class Block3D(torch.autograd.Function):
    """A DiscriminatorBlock3D: x (N, T, H, W, Cin) and the statistics partials of x -> ((conv2(..) + shortcut(x)) / sqrt 2, partials).
    The shortcut is blur + 1x1x1 conv in a downsampling block and a 1x1x1 conv in the final one."""

    @staticmethod
    def forward(ctx, x, part, g1, b1, w1, c1, g2, b2, w2, c2, ws, bs, down, stats_out, eps1, eps2):
        x = x.contiguous()
        N, T, H, W, Cin = x.shape
        Cout = w1.shape[0]
        _gn_check(x)
        st1 = gn_finalize(part, _f32(g1), _f32(b1), eps1)
        h1, part1 = conv3(x, pack_weight3(w1), _f32(c1), Cout, pro=(st1[2], st1[3]), stats=True)
        _gn_check(h1)
        st2 = gn_finalize(part1, _f32(g2), _f32(b2), eps2)
        wsp = pack_weight(ws.reshape(Cout, Cin, 1, 1))
        if down:
            b0 = blur3(x)
            sc = conv(_planes(b0), wsp, _f32(bs), Cout, 1)[0]
            pooled = blur3(h1, pro=(st2[2], st2[3]))
            out, part_o = conv3(pooled, pack_weight3(w2), _f32(c2), Cout, res=sc, res_scale=_SCALE, stats=stats_out)
            ctx.save_for_backward(x, h1, st1, st2, g1, g2, w1, w2, ws, pooled, b0)
        else:
            sc = conv(_planes(x), wsp, _f32(bs), Cout, 1)[0]
            out, part_o = conv3(h1, pack_weight3(w2), _f32(c2), Cout, pro=(st2[2], st2[3]), res=sc, res_scale=_SCALE,
                                stats=stats_out)
            ctx.save_for_backward(x, h1, st1, st2, g1, g2, w1, w2, ws)
        ctx.down = down
        ctx.mark_non_differentiable(*(() if part_o is None else (part_o,)))
        return out, part_o

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, h1, st1, st2, g1, g2, w1, w2, ws = ctx.saved_tensors[:9]
        need = ctx.needs_input_grad
        dout = dout.contiguous()
        N, T, H, W, Cin = x.shape
        Cout = w1.shape[0]
        dx = dg1 = db1 = dw1 = dc1 = dg2 = db2 = dw2 = dc2 = dws = dbs = None
        # conv2 and what it read
        if ctx.down:
            pooled, b0 = ctx.saved_tensors[9:]
            if need[8] or need[9]:
                dw2, dc2 = (g * _SCALE for g in wgrad3(pooled, dout))
            da2 = blur3_bwd(conv3(dout, pack_weight3_dgrad(w2, _SCALE), None, Cout)[0], T, H, W)
        else:
            if need[8] or need[9]:
                dw2, dc2 = (g * _SCALE for g in wgrad3(h1, dout, pro=(st2[2], st2[3])))
            da2 = conv3(dout, pack_weight3_dgrad(w2, _SCALE), None, Cout)[0]
        # norm2 + LeakyReLU
        dh1, sums2 = gn_bwd(da2, h1, st2, _f32(g2))
        if need[6]:
            dg2 = sums2[1].clone()
        if need[7]:
            db2 = sums2[0].clone()
        # conv1: its bias sits in front of a GroupNorm; where a group is one channel, the norm subtracts that channel's mean
        one = Cout == GROUPS
        if need[4] or (need[5] and not one):
            dw1, dc1 = wgrad3(x, dh1, pro=(st1[2], st1[3]))
        if need[5] and one:
            dc1 = torch.zeros(Cout, dtype=torch.float32, device=x.device)       # exactly zero, nothing computed
        # norm1 + LeakyReLU, plus the shortcut's share of dx
        if need[0] or need[2] or need[3]:
            da1 = conv3(dh1, pack_weight3_dgrad(w1), None, Cin)[0]
            add = None
            if need[0]:
                wsd = pack_weight_dgrad(ws.reshape(Cout, Cin, 1, 1), _SCALE)
                add = conv(_planes(dout), wsd, None, Cin, 1)[0].view(*dout.shape[:4], Cin)
                if ctx.down:
                    add = blur3_bwd(add, T, H, W)
            dx, sums1 = gn_bwd(da1, x, st1, _f32(g1), add, 1.0, want_dx=need[0])
            if need[2]:
                dg1 = sums1[1].clone()
            if need[3]:
                db1 = sums1[0].clone()
        if need[10] or need[11]:
            dws, dbs = wgrad(_planes(b0 if ctx.down else x), _planes(dout), 1)
            dws, dbs = (dws * _SCALE).reshape(ws.shape), dbs * _SCALE
        return dx, None, dg1, db1, dw1, dc1, dg2, db2, dw2, dc2, dws, dbs, None, None, None, None


class DiscriminatorBlock3D(nn.Module):
    def __init__(self, in_channels, out_channels, add_downsample=True):
        super().__init__()
        self.norm1 = nn.GroupNorm(32, in_channels)
        self.conv1 = nn.Conv3d(in_channels, out_channels, kernel_size=3, padding=1)
        self.downsampler = BlurPooling3D(out_channels) if add_downsample else nn.Identity()
        self.norm2 = nn.GroupNorm(32, out_channels)
        self.conv2 = nn.Conv3d(out_channels, out_channels, kernel_size=3, padding=1)
        if add_downsample:
            self.shortcut = nn.Sequential(BlurPooling3D(in_channels), nn.Conv3d(in_channels, out_channels, kernel_size=1))
        else:
            self.shortcut = nn.Sequential(nn.Conv3d(in_channels, out_channels, kernel_size=1))

    def forward(self, x):
        sc = self.shortcut(x)
        x = self.conv1(F.leaky_relu(self.norm1(x), 0.2))
        x = self.downsampler(F.leaky_relu(self.norm2(x), 0.2))
        return (self.conv2(x) + sc) / math.sqrt(2)


class Discriminator3D(nn.Module):
    """The reference's Discriminator3D (discriminator.py:242-283).  With model and input on the GPU it runs on HIP kernels, forward
    and backward (include/oniris.h: oniris_disc3d_*, csrc/disc3d.hip, csrc/disc_conv3d.h, csrc/disc_parts.h); with CPU tensors it is
    plain torch.nn code in the tensors' dtype.

    Native domain: in_channels 1..8; every width a multiple of 32 up to 256, any sequence of them (the final block's shortcut is a
    1x1x1 conv); any T, H, W >= 1; input (N, C, T, H, W), computed in fp32 -> logits (N, 2, T', H', W'), every extent halved
    len(widths) times by (n - 1) // 2 + 1 (conv_in has stride 2).  Anything else on the GPU raises NotImplementedError.  A
    GroupNorm over a single value raises the ValueError torch raises.  GroupNorm(32) and LeakyReLU never exist as tensors: a conv
    emits per-tile statistics of what it stores, a finalize launch turns them into per-(sample, channel) scale and shift, and the
    consumer applies lrelu(x s + t) while it stages its operand.  `conv_norm_out` exists and is unused, as in the reference: its
    gradients stay None.

    Gradients: of the input and of every used parameter; what nobody asked for (requires_grad, needs_input_grad) is not computed.
    Where `blocks.i.conv1` has 32 output channels, every group of the GroupNorm behind it is one channel and the norm subtracts
    that channel's mean: the bias gradient is exactly zero and zeros are returned without computing anything.  At wider groups it
    is not zero and is computed."""

    def __init__(self, in_channels=3, block_out_channels=(64,)):
        super().__init__()
        widths = [int(c) for c in block_out_channels]
        self.conv_in = nn.Conv3d(in_channels, widths[0], kernel_size=3, padding=1, stride=2)
        self.blocks = nn.ModuleList()
        cin = widths[0]
        for i, c in enumerate(widths):
            self.blocks.append(DiscriminatorBlock3D(cin, c, add_downsample=i < len(widths) - 1))
            cin = c
        self.conv_norm_out = nn.GroupNorm(32, widths[-1])
        self.conv_out = nn.Conv3d(widths[-1], 2, kernel_size=3, padding=1)
        self.widths = widths

    def _native_domain(self):
        cin = self.conv_in.in_channels
        if not 1 <= cin <= 8:
            raise NotImplementedError(f"Discriminator3D: in_channels {cin}: the HIP kernels take 1..8")
        if any(c % 32 or not 32 <= c <= MAX_WIDTH for c in self.widths):
            raise NotImplementedError(f"Discriminator3D: widths {self.widths}: the HIP kernels take multiples of 32 up to {MAX_WIDTH}")

    def forward_torch(self, x):
        """The reference's forward as plain torch.nn code, in the tensors' dtype, on any device."""
        x = self.conv_in(x)
        for blk in self.blocks:
            x = blk(x)
        return self.conv_out(x)

    def forward(self, x):
        if not x.is_cuda and not self.conv_in.weight.is_cuda:
            return self.forward_torch(x)
        if not (x.is_cuda and self.conv_in.weight.is_cuda):
            raise NotImplementedError("Discriminator3D: model and input must be on the same device (both on the GPU for the HIP "
                                      "kernels, both on the CPU for the torch code)")
        self._native_domain()
        if x.dim() != 5 or x.shape[1] != self.conv_in.in_channels:
            raise ValueError(f"Discriminator3D: input {tuple(x.shape)}, expected (N, {self.conv_in.in_channels}, T, H, W)")
        y = x.float().permute(0, 2, 3, 4, 1)
        y, part = Stem3D.apply(y, self.conv_in.weight, self.conv_in.bias)
        for i, blk in enumerate(self.blocks):
            down = i < len(self.blocks) - 1
            sc = blk.shortcut[1] if down else blk.shortcut[0]
            y, part = Block3D.apply(y, part, blk.norm1.weight, blk.norm1.bias, blk.conv1.weight, blk.conv1.bias, blk.norm2.weight,
                                    blk.norm2.bias, blk.conv2.weight, blk.conv2.bias, sc.weight, sc.bias, down, down, blk.norm1.eps,
                                    blk.norm2.eps)
        y = Head3D.apply(y, self.conv_out.weight, self.conv_out.bias)
        return y.permute(0, 4, 1, 2, 3)


class MixedDiscriminator(nn.Module):
    """The reference's MixedDiscriminator (discriminator.py:286-329): a per-frame critic and a spatio-temporal one over the same clip,
    their logits concatenated along time.  On the GPU both halves run on HIP kernels (`Discriminator2D`, `Discriminator3D`).  As in
    the reference, `block_out_channels` is accepted and the halves are built with widths (64, 64, 64) and (64, 64)."""

    def __init__(self, in_channels=6, block_out_channels=(64, 32)):
        super().__init__()
        self.discriminator2d = Discriminator2D(in_channels, (64, 64, 64))
        self.discriminator3d = Discriminator3D(in_channels, (64, 64))

    def forward(self, x):
        """x (B, C, T, H, W) -> logits (B, 2, T + T3, H', W'): the T per-frame maps, then the 3-D half's."""
        B, C, T, H, W = x.shape
        y3 = self.discriminator3d(x)
        y2 = self.discriminator2d(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W))
        y2 = y2.reshape(B, T, *y2.shape[1:]).permute(0, 2, 1, 3, 4)
        return torch.cat((y2, y3.to(y2.dtype)), dim=2)

    def cross_entropy(self, frames, recon_g, flip):
        """Class 1 = 'the real frames are in the second half of the channels'.  flip: the generator's view (gradients flow into
        recon_g, labels swapped); otherwise the critic's (inputs detached)."""
        real_first = torch.cat((frames, recon_g), dim=1)
        fake_first = torch.cat((recon_g, frames), dim=1)
        if flip:
            inputs = torch.cat((real_first, fake_first), dim=0)
        else:
            inputs = torch.cat((fake_first, real_first), dim=0).detach()
        logits = self(inputs)
        n = frames.shape[0]
        targets = torch.zeros(2 * n, *logits.shape[2:], dtype=torch.long, device=frames.device)
        targets[n:] = 1
        return F.cross_entropy(logits, targets) / np.log(2)

    def vae_loss(self, frames, recon_g):
        return self.cross_entropy(frames, recon_g, flip=True)

    def discriminator_loss(self, frames, recon_g):
        return self.cross_entropy(frames, recon_g, flip=False)

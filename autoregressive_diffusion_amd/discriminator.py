"""The VAE's adversarial critic (reference: edm2/vae/discriminator.py) -- `from autoregressive_diffusion_amd.discriminator import
MixedDiscriminator` instead of `from edm2.vae import MixedDiscriminator`.

`Discriminator2D`, the per-frame half and by far the larger one, runs on HIP kernels (include/oniris.h: oniris_disc_*, csrc/disc.hip,
csrc/disc_conv3.h, csrc/disc_parts.h): fp32 storage and fp32 arithmetic, every convolution an implicit GEMM on the exact-f32 matrix
instruction.  Activations travel channels-last [N][H][W][C].  BatchNorm and LeakyReLU never exist as tensors: a conv emits per-tile
(count, centre, S2, S1) of what it stores, a finalize launch turns them into the per-channel scale s and shift t, and the consumer
(the next conv, or the blur pool) applies lrelu(x s + t) while it stages its operand.  What stays in torch: the NCHW <->
channels-last copies at the two ends and permutations at parameter size.

`Discriminator3D`, the spatio-temporal half, runs on HIP kernels as well when model and input are on the GPU (oniris_disc3d_*,
csrc/disc3d.hip, csrc/disc_conv3d.h, the tile parts shared with the 2-D half in csrc/disc_parts.h): the same structure on
[N][T][H][W][C], a 27-tap conv being the sum over kt of 9-tap convs of neighbouring planes, GroupNorm(32) in place of BatchNorm with
scale and shift per (sample, channel), a stride-2 stem and a 3-D blur pool; with CPU tensors it stays plain torch.nn code.
`MixedDiscriminator` joins the two as the reference does.

Three layers.  The launches: thin wrappers, one per entry point, for either half.  The autograd code, written once for both halves:
two Functions, `Conv` (conv_in, conv_out) and `Block` (one per DiscriminatorBlock), which reach the launches through a kit --
`KIT2D`, `KIT3D`: a namespace of functions that names the packers, the conv and its gradients, the blur pool and the norm of one
dimensionality.  The modules: parameter holders with the reference's names, and one native driver for both `forward`s.

Gradients are summed in a fixed order into a bounded number of partial slabs and then over the slabs; nothing uses atomics, two runs
give the same bits."""
import math
from collections import namedtuple

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .vae import _p, _slab_sum, _stream

_REF = "the reference's edm2.vae (this package runs the 2-D discriminator on HIP kernels only)"
_SLAB_BYTES = 64 << 20          # the most memory one launch's partial slabs may take
_MAX_SLABS = 1024               # and the most slabs: tests lower it to make the work items wrap
MAX_WIDTH = 256
GROUPS = 32
_SCALE = 1.0 / math.sqrt(2.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: thin wrappers, one per entry point, on channels-last fp32 tensors of the GPU: (N, H, W, C) and, the names with a 3,
# (N, T, H, W, C)

def _nslab(work, size):
    """Partial slabs of `size` floats for `work` work items: one per item up to _MAX_SLABS, fewer when the slabs are large."""
    return int(max(1, min(work, _MAX_SLABS, max(64, _SLAB_BYTES // (4 * size)))))


def _nslab3(work, size):
    """Partial slabs for a 27-tap weight gradient: as _nslab, without its floor of 64 -- one launch stays within _SLAB_BYTES."""
    return int(max(1, min(work, _MAX_SLABS, _SLAB_BYTES // (4 * size))))


def _padc(c):
    return 8 if c <= 8 else c


def _half(n):
    return (n - 1) // 2 + 1


def _pack(w, dgrad, scale=1.0):
    """A conv weight (Cout, Cin, *k) of either rank -> [taps][CinP][CoutP] for the forward, or, for the data gradient, the conv
    Cout -> Cin on the flipped taps w'[taps - 1 - tap][co][ci] (times `scale`)."""
    taps, k = math.prod(w.shape[2:]), tuple(range(2, w.dim()))
    if dgrad:
        w = w.detach().float().flip(*k).permute(*k, 0, 1).reshape(taps, *w.shape[:2]) * scale
    else:
        w = w.detach().float().permute(*k, 1, 0).reshape(taps, w.shape[1], w.shape[0])
    out = torch.zeros(taps, _padc(w.shape[1]), -(-w.shape[2] // 32) * 32, dtype=torch.float32, device=w.device)
    out[:, :w.shape[1], :w.shape[2]] = w
    return out


def pack_weight(w):
    """nn.Conv2d weight (Cout, Cin, k, k) -> the forward layout [taps][CinP][CoutP] of oniris_disc_conv."""
    return _pack(w, False)


def pack_weight_dgrad(w, scale=1.0):
    """nn.Conv2d weight -> the layout of the data gradient: the conv Cout -> Cin on w'[8 - tap][co][ci] (times `scale`)."""
    return _pack(w, True, scale)


def pack_weight3(w):
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) -> the forward layout [27][CinP][CoutP] of oniris_disc3d_conv."""
    return _pack(w, False)


def pack_weight3_dgrad(w, scale=1.0):
    """nn.Conv3d weight -> the layout of the stride-1 data gradient: the conv Cout -> Cin on w'[26 - tap][co][ci] (times `scale`)."""
    return _pack(w, True, scale)


def conv(x, wp, bias, Cout, taps, pro=None, res=None, res_scale=1.0, stats=False):
    """oniris_disc_conv: x (N, H, W, Cin), wp packed -> (out (N, H, W, Cout), per-tile statistics or None)."""
    N, H, W, Cin = x.shape
    out = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x.device)
    part = torch.empty(N * -(-H // 16) * -(-W // 16), 4, Cout, dtype=torch.float32, device=x.device) if stats else None
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc_conv(_p(x), _p(wp), _p(bias), _p(s), _p(t), _p(res), res_scale, _p(out), _p(part), N, H, W, Cin,
                                         Cout, taps, _stream()), "disc_conv")
    return out, part


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


def _wgrad_slabs(launch, what, nslab, kernel, Cin, Cout, device):
    """The tail of both weight gradients: `nslab` partial slabs, launch(slab), the slab sum, and the split into (d weight in the
    nn.ConvNd layout (Cout, Cin, *kernel), d bias (Cout,))."""
    n = math.prod(kernel) * Cin * Cout + Cout
    slab = torch.empty(nslab, n, dtype=torch.float32, device=device)
    _lib.check(launch(slab), what)
    r, nd = _slab_sum(slab, n), len(kernel)
    return r[:n - Cout].view(*kernel, Cin, Cout).permute(nd + 1, nd, *range(nd)), r[n - Cout:]


def wgrad(x, dy, taps, pro=None):
    """oniris_disc_wgrad + the slab sum -> (d weight in nn.Conv2d's layout (Cout, Cin, k, k), d bias (Cout,))."""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    nslab = _nslab(N * -(-H // 16) * -(-W // 16), taps * Cin * Cout + Cout)
    s, t = (None, None) if pro is None else pro
    return _wgrad_slabs(lambda slab: _lib.lib.oniris_disc_wgrad(_p(x), _p(s), _p(t), _p(dy), _p(slab), nslab, N, H, W, Cin, Cout, taps,
                                                                _stream()),
                        "disc_wgrad", nslab, (3, 3) if taps == 9 else (1, 1), Cin, Cout, x.device)


def wgrad3(x, dy, stride=1, pro=None):
    """oniris_disc3d_wgrad + the slab sum -> (d weight in nn.Conv3d's layout (Cout, Cin, 3, 3, 3), d bias (Cout,))."""
    N, T, H, W, Cin = x.shape
    _, To, Ho, Wo, Cout = dy.shape
    nslab = _nslab3(N * To * -(-Ho // 16) * -(-Wo // 16), 27 * Cin * Cout + Cout)
    s, t = (None, None) if pro is None else pro
    return _wgrad_slabs(lambda slab: _lib.lib.oniris_disc3d_wgrad(_p(x), _p(s), _p(t), _p(dy), _p(slab), nslab, N, T, H, W, Cin, Cout,
                                                                  stride, _stream()),
                        "disc3d_wgrad", nslab, (3, 3, 3), Cin, Cout, x.device)


def finalize(part, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """oniris_disc_stats_finalize -> stats (5, C): mean, biased var, s, t, rstd; updates the running buffers in place."""
    P, _, C = part.shape
    stats = torch.empty(5, C, dtype=torch.float32, device=part.device)
    _lib.check(_lib.lib.oniris_disc_stats_finalize(_p(part), P, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum,
                                                   eps, _p(stats), _stream()), "disc_stats_finalize")
    return stats


def gn_finalize(part, gamma, beta, eps=1e-5):
    """oniris_disc3d_gn_finalize: partials (N, P, 4, C) -> stats (5, N, C): mean, biased var, s, t, rstd per (sample, channel)."""
    N, P, _, C = part.shape
    stats = torch.empty(5, N, C, dtype=torch.float32, device=part.device)
    _lib.check(_lib.lib.oniris_disc3d_gn_finalize(_p(part), N, P, C, _p(gamma), _p(beta), eps, _p(stats), _stream()),
               "disc3d_gn_finalize")
    return stats


def blur(x, pro=None):
    N, H, W, C = x.shape
    out = torch.empty(N, _half(H), _half(W), C, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc_blur(_p(x), _p(s), _p(t), _p(out), N, H, W, C, _stream()), "disc_blur")
    return out


def blur3(x, pro=None):
    N, T, H, W, C = x.shape
    out = torch.empty(N, _half(T), _half(H), _half(W), C, dtype=torch.float32, device=x.device)
    s, t = (None, None) if pro is None else pro
    _lib.check(_lib.lib.oniris_disc3d_blur(_p(x), _p(s), _p(t), _p(out), N, T, H, W, C, _stream()), "disc3d_blur")
    return out


def blur_bwd(dy, H, W):
    N, _, _, C = dy.shape
    dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_disc_blur_bwd(_p(dy), _p(dx), N, H, W, C, _stream()), "disc_blur_bwd")
    return dx


def blur3_bwd(dy, T, H, W):
    N, C = dy.shape[0], dy.shape[-1]
    dx = torch.empty(N, T, H, W, C, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_disc3d_blur_bwd(_p(dy), _p(dx), N, T, H, W, C, _stream()), "disc3d_blur_bwd")
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


def _f32(t):
    return t.detach().float().contiguous()


def _planes(x):
    """(N, T, H, W, C) -> the N T planes (N T, H, W, C) the 2-D entry points take (the 1x1x1 shortcut convs); (N, H, W, C) as it is."""
    return x.reshape(-1, *x.shape[-3:])


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


def _gn_check(x):
    N, T, H, W, C = x.shape
    if N * (C // GROUPS) * T * H * W == 1:
        raise ValueError("Expected more than 1 value per channel when training (GroupNorm)")


# ---------------------------------------------------------------------------------------------------------------------------------
# kits: what differs between the halves below the autograd code, one stateless namespace of functions per dimensionality (never
# instantiated).  Each function calls the launch wrapper above by its module-level name, at call time: tests and benchmarks wrap
# those.  emits(train): whether a conv in front of a norm emits statistics partials.  stats(norm, part, z, train): the statistics
# of norm(z) from the partials of z, st[2] and st[3] being scale and shift.  norm_bwd -> (dx or None, sums (2, C) = d beta |
# d gamma).  bias1_zero(train, Cout): whether the norm behind conv1 subtracts every channel's own mean, which makes conv1's bias
# gradient exactly zero.  stem_dgrad: the data gradient of the stride-2 conv_in, on the forward packing.

class KIT2D:
    """9-tap convs on (N, H, W, C); BatchNorm: batch statistics (and moving buffers) in training, the buffers in eval mode."""

    pack, pack_dgrad, stem_dgrad = pack_weight, pack_weight_dgrad, None

    def conv(x, wp, bias, Cout, stride=1, **kw):
        assert stride == 1
        return conv(x, wp, bias, Cout, 9, **kw)

    def wgrad(x, dy, stride=1, pro=None):
        assert stride == 1
        return wgrad(x, dy, 9, pro=pro)

    def blur(x, pro=None):
        return blur(x, pro=pro)

    def blur_bwd(dy, H, W):
        return blur_bwd(dy, H, W)

    def emits(train):
        return train

    def stats(norm, part, z, train):
        if train and z.numel() // z.shape[-1] < 2:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm2d)")
        return _norm_stats(norm, part, train)

    def norm_bwd(da, z, st, gamma, add=None, add_scale=1.0, train=True, want_dx=True):
        return bn_bwd(da, z, st, add, add_scale, eval_mode=not train, want_dx=want_dx)

    def bias1_zero(train, Cout):
        return train


class KIT3D:
    """27-tap convs on (N, T, H, W, C); GroupNorm(32): the same in both modes, its backward needs gamma."""

    pack, pack_dgrad = pack_weight3, pack_weight3_dgrad

    def conv(x, wp, bias, Cout, stride=1, **kw):
        return conv3(x, wp, bias, Cout, stride=stride, **kw)

    def wgrad(x, dy, stride=1, pro=None):
        return wgrad3(x, dy, stride=stride, pro=pro)

    def stem_dgrad(dy, wp, T, H, W, Cin):
        return stem_dgrad3(dy, wp, T, H, W, Cin)

    def blur(x, pro=None):
        return blur3(x, pro=pro)

    def blur_bwd(dy, T, H, W):
        return blur3_bwd(dy, T, H, W)

    def emits(train):
        return True

    def stats(norm, part, z, train):
        _gn_check(z)
        return gn_finalize(part, _f32(norm.weight), _f32(norm.bias), norm.eps)

    def norm_bwd(da, z, st, gamma, add=None, add_scale=1.0, train=True, want_dx=True):
        return gn_bwd(da, z, st, _f32(gamma), add, add_scale, want_dx=want_dx)

    def bias1_zero(train, Cout):
        return Cout == GROUPS


# ---------------------------------------------------------------------------------------------------------------------------------
# autograd: the arguments of each Function are named once (ARGS); needs_input_grad and the returned gradients go by those names

def _args(names):
    fields = names.split()
    return namedtuple("ARGS", fields, defaults=(None,) * len(fields))


class Conv(torch.autograd.Function):
    """conv_in / conv_out of either half: x channels-last -> (the conv at `stride` + bias, the statistics partials of it or None).
    The data gradient of a stride-2 conv is kit.stem_dgrad on the forward packing; every other one is a conv on pack_dgrad."""
    ARGS = _args("x weight bias kit stride stats")

    @staticmethod
    def forward(ctx, *args):
        a = Conv.ARGS(*args)
        x = a.x.contiguous()
        out, part = a.kit.conv(x, a.kit.pack(a.weight), _f32(a.bias), a.weight.shape[0], stride=a.stride, stats=a.stats)
        ctx.save_for_backward(x, a.weight)
        ctx.kit, ctx.stride = a.kit, a.stride
        ctx.mark_non_differentiable(*(() if part is None else (part,)))
        return out, part

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, weight = ctx.saved_tensors
        kit, need = ctx.kit, Conv.ARGS(*ctx.needs_input_grad)
        dout = dout.contiguous()
        dx = dw = db = None
        if need.weight or need.bias:
            dw, db = kit.wgrad(x, dout, stride=ctx.stride)
        if need.x and ctx.stride == 2:
            dx = kit.stem_dgrad(dout, kit.pack(weight), *x.shape[1:])
        elif need.x:
            dx = kit.conv(dout, kit.pack_dgrad(weight), None, weight.shape[1])[0]
        return tuple(Conv.ARGS(x=dx, weight=dw, bias=db))


class Block(torch.autograd.Function):
    """A DiscriminatorBlock of either half: x channels-last and the statistics partials of x -> ((conv2(..) + shortcut(x)) / sqrt 2,
    partials of that or None).  g, b: the norms' weight and bias; w, c: the convs'; ws, bs: the shortcut's 1x1 conv or None.  The
    shortcut, by (down, ws): blur + 1x1 conv in a downsampling block, the 1x1 conv alone (the final 3-D block), or the identity
    (the final 2-D block).  The 1x1 conv runs on the 2-D entry points over the planes in both halves."""
    ARGS = _args("x part g1 b1 w1 c1 g2 b2 w2 c2 ws bs kit blk down stats_out")

    @staticmethod
    def forward(ctx, *args):
        a = Block.ARGS(*args)
        kit, down, train = a.kit, a.down, a.blk.training
        x = a.x.contiguous()
        Cin, Cout = x.shape[-1], a.w1.shape[0]
        st1 = kit.stats(a.blk.norm1, a.part, x, train)
        h1, part1 = kit.conv(x, kit.pack(a.w1), _f32(a.c1), Cout, pro=(st1[2], st1[3]), stats=kit.emits(train))
        st2 = kit.stats(a.blk.norm2, part1, h1, train)
        b0 = kit.blur(x) if down else None
        sc = x
        if a.ws is not None:
            sc = conv(_planes(b0 if down else x), pack_weight(a.ws.reshape(Cout, Cin, 1, 1)), _f32(a.bs), Cout, 1)[0]
        pooled = kit.blur(h1, pro=(st2[2], st2[3])) if down else None
        out, part_o = kit.conv(pooled if down else h1, kit.pack(a.w2), _f32(a.c2), Cout, pro=None if down else (st2[2], st2[3]),
                               res=sc, res_scale=_SCALE, stats=a.stats_out)
        ctx.save_for_backward(x, h1, st1, st2, a.g1, a.g2, a.w1, a.w2, a.ws, pooled, b0)
        ctx.kit, ctx.down, ctx.train = kit, down, train
        ctx.mark_non_differentiable(*(() if part_o is None else (part_o,)))
        return out, part_o

    @staticmethod
    def backward(ctx, dout, _dpart):
        x, h1, st1, st2, g1, g2, w1, w2, ws, pooled, b0 = ctx.saved_tensors
        kit, down, train, need = ctx.kit, ctx.down, ctx.train, Block.ARGS(*ctx.needs_input_grad)
        dout = dout.contiguous()
        Cin, Cout, extents = x.shape[-1], w1.shape[0], x.shape[1:-1]
        g = {}
        # conv2 and what it read; its data gradient is packed with 1 / sqrt 2, its weight gradients are multiplied by it
        if need.w2 or need.c2:
            g["w2"], g["c2"] = (d * _SCALE for d in kit.wgrad(pooled if down else h1, dout, pro=None if down else (st2[2], st2[3])))
        da2 = kit.conv(dout, kit.pack_dgrad(w2, _SCALE), None, Cout)[0]
        if down:
            da2 = kit.blur_bwd(da2, *extents)
        # norm2 + LeakyReLU
        dh1, sums2 = kit.norm_bwd(da2, h1, st2, g2, train=train)
        if need.g2:
            g["g2"] = sums2[1].clone()
        if need.b2:
            g["b2"] = sums2[0].clone()
        # conv1: where the norm behind it subtracts each channel's own mean, its bias gradient is exactly zero, nothing computed
        zero = kit.bias1_zero(train, Cout)
        if need.w1 or (need.c1 and not zero):
            g["w1"], g["c1"] = kit.wgrad(x, dh1, pro=(st1[2], st1[3]))
        if need.c1 and zero:
            g["c1"] = torch.zeros(Cout, dtype=torch.float32, device=x.device)
        # norm1 + LeakyReLU, plus the shortcut's share of dx
        if need.x or need.g1 or need.b1:
            da1 = kit.conv(dh1, kit.pack_dgrad(w1), None, Cin)[0]
            add, add_scale = None, 1.0
            if need.x and ws is None:
                add, add_scale = dout, _SCALE
            elif need.x:
                wsd = pack_weight_dgrad(ws.reshape(Cout, Cin, 1, 1), _SCALE)
                add = conv(_planes(dout), wsd, None, Cin, 1)[0].view(*dout.shape[:-1], Cin)
                if down:
                    add = kit.blur_bwd(add, *extents)
            g["x"], sums1 = kit.norm_bwd(da1, x, st1, g1, add, add_scale, train=train, want_dx=need.x)
            if need.g1:
                g["g1"] = sums1[1].clone()
            if need.b1:
                g["b1"] = sums1[0].clone()
        if ws is not None and (need.ws or need.bs):
            dws, dbs = wgrad(_planes(b0 if down else x), _planes(dout), 1)
            g["ws"], g["bs"] = (dws * _SCALE).reshape(ws.shape), dbs * _SCALE
        return tuple(Block.ARGS(**g))


# ---------------------------------------------------------------------------------------------------------------------------------
# modules: parameter holders with the reference's names (load_state_dict(strict=True) takes a reference checkpoint)

def _blur_filter(channels, dims):
    f = torch.tensor([1.0, 2.0, 1.0])
    k = f
    for _ in range(dims - 1):
        k = k[..., None] * f
    k = k / k.sum()
    return k[None, None].repeat(channels, 1, *([1] * dims)).contiguous()


class _BlurPooling(nn.Module):
    def __init__(self, in_channels, out_channels=None):
        super().__init__()
        assert out_channels is None or out_channels == in_channels
        self.in_channels = self.out_channels = in_channels
        self.register_buffer("filt", _blur_filter(in_channels, self.dims))

    def forward(self, x):
        return getattr(F, f"conv{self.dims}d")(x, self.filt, stride=2, padding=1, groups=self.in_channels)


class BlurPooling2D(_BlurPooling):
    """The [1,2,1] x [1,2,1] / 16 filter at stride 2, padding 1, per channel (discriminator.py:154-178): the buffer `filt`."""
    dims = 2


class BlurPooling3D(_BlurPooling):
    dims = 3


class _DiscriminatorBlock(nn.Module):
    """The parameters and buffers of one block under the reference's names; on the GPU the computation is `Block`."""

    def __init__(self, in_channels, out_channels, add_downsample=True):
        super().__init__()
        norm, conv_nd, blur_nd = self.layers
        self.norm1 = norm(in_channels)
        self.conv1 = conv_nd(in_channels, out_channels, kernel_size=3, padding=1)
        self.downsampler = blur_nd(out_channels) if add_downsample else nn.Identity()
        self.norm2 = norm(out_channels)
        self.conv2 = conv_nd(out_channels, out_channels, kernel_size=3, padding=1)
        if add_downsample or self.final_shortcut_conv:
            self.shortcut = nn.Sequential(*([blur_nd(in_channels)] if add_downsample else []),
                                          conv_nd(in_channels, out_channels, kernel_size=1))
        else:
            self.shortcut = nn.Identity()
        self.add_downsample = add_downsample

    def shortcut_conv(self):
        """The shortcut's 1x1 conv, or None where the shortcut is the identity."""
        return self.shortcut[-1] if isinstance(self.shortcut, nn.Sequential) else None


class DiscriminatorBlock2D(_DiscriminatorBlock):
    """discriminator.py:11-67 (parameters and buffers only; the computation is `Block`)."""
    layers, final_shortcut_conv = (nn.BatchNorm2d, nn.Conv2d, BlurPooling2D), False


class DiscriminatorBlock3D(_DiscriminatorBlock):
    layers, final_shortcut_conv = (lambda c: nn.GroupNorm(GROUPS, c), nn.Conv3d, BlurPooling3D), True

    def forward(self, x):
        sc = self.shortcut(x)
        x = self.conv1(F.leaky_relu(self.norm1(x), 0.2))
        x = self.downsampler(F.leaky_relu(self.norm2(x), 0.2))
        return (self.conv2(x) + sc) / math.sqrt(2)


class _Discriminator(nn.Module):
    """What the two halves share: the layers under the reference's names and the native forward."""

    def _build(self, in_channels, widths, block, stride):
        norm, conv_nd, _ = block.layers
        self.conv_in = conv_nd(in_channels, widths[0], kernel_size=3, padding=1, stride=stride)
        self.blocks = nn.ModuleList()
        cin = widths[0]
        for i, c in enumerate(widths):
            self.blocks.append(block(cin, c, add_downsample=i < len(widths) - 1))
            cin = c
        self.conv_norm_out = norm(widths[-1])
        self.conv_out = conv_nd(widths[-1], 2, kernel_size=3, padding=1)

    def _native(self, x):
        """Channels-first x on the GPU -> logits: permute in; conv stage; Blocks; conv stage; permute out."""
        kit, emit = self.kit, self.kit.emits(self.training)
        y = x.float().permute(0, *range(2, x.dim()), 1)
        y, part = Conv.apply(*Conv.ARGS(y, self.conv_in.weight, self.conv_in.bias, kit, self.conv_in.stride[0], emit))
        for blk in self.blocks:
            sc = blk.shortcut_conv()
            y, part = Block.apply(*Block.ARGS(
                x=y, part=part, g1=blk.norm1.weight, b1=blk.norm1.bias, w1=blk.conv1.weight, c1=blk.conv1.bias, g2=blk.norm2.weight,
                b2=blk.norm2.bias, w2=blk.conv2.weight, c2=blk.conv2.bias, ws=None if sc is None else sc.weight,
                bs=None if sc is None else sc.bias, kit=kit, blk=blk, down=blk.add_downsample, stats_out=emit and blk.add_downsample))
        y, _ = Conv.apply(*Conv.ARGS(y, self.conv_out.weight, self.conv_out.bias, kit, 1, False))
        return y.permute(0, y.dim() - 1, *range(1, y.dim() - 1))


class Discriminator2D(_Discriminator):
    """The reference's Discriminator2D (discriminator.py:70-111) on HIP kernels, forward and backward.

    Domain: in_channels 1..8; every width a multiple of 32 up to 256; the last two widths equal (the final block's shortcut is the
    identity); any H, W >= 1; fp32 input (N, C, H, W) on the GPU -> logits (N, 2, H', W'), H' = H halved len(widths) - 1 times by
    (H - 1) // 2 + 1.  Anything else raises NotImplementedError.  Train mode normalises with batch statistics and moves the running
    buffers on every forward, eval mode uses the buffers, as nn.BatchNorm2d does.  `conv_norm_out` exists and is unused, as in the
    reference: its gradients stay None.

    Gradients: of the input and of every used parameter; what nobody asked for (requires_grad, needs_input_grad) is not computed --
    with the parameters frozen, a backward launches no weight-gradient kernel.  In train mode `blocks.i.conv1.bias` sits in front of
    a BatchNorm that subtracts the batch mean, so its gradient is exactly zero: zeros are returned without computing anything."""
    kit = KIT2D

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
        self._build(in_channels, widths, DiscriminatorBlock2D, 1)

    def forward(self, x):
        if not x.is_cuda or not self.conv_in.weight.is_cuda:
            raise NotImplementedError(f"Discriminator2D: runs on HIP kernels only (model and input on the GPU); on the CPU use {_REF}")
        if x.dim() != 4 or x.shape[1] != self.conv_in.in_channels:
            raise ValueError(f"Discriminator2D: input {tuple(x.shape)}, expected (N, {self.conv_in.in_channels}, H, W)")
        return self._native(x)


class Discriminator3D(_Discriminator):
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
    kit = KIT3D

    def __init__(self, in_channels=3, block_out_channels=(64,)):
        super().__init__()
        self.widths = [int(c) for c in block_out_channels]
        self._build(in_channels, self.widths, DiscriminatorBlock3D, 2)

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
        return self._native(x)


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

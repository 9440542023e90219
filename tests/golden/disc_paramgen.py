"""Seeded parameters for the discriminator fixtures G18 / G19: key names and shapes of the reference's state dicts
(edm2/vae/discriminator.py; make_golden_disc.py loads them strict=True into the reference, which pins both), with every value away
from its initialisation: BatchNorm / GroupNorm affine and all biases random, running statistics not at 0 / 1,
num_batches_tracked = 3.  The fixtures therefore store no state dicts."""
import numpy as np
import torch


def _filt(c, dims):
    f = torch.tensor([1.0, 2.0, 1.0])
    k = f
    for _ in range(dims - 1):
        k = k[..., None] * f
    return (k / k.sum())[None, None].repeat(c, 1, *([1] * dims))


def disc2d_shapes(in_channels, widths, prefix=""):
    """key -> shape (buffers included), in the reference's order."""
    s = {}

    def conv(name, co, ci, k):
        s[prefix + name + ".weight"] = (co, ci, k, k)
        s[prefix + name + ".bias"] = (co,)

    def bn(name, c):
        for k, shp in (("weight", (c,)), ("bias", (c,)), ("running_mean", (c,)), ("running_var", (c,)), ("num_batches_tracked", ())):
            s[prefix + name + "." + k] = shp

    conv("conv_in", widths[0], in_channels, 3)
    cin = widths[0]
    for i, c in enumerate(widths):
        b = f"blocks.{i}."
        down = i < len(widths) - 1
        bn(b + "norm1", cin)
        conv(b + "conv1", c, cin, 3)
        if down:
            s[prefix + b + "downsampler.filt"] = (c, 1, 3, 3)
        bn(b + "norm2", c)
        conv(b + "conv2", c, c, 3)
        if down:
            s[prefix + b + "shortcut.0.filt"] = (cin, 1, 3, 3)
            conv(b + "shortcut.1", c, cin, 1)
        cin = c
    bn("conv_norm_out", cin)
    conv("conv_out", 2, cin, 3)
    return s


def disc3d_shapes(in_channels, widths, prefix=""):
    s = {}

    def conv(name, co, ci, k):
        s[prefix + name + ".weight"] = (co, ci, k, k, k)
        s[prefix + name + ".bias"] = (co,)

    def gn(name, c):
        s[prefix + name + ".weight"] = (c,)
        s[prefix + name + ".bias"] = (c,)

    conv("conv_in", widths[0], in_channels, 3)
    cin = widths[0]
    for i, c in enumerate(widths):
        b = f"blocks.{i}."
        down = i < len(widths) - 1
        gn(b + "norm1", cin)
        conv(b + "conv1", c, cin, 3)
        if down:
            s[prefix + b + "downsampler.filt"] = (c, 1, 3, 3, 3)
        gn(b + "norm2", c)
        conv(b + "conv2", c, c, 3)
        if down:
            s[prefix + b + "shortcut.0.filt"] = (cin, 1, 3, 3, 3)
            conv(b + "shortcut.1", c, cin, 1)
        else:
            conv(b + "shortcut.0", c, cin, 1)
        cin = c
    gn("conv_norm_out", cin)
    conv("conv_out", 2, cin, 3)
    return s


def mixed_shapes(in_channels):
    s = disc2d_shapes(in_channels, (64, 64, 64), "discriminator2d.")
    s.update(disc3d_shapes(in_channels, (64, 64), "discriminator3d."))
    return s


def fill(shapes, seed):
    """Values for `shapes` from one seeded generator, in key order (float32; num_batches_tracked int64)."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, shp in shapes.items():
        leaf = k.rsplit(".", 1)[1]
        if leaf == "filt":
            p[k] = _filt(shp[0], len(shp) - 2)
        elif leaf == "num_batches_tracked":
            p[k] = torch.tensor(3, dtype=torch.int64)
        elif leaf == "running_mean":
            p[k] = 0.2 * torch.randn(shp, generator=g)
        elif leaf == "running_var":
            p[k] = 0.5 + torch.rand(shp, generator=g)
        elif leaf == "weight" and len(shp) == 1:
            p[k] = 1.0 + 0.3 * torch.randn(shp, generator=g)
        elif leaf == "bias":
            p[k] = 0.3 * torch.randn(shp, generator=g)
        else:
            p[k] = torch.randn(shp, generator=g) / float(np.sqrt(np.prod(shp[1:])))
    return p


G18_NETS = {"a": (3, (32,), (5, 3, 7, 5), 1801), "b": (6, (32, 32, 32), (3, 6, 24, 40), 1802), "c": (3, (32, 64, 64), (2, 3, 32, 64), 1803)}
G19_NETS = {"m3": (3, (2, 3, 4, 32, 32), 1901), "m6": (6, (2, 6, 4, 32, 32), 1902)}
G19_FULL = ("discriminator2d.conv_out.weight", "discriminator2d.conv_in.bias", "discriminator3d.conv_out.weight",
            "discriminator3d.conv_in.bias")


def inputs(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + 50))


def cot(shape, phi, dtype=torch.float64):
    """The cotangent cos(0.7 i + phi) over the flat index, as in G16."""
    n = int(np.prod(shape))
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64) + phi).reshape(shape).to(dtype)

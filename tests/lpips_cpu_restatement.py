"""LPIPS (net = 'alex', weights layout 0.1) restated in plain torch, runnable in float64 and float32 on the CPU, and the seeded
weights every LPIPS test uses.  Independent of autoregressive_diffusion_amd/lpips.py apart from the key table, which the CPU tests
compare with the one written here.

    x <- (x - shift) / scale;  f1 = relu(conv 11x11 stride 4 pad 2);  f2 = relu(conv 5x5 pad 2 (maxpool 3x3 s2 (f1)));
    f3 = relu(conv 3x3 pad 1 (maxpool 3x3 s2 (f2)));  f4 = relu(conv 3x3 pad 1 (f3));  f5 = relu(conv 3x3 pad 1 (f4));
    per layer n = f / (sqrt(sum_c f^2) + 1e-10), value = mean over pixels of sum_c w_c (n0 - n1)^2;  output = sum of the five values.

Where every channel of a pixel is zero the unit vector is 0 and the pixel takes no gradient (torch's own adjoint of the norm is 0 / 0
there); `distance` asserts that its float64 result is finite, so that case cannot hide."""
import math

import torch
from torch.nn import functional as F

TRUNK = (("net.slice1.0", 64, 3, 11), ("net.slice2.3", 192, 64, 5), ("net.slice3.6", 384, 192, 3), ("net.slice4.8", 256, 384, 3),
         ("net.slice5.10", 256, 256, 3))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def key_table():
    keys = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for name, co, ci, k in TRUNK:
        keys[name + ".weight"] = (co, ci, k, k)
        keys[name + ".bias"] = (co,)
    for i, t in enumerate(TRUNK):
        keys[f"lin{i}.model.1.weight"] = (1, t[1], 1, 1)
        keys[f"lins.{i}.model.1.weight"] = (1, t[1], 1, 1)
    return keys


def seeded_weights(seed=0, aliases=True):
    """Conv weights randn sqrt(2 / fan_in), biases 0.1 randn, head weights rand >= 0; fp32, the package's keys."""
    g = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    for name, co, ci, k in TRUNK:
        sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        sd[name + ".bias"] = 0.1 * torch.randn(co, generator=g)
    for i, t in enumerate(TRUNK):
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, t[1], 1, 1, generator=g)
        if aliases:
            sd[f"lins.{i}.model.1.weight"] = sd[f"lin{i}.model.1.weight"]
    return sd


def images(shape, seed):
    """Two operands (N, 3, H, W) in [-1, 1], fp32."""
    N, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(N, 3, H, W, generator=g) * 2 - 1, torch.rand(N, 3, H, W, generator=g) * 2 - 1


def cot(N, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return (0.5 + torch.rand(N, 1, 1, 1, generator=g))


def unit(f):
    """f / (|f| + eps) over the channels; 0 (and no gradient) where every channel is 0."""
    s = f.square().sum(1, keepdim=True)
    nz = s > 0
    return f * torch.where(nz, 1 / (torch.where(nz, s, torch.ones_like(s)).sqrt() + EPS), torch.zeros_like(s))


def head(fa, fb, w):
    """One layer's value (N, 1, 1, 1) from the two feature maps (N, C, h, w) and the head weight (1, C, 1, 1)."""
    return ((unit(fa) - unit(fb)).square() * w).sum(1, keepdim=True).mean((2, 3), keepdim=True)


def scaled(x, dtype):
    """(x - shift) / scale, shift and scale being the fp32 buffers the package stores (then widened), as for every other weight."""
    return (x - torch.tensor(SHIFT).to(dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE).to(dtype).view(1, 3, 1, 1)


def features(sd, x, dtype):
    p = lambda k: sd[k].to(dtype)
    f1 = F.relu(F.conv2d(scaled(x, dtype), p("net.slice1.0.weight"), p("net.slice1.0.bias"), stride=4, padding=2))
    f2 = F.relu(F.conv2d(F.max_pool2d(f1, 3, 2), p("net.slice2.3.weight"), p("net.slice2.3.bias"), padding=2))
    f3 = F.relu(F.conv2d(F.max_pool2d(f2, 3, 2), p("net.slice3.6.weight"), p("net.slice3.6.bias"), padding=1))
    f4 = F.relu(F.conv2d(f3, p("net.slice4.8.weight"), p("net.slice4.8.bias"), padding=1))
    f5 = F.relu(F.conv2d(f4, p("net.slice5.10.weight"), p("net.slice5.10.bias"), padding=1))
    return [f1, f2, f3, f4, f5]


def distance(sd, in0, in1, dtype, normalize=False):
    """(N, 1, 1, 1) in `dtype`; differentiable in in0 / in1."""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    fa, fb = features(sd, in0, dtype), features(sd, in1, dtype)
    out = sum(head(a, b, sd[f"lin{k}.model.1.weight"].to(dtype)) for k, (a, b) in enumerate(zip(fa, fb)))
    if dtype == torch.float64:
        assert bool(torch.isfinite(out).all())
    return out


def run(sd, in0, in1, dtype, c, normalize=False):
    """value, d in0, d in1 of (distance * c).sum() in `dtype`."""
    a, b = in0.detach().clone().to(dtype).requires_grad_(True), in1.detach().clone().to(dtype).requires_grad_(True)
    out = distance(sd, a, b, dtype, normalize)
    (out * c.to(dtype)).sum().backward()
    if dtype == torch.float64:
        assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())
    return dict(value=out.detach(), d_in0=a.grad, d_in1=b.grad)


def stem_terms(x, w, b):
    """The stem on fp32 operands in float64: the pre-activation and, per element, the sum of the absolute values of its terms."""
    xs = scaled(x.double(), torch.float64)
    v = F.conv2d(xs, w.double(), b.double(), stride=4, padding=2)
    m = F.conv2d(xs.abs(), w.double().abs(), b.double().abs(), stride=4, padding=2)
    return v, m


def stem_dgrad_terms(g, w, H, W):
    """The data gradient of the stem at g (N, 64, H1, W1) with respect to the unscaled image, and the sum of absolute terms."""
    sc = torch.tensor(SCALE).double().view(1, 3, 1, 1)
    op = ((H + 4 - 11) % 4, (W + 4 - 11) % 4)
    v = F.conv_transpose2d(g.double(), w.double(), stride=4, padding=2, output_padding=op) / sc
    m = F.conv_transpose2d(g.double().abs(), w.double().abs(), stride=4, padding=2, output_padding=op) / sc
    return v, m

"""The discriminator (reference: edm2/vae/discriminator.py) restated as functions of a parameter dict, in whatever dtype the
parameters have -- float64 is the oracle of tests/test_discriminator_gpu.py at shapes the fixtures G18 / G19 do not hold, and
tests/test_discriminator.py holds this file against the fixtures.  Also the per-stage expectations of the kernels of csrc/disc.hip
(activated operand, conv with its sum of absolute terms, statistics, blur pool and its transpose, BatchNorm backward), NCHW."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1


def lrelu(x):
    return torch.where(x > 0, x, 0.2 * x)


# ---- stages

def act(x, s, t):
    """The prologue: lrelu(x s[c] + t[c]), NCHW."""
    return lrelu(x * s[None, :, None, None] + t[None, :, None, None])


def conv_terms(a, w, bias=None, res=None, scale=1.0):
    """conv2d(a, w) + bias, then (. + res) scale; and per element the sum of the absolute values of its own terms."""
    pad = w.shape[-1] // 2
    v = F.conv2d(a, w, None, padding=pad)
    m = F.conv2d(a.abs(), w.abs(), None, padding=pad)
    if bias is not None:
        v = v + bias[None, :, None, None]
        m = m + bias.abs()[None, :, None, None]
    if res is not None:
        v = (v + res) * scale
        m = (m + res.abs()) * abs(scale)
    return v, m


def dgrad_terms(dy, w):
    """The data gradient of conv2d(., w) at dy, and the sum of absolute terms."""
    pad = w.shape[-1] // 2
    return F.conv_transpose2d(dy, w, padding=pad), F.conv_transpose2d(dy.abs(), w.abs(), padding=pad)


def wgrad(a, dy):
    """d weight (Cout, Cin, k, k) for k = 3 and d bias of conv2d(a, w) + bias at dy."""
    N, Cin, H, W = a.shape
    ap = F.pad(a, (1, 1, 1, 1))
    dw = torch.stack([torch.stack([torch.einsum("nchw,nohw->oc", ap[:, :, ky:ky + H, kx:kx + W], dy) for kx in range(3)], -1)
                      for ky in range(3)], -2)
    return dw, dy.sum((0, 2, 3))


def batch_stats(x):
    return x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)


def blur_filter(dtype):
    f = torch.tensor([1.0, 2.0, 1.0], dtype=dtype)
    return f[:, None] * f[None, :] / 16


def blur(a, terms=False):
    C = a.shape[1]
    k = blur_filter(a.dtype).to(a.device)[None, None].repeat(C, 1, 1, 1)
    y = F.conv2d(a, k, stride=2, padding=1, groups=C)
    return (y, F.conv2d(a.abs(), k, stride=2, padding=1, groups=C)) if terms else y


def blur_t(dy, H, W, terms=False):
    """The transpose of blur at an input of H x W."""
    C = dy.shape[1]
    k = blur_filter(dy.dtype).to(dy.device)[None, None].repeat(C, 1, 1, 1)
    Ho, Wo = dy.shape[2:]
    op = (H - 1 + 2 - 2 - 2 * (Ho - 1), W - 1 + 2 - 2 - 2 * (Wo - 1))
    f = lambda t: F.conv_transpose2d(t, k, stride=2, padding=1, output_padding=op, groups=C)
    return (f(dy), f(dy.abs())) if terms else f(dy)


def bn_backward(da, z, gamma, beta, mean, var):
    """BatchNorm (batch statistics) + LeakyReLU backward at z: dx, d gamma, d beta, and the sum of absolute terms of dx."""
    c = lambda v: v[None, :, None, None]
    rstd = 1 / torch.sqrt(var + EPS)
    s = gamma * rstd
    xh = (z - c(mean)) * c(rstd)
    dz = da * torch.where(xh * c(gamma) + c(beta) > 0, 1.0, 0.2)
    m1, m2 = dz.mean((0, 2, 3)), (dz * xh).mean((0, 2, 3))
    dx = c(s) * (dz - c(m1) - xh * c(m2))
    mag = c(s.abs()) * (dz.abs() + c(m1.abs()) + xh.abs() * c(m2.abs()))
    return dx, (dz * xh).sum((0, 2, 3)), dz.sum((0, 2, 3)), mag


# ---- the nets

def _bn(p, pre, x, train, new):
    if train:
        mean, var = batch_stats(x)
        n = x.numel() // x.shape[1]
        new[pre + "running_mean"] = (1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean.detach()
        new[pre + "running_var"] = (1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * var.detach() * n / (n - 1)
        new[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"], p[pre + "running_var"]
    c = lambda v: v[None, :, None, None]
    return (x - c(mean)) / torch.sqrt(c(var) + EPS) * c(p[pre + "weight"]) + c(p[pre + "bias"])


def disc2d(p, x, n_blocks, train=True, prefix=""):
    """-> (logits, {buffer key: value after this forward})."""
    new = {}
    cv = lambda name, t, pad: F.conv2d(t, p[prefix + name + ".weight"], p[prefix + name + ".bias"], padding=pad)
    x = cv("conv_in", x, 1)
    for i in range(n_blocks):
        b = f"{prefix}blocks.{i}."
        down = i < n_blocks - 1
        sc = cv(f"blocks.{i}.shortcut.1", blur(x), 0) if down else x
        h = cv(f"blocks.{i}.conv1", lrelu(_bn(p, b + "norm1.", x, train, new)), 1)
        h = lrelu(_bn(p, b + "norm2.", h, train, new))
        if down:
            h = blur(h)
        x = (cv(f"blocks.{i}.conv2", h, 1) + sc) / math.sqrt(2)
    return cv("conv_out", x, 1), new


def _blur3(x):
    C = x.shape[1]
    f = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype, device=x.device)
    k = (f[:, None, None] * f[None, :, None] * f[None, None, :] / 64)[None, None].repeat(C, 1, 1, 1, 1)
    return F.conv3d(x, k, stride=2, padding=1, groups=C)


def disc3d(p, x, n_blocks, prefix=""):
    cv = lambda name, t, pad, stride=1: F.conv3d(t, p[prefix + name + ".weight"], p[prefix + name + ".bias"], padding=pad, stride=stride)
    gn = lambda name, t: F.group_norm(t, 32, p[prefix + name + ".weight"], p[prefix + name + ".bias"], EPS)
    x = cv("conv_in", x, 1, 2)
    for i in range(n_blocks):
        b = f"blocks.{i}."
        down = i < n_blocks - 1
        sc = cv(b + "shortcut.1", _blur3(x), 0) if down else cv(b + "shortcut.0", x, 0)
        h = cv(b + "conv1", lrelu(gn(b + "norm1", x)), 1)
        h = lrelu(gn(b + "norm2", h))
        if down:
            h = _blur3(h)
        x = (cv(b + "conv2", h, 1) + sc) / math.sqrt(2)
    return cv("conv_out", x, 1)


def mixed(p, x, train=True):
    """MixedDiscriminator.forward: x (B, C, T, H, W) -> (logits (B, 2, T + T3, h, w), new buffers)."""
    B, C, T, H, W = x.shape
    y3 = disc3d(p, x, 2, "discriminator3d.")
    y2, new = disc2d(p, x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), 3, train, "discriminator2d.")
    y2 = y2.reshape(B, T, *y2.shape[1:]).permute(0, 2, 1, 3, 4)
    return torch.cat((y2, y3), dim=2), new


def mixed_loss(p, frames, recon, flip):
    """vae_loss (flip) / discriminator_loss: cross entropy in bits against 'which half of the channels holds the real frames'."""
    a, b = torch.cat((frames, recon), 1), torch.cat((recon, frames), 1)
    inp = torch.cat((a, b), 0) if flip else torch.cat((b, a), 0).detach()
    logits, _ = mixed(p, inp)
    n = frames.shape[0]
    tgt = torch.zeros(2 * n, *logits.shape[2:], dtype=torch.long, device=logits.device)
    tgt[n:] = 1
    return F.cross_entropy(logits, tgt) / np.log(2)


def run2d(params, x, n_blocks, dtype, phi=0.3):
    """Everything G18 records for one net: params (any dtype) are cast to `dtype`; -> dict of detached tensors."""
    from disc_paramgen import cot
    p = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in params.items()}
    for k, v in p.items():
        if v.is_floating_point() and k.rsplit(".", 1)[1] in ("weight", "bias"):
            v.requires_grad_(True)
    xi = x.to(dtype).requires_grad_(True)
    logits, new = disc2d(p, xi, n_blocks, True)
    (logits * cot(logits.shape, phi, dtype)).sum().backward()
    p2 = dict(p)
    p2.update(new)
    with torch.no_grad():
        _, new2 = disc2d(p2, xi, n_blocks, True)
        p3 = dict(p)
        ev, _ = disc2d(p3, xi, n_blocks, False)
    out = {"logits": logits.detach(), "dx": xi.grad, "eval_logits": ev}
    for k, v in p.items():
        if v.requires_grad and v.grad is not None:
            out["grad/" + k] = v.grad
    for k, v in new2.items():
        out["buf2/" + k] = v
    for k, v in p.items():                       # conv_norm_out is never called: its buffers stay
        if ("running" in k or "num_batches" in k) and "buf2/" + k not in out:
            out["buf2/" + k] = v.detach()
    return out


# ---- fixtures

def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


_npz = {}


def fixture(fn, net):
    """The entries `<net>/...` of tests/golden/<fn> as {name: tensor} (strings stay numpy arrays)."""
    import os
    if fn not in _npz:
        _npz[fn] = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fn), allow_pickle=False)
    z = _npz[fn]
    out = {}
    for k in z.files:
        if k.startswith(net + "/"):
            v = z[k]
            out[k[len(net) + 1:]] = v if v.dtype.kind in "US" else torch.from_numpy(np.asarray(v))
    return out


def margin(ref32_rel):
    """The margin rule for relative comparisons without an element bound: max(5e-5, 4 x the reference's own float32 error)."""
    return max(5e-5, 4.0 * float(ref32_rel))

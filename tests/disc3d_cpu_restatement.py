"""Per-stage float64 expectations of the 3-D discriminator kernels (csrc/disc3d.hip, csrc/disc_conv3d.h), NCTHW, and `run3d`, which
computes everything fixture G20 records from disc_cpu_restatement.disc3d.  tests/test_discriminator3d.py holds every function
here against torch autograd in float64 and `run3d` against G20; tests/test_discriminator3d_gpu.py uses them as the oracle."""
import torch
import torch.nn.functional as F

import disc_cpu_restatement as R

EPS = 1e-5
GROUPS = 32


def _c(v):
    """(N, C) or (C,) -> broadcastable against (N, C, T, H, W)."""
    return v[:, :, None, None, None] if v.dim() == 2 else v[None, :, None, None, None]


def act(x, s, t):
    """The prologue lrelu(x s + t) with s, t per (sample, channel) (N, C) or per channel (C,)."""
    return R.lrelu(x * _c(s) + _c(t))


def conv_terms(a, w, bias=None, res=None, scale=1.0, stride=1):
    """conv3d(a, w, padding 1 (0 for a 1x1x1 kernel), stride) + bias, then (. + res) scale; and the sum of absolute terms."""
    pad = w.shape[-1] // 2
    v = F.conv3d(a, w, None, stride=stride, padding=pad)
    m = F.conv3d(a.abs(), w.abs(), None, stride=stride, padding=pad)
    if bias is not None:
        v = v + _c(bias)
        m = m + _c(bias.abs())
    if res is not None:
        v = (v + res) * scale
        m = (m + res.abs()) * abs(scale)
    return v, m


def _out_pad(n, stride):
    return n - 1 - stride * ((n - 1) // stride)


def dgrad_terms(dy, w, shape, stride=1):
    """The data gradient of conv3d(., w, stride) at dy for an input of spatial `shape` (T, H, W); the sum of absolute terms; and per
    element the number of (output position, tap) pairs that contribute."""
    pad = w.shape[-1] // 2
    op = tuple(_out_pad(n, stride) for n in shape) if pad else (0, 0, 0)
    f = lambda d, k: F.conv_transpose3d(d, k, stride=stride, padding=pad, output_padding=op)
    pairs = f(torch.ones_like(dy[:1, :1]), torch.ones_like(w[:1, :1]))
    return f(dy, w), f(dy.abs(), w.abs()), pairs


def wgrad(a, dy, stride=1):
    """d weight (Cout, Cin, 3, 3, 3) and d bias of conv3d(a, w, padding 1, stride) + bias at dy."""
    To, Ho, Wo = dy.shape[2:]
    ap = F.pad(a, (1, 1, 1, 1, 1, 1))
    sl = lambda k, n: slice(k, k + stride * (n - 1) + 1, stride)
    dw = torch.stack([torch.stack([torch.stack([torch.einsum("ncthw,nothw->oc", ap[:, :, sl(kt, To), sl(ky, Ho), sl(kx, Wo)], dy)
                                                for kx in range(3)], -1) for ky in range(3)], -2) for kt in range(3)], -3)
    return dw, dy.sum((0, 2, 3, 4))


def group_stats(x):
    """Per (sample, group) mean and biased variance over C / 32 channels x T x H x W: two (N, 32) tensors."""
    N = x.shape[0]
    xg = x.reshape(N, GROUPS, -1)
    return xg.mean(2), xg.var(2, unbiased=False)


def per_channel(v, C):
    """(N, 32) per group -> (N, C) per channel."""
    return v.repeat_interleave(C // GROUPS, dim=1)


def gn_vectors(x, gamma, beta):
    """-> mean, var, s, t, rstd, each (N, C): what oniris_disc3d_gn_finalize writes."""
    C = x.shape[1]
    mean, var = (per_channel(v, C) for v in group_stats(x))
    rstd = 1 / torch.sqrt(var + EPS)
    s = gamma[None] * rstd
    return mean, var, s, beta[None] - mean * s, rstd


def gn_backward(da, z, gamma, beta, mean, rstd):
    """GroupNorm(32) + LeakyReLU backward at z with the statistics given per (sample, channel) (N, C): dx, d gamma, d beta, and per
    element the sum of the magnitudes of dx's terms, the two group means taken as means of magnitudes (what their own rounding
    errors are proportional to)."""
    N, C = z.shape[:2]
    xh = (z - _c(mean)) * _c(rstd)
    dz = torch.where(xh * _c(gamma) + _c(beta) > 0, da, 0.2 * da)
    gdz = dz * _c(gamma)
    gmean = lambda v: per_channel(v.reshape(N, GROUPS, -1).mean(2), C)
    m1, m2 = gmean(gdz), gmean(gdz * xh)
    dx = _c(rstd) * (gdz - _c(m1) - xh * _c(m2))
    mag = _c(rstd) * (gdz.abs() + _c(gmean(gdz.abs())) + xh.abs() * _c(gmean((gdz * xh).abs())))
    return dx, (dz * xh).sum((0, 2, 3, 4)), dz.sum((0, 2, 3, 4)), mag


def _blur_kernel(C, like):
    f = torch.tensor([1.0, 2.0, 1.0], dtype=like.dtype, device=like.device)
    return (f[:, None, None] * f[None, :, None] * f[None, None, :] / 64)[None, None].repeat(C, 1, 1, 1, 1)


def blur(a, terms=False):
    C = a.shape[1]
    k = _blur_kernel(C, a)
    y = F.conv3d(a, k, stride=2, padding=1, groups=C)
    return (y, F.conv3d(a.abs(), k, stride=2, padding=1, groups=C)) if terms else y


def blur_t(dy, shape, terms=False):
    """The transpose of blur at an input of spatial `shape` (T, H, W)."""
    C = dy.shape[1]
    k = _blur_kernel(C, dy)
    op = tuple(_out_pad(n, 2) for n in shape)
    f = lambda t: F.conv_transpose3d(t, k, stride=2, padding=1, output_padding=op, groups=C)
    return (f(dy), f(dy.abs())) if terms else f(dy)


def full_grads(params, x, n_blocks, dtype):
    """R.disc3d at params (any dtype, cast to `dtype`) and its backward at the cotangent cot(., 0.3): logits, dx and every parameter
    gradient in full ({'grad/<key>': tensor})."""
    from disc_paramgen import cot
    import disc3d_paramgen as G3
    p = {k: v.to(dtype).requires_grad_(k.rsplit(".", 1)[1] in ("weight", "bias")) for k, v in params.items()}
    xi = x.to(dtype).requires_grad_(True)
    logits = R.disc3d(p, xi, n_blocks)
    (logits * cot(logits.shape, G3.PHI, dtype)).sum().backward()
    out = {"logits": logits.detach(), "dx": xi.grad}
    out.update({"grad/" + k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None})
    return out


def run3d(params, x, n_blocks, dtype):
    """Everything G20 records for one net, from R.disc3d: full_grads with the gradients through disc3d_paramgen.grad_entries."""
    import disc3d_paramgen as G3
    out = {}
    for k, v in full_grads(params, x, n_blocks, dtype).items():
        out.update(G3.grad_entries(k[len("grad/"):], v) if k.startswith("grad/") else {k: v})
    return out

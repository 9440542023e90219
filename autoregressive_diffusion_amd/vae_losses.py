"""The VAE's training objective on HIP kernels (reference: edm2/utils.py GaussianLoss, F.l1_loss / F.mse_loss as the VAE scripts call
them, edm2/vae/utils.py worst_k_percent_loss) -- `from autoregressive_diffusion_amd.vae_losses import GaussianLoss, l1_loss,
mse_loss, recon_losses, worst_k_percent_loss` with the reference's call shapes; each returns a 0-d fp32 tensor on the autograd graph.

Native domain: fp32 tensors of one shape on the GPU, up to 5 dimensions, at least one element.  Anything else takes the torch formula
of the reference.  Operands are addressed by their element strides (a permuted channels-last view of the frames is read in place, never
copied); when every operand is contiguous and 16-byte aligned the kernels read and write 16 bytes per lane.

  recon_losses(mean, logvar, target) -> (gaussian, l1, mse): ONE launch over the three operands + the sum of its per-workgroup
      partials, ONE backward launch that reads the three upstream cotangents on the device.  GaussianLoss, l1_loss and mse_loss
      are the same kernels with the other sums switched off, and give the same bits as recon_losses does.
  worst_k_percent_loss(recon, frames, percent): a radix select over the bit patterns of the squared errors (csrc/vae_loss.hip):
      no sort, no index tensor; the backward reads 12 saved bytes (threshold key, count above, count equal).  Elements tied with the
      threshold share its remaining weight equally, (k - count_gt) / count_eq each: a valid subgradient, the same on every run, and
      torch's own gradient whenever the threshold value is unique.

Nothing synchronises with the host; every float sum has a fixed order (no float atomics): two runs give the same bits."""
import ctypes

import torch
from torch.nn import functional as F

from . import _lib
from .vae import _p, _stream

_MAX_BLOCKS = 2048              # workgroups of a pass (256 CUs x 8); tests lower it to make every grid-stride loop wrap
_MERGE_CAP = 1 << 30            # merged loop dimensions stay below the kernels' limit for one strided dimension
_GAUSS, _L1, _MSE = 1, 2, 4


def _native(*ts):
    t0 = ts[0]
    return (t0.is_cuda and 1 <= t0.dim() <= 5 and t0.numel() > 0
            and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.shape == t0.shape and t.device == t0.device
                    for t in ts))


def _layout(tensors):
    """Loop order and strides for one launch over `tensors` (None entries keep a row of zeros): -> (nd, size array, stride array or
    None when everything is flat).  The loop runs in the memory order of the first operand that is not contiguous, so that operand
    is read front to back; neighbouring dimensions that every operand can step through with one stride are merged."""
    real = [t for t in tensors if t is not None]
    shape = real[0].shape
    if all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in real):
        return 1, (ctypes.c_longlong * 1)(real[0].numel()), None
    lead = next((t for t in real if not t.is_contiguous()), real[0])
    dims = sorted((d for d in range(len(shape)) if shape[d] != 1), key=lambda d: -abs(lead.stride(d))) or [0]
    sizes, strides = [], [[] for _ in real]
    for d in dims:
        if sizes and sizes[-1] * shape[d] <= _MERGE_CAP and all(st[-1] == t.stride(d) * shape[d] for st, t in zip(strides, real)):
            sizes[-1] *= shape[d]
            for st, t in zip(strides, real):
                st[-1] = t.stride(d)
        else:
            sizes.append(shape[d])
            for st, t in zip(strides, real):
                st.append(t.stride(d))
    nd = len(sizes)
    rows, it = [], iter(strides)
    for t in tensors:
        rows += [0] * nd if t is None else next(it)
    return nd, (ctypes.c_longlong * nd)(*sizes), (ctypes.c_longlong * len(rows))(*rows)


class _Pointwise(torch.autograd.Function):
    """(mean, logvar or None, target, which) -> the three means; the ones `which` leaves out are zeros."""

    @staticmethod
    def forward(ctx, mean, logvar, target, which):
        nd, size, stride = _layout([mean, logvar, target])
        part = torch.empty(min(_MAX_BLOCKS, -(-mean.numel() // 1024)), 3, dtype=torch.float32, device=mean.device)
        blocks = ctypes.c_int(0)
        _lib.check(_lib.lib.oniris_vae_loss_fwd(_p(mean), _p(logvar), _p(target), which, nd, size, stride, _p(part), part.shape[0],
                                                ctypes.byref(blocks), _stream()), "vae_loss_fwd")
        assert blocks.value == part.shape[0]
        out = torch.empty(3, dtype=torch.float32, device=mean.device)
        _lib.check(_lib.lib.oniris_disc_part_sum(_p(part), part.shape[0], 3, _p(out), _stream()), "disc_part_sum")
        ctx.save_for_backward(mean, logvar, target)
        ctx.which = which
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, cg, cl, cm):
        mean, logvar, target = ctx.saved_tensors
        need_m, need_lv, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and logvar is not None, ctx.needs_input_grad[2]
        cots = [None if c is None else c.to(torch.float32) for c in (cg, cl, cm)]
        which = ctx.which & sum(1 << i for i, c in enumerate(cots) if c is not None)
        need_lv = need_lv and bool(which & _GAUSS)            # without the Gaussian loss logvar gets no gradient, not a zero tensor
        if which == 0 or not (need_m or need_lv or need_t):
            return None, None, None, None
        dm = torch.empty_like(mean) if need_m else None
        dlv = torch.empty_like(logvar) if need_lv else None
        dt = torch.empty_like(target) if need_t else None
        nd, size, stride = _layout([mean, logvar if which & _GAUSS else None, target, dm, dlv, dt])
        _lib.check(_lib.lib.oniris_vae_loss_bwd(_p(mean), _p(logvar) if which & _GAUSS else None, _p(target), which, nd, size, stride,
                                                _p(cots[0]), _p(cots[1]), _p(cots[2]), _p(dm), _p(dlv), _p(dt), _MAX_BLOCKS,
                                                _stream()), "vae_loss_bwd")
        return dm, dlv, dt, None


def worst_k_select(recon, target, k):
    """The forward launches of the worst-k loss without autograd: -> (loss, state), state = int32 [3] on the device holding the bit
    patterns of (threshold key, count_gt, count_eq)."""
    n, dev = recon.numel(), recon.device
    if not 1 <= k <= n:
        raise RuntimeError(f"worst_k_percent_loss: k = {k} out of range for {n} elements")
    nd, size, stride = _layout([recon, target])
    ws = torch.zeros(2048 + 1024 + 1024 + 4, dtype=torch.int32, device=dev)
    hist, state = ws, ws[4096:]
    e = torch.empty(n, dtype=torch.float32, device=dev)
    part = torch.empty(min(_MAX_BLOCKS, -(-n // 1024)), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    s, lib, blocks = _stream(), _lib.lib, ctypes.c_int(0)
    _lib.check(lib.oniris_vae_loss_topk_keys(_p(recon), _p(target), nd, size, stride, _p(e), _p(hist), _MAX_BLOCKS, s), "vae_loss_topk_keys")
    _lib.check(lib.oniris_vae_loss_topk_select(_p(hist), 0, k, _p(state), None, 0, None, s), "vae_loss_topk_select")
    _lib.check(lib.oniris_vae_loss_topk_count(_p(e), n, 0, _p(state), _p(hist[2048:]), None, _MAX_BLOCKS, ctypes.byref(blocks), s),
               "vae_loss_topk_count")
    _lib.check(lib.oniris_vae_loss_topk_select(_p(hist[2048:]), 1, k, _p(state), None, 0, None, s), "vae_loss_topk_select")
    _lib.check(lib.oniris_vae_loss_topk_count(_p(e), n, 1, _p(state), _p(hist[3072:]), _p(part), _MAX_BLOCKS, ctypes.byref(blocks), s),
               "vae_loss_topk_count")
    assert blocks.value == part.shape[0]
    _lib.check(lib.oniris_vae_loss_topk_select(_p(hist[3072:]), 2, k, _p(state), _p(part), part.shape[0], _p(loss), s),
               "vae_loss_topk_select")
    return loss, state[:3].clone()                            # 12 bytes outlive the work space


class _WorstK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recon, target, k):
        loss, state = worst_k_select(recon, target, k)
        ctx.save_for_backward(recon, target, state)
        ctx.k = k
        return loss

    @staticmethod
    def backward(ctx, g):
        recon, target, state = ctx.saved_tensors
        need_r, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_r or need_t):
            return None, None, None
        dr = torch.empty_like(recon) if need_r else None
        dt = torch.empty_like(target) if need_t else None
        nd, size, stride = _layout([recon, target, dr, dt])
        _lib.check(_lib.lib.oniris_vae_loss_topk_bwd(_p(recon), _p(target), nd, size, stride, _p(state), _p(g.to(torch.float32)), ctx.k,
                                                     _p(dr), _p(dt), _MAX_BLOCKS, _stream()), "vae_loss_topk_bwd")
        return dr, dt, None


def recon_losses(mean, logvar, target):
    """(GaussianLoss(mean, logvar, target), F.l1_loss(mean, target), F.mse_loss(mean, target)) from one pass forward and one backward."""
    if _native(mean, logvar, target):
        return _Pointwise.apply(mean, logvar, target, _GAUSS | _L1 | _MSE)
    return GaussianLoss(mean, logvar, target), F.l1_loss(mean, target), F.mse_loss(mean, target)


def GaussianLoss(mean, logvar, target, eps=1e-4):
    """((logvar + (mean - target)^2 exp(-logvar)) / 2 + 0.918).mean() (edm2/utils.py:209-210; eps is unused there as well)."""
    if _native(mean, logvar, target):
        return _Pointwise.apply(mean, logvar, target, _GAUSS)[0]
    return ((logvar + (mean - target) ** 2 * (torch.exp(-logvar))) * .5 + 0.918).mean()


def l1_loss(input, target):
    """F.l1_loss(input, target), 'mean' reduction."""
    if _native(input, target):
        return _Pointwise.apply(input, None, target, _L1)[1]
    return F.l1_loss(input, target)


def mse_loss(input, target):
    """F.mse_loss(input, target), 'mean' reduction."""
    if _native(input, target):
        return _Pointwise.apply(input, None, target, _MSE)[2]
    return F.mse_loss(input, target)


def worst_k(numel, percent):
    return max(1, int(numel * (percent / 100.0)))


def worst_k_percent_loss(recon, frames, percent=0.5):
    """The mean of the k = max(1, int(numel * (percent / 100.0))) largest squared errors (edm2/vae/utils.py:54-68)."""
    k = worst_k(recon.numel(), percent)
    if _native(recon, frames) and recon.numel() < 2 ** 32:
        return _WorstK.apply(recon, frames, k)
    return torch.topk(F.mse_loss(recon, frames, reduction='none').flatten(), k)[0].mean()

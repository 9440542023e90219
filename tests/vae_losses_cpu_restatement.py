"""The specification of the VAE losses (autoregressive_diffusion_amd/vae_losses.py, csrc/vae_loss.hip) restated on the CPU.

Fused pointwise losses: the reference's formulas in torch, in whatever dtype the operands have (float64 gives the yardstick).

Worst-k% selection, in numpy, from float32 operands:
  d = recon - target and e = d * d, each rounded once in float32 (bit for bit what F.mse_loss(reduction='none') gives);
  key = the bit pattern of e with the sign bit cleared (monotone in e for e >= 0; NaN sorts above +inf);
  threshold = the k-th largest key, count_gt = keys above it, count_eq = keys equal to it (count_gt < k <= count_gt + count_eq);
  loss = (sum of e over key > threshold + (k - count_gt) e_k) / k;
  weight = 1 above the threshold, (k - count_gt) / count_eq at it, 0 below;  d loss / d recon = g 2 d weight / k = -d loss / d target.
Tests hold it to fixture G21 (tests/test_vae_losses.py) and the kernels to it (tests/test_vae_losses_gpu.py)."""
import math

import numpy as np
import torch


def gaussian(mean, logvar, target):
    return ((logvar + (mean - target) ** 2 * torch.exp(-logvar)) * .5 + 0.918).mean()


def l1(mean, target):
    return (mean - target).abs().mean()


def mse(mean, target):
    return ((mean - target) ** 2).mean()


def fused(mean, logvar, target, cots, dtype=torch.float64):
    """-> (losses (gaussian, l1, mse) as floats, mean |term| of each, gradients (d mean, d logvar, d target) of sum_i cots[i] loss_i)."""
    m, lv, tg = (t.detach().to(dtype).requires_grad_(True) for t in (mean, logvar, target))
    losses = (gaussian(m, lv, tg), l1(m, tg), mse(m, tg))
    sum(c * v for c, v in zip(cots, losses)).backward()
    with torch.no_grad():
        term_abs = (((lv + (m - tg) ** 2 * torch.exp(-lv)) * .5 + 0.918).abs().mean().item(), losses[1].item(), losses[2].item())
    return tuple(v.item() for v in losses), term_abs, (m.grad, lv.grad, tg.grad)


def select(recon, target, k):
    """-> dict(d, e, key, thr (uint32), count_gt, count_eq) from float32 operands (any shape; flattened)."""
    r, t = (np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).ravel() for x in (recon, target))
    with np.errstate(all="ignore"):
        d = (r - t).astype(np.float32)
        e = (d * d).astype(np.float32)
    key = e.view(np.uint32) & np.uint32(0x7fffffff)
    assert 1 <= k <= key.size
    thr = np.partition(key, key.size - k)[key.size - k]
    gt, eq = int((key > thr).sum()), int((key == thr).sum())
    assert gt < k <= gt + eq
    return dict(d=d, e=e, key=key, thr=np.uint32(thr), count_gt=gt, count_eq=eq, k=k)


def worst_k_loss(sel):
    """The loss in float64 from the float32 squared errors."""
    k, thr = sel["k"], sel["thr"]
    e64 = sel["e"].astype(np.float64)
    with np.errstate(all="ignore"):
        e_k = float(np.array([thr], dtype=np.uint32).view(np.float32)[0])
        above = e64[sel["key"] > thr]
        s = float(above.sum()) if not np.isfinite(above).all() else math.fsum(above)
        return (s + (k - sel["count_gt"]) * e_k) / k


def worst_k_weights(sel):
    w = np.zeros(sel["key"].size, dtype=np.float64)
    w[sel["key"] > sel["thr"]] = 1.0
    w[sel["key"] == sel["thr"]] = (sel["k"] - sel["count_gt"]) / sel["count_eq"]
    return w


def worst_k_grad(sel, g):
    """d loss / d recon in float64 (flat); d loss / d target is its negative."""
    with np.errstate(all="ignore"):
        w = worst_k_weights(sel)
        out = g * 2.0 * sel["d"].astype(np.float64) * w / sel["k"]
        out[w == 0.0] = 0.0                                   # an infinite or NaN difference below the threshold still gets 0
        return out

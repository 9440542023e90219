"""Inputs of fixture G21 (tests/golden/g21_vae_losses.npz) and of the VAE-loss tests, regenerated from seeds: the fixture stores
results, never inputs.  Everything is float32 on the CPU in the logical layout (b, c, t, h, w), contiguous."""
import numpy as np
import torch

# fused pointwise losses and worst-k: shape, seed
CASES = {
    "tail": ((2, 3, 5, 17, 19), 2101),      # 9690 elements: not a multiple of 4 (the vector tail), ten tiles
    "tiny": ((1, 3, 1, 5, 7), 2102),        # 105 elements: less than one workgroup
    "mid": ((2, 3, 8, 33, 31), 2103),       # 49104 elements: 48 tiles
}
# worst-k cases on the inputs above (recon = mean, frames = target): case, percent
WORSTK = {
    "tail_p05": ("tail", 0.5),              # k = 48
    "tail_p02": ("tail", 0.2),              # k = 19
    "tiny_k1": ("tiny", 0.5),               # k = 1: the loss is the maximum
    "mid_all": ("mid", 100.0),              # k = numel: the loss is mse_loss
}
COTS = (0.7, 1.3, -0.4)                     # upstream cotangents of (gaussian, l1, mse)
WK_COT = 1.7                                # and of the worst-k loss
FULL_GRADS = 10000                          # gradients of at most this many elements are stored in full, larger ones as norms


def worst_k(numel, percent):
    return max(1, int(numel * (percent / 100.0)))


def inputs(case):
    shape, seed = CASES[case]
    g = torch.Generator().manual_seed(seed)
    mean = 0.6 * torch.randn(shape, generator=g)
    logvar = 0.7 * torch.randn(shape, generator=g) - 1.0
    target = torch.rand(shape, generator=g) * 2 - 1
    return mean, logvar, target


def crafted(name):
    """Key sets built to break a radix select: -> (recon, target, k), 1-D or 5-D float32."""
    g = torch.Generator().manual_seed(2110)
    if name == "low_digit":                  # d = 1 + i 2^-23: the squared errors agree in the upper 21 bits of the key
        n = 500
        d = (1.0 + torch.arange(n, dtype=torch.float64) * 2.0 ** -23).float()[torch.randperm(n, generator=g)]
        return d, torch.zeros(n), 100
    if name in ("spread", "spread_inf"):     # zeros, denormal squares, every fourth exponent, and (spread_inf) two +inf
        mant = 1.0 + torch.arange(8, dtype=torch.float64) / 8
        vals = [torch.zeros(40, dtype=torch.float64), torch.full((7,), 1e-22, dtype=torch.float64),
                torch.tensor([3e-23, 4e-23, 1.1e-22], dtype=torch.float64)]
        vals += [mant * 2.0 ** j for j in range(-60, 61, 4)]
        d = torch.cat(vals)
        if name == "spread_inf":
            d = torch.cat([d, torch.tensor([float("inf"), float("-inf")], dtype=torch.float64)])
        d = d.float()
        d = d * (torch.randint(0, 2, d.shape, generator=g) * 2 - 1).float()
        d = d[torch.randperm(d.numel(), generator=g)]
        return d, torch.zeros_like(d), 60
    if name == "ties":                       # uint8 frames against a uint8 reconstruction: a handful of distinct errors
        shape = (2, 3, 4, 16, 16)
        q = torch.randint(0, 256, shape, generator=g)
        r = (q + torch.randint(-3, 4, shape, generator=g)).clamp(0, 255)
        return (r.float() / 127.5 - 1), (q.float() / 127.5 - 1), worst_k(q.numel(), 20.0)
    if name == "equal":                      # recon == target everywhere
        x = torch.randn(2, 3, 2, 9, 11, generator=g)
        return x.clone(), x, worst_k(x.numel(), 0.5)
    if name == "nan":                        # one NaN element
        mean, _, target = inputs("tail")
        mean = mean.clone()
        mean.view(-1)[4321] = float("nan")
        return mean, target, 48
    raise KeyError(name)


CRAFTED = ("low_digit", "spread", "spread_inf", "ties", "equal", "nan")

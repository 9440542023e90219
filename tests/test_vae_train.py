"""CPU checks of VAE training (autoregressive_diffusion_amd/vae.py VAE.forward, vae_train.py): the training restatement against
fixture G16 (the reference's float64 outputs and parameter gradients), the refusals of `forward`, and the data-gradient weight
layouts of the two ResBlock convs against autograd.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_train_cpu_restatement as RT
from test_vae_encoder import g15

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel64(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


def g16():
    """(outputs and draws, parameter gradients, ref32_rel per parameter, x, state dict, kwargs) of fixture G16."""
    z = np.load(os.path.join(G, "g16_vae_train.npz"), allow_pickle=False)
    zg = np.load(os.path.join(G, "g16_vae_train_grads.npz"), allow_pickle=False)
    _, _, x, sd, kw = g15()
    grads = {k: torch.from_numpy(zg[k]) for k in zg.files if not k.startswith("ref32_rel/")}
    ref32 = {k[len("ref32_rel/"):]: float(zg[k]) for k in zg.files if k.startswith("ref32_rel/")}
    return z, grads, ref32, x, sd, kw


_REF = {}


def g16_restatement64():
    """The restatement's float64 run on G16's inputs, computed once and shared."""
    if not _REF:
        z, _, _, x, sd, kw = g16()
        _REF["v"] = RT.grads(sd, kw, x, torch.from_numpy(z["t_sample"]), torch.from_numpy(z["noise"]))
    return _REF["v"]


def test_restatement_against_g16():
    """The restatement in float64 reproduces the reference's float64 outputs and every one of its 174 767 parameter gradients to
    rel L2 1e-6 (the fixture is stored as float32: rounding alone gives about 3e-8)."""
    z, grads, ref32, x, sd, kw = g16()
    assert x.shape == (2, 3, 12, 24, 40) and z["noise"].shape == (2, 8, 3, 6, 10) and z["t_sample"].shape == (2,)
    assert sum(v.numel() for v in grads.values()) == 174767 and set(ref32) == set(grads)
    assert set(grads) == {k for k in sd if "fourier_cond" not in k}
    outs, g = g16_restatement64()
    for k in ("mean", "r_mean", "r_logvar"):
        print(f"restatement vs G16: {k} {rel64(outs[k], z[k]):.2e}")
        assert rel64(outs[k], z[k]) <= 1e-6, k
    worst = max(grads, key=lambda k: rel64(g[k], grads[k]))
    print(f"restatement vs G16: worst gradient {worst} {rel64(g[worst], grads[worst]):.2e}")
    for k in grads:
        assert rel64(g[k], grads[k]) <= 1e-6, k
    print("reference float32 vs float64, worst:", max(ref32, key=ref32.get), max(ref32.values()))


def test_forward_refusals():
    """`forward` on a CPU-resident model or a CPU input keeps pointing to the reference's edm2.vae; bad shapes (frames, t_sample,
    noise) raise ValueError first."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(channels=[3, 8, 8, 8], n_res_blocks=1)
    x = torch.zeros(1, 3, 4, 16, 16)
    for kw in ({}, dict(t_sample=torch.zeros(1), noise=torch.zeros(1, 8, 1, 4, 4))):
        with pytest.raises(NotImplementedError, match="edm2.vae"):
            vae(x, **kw)
    vae.eval()
    with pytest.raises(NotImplementedError, match="edm2.vae"):
        vae(x)
    for shape in ((1, 3, 6, 16, 16), (1, 3, 4, 18, 16), (1, 3, 4, 16, 14), (3, 4, 16, 16), (1, 4, 4, 16, 16), (1, 3, 0, 16, 16)):
        with pytest.raises(ValueError):
            vae(torch.zeros(shape))
    with pytest.raises(ValueError, match="t_sample"):
        vae(x, t_sample=torch.zeros(2))
    with pytest.raises(ValueError, match="noise"):
        vae(x, noise=torch.zeros(1, 8, 1, 4, 5))


@pytest.mark.parametrize("C,g", [(8, 4), (16, 2), (5, 1), (3, 2)])
def test_dgrad_weight_layouts_against_autograd(C, g):
    """vae_train._pack_dgrad: the packed data-gradient weights of conv A (mirrored causality: 2g frames of da, the own group and
    the next one, zero beyond the end) and of conv B, applied as include/oniris.h states them, give autograd's gradient of the
    two convs with the detached prefix."""
    from autoregressive_diffusion_amd.vae import _gpt, _nch
    from autoregressive_diffusion_amd.vae_train import _pack_dgrad
    gen = torch.Generator().manual_seed(C * 10 + g)
    B, T, H, W = 2, 3 * g, 5, 4
    wa = torch.randn(C * g, C, 2 * g, 3, 3, generator=gen, dtype=torch.float64)
    wb = torch.randn(C, C, 1, 3, 3, generator=gen, dtype=torch.float64)
    y = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    yp = F.pad(y, (1, 1, 1, 1))
    a = F.conv3d(torch.cat((yp[:, :, :g].detach(), yp), dim=2), wa, None, stride=(g, 1, 1))
    a = a.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)
    da = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64)
    (dy,) = torch.autograd.grad(a, y, da)
    wda, wdb = _pack_dgrad(wa, wb, C, g)
    nch, gpt = _nch(C), _gpt(C, g)
    assert wda.shape == (g // gpt, 2 * g, 3, 3, C, nch, gpt) and wdb.shape == (3, 3, C, nch)
    dap = F.pad(torch.cat((da, torch.zeros(B, C, g, H, W, dtype=torch.float64)), dim=2), (1, 1, 1, 1)).float()
    got = torch.zeros(B, C, T, H, W)
    for q in range(T // g):
        for r in range(g):
            for j in range(2 * g):
                for ky in range(3):
                    for kx in range(3):
                        w = wda[r // gpt, j, ky, kx, :, :C, r % gpt]                   # c, ci
                        got[:, :, q * g + r] += torch.einsum("bchw,ci->bihw", dap[:, :, q * g + j, ky:ky + H, kx:kx + W], w)
    assert rel64(got, dy) <= 1e-6
    assert float(wda[..., C:, :].abs().sum()) == 0 and float(wdb[..., C:].abs().sum()) == 0
    u = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64)
    (du,) = torch.autograd.grad(F.conv3d(u, wb, None, padding=(0, 1, 1)), u, dout)
    dop = F.pad(dout, (1, 1, 1, 1)).float()
    got = torch.zeros(B, C, T, H, W)
    for ky in range(3):
        for kx in range(3):
            got += torch.einsum("bcthw,ci->bithw", dop[:, :, :, ky:ky + H, kx:kx + W], wdb[ky, kx, :, :C])
    assert rel64(got, du) <= 1e-6

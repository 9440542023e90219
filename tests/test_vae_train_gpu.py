"""VAE training on HIP kernels (autoregressive_diffusion_amd/vae.py VAE.forward, vae_train.py, csrc/vae_train.hip) against fixture
G16 (the reference's float64 outputs and parameter gradients), against the float64 restatement at every channel width, against
the autograd contract, against itself (determinism, the inference path) and in a short optimisation."""
import os

import pytest
import torch

import vae_train_cpu_restatement as RT
from test_vae import rel
from test_vae_train import g16, g16_restatement64

DEV = "cuda"
pytestmark = pytest.mark.gpu
OUT_TOL, GRAD_TOL = 1e-5, 5e-5     # outputs: the project's criterion for G14 / G15; gradients: 5 x the worst deviation of the
                                   # reference's own float32 run from its float64 run (1.0e-5), for another fixed summation order


def seed_params(vae, seed):
    """Every parameter non-zero, as tests/golden/make_golden_vae.py seeds them: conv weights ~ N(0, 1 / fan_in), biases
    ~ 0.1 N(0, 1), the t_cond linear ~ 0.5 N(0, 1 / fan_in); logvar_multiplier -1.7."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in vae.named_parameters():
            if name.endswith("logvar_multiplier"):
                p.fill_(-1.7)
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                s = 0.5 if ".t_cond." in name else 1.0
                p.copy_(s * torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
    return vae


def _g16_vae():
    from autoregressive_diffusion_amd.vae import VAE
    z, grads, ref32, x, sd, kw = g16()
    vae = VAE(**kw)
    vae.load_state_dict(sd, strict=True)
    return vae.to(DEV).train(), z, grads, x.to(DEV), torch.from_numpy(z["t_sample"]).to(DEV), torch.from_numpy(z["noise"]).to(DEV)


def _step(vae, x, ts, noise, phis=RT.PHIS):
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, mean, cache = vae(x, t_sample=ts, noise=noise)
    RT.loss(r_mean, r_logvar, mean, phis).backward()
    return dict(r_mean=r_mean, r_logvar=r_logvar, mean=mean), {n: p.grad for n, p in vae.named_parameters()}, cache


def _compare(outs, grads, ref_outs, ref_grads, what):
    for k in ("mean", "r_mean", "r_logvar"):
        print(f"{what}: {k} {rel(outs[k].detach().cpu(), ref_outs[k]):.2e}")
    errs = {k: rel(grads[k].cpu(), ref_grads[k]) for k in ref_grads}
    for k in sorted(errs, key=errs.get, reverse=True):
        print(f"{what}: grad {k} {errs[k]:.2e}")
    for k in ("mean", "r_mean", "r_logvar"):
        assert rel(outs[k].detach().cpu(), ref_outs[k]) <= OUT_TOL, k
    assert set(grads) == set(ref_grads)
    for k, e in errs.items():
        assert e <= GRAD_TOL, (k, e)


def test_g16_on_the_hip_path():
    """mean, r_mean, r_logvar within 1e-5 of the reference and every parameter gradient within rel L2 5e-5 of its float64
    gradient; the returned cache has the reference's keys with None leaves."""
    vae, z, ref_grads, x, ts, noise = _g16_vae()
    outs, grads, cache = _step(vae, x, ts, noise)
    assert outs["mean"].shape == (2, 8, 3, 6, 10) and outs["r_mean"].shape == (2, 3, 12, 24, 40) == outs["r_logvar"].shape
    assert all(o.grad_fn is not None and o.dtype == torch.float32 for o in outs.values())
    _compare(outs, grads, z, ref_grads, "G16")
    assert set(cache) == {"encoder", "decoder"}
    for side in cache.values():
        assert set(side) == {"encoder_block_0", "encoder_block_1", "encoder_block_2"}
        for blk in side.values():
            assert set(blk) == {"res_block_0", "res_block_1"}
            assert all(set(rb) == {"conv3d_res0"} and rb["conv3d_res0"] is None for rb in blk.values())
    for n, b in vae.named_buffers():
        assert b.grad is None, n


def step_against_the_restatement(vae, x, ts, noise, what, ref=None):
    """One training step of `vae` (on the GPU, in training mode) on CPU inputs against the restatement in float64 on the CPU (or
    its ready result `ref`), with the bounds of G16; mean is bit for bit what encode gives."""
    outs, grads, _ = _step(vae, x.to(DEV), ts.to(DEV), noise.to(DEV))
    ref_outs, ref_grads = ref or RT.grads({k: v.cpu() for k, v in vae.state_dict().items()}, vae.kwargs, x, ts, noise)
    _compare(outs, grads, ref_outs, ref_grads, what)
    assert torch.equal(outs["mean"].detach(), vae.encode(x.to(DEV))[0])


def test_every_width_against_the_restatement():
    """channels [3, 32, 64, 8]: encoder widths 32 / 64 / 8 at g = 4 / 2 / 1, decoder widths 8 / 64 / 32 at g = 1 / 2 / 4, K = 256
    and 512 into the compressions -- with G16 every (channel capacity, frames per thread) pair of the training path -- against
    the restatement in float64 on the CPU, with the bounds of G16."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = seed_params(VAE(channels=[3, 32, 64, 8], n_res_blocks=1), 1611).to(DEV).train()
    g = torch.Generator().manual_seed(1612)
    x = torch.rand(2, 3, 8, 8, 12, generator=g) * 2 - 1
    ts, noise = torch.rand(2, generator=g) * 0.1, torch.randn(2, 8, 2, 2, 3, generator=g)
    step_against_the_restatement(vae, x, ts, noise, "widths 32/64/8")


def test_autograd_contract():
    """backward(retain_graph=True) on L1 then backward() on L2 accumulates the gradients of L1 + L2 (against the float64
    restatement, the bound of G16); a frozen parameter gets no .grad and the others are unchanged by it; x.requires_grad and a
    cache with tensors in it raise on the training path."""
    vae, z, _, x, ts, noise = _g16_vae()
    ph2 = (0.9, 2.1, 0.4)
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, mean, _ = vae(x, t_sample=ts, noise=noise)
    RT.loss(r_mean, r_logvar, mean).backward(retain_graph=True)
    RT.loss(r_mean, r_logvar, mean, ph2).backward()
    grads = {n: p.grad.clone() for n, p in vae.named_parameters()}
    _, _, _, xc, sd, kw = g16()
    _, ref = RT.grads(sd, kw, xc, ts.cpu(), noise.cpu(), phis=(RT.PHIS, ph2))
    errs = {k: rel(grads[k].cpu(), ref[k]) for k in ref}
    print("L1 + L2, worst:", max(errs, key=errs.get), max(errs.values()))
    assert set(grads) == set(ref) and max(errs.values()) <= GRAD_TOL
    _, ref1 = g16_restatement64()
    frozen = ["encoder.encoder_blocks.1.res_blocks.0.conv3d0.conv3d.weight", "decoder.encoder_blocks.0.res_blocks.1.t_cond.weight",
              "decoder.encoder_blocks.2.final_conv.bias", "encoder.encoder_blocks.0.compression_block.weight"]
    params = dict(vae.named_parameters())
    for n in frozen:
        params[n].requires_grad_(False)
    _, grads, _ = _step(vae, x, ts, noise)
    for n, gr in grads.items():
        if n in frozen:
            assert gr is None, n
        else:
            assert rel(gr.cpu(), ref1[n]) <= GRAD_TOL, n
    with pytest.raises(ValueError, match="requires grad"):
        vae(x.clone().requires_grad_(True), t_sample=ts, noise=noise)
    vae.eval()
    _, _, _, cache = vae(x, t_sample=ts, noise=noise)
    vae.train()
    with pytest.raises(ValueError, match="cache"):
        vae(x, cache=cache, t_sample=ts, noise=noise)
    with torch.no_grad():                                    # not the training path: the cache is carried
        vae(x, cache=cache, t_sample=ts, noise=noise)


@pytest.mark.selfcheck
def test_determinism_and_consistency_with_inference():
    """Two forward + backward runs give bit-identical outputs and gradients; mean from the training path is bit-identical to
    encode(x)[0]; eval-mode forward with the same draws returns real caches and outputs within 1e-5 of the training path's,
    without a grad_fn."""
    vae, z, _, x, ts, noise = _g16_vae()
    o1, g1, _ = _step(vae, x, ts, noise)
    g1 = {k: v.clone() for k, v in g1.items()}
    o2, g2, _ = _step(vae, x, ts, noise)
    assert all(torch.equal(o1[k], o2[k]) for k in o1)
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert torch.equal(o1["mean"].detach(), vae.encode(x)[0])
    vae.eval()
    r_mean, r_logvar, mean, cache = vae(x, t_sample=ts, noise=noise)
    assert r_mean.grad_fn is None and r_logvar.grad_fn is None and mean.grad_fn is None
    assert tuple(cache["encoder"]["encoder_block_0"]["res_block_1"]["conv3d_res0"].shape) == (2, 4, 24, 40, 8)
    assert tuple(cache["decoder"]["encoder_block_2"]["res_block_0"]["conv3d_res0"].shape) == (2, 4, 24, 40, 8)
    for k, v in (("r_mean", r_mean), ("r_logvar", r_logvar), ("mean", mean)):
        print(f"eval vs training path: {k} {rel(v, o1[k].detach()):.2e}")
        assert rel(v, o1[k].detach()) <= 1e-5, k
    vae.train()
    with torch.no_grad():
        r2, _, _, c2 = vae(x, t_sample=ts, noise=noise)
    assert torch.equal(r2, r_mean) and c2["decoder"]["encoder_block_0"]["res_block_0"]["conv3d_res0"] is not None
    torch.manual_seed(5)                                     # without t_sample / noise: rand, then randn_like, on x.device
    a = vae(x)[0]
    torch.manual_seed(5)
    t_b = torch.rand(2, device=DEV) * 0.1
    b = vae(x, t_sample=t_b, noise=torch.randn_like(mean))[0]
    assert torch.equal(a, b)


def test_it_trains():
    """A fresh VAE([3, 8, 8, 8], 2 ResBlocks) on a fixed smooth batch (2, 3, 8, 32, 48) with fixed draws, the Gaussian loss of
    the reference's training loops, 30 steps of torch AdamW(lr=3e-4) with clip_grad_norm_(1.0): every loss finite, the last below
    half the first (the training restatement alone, with exactly this recipe on the CPU: 0.1361 -> 0.0253, ratio 0.186, every
    step below the one before)."""
    from autoregressive_diffusion_amd.vae import VAE
    torch.manual_seed(1613)
    vae = VAE([3, 8, 8, 8], n_res_blocks=2).to(DEV).train()
    ti, yi, xi = torch.meshgrid(torch.arange(8.), torch.arange(32.), torch.arange(48.), indexing="ij")
    x = torch.stack([torch.sin(0.21 * xi + c) * torch.sin(0.17 * yi + 0.5 * c) * torch.sin(0.4 * ti + b + c)
                     for b in range(2) for c in range(3)]).reshape(2, 3, 8, 32, 48).to(DEV)
    g = torch.Generator().manual_seed(1614)
    ts, noise = (torch.rand(2, generator=g) * 0.1).to(DEV), torch.randn(2, 8, 2, 8, 12, generator=g).to(DEV)
    opt = torch.optim.AdamW(vae.parameters(), lr=3e-4)
    losses = []
    for _ in range(30):
        r_mean, r_logvar, _, _ = vae(x, t_sample=ts, noise=noise)
        loss = 0.5 * (r_logvar + (x - r_mean) ** 2 / torch.exp(r_logvar)).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(vae.parameters(), 1.0)
        opt.step()
        losses.append(loss.item())
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < 0.5 * losses[0]

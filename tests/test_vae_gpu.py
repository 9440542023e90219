"""The VAE decoder on HIP kernels (autoregressive_diffusion_amd/vae.py, csrc/vae.hip) against fixture G14 (the reference's own
outputs), against the CPU restatement at the gym VAE's full size, against itself (streaming, batch rows) and inside a rollout."""
import os

import numpy as np
import pytest
import torch

import vae_cpu_restatement as R
from test_vae import g14, rel

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
pytestmark = pytest.mark.gpu


def _g14_vae():
    from autoregressive_diffusion_amd.vae import VAE
    z, sd, kw = g14()
    vae = VAE(**kw)
    vae.load_state_dict(sd, strict=True)
    return z, vae.to(DEV), sd, kw


def _gym_vae():
    from autoregressive_diffusion_amd.vae import VAE
    return VAE.from_pretrained(os.path.join(G, "g14_vae_gym.pt")).to(DEV)


def _frames_match(frames, pre):
    """uint8 frames equal to trunc(pre), except where pre lies within 1e-2 of an integer: there one level either way."""
    frames = torch.as_tensor(np.asarray(frames)).long().cpu()
    pre = torch.as_tensor(pre).float().cpu()
    want = pre.long()
    near = (pre - pre.round()).abs() <= 1e-2
    diff = (frames - want).abs()
    bad = (diff > 1) | ((diff == 1) & ~near)
    return int(bad.sum()), int((diff == 1).sum())


def test_decode_against_g14():
    """decode (mean, logvar) within rel L2 1e-5 of the reference; latents_to_frames equal to the reference's frames up to one
    level where the pre-truncation value is within 1e-2 of an integer; the chunked decode (1 + 2 frames) as the reference's."""
    z, vae, _, _ = _g14_vae()
    zz, t = torch.from_numpy(z["z"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    mean, logvar, cache = vae.decode(zz, t)
    assert mean.shape == (2, 3, 12, 24, 24) and logvar.shape == mean.shape
    assert rel(mean.cpu(), z["mean"]) <= 1e-5 and rel(logvar.cpu(), z["logvar"]) <= 1e-5
    assert set(cache) == {"encoder_block_0", "encoder_block_1", "encoder_block_2"}
    assert set(cache["encoder_block_2"]) == {"res_block_0", "res_block_1"}
    assert tuple(cache["encoder_block_2"]["res_block_1"]["conv3d_res0"].shape) == (2, 4, 24, 24, 8)
    frames = vae.latents_to_frames(torch.from_numpy(z["latents"]).to(DEV))
    assert isinstance(frames, np.ndarray) and frames.shape == (2, 12, 24, 24, 3) and np.issubdtype(frames.dtype, np.integer)
    bad, _ = _frames_match(frames, z["frames_pre"])
    assert bad == 0
    m0, _, c = vae.decode(zz[:, :, :1], t)
    m1, _, _ = vae.decode(zz[:, :, 1:], t, c)
    assert rel(torch.cat((m0, m1), dim=2).cpu(), z["chunked_mean"]) <= 1e-5


@pytest.mark.slow
def test_gym_vae_full_size_against_restatement():
    """The gym VAE (channels [3, 8, 8, 8], seeded weights from a reference-written checkpoint) at 64x64 latents, B = 2, T = 3,
    t = [0.1, 0.35], against the CPU restatement: rel L2 1e-5 for mean and logvar; frames within the G14 rule."""
    vae = _gym_vae()
    sd = {k: v.cpu() for k, v in vae.state_dict().items()}
    g = torch.Generator().manual_seed(2024)
    latents = torch.randn(2, 3, 8, 64, 64, generator=g)
    t = torch.tensor([0.1, 0.35])
    std, mu = vae.std.cpu()[:, None, None], vae.mean.cpu()[:, None, None]
    z = (latents * std + mu).permute(0, 2, 1, 3, 4).contiguous()
    mean, logvar, _ = vae.decode(z.to(DEV), t.to(DEV))
    rm, rl, _ = R.decode(sd, vae.kwargs, z, t)
    assert rel(mean.cpu(), rm) <= 1e-5 and rel(logvar.cpu(), rl) <= 1e-5
    frames = vae.latents_to_frames(latents.to(DEV))
    bad, _ = _frames_match(frames, R.frames_pre(sd, vae.kwargs, latents))
    assert bad == 0


@pytest.mark.selfcheck
def test_streaming_and_batch_rows_are_bit_identical():
    """Decoding in 1-frame chunks and in 2 + 1 chunks through the cache, and each batch row alone, gives bit for bit what the
    whole-sequence batched decode gives (mean, logvar and uint8 frames)."""
    vae = _gym_vae()
    g = torch.Generator().manual_seed(7)
    z = torch.randn(2, 8, 3, 20, 28, generator=g).to(DEV)           # ragged tiles (80 x 112 frames)
    t = torch.tensor([0.1, 0.35], device=DEV)
    mean, logvar, _ = vae.decode(z, t)
    for cuts in ((1, 1, 1), (2, 1)):
        ms, ls, cache, s = [], [], None, 0
        for n in cuts:
            m, lv, cache = vae.decode(z[:, :, s:s + n], t, cache)
            ms.append(m); ls.append(lv); s += n
        assert torch.equal(torch.cat(ms, dim=2), mean) and torch.equal(torch.cat(ls, dim=2), logvar), cuts
    for b in range(2):
        m, lv, _ = vae.decode(z[b:b + 1], t[b:b + 1])
        assert torch.equal(m, mean[b:b + 1]) and torch.equal(lv, logvar[b:b + 1]), b
    latents = torch.randn(2, 3, 8, 20, 28, generator=g).to(DEV)
    whole, _ = vae.decode_frames(latents)
    parts, cache = [], None
    for i in range(3):
        f, cache = vae.decode_frames(latents[:, i:i + 1], cache=cache)
        parts.append(f)
    assert whole.dtype == torch.uint8 and whole.shape == (2, 12, 80, 112, 3)
    assert torch.equal(torch.cat(parts, dim=1), whole)
    assert np.array_equal(vae.latents_to_frames(latents), whole.cpu().numpy().astype(int))


@pytest.mark.selfcheck
def test_rollout_frames_stream_per_generated_frame():
    """A small UNet is prefilled with 2 context frames and samples 2 frames with edm_sampler_with_mse; decode_frames after the
    prefill and after each sampled frame, through its cache, equals latents_to_frames over the concatenated latents."""
    import paramgen
    from edm2.networks_edm2 import UNet, Precond
    from edm2.sampler import edm_sampler_with_mse
    from test_model_gpu import C1_CFG, load_params
    p = paramgen.prenormalise(paramgen.precond_params(C1_CFG, 11))
    net = load_params(Precond(UNet(**C1_CFG), sigma_data=1.0), p).eval()
    vae = _gym_vae()
    g = torch.Generator().manual_seed(12)
    B = 2
    context = torch.randn(B, 2, 8, 64, 64, generator=g).to(DEV)
    labels = torch.randint(0, 4, (B, 4), generator=g).to(DEV)
    with torch.no_grad():
        _, cache = net(context, torch.full((B, 2), 0.05, device=DEV), labels[:, :2], update_cache=True)
        frames, vcache = vae.decode_frames(context)
        out = [frames]
        for i in range(2):
            noise = torch.randn(B, 1, 8, 64, 64, generator=g).to(DEV)
            x, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=labels[:, 2 + i:3 + i], num_steps=4, sigma_min=0.4,
                                                  sigma_max=80, rho=2, noise=noise)
            context = torch.cat((context, x.float()), dim=1)
            f, vcache = vae.decode_frames(x, cache=vcache)
            out.append(f)
    streamed = torch.cat(out, dim=1)
    assert streamed.shape == (B, 16, 256, 256, 3)
    assert np.array_equal(streamed.cpu().numpy().astype(int), vae.latents_to_frames(context))

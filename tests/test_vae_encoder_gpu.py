"""The VAE encoder on HIP kernels (autoregressive_diffusion_amd/vae.py, csrc/vae_encoder.hip, csrc/vae.hip) against fixture G15
(the reference's own outputs), against the CPU restatement at the gym VAE's full size, against itself (streaming, batch rows,
uint8 against float frames) and in a closed loop with the sampler and the decoder."""
import os

import numpy as np
import pytest
import torch

import vae_encoder_cpu_restatement as RE
from test_vae import rel
from test_vae_encoder import g15

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
pytestmark = pytest.mark.gpu


def _g15_vae(kw, sd):
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(**kw)
    vae.load_state_dict(sd, strict=True)
    return vae.to(DEV)


def _gym_vae():
    from autoregressive_diffusion_amd.vae import VAE
    return VAE.from_pretrained(os.path.join(G, "g14_vae_gym.pt")).to(DEV)


def test_encode_against_g15():
    """encode on the fp32 input within rel L2 1e-5 of the reference's mean; encode_frames / frames_to_latents on the uint8 frames
    within 1e-5 of the normalised latents; the chunked encode (4 + 8 frames) within 1e-5 of the reference's chunked mean."""
    z, frames, x, sd, kw = g15()
    vae = _g15_vae(kw, sd)
    mean, cache = vae.encode(x.to(DEV))
    assert mean.shape == (2, 8, 3, 6, 10) and mean.dtype == torch.float32
    print("encode vs G15:", rel(mean.cpu(), z["mean"]))
    assert rel(mean.cpu(), z["mean"]) <= 1e-5
    assert set(cache) == {"encoder_block_0", "encoder_block_1", "encoder_block_2"}
    assert set(cache["encoder_block_0"]) == {"res_block_0", "res_block_1"}
    assert tuple(cache["encoder_block_0"]["res_block_1"]["conv3d_res0"].shape) == (2, 4, 24, 40, 8)
    assert tuple(cache["encoder_block_2"]["res_block_0"]["conv3d_res0"].shape) == (2, 1, 6, 10, 8)
    lat, _ = vae.encode_frames(frames.to(DEV))
    lat2 = vae.frames_to_latents(frames.to(DEV))
    assert lat.shape == (2, 3, 8, 6, 10) and torch.equal(lat, lat2)
    print("encode_frames vs G15:", rel(lat.cpu(), z["latents"]))
    assert rel(lat.cpu(), z["latents"]) <= 1e-5
    m0, c = vae.encode(x[:, :, :4].to(DEV))
    m1, _ = vae.encode(x[:, :, 4:].to(DEV), c)
    print("chunked encode vs G15:", rel(torch.cat((m0, m1), dim=2).cpu(), z["chunked_mean"]))
    assert rel(torch.cat((m0, m1), dim=2).cpu(), z["chunked_mean"]) <= 1e-5
    long = vae.encode_long_sequence(x, split_size=4)                 # CPU frames, moved chunk by chunk
    assert rel(long.cpu(), z["mean"]) <= 1e-5
    with pytest.raises(ValueError, match="cache"):
        vae.encode(x[:1, :, 4:].to(DEV), c)


@pytest.mark.slow
def test_gym_vae_full_size_against_restatement():
    """The gym VAE (channels [3, 8, 8, 8], seeded weights from a reference-written checkpoint), B = 2, 8 seeded uint8 frames of
    256x256, against the CPU restatement: rel L2 1e-5 for the raw mean and the normalised latents."""
    vae = _gym_vae()
    sd = {k: v.cpu() for k, v in vae.state_dict().items()}
    g = torch.Generator().manual_seed(2025)
    frames = torch.randint(0, 256, (2, 8, 256, 256, 3), generator=g, dtype=torch.uint8)
    x = (frames / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    mean, _ = vae.encode(x.to(DEV))
    rm, _ = RE.encode(sd, vae.kwargs, x)
    assert mean.shape == (2, 8, 2, 64, 64)
    print("gym encode vs restatement:", rel(mean.cpu(), rm))
    assert rel(mean.cpu(), rm) <= 1e-5
    lat = vae.frames_to_latents(frames.to(DEV))
    rl = RE.frames_to_latents(sd, vae.kwargs, frames)
    print("gym frames_to_latents vs restatement:", rel(lat.cpu(), rl))
    assert lat.shape == (2, 2, 8, 64, 64) and rel(lat.cpu(), rl) <= 1e-5


@pytest.mark.selfcheck
def test_streaming_and_batch_rows_are_bit_identical():
    """Encoding in 4-frame chunks and in 8 + 4 chunks through the cache, and each batch row alone, gives bit for bit what the
    whole-sequence batched encode gives, for encode and for encode_frames; uint8 frames and the same frames as float agree bit
    for bit.  The frame size is ragged against the 16x16 tile (80 x 112)."""
    vae = _gym_vae()
    g = torch.Generator().manual_seed(8)
    frames = torch.randint(0, 256, (2, 12, 80, 112, 3), generator=g, dtype=torch.uint8).to(DEV)
    x = (frames / 127.5 - 1).permute(0, 4, 1, 2, 3)                  # a strided view: read in place
    mean, _ = vae.encode(x)
    lat, _ = vae.encode_frames(frames)
    assert mean.shape == (2, 8, 3, 20, 28) and lat.shape == (2, 3, 8, 20, 28)
    assert torch.equal(vae.encode(x.contiguous())[0], mean)
    for cuts in ((4, 4, 4), (8, 4)):
        ms, ls, cm, cl, s = [], [], None, None, 0
        for n in cuts:
            m, cm = vae.encode(x[:, :, s:s + n], cm)
            lt, cl = vae.encode_frames(frames[:, s:s + n], cl)
            ms.append(m); ls.append(lt); s += n
        assert torch.equal(torch.cat(ms, dim=2), mean) and torch.equal(torch.cat(ls, dim=1), lat), cuts
    for b in range(2):
        assert torch.equal(vae.encode(x[b:b + 1])[0], mean[b:b + 1]), b
        assert torch.equal(vae.encode_frames(frames[b:b + 1])[0], lat[b:b + 1]), b
    for dtype in (torch.float32, torch.float64, torch.int32):
        assert torch.equal(vae.encode_frames(frames.to(dtype))[0], lat), dtype
    assert torch.equal(vae.frames_to_latents(frames), lat)
    assert torch.equal(vae.encode_long_sequence(x.cpu(), split_size=8), mean)


@pytest.mark.selfcheck
def test_closed_loop_frames_to_frames():
    """The generation_code.py flow on this package alone: uint8 frames -> encode_frames in 4-frame chunks -> Precond prefill
    (update_cache=True) -> two frames from edm_sampler_with_mse -> decode_frames through its cache.  The streamed context equals
    frames_to_latents of all frames; the output frames equal latents_to_frames over the concatenated latents."""
    import paramgen
    from edm2.networks_edm2 import UNet, Precond
    from edm2.sampler import edm_sampler_with_mse
    from test_model_gpu import C1_CFG, load_params
    p = paramgen.prenormalise(paramgen.precond_params(C1_CFG, 11))
    net = load_params(Precond(UNet(**C1_CFG), sigma_data=1.0), p).eval()
    vae = _gym_vae()
    g = torch.Generator().manual_seed(13)
    B = 2
    frames = torch.randint(0, 256, (B, 8, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV)
    labels = torch.randint(0, 4, (B, 4), generator=g).to(DEV)
    with torch.no_grad():
        parts, ecache = [], None
        for s in range(0, 8, 4):
            lt, ecache = vae.encode_frames(frames[:, s:s + 4], ecache)
            parts.append(lt)
        context = torch.cat(parts, dim=1)
        assert context.shape == (B, 2, 8, 64, 64) and torch.equal(context, vae.frames_to_latents(frames))
        _, cache = net(context, torch.full((B, 2), 0.05, device=DEV), labels[:, :2], update_cache=True)
        out, vcache = vae.decode_frames(context)
        out = [out]
        for i in range(2):
            noise = torch.randn(B, 1, 8, 64, 64, generator=g).to(DEV)
            x, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=labels[:, 2 + i:3 + i], num_steps=4, sigma_min=0.4,
                                                  sigma_max=80, rho=2, noise=noise)
            context = torch.cat((context, x.float()), dim=1)
            f, vcache = vae.decode_frames(x, cache=vcache)
            out.append(f)
    streamed = torch.cat(out, dim=1)
    assert streamed.shape == (B, 16, 256, 256, 3) and streamed.dtype == torch.uint8
    assert np.array_equal(streamed.cpu().numpy().astype(int), vae.latents_to_frames(context))

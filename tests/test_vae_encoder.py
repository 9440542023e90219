"""CPU checks of the VAE encoder's surface (autoregressive_diffusion_amd/vae.py): the CPU restatement against fixture G15, the
shape refusals (which come before anything else) and the coverage of the encoder's packed weights.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

import vae_encoder_cpu_restatement as RE
from test_vae import g14, rel

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def g15():
    z = np.load(os.path.join(G, "g15_vae_enc.npz"), allow_pickle=False)
    _, sd, kw = g14()
    frames = torch.from_numpy(z["frames"])
    x = (frames / 127.5 - 1).permute(0, 4, 1, 2, 3).contiguous()
    return z, frames, x, sd, kw


def test_restatement_against_g15():
    """The CPU restatement reproduces the reference's encode, its chunked encode through the cache (4 + 8 frames) and the
    normalised latents to rel L2 1e-5."""
    z, frames, x, sd, kw = g15()
    assert frames.dtype == torch.uint8 and frames.shape == (2, 12, 24, 40, 3) and z["mean"].shape == (2, 8, 3, 6, 10)
    mean, _ = RE.encode(sd, kw, x)
    print("restatement vs G15: whole", rel(mean, z["mean"]))
    assert rel(mean, z["mean"]) <= 1e-5
    m0, c = RE.encode(sd, kw, x[:, :, :4])
    m1, _ = RE.encode(sd, kw, x[:, :, 4:], c)
    print("restatement vs G15: chunked", rel(torch.cat((m0, m1), dim=2), z["chunked_mean"]))
    assert rel(torch.cat((m0, m1), dim=2), z["chunked_mean"]) <= 1e-5
    lat = RE.frames_to_latents(sd, kw, frames)
    assert lat.shape == (2, 3, 8, 6, 10) and rel(lat, z["latents"]) <= 1e-5


def test_shape_refusals_come_first():
    """Bad T, H, W, rank and channel count raise ValueError from every encoder entry point, on a CPU-resident model too: the shape
    checks come before the device check (whose NotImplementedError tests/test_vae.py::test_refusals pins)."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(channels=[3, 8, 8, 8], n_res_blocks=1, mean=[0.0] * 8, std=[1.0] * 8)
    for shape in ((1, 3, 6, 16, 16), (1, 3, 4, 18, 16), (1, 3, 4, 16, 14), (3, 4, 16, 16), (1, 4, 4, 16, 16), (1, 3, 0, 16, 16)):
        for call in (vae.encode, vae.encode_long_sequence):
            with pytest.raises(ValueError):
                call(torch.zeros(shape))
    for shape in ((1, 6, 16, 16, 3), (1, 4, 18, 16, 3), (1, 4, 16, 14, 3), (4, 16, 16, 3), (1, 4, 16, 16, 4), (1, 3, 4, 16, 16)):
        for call in (vae.encode_frames, vae.frames_to_latents):
            with pytest.raises(ValueError):
                call(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="split_size"):
        vae.encode_long_sequence(torch.zeros(1, 3, 8, 16, 16), split_size=6)
    with pytest.raises(NotImplementedError, match="edm2.vae"):
        vae.encode_frames(torch.zeros(1, 4, 16, 16, 3, dtype=torch.uint8))


def test_encoder_pack_covers_every_encoder_parameter():
    """The packed encoder weights name every encoder.* entry of a reference-written checkpoint, once each, and hold their values
    in the kernels' layouts."""
    from autoregressive_diffusion_amd.vae import VAE
    path = os.path.join(G, "g14_vae_gym.pt")
    ck = torch.load(path, weights_only=True)
    vae = VAE.from_pretrained(path)
    pk = vae._pack_encoder(torch.device("cpu"))
    want = [k for k in ck["state_dict"] if k.startswith("encoder.")]
    assert len(want) == 3 * (2 + 2 * 4) and sorted(pk["params"]) == sorted(want) and len(set(pk["params"])) == len(want)
    assert [(b["Cin"], b["C"], b["g"], b["tc"], b["sc"]) for b in pk["blocks"]] == [(3, 8, 4, 1, 1), (8, 8, 2, 2, 2), (8, 8, 1, 2, 2)]
    for i, b in enumerate(pk["blocks"]):
        w = ck["state_dict"][f"encoder.encoder_blocks.{i}.compression_block.weight"]
        assert torch.equal(b["wd"][:, 0, :b["C"]].t().reshape(w.shape), w) and len(b["res"]) == 2
        assert torch.equal(b["bd"][0, :b["C"]], ck["state_dict"][f"encoder.encoder_blocks.{i}.compression_block.bias"])
        assert torch.equal(b["wd"][:, 1].sum(dim=0), b["bd"][1] * (torch.arange(b["bd"].shape[1]) < b["C"]))   # the area windows
        for j, rb in enumerate(b["res"]):
            w1 = ck["state_dict"][f"encoder.encoder_blocks.{i}.res_blocks.{j}.conv3d1.weight"]
            assert torch.equal(rb["wb"][..., :b["C"]].permute(3, 2, 0, 1), w1[:, :, 0])
            assert rb["wa"].abs().sum() > 0 and rb["ba"].abs().sum() > 0
    assert vae._pack_encoder(torch.device("cpu")) is pk
    with torch.no_grad():
        vae.encoder.encoder_blocks[0].compression_block.bias.add_(1.0)
    assert vae._pack_encoder(torch.device("cpu")) is not pk

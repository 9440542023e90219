"""CPU checks of the VAE decoder's surface (autoregressive_diffusion_amd/vae.py): the CPU restatement against fixture G14, checkpoint
compatibility with the reference's VAE (keys, values, kwargs, round trip), and the refusals.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

import vae_cpu_restatement as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G14_KW = dict(channels=[3, 8, 16, 8], n_res_blocks=2, time_compressions=[1, 2, 2], spatial_compressions=[1, 2, 2])


def g14():
    z = np.load(os.path.join(G, "g14_vae.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(G, "g14_vae_sd.npz"), allow_pickle=False).items()}
    kw = dict(G14_KW, mean=z["kw_mean"].tolist(), std=z["kw_std"].tolist())
    return z, sd, kw


def rel(a, b):
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    return ((a - b).norm() / b.norm()).item()


def test_restatement_against_g14():
    """The CPU restatement reproduces the reference's decode (mean, logvar), its chunked decode through the cache (1 + 2 frames) and
    latents_to_frames' pre-truncation value to 1e-5."""
    z, sd, kw = g14()
    zz, t = torch.from_numpy(z["z"]), torch.from_numpy(z["t"])
    mean, logvar, _ = R.decode(sd, kw, zz, t)
    assert rel(mean, z["mean"]) <= 1e-5 and rel(logvar, z["logvar"]) <= 1e-5
    m0, _, c = R.decode(sd, kw, zz[:, :, :1], t)
    m1, _, _ = R.decode(sd, kw, zz[:, :, 1:], t, c)
    assert rel(torch.cat((m0, m1), dim=2), z["chunked_mean"]) <= 1e-5
    pre = R.frames_pre(sd, kw, torch.from_numpy(z["latents"]))
    assert (pre - torch.from_numpy(z["frames_pre"])).abs().max().item() <= 1e-5 * 255
    assert np.array_equal(z["frames"], z["frames_pre"].astype(int).astype(np.uint8))


def test_from_pretrained_reference_checkpoint(tmp_path):
    """A checkpoint the reference's VAE wrote loads into this VAE through the restricted loader: the same keys in the same order,
    the same values, the same kwargs; save_to_state_dict writes it back unchanged."""
    from autoregressive_diffusion_amd.vae import VAE
    path = os.path.join(G, "g14_vae_gym.pt")
    ck = torch.load(path, weights_only=True)
    vae = VAE.from_pretrained(path)
    sd = vae.state_dict()
    assert list(sd) == list(ck["state_dict"])
    assert all(torch.equal(sd[k], ck["state_dict"][k]) for k in sd)
    assert vae.kwargs == ck["kwargs"]
    assert vae.latent_channels == 8 and int(vae.time_compression) == 4 and int(vae.spatial_compression) == 4
    assert torch.allclose(vae.std, torch.tensor(ck["kwargs"]["std"])) and torch.allclose(vae.mean, torch.tensor(ck["kwargs"]["mean"]))
    out = str(tmp_path / "again.pt")
    vae.save_to_state_dict(out)
    back = torch.load(out, weights_only=True)
    assert back["kwargs"] == ck["kwargs"] and list(back["state_dict"]) == list(ck["state_dict"])
    assert all(torch.equal(back["state_dict"][k], ck["state_dict"][k]) for k in sd)
    again = VAE.from_pretrained(dict(back))
    assert all(torch.equal(again.state_dict()[k], sd[k]) for k in sd)


def test_fresh_vae_has_the_reference_keys_for_g14():
    """A VAE built from G14's kwargs has exactly the keys and shapes of the reference's state dict (strict load)."""
    from autoregressive_diffusion_amd.vae import VAE
    _, sd, kw = g14()
    vae = VAE(**kw)
    assert {k: tuple(v.shape) for k, v in vae.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    vae.load_state_dict(sd, strict=True)


def test_refusals():
    """Encoder-side entry points point to the reference; unsupported configurations fail when the model is built; the decoder has
    no CPU path."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(channels=[3, 8, 8, 8], n_res_blocks=1, mean=[0.0] * 8, std=[1.0] * 8)
    x = torch.zeros(1, 3, 4, 16, 16)
    for call in (lambda: vae.encode(x), lambda: vae(x), lambda: vae.frames_to_latents(torch.zeros(1, 4, 16, 16, 3)),
                 lambda: vae.encode_long_sequence(x)):
        with pytest.raises(NotImplementedError, match="edm2.vae"):
            call()
    with pytest.raises(NotImplementedError):
        VAE(channels=[3, 32, 128, 512, 8], n_res_blocks=2, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
    with pytest.raises(NotImplementedError):
        VAE(channels=[3, 8, 8, 8], n_res_blocks=2, time_compressions=[1, 3, 2])
    with pytest.raises(NotImplementedError):
        VAE(channels=[3, 8, 8, 8], n_res_blocks=2, spatial_compressions=[1, 2, 4])
    with pytest.raises(RuntimeError, match="GPU"):
        vae.decode(torch.zeros(1, 8, 1, 4, 4), torch.ones(1))

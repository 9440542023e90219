"""CPU checks of the wide VAE decoder's boundary: the float64 oracle (tests/vae_wide_oracle.py) against fixture G22 (the
reference in float64), the fixture's own consistency, which models construct, and which entry points refuse.  No kernel runs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vae_wide_oracle as O  # noqa: E402

CS_KW = dict(channels=[3, 16, 64, 256, 8], n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])


def g22():
    z = np.load(os.path.join(HERE, "golden", "g22_vae_wide.npz"))
    kw = dict(channels=z["kw_channels"].tolist(), n_res_blocks=int(z["kw_n_res_blocks"]), mean=z["kw_mean"].tolist(),
              std=z["kw_std"].tolist())
    return z, kw


def g22_vae():
    from autoregressive_diffusion_amd.vae import VAE
    z, kw = g22()
    return z, kw, O.seed_params(VAE(**kw), int(z["seed"])).eval()


def test_oracle_matches_g22():
    """Both are float64, so only the order of operations differs: 1e-10 rel L2 on decode, the chunked decode and frames_pre."""
    z, kw, vae = g22_vae()
    sd = vae.state_dict()
    zz, t = torch.from_numpy(z["z"]), torch.from_numpy(z["t"])
    assert zz.dtype == torch.float64 and z["mean"].dtype == np.float64
    mean, logvar, _ = O.decode(sd, kw, zz, t)
    assert O.rel_l2(mean, z["mean"]) <= 1e-10 and O.rel_l2(logvar, z["logvar"]) <= 1e-10
    m0, _, cache = O.decode(sd, kw, zz[:, :, :1], t)
    m1, _, _ = O.decode(sd, kw, zz[:, :, 1:], t, cache)
    assert O.rel_l2(torch.cat((m0, m1), dim=2), z["chunked_mean"]) <= 1e-10
    assert O.rel_l2(O.frames_pre(sd, kw, torch.from_numpy(z["latents"])), z["frames_pre"]) <= 1e-10


def test_g22_parameters_and_keys():
    """The re-seeded parameters are the ones the fixture was made with (their float64 sums and sums of squares), and a VAE built
    here from G22's kwargs has exactly the reference's state-dict keys and shapes."""
    z, kw, vae = g22_vae()
    # float64 sums of fp32 values: a host may add them in another order (1e-16 relative per addition, far below 1e-9), while one
    # redrawn element moves a sum by about its own size
    got = O.param_sums(vae)
    assert got.shape == z["param_sums"].shape and np.allclose(got, z["param_sums"], rtol=1e-9, atol=1e-9)
    sd = vae.state_dict()
    assert list(sd) == [str(k) for k in z["sd_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in z["sd_shapes"]]
    assert vae.decoder.in_channels == [8, 160, 72] and vae.decoder.group_sizes == [1, 2, 4]


def test_wide_models_construct():
    from autoregressive_diffusion_amd import vae as V
    assert V.MAX_WIDTH == 256 and V.MAX_NARROW == 64
    vae = V.VAE(**CS_KW)
    assert vae.decoder.in_channels == [8, 256, 64, 16]
    V.VAE(channels=[3, 16, 256, 8], n_res_blocks=1, time_compressions=[1, 1, 2])
    V.VAE(channels=[3, 65, 8], n_res_blocks=1, time_compressions=[1, 2], spatial_compressions=[1, 2])
    sd = vae.state_dict()
    again = V.VAE(**CS_KW)
    again.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), sd.values()))


def test_too_wide_is_refused():
    from autoregressive_diffusion_amd.vae import VAE
    for channels in ([3, 16, 64, 257, 8], [3, 32, 128, 512, 8], [3, 257, 8, 8, 8]):
        with pytest.raises(NotImplementedError):
            VAE(channels=channels, n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
    with pytest.raises(NotImplementedError, match="latent"):
        VAE(channels=[3, 16, 96, 72], n_res_blocks=1)


def test_wide_model_has_no_encoder_or_training():
    """Every encoder and training entry point of a model with a width above 64 raises NotImplementedError that names the width and
    points to the reference -- after the shape checks, on a CPU-resident model too, and never a StopIteration from the packing."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(mean=[0.0] * 8, std=[1.0] * 8, **CS_KW)
    x = torch.zeros(1, 3, 4, 16, 16)
    frames = torch.zeros(1, 4, 16, 16, 3)
    calls = {"encode": lambda: vae.encode(x), "encode_long_sequence": lambda: vae.encode_long_sequence(x),
             "frames_to_latents": lambda: vae.frames_to_latents(frames), "encode_frames": lambda: vae.encode_frames(frames),
             "forward (training)": lambda: vae.train()(x), "forward (eval)": lambda: vae.eval()(x)}
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=r"256 channels.*decoder.*edm2\.vae"):
            call()
    with pytest.raises(ValueError):                               # the shape checks still come first
        vae.encode(torch.zeros(1, 3, 3, 16, 16))
    with pytest.raises(ValueError):
        vae(torch.zeros(1, 4, 4, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):                # the decoder: no CPU path, as at narrow widths
        vae.decode(torch.zeros(1, 8, 1, 4, 4), torch.ones(1))


def test_narrow_model_refusals_unchanged():
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(channels=[3, 8, 64, 8], n_res_blocks=1, mean=[0.0] * 8, std=[1.0] * 8)
    x = torch.zeros(1, 3, 4, 16, 16)
    for call in (lambda: vae.encode(x), lambda: vae(x), lambda: vae.frames_to_latents(torch.zeros(1, 4, 16, 16, 3)),
                 lambda: vae.encode_long_sequence(x), lambda: vae.encode_frames(torch.zeros(1, 4, 16, 16, 3))):
        with pytest.raises(NotImplementedError, match="the encoder runs on HIP kernels only") as e:
            call()
        assert "edm2.vae" in str(e.value) and "channels" not in str(e.value)
    for kw in (dict(time_compressions=[1, 3, 2]), dict(spatial_compressions=[1, 2, 4])):
        with pytest.raises(NotImplementedError):
            VAE(channels=[3, 8, 8, 8], n_res_blocks=2, **kw)


def test_wide_packing_layouts():
    """The packed operands of a wide block (host side only): conv channel c g + gl at gl CP + c, zero padding, even CinP."""
    from autoregressive_diffusion_amd import vae as V
    vae = O.seed_params(V.VAE(channels=[3, 72, 8], n_res_blocks=1, time_compressions=[1, 2], spatial_compressions=[1, 2]), 7)
    pk = vae._pack(torch.device("cpu"))
    narrow, wide = pk["blocks"]
    assert not narrow["wide"] and wide["wide"] and wide["C"] == 72 and wide["g"] == 2
    rb, mod = wide["res"][0], vae.decoder.encoder_blocks[1].res_blocks[0]
    assert tuple(rb["wa"].shape) == (4, 3, 3, 72, 2, 96) and tuple(rb["wb"].shape) == (3, 3, 72, 96)
    w = mod.conv3d0.conv3d.weight.detach()
    assert rb["wa"][3, 1, 2, 5, 1, 70] == w[70 * 2 + 1, 5, 3, 1, 2] and rb["wa"][..., 72:].abs().max() == 0
    assert rb["ba"][1, 9] == mod.conv3d0.conv3d.bias[9 * 2 + 1]
    assert rb["wb"][2, 0, 4, 71] == mod.conv3d1.weight[71, 4, 0, 2, 0]
    assert tuple(wide["wu"].shape) == (72, 8, 96) and wide["wu"][3, 5, 60] == vae.decoder.encoder_blocks[1].decompression_block.weight[5 * 72 + 60, 3, 0, 0, 0]
    assert tuple(wide["wo"].shape) == (72, 1, 32) and wide["wo"][9, 0, 4] == vae.decoder.encoder_blocks[1].final_conv.weight[4, 9, 0, 0, 0]

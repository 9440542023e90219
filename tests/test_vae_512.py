"""CPU checks of `VAE512` (autoregressive_diffusion_amd/vae.py: the VAE at block widths up to 512 channels, the full-size
Counter-Strike model): what constructs and what is refused, checkpoints between `VAE512` and `VAE`, the packed layouts of a
512-wide block, the weight-gradient slab policy of vae_train._nslab above and below 256 channels, the binding of the conv A tile
knob, and the float64 training restatement (tests/vae_train_cpu_restatement.py) and the float64 inference oracles against fixture
G25 (the reference in float64 at a 512-channel block).  No kernel runs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import vae_wide_oracle as O  # noqa: E402
import vae_wide_encoder_oracle as E  # noqa: E402
import vae_train_cpu_restatement as R  # noqa: E402
from test_vae_wide_train import g24_grad_error, g24_stride  # noqa: E402

CS_COMP = dict(time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
CS512_KW = dict(channels=[3, 32, 128, 512, 8], n_res_blocks=1, **CS_COMP)


def g25():
    z = np.load(os.path.join(HERE, "golden", "g25_vae_512.npz"))
    kw = dict(channels=z["kw_channels"].tolist(), n_res_blocks=int(z["kw_n_res_blocks"]),
              time_compressions=z["kw_time_compressions"].tolist(), spatial_compressions=z["kw_spatial_compressions"].tolist())
    return z, kw


def g25_vae():
    from autoregressive_diffusion_amd.vae import VAE512
    z, kw = g25()
    return z, kw, O.seed_params(VAE512(**kw), int(z["seed"]))


def g25_inputs(z):
    """x (B, 3, T, H, W) float64, t_sample, noise of the fixture."""
    x = (torch.from_numpy(z["frames"]).double() / 127.5 - 1).permute(0, 4, 1, 2, 3)
    return x, torch.from_numpy(z["t_sample"]), torch.from_numpy(z["noise"])


g25_grad_error = g24_grad_error        # G25 stores its gradients exactly as G24 does (stride, norm/, sum/)


def test_construction_and_refusals():
    from autoregressive_diffusion_amd import vae as V
    assert V.VAE512.max_width == 512 and V.VAE.max_width == 256 == V.MAX_WIDTH and issubclass(V.VAE512, V.VAE)
    vae = V.VAE512(channels=[3, 32, 128, 512, 8], n_res_blocks=5, **CS_COMP)
    assert vae.decoder.in_channels == [8, 512, 128, 32] and vae.decoder.group_sizes == [1, 2, 4, 4] and vae._wide == 512
    assert vae.encoder.out_channels == [32, 128, 512, 8] and vae.encoder.group_sizes == [4, 4, 2, 1]
    assert len(vae.decoder.encoder_blocks[1].res_blocks) == 5
    with pytest.raises(NotImplementedError, match="512"):
        V.VAE512(channels=[3, 32, 128, 513, 8], n_res_blocks=1, **CS_COMP)
    with pytest.raises(NotImplementedError, match="latent"):
        V.VAE512(channels=[3, 16, 96, 72], n_res_blocks=1)
    for kw in (dict(time_compressions=[1, 3, 2]), dict(spatial_compressions=[1, 2, 4])):
        with pytest.raises(NotImplementedError):
            V.VAE512(channels=[3, 8, 8, 8], n_res_blocks=1, **kw)
    with pytest.raises(ValueError):
        V.VAE512(channels=[3, 8, 8], n_res_blocks=1)
    with pytest.raises(NotImplementedError, match="256"):           # plain VAE has not moved
        V.VAE(**CS512_KW)


def test_training_path_is_on_as_constructed():
    import copy
    from autoregressive_diffusion_amd.vae import VAE, VAE512
    vae = VAE512(**CS512_KW).train()
    assert vae._wide_training is True and copy.deepcopy(vae)._wide_training is True
    assert VAE(channels=[3, 16, 96, 160, 8], n_res_blocks=1, **CS_COMP)._wide_training is False
    x = torch.zeros(1, 3, 8, 16, 16)
    with pytest.raises(NotImplementedError, match=r"512 channels.*HIP kernels only.*edm2\.vae"):     # a CPU model: the device refusal
        vae(x)
    assert vae.wide_training(False) is vae and vae._wide_training is False
    with pytest.raises(NotImplementedError, match=r"512 channels.*edm2\.vae"):
        vae(x)
    with pytest.raises(ValueError):                               # the shape checks still come first
        vae(torch.zeros(1, 3, 6, 16, 16))
    assert "wide_training" not in str(vae.kwargs) and not any("wide" in k for k in vae.state_dict())


def test_checkpoints_between_vae512_and_vae(tmp_path):
    """kwargs and state_dict of a 160-wide model round-trip both ways, through the checkpoint file too; a 512-wide file loads
    into VAE512 and is still refused by VAE."""
    from autoregressive_diffusion_amd.vae import VAE, VAE512
    kw = dict(channels=[3, 16, 96, 160, 8], n_res_blocks=1, mean=[0.1] * 8, std=[1.5] * 8, **CS_COMP)
    a = O.seed_params(VAE512(**kw), 11)
    b = VAE(**a.kwargs)
    assert a.kwargs == b.kwargs == kw and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    for src, cls in ((a, VAE), (b, VAE512)):
        path = str(tmp_path / f"{cls.__name__}.pt")
        src.save_to_state_dict(path)
        got = cls.from_pretrained(path)
        assert type(got) is cls and got.kwargs == kw
        assert all(torch.equal(u, v) for u, v in zip(src.state_dict().values(), got.state_dict().values()))
        assert torch.equal(got.mean, src.mean) and torch.equal(got.std, src.std)
    wide = O.seed_params(VAE512(**CS512_KW), 12)
    path = str(tmp_path / "cs512.pt")
    wide.save_to_state_dict(path)
    got = VAE512.from_pretrained(path)
    assert got._wide_training is True and got.kwargs == dict(CS512_KW, mean=None, std=None) == wide.kwargs
    assert all(torch.equal(u, v) for u, v in zip(wide.state_dict().values(), got.state_dict().values()))
    with pytest.raises(NotImplementedError):
        VAE.from_pretrained(path)


def test_packing_layouts_at_512():
    """The packed operands of a 512-wide block and of a ragged one above 256 (host side only), as test_wide_packing_layouts does
    at 72: conv channel c g + gl at gl CP + c, zero padding, even CinP."""
    from autoregressive_diffusion_amd import vae as V, vae_train
    vae = O.seed_params(V.VAE512(channels=[3, 512, 8], n_res_blocks=1, time_compressions=[1, 2], spatial_compressions=[1, 2]), 7)
    dev = torch.device("cpu")
    narrow, wide = vae._pack(dev)["blocks"]
    assert not narrow["wide"] and wide["wide"] and wide["C"] == 512 and wide["g"] == 2
    dec = vae.decoder.encoder_blocks[1]
    rb, mod = wide["res"][0], dec.res_blocks[0]
    assert tuple(rb["wa"].shape) == (4, 3, 3, 512, 2, 512) and tuple(rb["wb"].shape) == (3, 3, 512, 512) and tuple(rb["ba"].shape) == (2, 512)
    w = mod.conv3d0.conv3d.weight.detach()
    assert rb["wa"][3, 1, 2, 5, 1, 510] == w[510 * 2 + 1, 5, 3, 1, 2] and rb["wa"][0, 2, 0, 511, 0, 3] == w[3 * 2, 511, 0, 2, 0]
    assert rb["ba"][1, 9] == mod.conv3d0.conv3d.bias[9 * 2 + 1]
    assert rb["wb"][2, 0, 4, 511] == mod.conv3d1.weight[511, 4, 0, 2, 0]
    assert tuple(wide["wu"].shape) == (512, 8, 512) and wide["wu"][3, 5, 500] == dec.decompression_block.weight[5 * 512 + 500, 3, 0, 0, 0]
    assert tuple(wide["wo"].shape) == (512, 1, 32) and wide["wo"][509, 0, 4] == dec.final_conv.weight[4, 509, 0, 0, 0]
    assert wide["wo"][:, :, 6:].abs().max() == 0
    enc = vae._pack_encoder(dev)["blocks"]
    assert enc[0]["wide"] and enc[0]["wide_down"] and tuple(enc[0]["wd"].shape) == (1, 4, 512) and enc[0]["wd"][0, 3].abs().max() == 0
    assert enc[1]["wide_down"] and not enc[1].get("wide") and tuple(enc[1]["wd"].shape) == (8, 512, 32)     # K = 4096 -> 8
    assert enc[1]["wd"][5, 100, 7] == vae.encoder.encoder_blocks[1].compression_block.weight[7, 5 * 512 + 100, 0, 0, 0]
    # a ragged width above 256: CP = 288, CinP = 264 at 264; an odd one pads the input channels too
    for C, CP, CinP in ((264, 288, 264), (321, 352, 322)):
        r = V.ResBlock(C, (4, 3, 3), 2)
        with torch.no_grad():
            r.conv3d1.weight.normal_()
        p = V._pack_res_wide(r, C, 2, dict(device=dev, dtype=torch.float32))
        assert tuple(p["wa"].shape) == (4, 3, 3, CinP, 2, CP) and tuple(p["wb"].shape) == (3, 3, CinP, CP)
        assert p["wa"][..., C:].abs().max() == 0 and p["wb"][..., C:].abs().max() == 0 and p["wb"][:, :, C:].abs().sum() == 0
        assert p["wa"][0:2].abs().max() == 0 and p["wa"][2:, :, :, :C, :, :C].abs().min() > 0       # the causal half is zero (vae.py:29-31)
        wda, wdb, zb = vae_train._pack_dgrad_wide(r.conv3d0.conv3d.weight, r.conv3d1.weight, C, 2)
        assert tuple(wda.shape) == (4, 3, 3, CinP, 2, CP) and tuple(wdb.shape) == (3, 3, CinP, CP) and zb.abs().sum() == 0
        assert wdb[0, 2, 7, C - 1] == r.conv3d1.weight[7, C - 1, 0, 2, 0]


def test_slab_policy():
    """Up to 256 channels: min(work, 1024, max(64, _SLAB_BYTES // (4 size))), at least 1, with or without the width given -- the
    counts every existing model's summation order depends on.  Above: at least 1 and within _SLAB_BYTES, or a single slab."""
    from autoregressive_diffusion_amd import vae_train as T
    assert T._SLAB_BYTES == 64 << 20
    sizes = [1, 9 * 65 * 65 + 65, 9 * 72 * 72 + 72, 8 * 9 * 160 * 160 + 2 * 160, 32 * 9 * 256 * 256 + 4 * 256, 128 * 9 * 256 * 256 + 8 * 256,
             262144, 262145, 16777216, 16777217, 4096 * 8 + 8, 8 * 9 * 512 * 512 + 2 * 512, 32 * 9 * 512 * 512 + 4 * 512]
    works = [1, 2, 3, 16, 63, 64, 65, 1000, 1024, 1025, 100000]
    for size in sizes:
        for work in works:
            old = max(1, min(work, 1024, max(64, T._SLAB_BYTES // (4 * size))))
            assert T._nslab(work, size) == old
            for width in (1, 64, 65, 72, 160, 256):
                assert T._nslab(work, size, width) == old, (work, size, width)
            for width in (257, 264, 320, 384, 512):
                n = T._nslab(work, size, width)
                assert isinstance(n, int) and 1 <= n <= max(1, T._SLAB_BYTES // (4 * size)) and n <= work and n <= 1024, (work, size, width)
                assert n == min(old, n)                              # never more slabs than below 256
    conv_a_512_g4 = 2 * 4 * 4 * 9 * 512 * 512 + 4 * 512
    assert 4 * conv_a_512_g4 > 300e6 and T._nslab(2 * 8 * 16, conv_a_512_g4, 512) == 1 and T._nslab(2 * 8 * 16, conv_a_512_g4) == 64
    assert T._nslab(64, 9 * 512 * 512 + 512, 512) == 7                # conv B at 512: 9.4 MB a slab, seven fit
    assert T._nslab(64, 9 * 264 * 264 + 264, 264) == 26 and T._nslab(3, 9 * 264 * 264 + 264, 264) == 3


def test_knob_is_bound_and_declared():
    """oniris_vae_wide_set_nb_max is exported, bound and declared; it returns the previous value, and the ABI version has not moved."""
    import re
    from autoregressive_diffusion_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "oniris.h")).read()
    name = "oniris_vae_wide_set_nb_max"
    assert name in _lib.EXPORTED and re.search(r"\bint " + name + r"\(int nb\);", header)
    was = _lib.lib.oniris_vae_wide_set_nb_max(2)
    try:
        assert was in (2, 4) and _lib.lib.oniris_vae_wide_set_nb_max(4) == 2 and _lib.lib.oniris_vae_wide_set_nb_max(7) == 4
        assert _lib.lib.oniris_vae_wide_set_nb_max(0) == 4 and _lib.lib.oniris_vae_wide_set_nb_max(2) == 2
    finally:
        _lib.lib.oniris_vae_wide_set_nb_max(was)
    assert _lib.lib.oniris_abi_version() == 14


def test_restatement_matches_g25():
    """Both are float64, so only the order of operations differs: 1e-10 on the training outputs and on every parameter gradient,
    the way tests/test_vae_wide_train.py holds G24."""
    z, kw, vae = g25_vae()
    assert os.path.getsize(os.path.join(HERE, "golden", "g25_vae_512.npz")) < 1000 * 1000
    assert np.allclose(O.param_sums(vae), z["param_sums"], rtol=1e-9, atol=1e-9)
    assert kw["channels"] == [3, 8, 512, 8] and vae.encoder.out_channels == [8, 512, 8]
    assert vae.encoder.group_sizes == [2, 2, 1] and vae.decoder.group_sizes == [1, 2, 2]
    x, t_sample, noise = g25_inputs(z)
    outs, grads = R.grads(vae.state_dict(), kw, x, t_sample, noise)
    for k in ("mean", "r_mean", "r_logvar"):
        assert z[k].dtype == np.float64 and O.rel_l2(outs[k], z[k]) <= 1e-10, k
    names = [n for n, _ in vae.named_parameters()]
    sampled = [k[5:] for k in z.files if k.startswith("norm/")]
    assert sorted(grads) == sorted(names) and len(sampled) == 7
    assert all(z["grad/" + n].size == -(-grads[n].numel() // g24_stride(grads[n].numel())) for n in sampled)
    for n in names:
        assert g25_grad_error(z, n, grads[n]) <= 1e-10, n


def test_inference_oracles_match_g25():
    """The eval-mode targets of G25 against the float64 inference oracles: encode, and decode on latents no encoder made.  With
    no cache the eval-mode prefix holds the values of the training-mode one, so encode's mean is also the training mean."""
    z, kw, vae = g25_vae()
    sd = vae.state_dict()
    x, t_sample, noise = g25_inputs(z)
    assert O.rel_l2(z["eval_mean"], z["mean"]) <= 1e-12
    mean, _ = E.encode(sd, kw, x)
    assert O.rel_l2(mean, z["eval_mean"]) <= 1e-10
    r_mean, r_logvar, _ = O.decode(sd, kw, noise, t_sample)
    assert O.rel_l2(r_mean, z["eval_r_mean"]) <= 1e-10 and O.rel_l2(r_logvar, z["eval_r_logvar"]) <= 1e-10

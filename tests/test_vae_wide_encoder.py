"""CPU checks of the wide VAE encoder's boundary: the float64 oracle (tests/vae_wide_encoder_oracle.py) against fixture G23 (the
reference in float64), the fixture's own consistency, how _pack_encoder routes the blocks, what the packed `down` operands hold,
and the C entry point's declaration and binding.  No kernel runs."""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vae_wide_oracle as O  # noqa: E402
import vae_wide_encoder_oracle as E  # noqa: E402

CS_KW = dict(channels=[3, 16, 64, 256, 8], n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
NARROW_KEYS = {"Cin", "C", "g", "nch", "gpt", "tc", "sc", "wd", "bd", "res"}


def g23():
    z = np.load(os.path.join(HERE, "golden", "g23_vae_wide_enc.npz"))
    kw = dict(channels=z["kw_channels"].tolist(), n_res_blocks=int(z["kw_n_res_blocks"]), mean=z["kw_mean"].tolist(),
              std=z["kw_std"].tolist())
    return z, kw


def g23_vae():
    from autoregressive_diffusion_amd.vae import VAE
    z, kw = g23()
    return z, kw, O.seed_params(VAE(**kw), int(z["seed"])).eval()


def test_oracle_matches_g23():
    """Both are float64, so only the order of operations differs: 1e-10 rel L2 on encode, the chunked encode and the latents."""
    z, kw, vae = g23_vae()
    sd = vae.state_dict()
    frames, x = torch.from_numpy(z["frames"]), torch.from_numpy(z["x"])
    assert frames.dtype == torch.uint8 and frames.shape == (2, 8, 20, 28, 3)
    assert x.dtype == torch.float64 and z["mean"].dtype == np.float64 and z["mean"].shape == (2, 8, 2, 5, 7)
    assert torch.equal(x, (frames.double() / 127.5 - 1).permute(0, 4, 1, 2, 3))
    mean, _ = E.encode(sd, kw, x)
    assert O.rel_l2(mean, z["mean"]) <= 1e-10
    m0, cache = E.encode(sd, kw, x[:, :, :4])
    m1, _ = E.encode(sd, kw, x[:, :, 4:], cache)
    assert O.rel_l2(torch.cat((m0, m1), dim=2), z["chunked_mean"]) <= 1e-10
    lat = E.frames_to_latents(sd, kw, frames)
    assert lat.shape == (2, 2, 8, 5, 7) and O.rel_l2(lat, z["latents"]) <= 1e-10


def test_g23_parameters():
    """The re-seeded parameters are the ones the fixture was made with (float64 sums of fp32 values: a host may add them in another
    order, 1e-16 relative per addition, while one redrawn element moves a sum by about its own size)."""
    z, kw, vae = g23_vae()
    got = O.param_sums(vae)
    assert got.shape == z["param_sums"].shape and np.allclose(got, z["param_sums"], rtol=1e-9, atol=1e-9)
    assert vae.encoder.out_channels == [72, 160, 8] and vae.encoder.group_sizes == [4, 2, 1]


def _routes(vae):
    pk = vae._pack_encoder(torch.device("cpu"))
    return pk, [(bool(bk.get("wide")), bool(bk.get("wide_down"))) for bk in pk["blocks"]]


def test_pack_encoder_routes_blocks():
    """ResBlocks run wide above 64 channels; `down` is the GEMM above 64 output channels or above K = 512, else the narrow kernel."""
    from autoregressive_diffusion_amd import vae as V
    _, _, vae = g23_vae()
    pk, routes = _routes(vae)
    assert routes == [(True, True), (True, True), (False, True)]          # K = 3, 576, 1280
    b0, b1, b2 = pk["blocks"]
    assert tuple(b0["wd"].shape) == (1, 4, 96) and tuple(b0["bd"].shape) == (96,) and (b0["nch"], b0["gpt"]) == (0, 0)
    assert tuple(b1["wd"].shape) == (8, 72, 160) and tuple(b1["res"][0]["wa"].shape) == (4, 3, 3, 160, 2, 160)
    assert tuple(b2["wd"].shape) == (8, 160, 32) and (b2["nch"], b2["gpt"]) == (8, 1)
    assert tuple(b2["res"][0]["wa"].shape) == (1, 2, 3, 3, 8, 8, 1)       # the narrow layout of csrc/vae_conv3.h
    assert len(pk["params"]) == len(set(pk["params"])) == len([k for k in vae.state_dict() if k.startswith("encoder.")])
    _, routes = _routes(V.VAE(**CS_KW))
    assert routes == [(False, False), (False, False), (True, True), (False, True)]     # K = 3, 128, 512, 1024
    _, routes = _routes(V.VAE(channels=[3, 64, 64, 8], n_res_blocks=1))                # K = 3, 512, 512: all narrow
    assert routes == [(False, False)] * 3


def test_packed_down_reproduces_the_oracle():
    """w [pos][CinP][CP] and bias [CP] multiplied out in float64, plus the area windows, against the oracle's `down`; the padding
    is zero."""
    _, _, vae = g23_vae()
    pk = vae._pack_encoder(torch.device("cpu"))
    gen = torch.Generator().manual_seed(2310)
    for i, bk in enumerate(pk["blocks"]):
        blk = vae.encoder.encoder_blocks[i]
        Cin, C, tc, sc = bk["Cin"], bk["C"], bk["tc"], bk["sc"]
        x = torch.randn(1, 2 * tc, 3 * sc, 2 * sc, Cin, generator=gen).double()
        want = E.down(x, blk.compression_block.weight.detach(), blk.compression_block.bias.detach(), tc, sc)
        r = E.rearrange_down(x, tc, sc)
        w, b = bk["wd"].double(), bk["bd"].double()
        assert w.shape[1] == Cin + (Cin & 1) and w.shape[2] % 32 == 0
        assert w[:, Cin:].abs().sum().item() == 0
        assert w[:, :, C:].abs().sum().item() == 0 and b[C:].abs().sum().item() == 0
        y = torch.einsum("bthwpc,pco->bthwo", r.reshape(*r.shape[:4], tc * sc * sc, Cin), w[:, :Cin, :C]) + b[:C]
        area = torch.stack([r[..., s0:s1].mean(dim=-1) for s0, s1 in O.area_windows(r.shape[-1], C)], dim=-1)
        assert O.rel_l2(y + area, want) <= 1e-12


def test_short_chunks_are_refused_by_shape():
    """[3,16,64,256,8] with time compressions [1,2,2,1]: group sizes [4,4,2,1], block 1 sees T / 2 frames in groups of 4, so a chunk
    has a multiple of 8 frames (in the reference too, whose conv fails otherwise): a ValueError of the encoder's run, after the
    device check (the entry points of a CPU-resident model keep their refusals)."""
    import pytest
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(mean=[0.0] * 8, std=[1.0] * 8, **CS_KW)
    for T in (4, 12, 20):
        with pytest.raises(ValueError, match="multiple of 8"):
            vae._check_groups(T)
    vae._check_groups(8)
    vae._check_groups(16)
    narrow = VAE(channels=[3, 8, 8, 8], n_res_blocks=1)           # the default compressions ask for what they asked before: 4
    narrow._check_groups(4)
    with pytest.raises(NotImplementedError):
        vae.encode(torch.zeros(1, 3, 4, 16, 16))


def test_entry_point_is_bound_and_declared():
    from autoregressive_diffusion_amd import _lib
    assert "oniris_vae_wide_down" in _lib.EXPORTED and callable(_lib.lib.oniris_vae_wide_down)
    header = open(os.path.join(os.path.dirname(HERE), "include", "oniris.h")).read()
    assert re.search(r"\bint oniris_vae_wide_down\(const void\* x, int x_is_u8,", header)
    assert _lib.lib.oniris_abi_version() == 14


def test_narrow_model_packs_as_before():
    """channels=[3,8,8,8]: the encoder pack has the keys and shapes it had before there was a wide path."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = O.seed_params(VAE(channels=[3, 8, 8, 8], n_res_blocks=2), 5)
    pk = vae._pack_encoder(torch.device("cpu"))
    assert set(pk) == {"sig", "blocks", "params", "zeros"}
    shapes = [((3, 2, 8), 1, 1, 4, 4), ((64, 2, 8), 2, 2, 2, 2), ((64, 2, 8), 2, 2, 1, 1)]
    for bk, (wd, tc, sc, g, gpt) in zip(pk["blocks"], shapes):
        assert set(bk) == NARROW_KEYS
        assert tuple(bk["wd"].shape) == wd and tuple(bk["bd"].shape) == (2, 8)
        assert (bk["tc"], bk["sc"], bk["g"], bk["nch"], bk["gpt"], bk["C"]) == (tc, sc, g, 8, gpt, 8)
        assert len(bk["res"]) == 2
        for rb in bk["res"]:
            assert set(rb) == {"wa", "ba", "wb", "bb"}
            assert tuple(rb["wa"].shape) == (g // gpt, 2 * g, 3, 3, 8, 8, gpt) and tuple(rb["ba"].shape) == (g // gpt, 8, gpt)
            assert tuple(rb["wb"].shape) == (3, 3, 8, 8) and tuple(rb["bb"].shape) == (8,)

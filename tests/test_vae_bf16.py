"""CPU checks of `VAE.bf16_inference()` (autoregressive_diffusion_amd/vae.py, csrc/vae_wide_bf16.h): the switch as an attribute
(deepcopy, state_dict, kwargs, the pack signature), the packed bf16 weights against `weight.to(torch.bfloat16)` in the documented
layout at 72 and 512 channels, the binding of the five entry points, and the comparator of tests/test_vae_bf16_gpu.py against the
bf16-faithful oracle with one defect at a time (tests/vae_bf16_oracle.py DEFECTS): each lies outside the bound the GPU test
applies, at the smallest Gaussian case of every stage.  No kernel runs."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vae_bf16_oracle as BO  # noqa: E402
import vae_wide_oracle as O  # noqa: E402

CS_COMP = dict(time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)


def smallest_case(kind, gen):
    """The operands (unrounded fp32 on the CPU) of the smallest Gaussian case of a stage in tests/test_vae_bf16_gpu.py: 72 channels,
    g = 1, a 5x7 plane, T = 2, B = 2 for the convs; 128 channels for up and down; 512 -> 8 for out."""
    r = lambda *s: torch.randn(*s, generator=gen)
    if kind == "conv_a":
        C, g = 72, 1
        return r(2, g + 2, 5, 7, C), r(C * g, C, 2 * g, 3, 3) / (C * 2 * g * 9) ** 0.5, 0.1 * r(C * g), g
    if kind == "conv_b":
        C = 72
        return r(2, 2, 5, 7, C), r(2, 2, 5, 7, C), r(C, C, 1, 3, 3) / (C * 9) ** 0.5, 0.1 * r(C)
    if kind == "up":
        C, tc, sc = 128, 2, 2
        return r(2, 2, 5, 7, C), r(C * tc * sc * sc, C, 1, 1, 1) / C ** 0.5, 0.1 * r(C * tc * sc * sc), tc, sc
    if kind == "out":
        return r(2, 2, 5, 7, 512), r(8, 512, 1, 1, 1) / 512 ** 0.5, 0.1 * r(8)
    Cin, tc, sc, C = 128, 2, 2, 512
    return r(2, 2 * tc, 5 * sc, 7 * sc, Cin), r(C, Cin * tc * sc * sc, 1, 1, 1) / (Cin * tc * sc * sc) ** 0.5, 0.1 * r(C), tc, sc


@pytest.mark.parametrize("kind", ["conv_a", "conv_b", "up", "out", "down"])
def test_the_comparator_can_tell(kind):
    """The faithful oracle is inside its own bound (trivially: distance 0, and the float32 evaluation within a fifth of it); every
    defective oracle is outside.  `residual_rounded` is defined for the stages that add a term from the input (conv B, out, down)."""
    args = smallest_case(kind, torch.Generator().manual_seed(7100))
    ref, bnd, f32 = BO.bound(kind, *args)
    assert bnd[0] >= BO.FLOOR and f32[0] < 1e-5, (bnd, f32)                 # the float32 evaluation is a float32-level distance away
    assert not BO.outside(ref, ref, bnd)[1]
    for defect in BO.DEFECTS:
        if defect == "residual_rounded" and kind not in BO.HAS_RESIDUAL:
            assert torch.equal(BO.stage(kind, *args, defect=defect), ref)
            continue
        m, bad = BO.outside(BO.stage(kind, *args, defect=defect), ref, bnd)
        print(f"vae_bf16: defect {kind} {defect} rel={m[0]:.3g} max/rms={m[1]:.3g} bound=({bnd[0]:.3g}, {bnd[1]:.3g})")
        assert bad, (kind, defect, m, bnd)
    # the rounding is visible: the faithful oracle is farther than 1e-4 from the unrounded one (item 3 of the GPU tests)
    unrounded = dict(conv_a=O.conv_a, conv_b=O.conv_b, up=O.up, out=O.out)
    if kind in unrounded:
        assert O.rel_l2(ref, unrounded[kind](*args)) > 1e-4


def test_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20, 1.0 + 3 * 2 ** -8, -1.0 - 2 ** -8 - 2 ** -20, 3.0, -2.0])
    assert BO.rne(x).tolist() == [1.0, 1.0, 1.0 + 2 ** -7, 1.0 + 2 ** -6, -1.0 - 2 ** -7, 3.0, -2.0]      # ties to even
    assert BO.trunc(x).tolist() == [1.0, 1.0, 1.0, 1.0 + 2 ** -7, -1.0, 3.0, -2.0]


def test_the_switch_is_a_plain_attribute(tmp_path):
    from autoregressive_diffusion_amd.vae import VAE, VAE512
    kw = dict(channels=[3, 16, 96, 160, 8], n_res_blocks=1, **CS_COMP)
    for cls in (VAE, VAE512):
        vae = O.seed_params(cls(**kw), 3)
        assert vae._bf16_inference is False                          # off as constructed
        sd, kwargs = {k: v.clone() for k, v in vae.state_dict().items()}, copy.deepcopy(vae.kwargs)
        assert vae.bf16_inference() is vae and vae._bf16_inference is True
        assert copy.deepcopy(vae)._bf16_inference is True
        assert vae.kwargs == kwargs and list(vae.state_dict()) == list(sd)
        assert all(torch.equal(sd[k], v) for k, v in vae.state_dict().items())
        assert "bf16" not in str(vae.kwargs) and not any("bf16" in k for k in vae.state_dict())
        path = str(tmp_path / f"{cls.__name__}.pt")
        vae.save_to_state_dict(path)
        assert cls.from_pretrained(path)._bf16_inference is False    # a checkpoint does not carry it
        assert vae.bf16_inference(False) is vae and vae._bf16_inference is False
    narrow = VAE(channels=[3, 8, 8], n_res_blocks=1, time_compressions=[1, 2], spatial_compressions=[1, 2])
    dev = torch.device("cpu")
    before = narrow._pack(dev)
    assert narrow.bf16_inference() is narrow                         # accepted on a model without a wide block ...
    after = narrow._pack(dev)
    assert all("bf16" not in bk and all("bf16" not in rb for rb in bk["res"]) for bk in after["blocks"])      # ... and changes nothing
    assert all(torch.equal(a["wu"], b["wu"]) and a["wu"].dtype == torch.float32 for a, b in zip(before["blocks"], after["blocks"]))


def test_the_switch_is_part_of_the_pack_signature():
    from autoregressive_diffusion_amd.vae import VAE
    vae = O.seed_params(VAE(channels=[3, 16, 96, 8], n_res_blocks=1, time_compressions=[1, 2, 2], spatial_compressions=[1, 2, 2]), 4)
    dev = torch.device("cpu")
    p0, e0 = vae._pack(dev), vae._pack_encoder(dev)
    assert vae._pack(dev) is p0 and vae._pack_encoder(dev) is e0
    vae.bf16_inference()
    p1, e1 = vae._pack(dev), vae._pack_encoder(dev)
    assert p1 is not p0 and e1 is not e0 and vae._pack(dev) is p1 and vae._pack_encoder(dev) is e1
    narrow, wide = p1["blocks"][0], p1["blocks"][1]
    assert not narrow["wide"] and "bf16" not in narrow and narrow["wu"].dtype == torch.float32
    assert wide["wide"] and wide["bf16"] and wide["res"][0]["bf16"]
    assert {wide[k].dtype for k in ("wu", "wo")} | {wide["res"][0][k].dtype for k in ("wa", "wb")} == {torch.bfloat16}    # no fp32 copy kept
    assert {wide[k].dtype for k in ("bu", "bo")} | {wide["res"][0][k].dtype for k in ("ba", "bb")} == {torch.float32}
    enc = e1["blocks"]
    # block 2 is narrow (8 channels) but compresses K = 768 > MAX_DOWN_K channels: its `down` is the GEMM, an MFMA launch
    assert [bool(b.get("bf16")) for b in enc] == [False, True, True] and enc[1]["wd"].dtype == enc[2]["wd"].dtype == torch.bfloat16
    assert enc[0]["wd"].dtype == torch.float32 and not enc[2].get("wide") and enc[2]["res"][0]["wa"].dtype == torch.float32
    # the training path asks for fp32 packs whatever the switch says
    assert "bf16" not in vae._pack(dev, bf16=False)["blocks"][1] and vae._pack(dev, bf16=False)["blocks"][1]["wu"].dtype == torch.float32
    vae.bf16_inference(False)
    p2 = vae._pack(dev)
    assert p2 is not p1 and "bf16" not in p2["blocks"][1] and all(torch.equal(p2["blocks"][1][k], p0["blocks"][1][k]) for k in ("wu", "wo"))


@pytest.mark.parametrize("C,g", [(72, 2), (512, 1)], ids=["72", "512"])
def test_packed_bf16_weights(C, g):
    """Every packed weight equals weight.to(torch.bfloat16) at its place in the documented layout [tap][CinP][nsub CP], CinP = C
    rounded up to a multiple of 16, CP to a multiple of 32, zero where padded; the biases are the fp32 ones."""
    from autoregressive_diffusion_amd import vae as V
    gen = torch.Generator().manual_seed(7200 + C)
    rb = V.ResBlock(C, (2 * g, 3, 3), g)
    with torch.no_grad():
        for p in rb.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
    CP, CinP = -(-C // 32) * 32, -(-C // 16) * 16
    assert (CP, CinP) == ((96, 80) if C == 72 else (512, 512))
    pk, ref = V._pack_res_wide(rb, C, g, CPU, bf16=True), V._pack_res_wide(rb, C, g, CPU)
    assert pk["bf16"] is True and "bf16" not in ref
    assert pk["wa"].dtype == pk["wb"].dtype == torch.bfloat16 and pk["wa"].is_contiguous() and pk["wb"].is_contiguous()
    assert tuple(pk["wa"].shape) == (2 * g, 3, 3, CinP, g, CP) and tuple(pk["wb"].shape) == (3, 3, CinP, CP)
    wa = rb.conv3d0.conv3d.weight.detach().to(torch.bfloat16).reshape(C, g, C, 2 * g, 3, 3).permute(3, 4, 5, 2, 1, 0)      # kt, ky, kx, ci, gl, c
    assert torch.equal(pk["wa"][:, :, :, :C, :, :C], wa)
    wb = rb.conv3d1.weight.detach().to(torch.bfloat16)[:, :, 0].permute(2, 3, 1, 0)                                         # ky, kx, ci, co
    assert torch.equal(pk["wb"][:, :, :C, :C], wb)
    for w in (pk["wa"], pk["wb"]):
        assert w[..., C:].float().abs().max() == 0 if CP > C else True
    assert pk["wa"][:, :, :, C:].float().abs().sum() == 0 and pk["wb"][:, :, C:].float().abs().sum() == 0
    assert torch.equal(pk["ba"], ref["ba"]) and torch.equal(pk["bb"], ref["bb"]) and pk["ba"].dtype == torch.float32
    # the 1x1 stages
    npos = 4
    wu, bu = torch.randn(C * npos, C, 1, 1, 1, generator=gen), torch.randn(C * npos, generator=gen)
    w, b = V._pack_lin_wide(wu, bu, C, C, npos, CPU, bf16=True)
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (CinP, npos, CP) and b.dtype == torch.float32
    assert torch.equal(w[:C, :, :C], wu.to(torch.bfloat16).reshape(npos, C, C).permute(2, 0, 1)) and w[C:].float().abs().sum() == 0
    assert torch.equal(b, V._pack_lin_wide(wu, bu, C, C, npos, CPU)[1])
    wo, bo = torch.randn(6, C, 1, 1, 1, generator=gen), torch.randn(6, generator=gen)
    w, b = V._pack_lin_wide(wo, bo, C, 6, 1, CPU, bf16=True)
    assert tuple(w.shape) == (CinP, 1, 32) and torch.equal(w[:C, 0, :6], wo.to(torch.bfloat16).reshape(6, C).t()) and w[:, :, 6:].float().abs().sum() == 0
    wd, bd = torch.randn(C, 24 * npos, 1, 1, 1, generator=gen), torch.randn(C, generator=gen)
    w, b = V._pack_down_wide(wd, bd, 24, C, npos, CPU, bf16=True)
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (npos, 32, CP) and tuple(b.shape) == (CP,)
    assert torch.equal(w[:, :24, :C], wd.to(torch.bfloat16).reshape(C, npos, 24).permute(1, 2, 0)) and w[:, 24:].float().abs().sum() == 0


def test_entry_points_are_bound():
    from autoregressive_diffusion_amd import _lib, vae as V
    for stage in ("conv_a", "conv_b", "up", "out", "down"):
        name = f"oniris_vae_wide_{stage}_bf16"
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
        fn, sibling = getattr(_lib.lib, name), getattr(_lib.lib, f"oniris_vae_wide_{stage}")
        assert fn.argtypes == sibling.argtypes and fn.restype == sibling.restype      # the sibling's signature
        assert V._wide_entry(stage, dict(bf16=True))[1] == f"vae_wide_{stage}_bf16" and V._wide_entry(stage, {})[1] == f"vae_wide_{stage}"
    assert _lib.lib.oniris_abi_version() == 14


def test_whole_model_oracle_rounds_only_in_wide_blocks():
    """A model without a wide block: the faithful oracle is the unrounded one, bit for bit.  With one: the two differ at the bf16
    level (the E of the GPU test, here below 2e-2)."""
    from autoregressive_diffusion_amd.vae import VAE
    import vae_wide_encoder_oracle as E
    gen = torch.Generator().manual_seed(7300)
    for channels, wide in (([3, 8, 16, 4], False), ([3, 16, 72, 4], True)):
        kw = dict(channels=channels, n_res_blocks=1, time_compressions=[1, 2, 2], spatial_compressions=[1, 2, 2])
        sd = O.seed_params(VAE(**kw), 9).state_dict()
        z, x, t = torch.randn(1, 4, 2, 2, 3, generator=gen), torch.rand(1, 3, 8, 8, 12, generator=gen) * 2 - 1, torch.tensor([0.07])
        for got, ref in ((BO.decode(sd, kw, z, t)[0], O.decode(sd, kw, z, t)[0]), (BO.encode(sd, kw, x)[0], E.encode(sd, kw, x)[0])):
            e = O.rel_l2(got, ref)
            assert (1e-4 < e < 2e-2) if wide else torch.equal(got, ref), (channels, e)
        assert torch.equal(BO.decode(sd, kw, z, t, faithful=False)[0], O.decode(sd, kw, z, t)[0])

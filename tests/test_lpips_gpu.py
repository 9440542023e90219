"""The native LPIPS (autoregressive_diffusion_amd/lpips.py, csrc/lpips.hip, csrc/lpips_conv.h) on the GPU: every kernel stage against
float64, the whole net against the float64 restatement (tests/lpips_cpu_restatement.py), bit-for-bit self-consistency, and one VAE
training step with the perceptual term in its loss.  Weights are seeded, not pretrained (R.seeded_weights).

Bounds.  u = 2^-24.
 * Convs and their data gradients: the element bound (K + 4) u sum|terms| that tests/test_discriminator_gpu.py derives for its conv
   stages (a sum of K products and addends in fp32 with fused multiply-adds in any order; + 4 for the roundings of a prologue and an
   epilogue: here (x - shift) / scale in front of the stem, / scale behind its gradient, + add in the gradient epilogue).  K = taps Cin
   + 1 forward, taps Cout + 1 for a gradient (the stem's gradient: at most 9 x 64 terms + 1).  The oracle forms sum|terms| in float64
   from the same fp32 operands.
 * Outputs behind a ReLU: ReLU is 1-Lipschitz, |relu(a) - relu(b)| <= |a - b|, so the bound of the pre-activation holds for the
   output at EVERY element, also where the float64 pre-activation is nearer to 0 than the bound and the two signs may differ.
   Nothing is left out (the share left out is 0 < 1e-3); the share of such elements is printed for information (1.6e-3 .. 2.6e-3 at
   K = 1601 .. 3457 with these operands: the bound grows with K).  The mask of a data gradient comes from the saved feature map
   the kernel is handed, so nothing is uncertain there either.
 * The pool forward is exact (a maximum); its adjoint adds at most four numbers (+ add): K = 5.
 * Heads and the whole net: the project's margin rule rel L2 <= max(5e-5, 4 ref32_rel) (disc_cpu_restatement.margin), ref32_rel the
   float32 restatement's own error against float64 on the CPU, computed here.
Every compared figure is printed (pytest -s); profiles/lpips_tests.txt is that output."""
import functools

import pytest
import torch
from torch.nn import functional as F

import disc_cpu_restatement as DR
import lpips_cpu_restatement as R

DEV = "cuda"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SEED = 3


def L():
    from autoregressive_diffusion_amd import lpips
    return lpips


def cl(t):
    return t.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).double().cpu()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def check_elements(what, got, want, mag, K, pre=None):
    """|got - want| <= (K + 4) u mag at EVERY element.  `pre` = the float64 pre-activation of a ReLU output: the share of elements
    whose pre-activation is nearer to 0 than the bound is printed, and none of them is left out (see the module docstring)."""
    assert tuple(got.shape) == tuple(want.shape), what
    err = (got - want).abs()
    bound = (K + 4) * U * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    near = "" if pre is None else f", {(pre.abs() <= bound).double().mean().item():.2e} of the pre-activations within the bound of 0"
    print(f"{what}: worst |err| / bound = {ratio:.3f} (K = {K}, max |err| {err.max().item():.2e}, left out 0{near})")
    assert bool((err <= bound).all()), what


def check_margin(what, got, want, ref32):
    e, m = DR.rel(got, want), DR.margin(ref32)
    print(f"{what}: rel L2 {e:.2e} (reference float32 {float(ref32):.2e}, bound {m:.2e})")
    assert tuple(got.shape) == tuple(want.shape), what
    assert e <= m, (what, e, m)


@functools.lru_cache(maxsize=None)
def weights():
    return R.seeded_weights(SEED)


@functools.lru_cache(maxsize=None)
def module():
    return L().LPIPS(net="alex", weights=weights()).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# stages

@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 67, 45), (1, 35, 75)], ids=lambda s: "x".join(map(str, s)))
def test_stem_stage(shape):
    """Scaling + 11x11 stride-4 conv + bias + ReLU from two operands, and its data gradient into (N, 3, H, W).  (1, 35, 75) has 18
    output columns: two tiles across, which neither of the other shapes has."""
    lp, sd = L(), weights()
    N, H, W = shape
    a, b = R.images(shape, 11)
    w, bias = sd["net.slice1.0.weight"], sd["net.slice1.0.bias"]
    shift, scale = torch.tensor(R.SHIFT).to(DEV), torch.tensor(R.SCALE).to(DEV)
    f1 = lp.stem(a.to(DEV), b.to(DEV), shift, scale, lp.pack_stem(w.to(DEV)), bias.to(DEV))
    pre, mag = R.stem_terms(torch.cat([a, b]), w, bias)
    check_elements(f"stem {shape}", nchw(f1), F.relu(pre), mag, 364, pre=pre)
    g = torch.randn(2 * N, 64, pre.shape[2], pre.shape[3], generator=gen(12))
    like = torch.empty(2 * N, 3, H, W, device=DEV)
    dx = lp.stem_dgrad(cl(g), lp.pack_stem_dgrad(w.to(DEV)), scale, like)
    want, mag = R.stem_dgrad_terms(g, w, H, W)
    check_elements(f"stem dgrad {shape}", dx.double().cpu(), want, mag, 9 * 64 + 1)
    dn = lp.stem_dgrad(cl(g), lp.pack_stem_dgrad(w.to(DEV)), scale, like, normalize=True)
    assert torch.equal(dn, 2 * dx)


# (ksize, Cin, Cout, (NI, H, W))
CONV_CASES = [(5, 64, 192, (2, 7, 5)), (5, 64, 192, (2, 16, 10)), (3, 192, 384, (3, 3, 1)), (3, 192, 384, (2, 15, 15)),
              (3, 384, 256, (3, 3, 1)), (3, 384, 256, (2, 15, 15))]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"k{c[0]}_{c[1]}to{c[2]}_" + "x".join(map(str, c[3])))
def test_conv_stage(case):
    """relu(conv + bias) and the data gradient (conv^T(dy) + add) * (f > 0), with and without add / f, in both tilings of the
    kernel (256 and 64 pixels per workgroup): each against float64, and the same bits."""
    lp = L()
    k, Cin, Cout, (NI, H, W) = case
    g = gen(100 + k + Cin + H)
    x = torch.randn(NI, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    dy, add, f = torch.randn(NI, Cout, H, W, generator=g), torch.randn(NI, Cin, H, W, generator=g), torch.randn(NI, Cin, H, W, generator=g)
    pre, mag = DR.conv_terms(x.double(), w.double(), b.double())
    wp, wd = lp.pack_conv(w.to(DEV)), lp.pack_conv_dgrad(w.to(DEV))
    want, dmag = DR.dgrad_terms(dy.double(), w.double())
    outs = {}
    for tile in (256, 64):          # both tilings of the kernel against float64; 0 = the library's choice (64 at these sizes)
        out = lp.conv(cl(x), wp, b.to(DEV), k, tile=tile)
        check_elements(f"conv {case} tile {tile}", nchw(out), F.relu(pre), mag, k * k * Cin + 1, pre=pre)
        plain = lp.conv_dgrad(cl(dy), wd, k, tile=tile)
        check_elements(f"dgrad {case} tile {tile}", nchw(plain), want, dmag, k * k * Cout + 1)
        got = lp.conv_dgrad(cl(dy), wd, k, add=cl(add), f=cl(f), tile=tile)
        check_elements(f"dgrad {case} tile {tile} + add, masked", nchw(got), (want + add.double()) * (f > 0), dmag + add.double().abs(),
                       k * k * Cout + 1)
        buf = cl(add)
        assert lp.conv_dgrad(cl(dy), wd, k, add=buf, f=cl(f), out=buf, tile=tile) is buf and torch.equal(buf, got)      # in place
        outs[tile] = (out, plain, got)
    assert all(torch.equal(p, q) for p, q in zip(outs[256], outs[64]))
    assert torch.equal(lp.conv(cl(x), wp, b.to(DEV), k), outs[64][0])


@pytest.mark.parametrize("hw", [(7, 7), (16, 10)], ids=lambda s: "x".join(map(str, s)))
def test_pool_stage(hw):
    """7 -> 3 and 16 x 10 -> 7 x 4: the forward bit for bit, the gather adjoint (+ add, ReLU mask) at K = 5."""
    lp = L()
    H, W = hw
    g = gen(200 + H)
    x = torch.randn(2, 64, H, W, generator=g)
    out = lp.pool(cl(x))
    want = F.max_pool2d(x, 3, 2)
    assert tuple(out.shape) == (2, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 64)
    assert torch.equal(out.permute(0, 3, 1, 2).cpu(), want)
    dp, add = torch.randn(want.shape, generator=g), torch.randn(x.shape, generator=g)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2).backward(dp.double())
    xa = x.double().requires_grad_(True)
    F.max_pool2d(xa, 3, 2).backward(dp.double().abs())
    check_elements(f"pool adjoint {hw}", nchw(lp.pool_bwd(cl(dp), cl(x))), x64.grad, xa.grad + 1e-300, 5)
    got = lp.pool_bwd(cl(dp), cl(x), add=cl(add), mask=True)
    check_elements(f"pool adjoint {hw} + add, masked", nchw(got), (x64.grad + add.double()) * (x > 0), xa.grad + add.double().abs(), 5)


@pytest.mark.parametrize("case", [(64, 7, 7), (192, 9, 8), (384, 3, 1), (256, 3, 3)], ids=lambda s: "x".join(map(str, s)))
def test_head_stage(case):
    """One layer's value and d f for both operands against float64, an all-zero pixel planted in each operand: its gradient is
    exactly zero and everything stays finite.  (192, 9, 8) has 72 pixels: two chunks of partial sums."""
    lp = L()
    C, h, w = case
    N = 2
    g = gen(300 + C)
    fa, fb = F.relu(torch.randn(N, C, h, w, generator=g)), F.relu(torch.randn(N, C, h, w, generator=g))
    fa[0, :, h // 2, 0] = 0
    fb[1, :, 0, w - 1] = 0
    wt, c = torch.rand(1, C, 1, 1, generator=g), R.cot(N, 5)

    def ref(dtype):
        a, b = fa.to(dtype).requires_grad_(True), fb.to(dtype).requires_grad_(True)
        v = R.head(a, b, wt.to(dtype))
        (v * c.to(dtype)).sum().backward()
        return v.detach(), a.grad, b.grad
    want, o32 = ref(torch.float64), ref(torch.float32)
    assert all(bool(torch.isfinite(t).all()) for t in want)
    f = torch.cat([cl(fa), cl(fb)])
    wv = wt.flatten().to(DEV)
    val = lp.heads([f], [wv], N)
    check_margin(f"head {case} value", val.cpu().view(N, 1, 1, 1), want[0], DR.rel(o32[0], want[0]))
    gr = lp.head_bwd(f, wv, c.flatten().to(DEV), True, True)
    assert bool(torch.isfinite(gr).all())
    check_margin(f"head {case} d f0", nchw(gr[:N]), want[1], DR.rel(o32[1], want[1]))
    check_margin(f"head {case} d f1", nchw(gr[N:]), want[2], DR.rel(o32[2], want[2]))
    assert not bool(gr[0, h // 2, 0].any()) and not bool(gr[N + 1, 0, w - 1].any()) and bool(gr[0, 0, 0].any())
    assert torch.equal(lp.head_bwd(f, wv, c.flatten().to(DEV), True, False), gr[:N])
    assert torch.equal(lp.head_bwd(f, wv, c.flatten().to(DEV), False, True), gr[N:])
    assert torch.equal(lp.head_bwd(f, wv, c.flatten().to(DEV), True, True, mask=True), gr * (f > 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole net

NET_SHAPES = [(3, 32, 32), (2, 67, 45), (2, 31, 64), (4, 64, 64)]


@functools.lru_cache(maxsize=None)
def reference(shape):
    a, b = R.images(shape, 21)
    c = R.cot(shape[0], 1)
    return a, b, c, R.run(weights(), a, b, torch.float64, c), R.run(weights(), a, b, torch.float32, c)


def native(a, b, c, grad0=True, grad1=True, normalize=False):
    x, y = a.detach().to(DEV).requires_grad_(grad0), b.detach().to(DEV).requires_grad_(grad1)
    out = module()(x, y, normalize=normalize)
    assert out.dtype == torch.float32 and tuple(out.shape) == (a.shape[0], 1, 1, 1)
    if grad0 or grad1:
        (out * c.to(DEV)).sum().backward()
    return dict(value=out.detach(), d_in0=x.grad, d_in1=y.grad)


@pytest.mark.parametrize("shape", NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_net(shape):
    """Values, d in0 and d in1 against the float64 restatement by the margin rule."""
    a, b, c, want, o32 = reference(shape)
    got = native(a, b, c)
    for k in ("value", "d_in0", "d_in1"):
        check_margin(f"net {shape} {k}", got[k].cpu(), want[k], DR.rel(o32[k], want[k]))
    # normalize=True is the call on 2 x - 1 (one rounding either way: the same bits), its gradients twice as large
    ha, hb = (a + 1) / 2, (b + 1) / 2
    half, full = native(ha, hb, c, normalize=True), native(2 * ha - 1, 2 * hb - 1, c)
    assert torch.equal(half["value"], full["value"])
    assert torch.equal(half["d_in0"], 2 * full["d_in0"]) and torch.equal(half["d_in1"], 2 * full["d_in1"])


def test_whole_net_at_frame_size():
    """One pair of 256 x 256 frames, the size the training scripts run: 4 x 8 stem tiles, 8 x 8 tiles of the stem's gradient, every
    M tile of the convs full.  The same comparison as test_whole_net."""
    shape = (1, 256, 256)
    a, b, c, want, o32 = reference(shape)
    got = native(a, b, c)
    for k in ("value", "d_in0", "d_in1"):
        check_margin(f"net {shape} {k}", got[k].cpu(), want[k], DR.rel(o32[k], want[k]))


@pytest.mark.selfcheck
def test_two_runs_and_each_image_alone_give_the_same_bits():
    for shape in ((4, 64, 64), (2, 67, 45)):
        a, b, c, _, _ = reference(shape)
        one, two = native(a, b, c), native(a, b, c)
        for k in one:
            assert torch.equal(one[k], two[k]), (shape, k)
        for i in range(shape[0]):
            alone = native(a[i:i + 1], b[i:i + 1], c[i:i + 1])
            for k in one:
                assert torch.equal(alone[k], one[k][i:i + 1]), (shape, i, k)


@pytest.mark.selfcheck
def test_a_batch_on_the_large_tiles_gives_the_bits_of_its_images_alone():
    """12 pairs of 256 x 256 frames: conv2 is 24 x 961 pixels x 3 column blocks = 273 tiles of 256, so its forward runs on
    256-pixel tiles, everything else on 64-pixel ones; one pair alone runs everything on 64-pixel tiles (the net of test_whole_net_at_frame_size,
    which is held to float64).  Values and gradients of pairs 0 and 11 are the same bits either way."""
    a, b = R.images((12, 256, 256), 31)
    c = R.cot(12, 2)
    batch = native(a, b, c)
    for i in (0, 11):
        alone = native(a[i:i + 1], b[i:i + 1], c[i:i + 1])
        for k in batch:
            assert torch.equal(alone[k], batch[k][i:i + 1]), (i, k)


@pytest.mark.selfcheck
def test_strided_views_are_read_in_place():
    """The two layouts the training scripts hand over -- the (b t) c h w view of a (B, C, T, H, W) r_mean and of frames stored
    (b, t, h, w, c) -- give the bits of their contiguous copies, and each gradient has its operand's strides."""
    shape = (2, 67, 45)
    a, b, c, _, _ = reference(shape)
    base = native(a, b, c)
    r_mean = a.to(DEV).permute(1, 0, 2, 3).contiguous()[None]                      # (1, C, T, H, W)
    frames = b.to(DEV).permute(0, 2, 3, 1).contiguous()[None]                       # stored (1, T, H, W, C)
    x = r_mean.permute(0, 2, 1, 3, 4).reshape(-1, 3, shape[1], shape[2])
    y = frames.permute(0, 4, 1, 2, 3).permute(0, 2, 1, 3, 4).reshape(-1, 3, shape[1], shape[2])
    assert x.data_ptr() == r_mean.data_ptr() and y.data_ptr() == frames.data_ptr()
    assert not x.is_contiguous() and not y.is_contiguous()
    x.requires_grad_(True)
    y.requires_grad_(True)
    out = module()(x, y)
    (out * c.to(DEV)).sum().backward()
    assert torch.equal(out, base["value"]) and torch.equal(x.grad, base["d_in0"]) and torch.equal(y.grad, base["d_in1"])
    assert x.grad.stride() == x.stride() and y.grad.stride() == y.stride()


@pytest.mark.selfcheck
def test_one_sided_gradients():
    """Only in1 (or only in0) requiring grad gives the bits of the run where both do; neither gives an output off the graph."""
    shape = (2, 31, 64)
    a, b, c, _, _ = reference(shape)
    both = native(a, b, c)
    only1, only0 = native(a, b, c, grad0=False), native(a, b, c, grad1=False)
    assert only1["d_in0"] is None and torch.equal(only1["d_in1"], both["d_in1"]) and torch.equal(only1["value"], both["value"])
    assert only0["d_in1"] is None and torch.equal(only0["d_in0"], both["d_in0"])
    assert not module()(a.to(DEV), b.to(DEV)).requires_grad


def test_in_the_training_loop():
    """VAE([3, 8, 8, 8], 1 ResBlock) on frames (1, 3, 4, 32, 32): GaussianLoss + 0.1 log(lpips + 1e-8).mean() backward, as
    cs_vae_train.py:109-125 forms it.  Every VAE gradient is finite and within the margin rule's 5e-5 of the same step with the
    module's torch formula forced on the same GPU tensors."""
    from autoregressive_diffusion_amd import vae_losses as V
    from autoregressive_diffusion_amd.vae import VAE
    from test_vae_train_gpu import seed_params
    vae = seed_params(VAE(channels=[3, 8, 8, 8], n_res_blocks=1), 1701).to(DEV).train()
    g = gen(1702)
    frames = (torch.rand(1, 3, 4, 32, 32, generator=g) * 2 - 1).to(DEV)
    ts, noise = (torch.rand(1, generator=g) * 0.1).to(DEV), torch.randn(1, 8, 1, 8, 8, generator=g).to(DEV)
    m = module()
    flat = lambda t: t.permute(0, 2, 1, 3, 4).reshape(-1, 3, 32, 32).clip(-1, 1)
    grads, losses = [], []
    for fn in (m, m.forward_torch):
        vae.zero_grad(set_to_none=True)
        r_mean, r_logvar, _, _ = vae(frames, t_sample=ts, noise=noise)
        lp = fn(flat(r_mean), flat(frames))
        loss = V.GaussianLoss(r_mean, r_logvar, frames) + 0.1 * torch.log(lp + 1e-8).mean()
        loss.backward()
        losses.append(loss.item())
        grads.append({n: p.grad.clone() for n, p in vae.named_parameters() if p.grad is not None})
    assert grads[0] and set(grads[0]) == set(grads[1])
    print(f"loss native {losses[0]:.8f} torch formula {losses[1]:.8f}")
    errs = {n: DR.rel(grads[0][n], grads[1][n]) for n in grads[0]}
    for n in sorted(errs, key=errs.get, reverse=True)[:8]:
        print(f"grad {n}: rel L2 native vs torch formula {errs[n]:.2e} (bound {DR.margin(0):.2e})")
    assert all(bool(torch.isfinite(v).all()) for v in grads[0].values())
    assert max(errs.values()) <= DR.margin(0), max(errs.values())

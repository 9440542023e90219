"""The native Discriminator3D (autoregressive_diffusion_amd/discriminator.py, csrc/disc3d.hip, csrc/disc_conv3d.h,
csrc/disc_parts.h) on the GPU: every kernel stage element by element against the float64 expectations (tests/disc3d_cpu_restatement.py), whole nets against the
reference's fixture G20 and against the float64 restatement, the all-native MixedDiscriminator against G19 with torch's conv3d and
group_norm replaced by functions that raise, determinism and the frozen-critic step.

Bounds (those of tests/test_discriminator_gpu.py).  u = 2^-24 is the unit roundoff of fp32.
 * Element bounds (K + 4) u sum|terms|: a sum of K products (and addends) in fp32 with fused multiply-adds, in ANY order, differs from
   the exact sum by at most gamma_K sum|a_i b_i|, gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability, sec. 3.1: each term
   passes through at most K roundings).  For a conv K = taps Cin + 1 (the bias); for a data gradient K = (contributing (output
   position, tap) pairs) Cout, 27 Cout at stride 1 and counted per element at stride 2.  The prologue a = lrelu(x s + t) adds two
   roundings to each operand (the fma and the 0.2 multiply), the residual epilogue two more (the add and the scale), which only
   ever act on quantities bounded by sum|terms|: + 4.  The oracle forms sum|terms| in float64 from the same fp32 inputs.  One missing
   or misplaced tap changes an element by about sum|terms| / taps: orders of magnitude above the bound.  The blur pool has K = 26
   (27 fused products; the prologue's two roundings are in the + 4).
 * GroupNorm + LeakyReLU backward, dx = rstd (gamma dz - m1 - xhat m2) + add_scale add with m1, m2 the group means of gamma dz and
   gamma dz xhat: sum|terms| = rstd (|gamma dz| + mean_g |gamma dz| + |xhat| mean_g |gamma dz xhat|) + |add_scale add|, the two
   means entering by the means of the MAGNITUDES of their terms, which is what their own rounding errors are proportional to.
   K = 160 counts the roundings one term of such a mean passes through: 3 to form it (0.2 da, z - mean, . rstd), at most 128 in its
   thread's running sum (1024 positions per workgroup in 8 runs), 8 across the runs, 1 + 8 across workgroups (strided, then a
   tree of 256), at most 8 over the channels of a group (fma by gamma), 1 for 1 / count, and 9 in the element's own expression:
   158, rounded up.  At the shapes below a wrong statistic or a neighbour's group mean moves dx by about sum|terms| itself.
 * Statistics (the 2-D test's bounds): mean 4 u (|mean| + std); biased variance 8 u relative; s = gamma rstd 8 u relative; t = beta
   - mean s 16 u of the sum of the magnitudes of its terms.
 * Margin rule for relative comparisons without an element bound: rel L2 <= max(5e-5, 4 ref32_rel), ref32_rel the reference's own
   float32 run against its float64 run (from the fixture; where there is none, the restatement's float32 run on the CPU, computed
   here) -- never the code under test.
Every compared figure is printed (pytest -s); profiles/discriminator3d_tests.txt is that output."""
import math

import numpy as np
import pytest
import torch

import disc_paramgen as G
import disc3d_paramgen as G3
import disc_cpu_restatement as R
import disc3d_cpu_restatement as R3

DEV = "cuda"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
K_GN = 160


def D():
    from autoregressive_diffusion_amd import discriminator
    return discriminator


def cl(t):
    """NCTHW (any dtype, CPU) -> channels-last fp32 (N, T, H, W, C) on the GPU."""
    return t.float().permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def ncthw(t):
    return t.detach().permute(0, 4, 1, 2, 3).double().cpu()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def check_elements(what, got, want, mag, K):
    """|got - want| <= (K + 4) u mag element by element (K a number or a tensor); prints the worst ratio."""
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    err = (got - want).abs()
    bound = (K + 4) * U * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    kmax = int(K.max()) if torch.is_tensor(K) else K
    print(f"{what}: worst |err| / bound = {ratio:.3f} (K = {kmax}, max |err| {err.max().item():.2e})")
    assert bool((err <= bound).all()), what


def check_margin(what, got, want, ref32):
    e, m = R.rel(got, want), R.margin(ref32)
    print(f"{what}: rel L2 {e:.2e} (reference float32 {float(ref32):.2e}, bound {m:.2e})")
    assert e <= m, (what, e, m)


def ident(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


# (N, T, H, W, Cin, Cout, taps)
CONV_SHAPES = [(2, 1, 7, 5, 32, 32, 27), (1, 3, 18, 20, 32, 64, 27), (2, 4, 9, 11, 96, 32, 27), (2, 2, 8, 8, 64, 2, 27),
               (2, 3, 6, 10, 32, 64, 1)]
# (N, T, H, W, Cin, Cout): the stem, stride 2
STEM_SHAPES = [(2, 1, 7, 5, 3, 32), (2, 5, 18, 22, 6, 32), (3, 2, 33, 17, 8, 64), (1, 4, 4, 4, 1, 32)]


def sign(shape, g):
    return torch.where(torch.rand(shape, generator=g) > 0.5, 1.0, -1.0)


def conv_case(shape, stride=1, seed=0):
    """Inputs of one conv: the prologue vectors differ per sample and |t| is 2..3."""
    N, T, H, W, Cin, Cout = shape[:6]
    k = 1 if len(shape) > 6 and shape[6] == 1 else 3
    g = gen(300 + seed + Cin + Cout + T)
    o = lambda n: (n - 1) // stride + 1
    out = (N, Cout, o(T), o(H), o(W))
    return dict(x=torch.randn(N, Cin, T, H, W, generator=g), w=torch.randn(Cout, Cin, k, k, k, generator=g) / math.sqrt(k ** 3 * Cin),
                b=0.3 * torch.randn(Cout, generator=g), s=0.5 + torch.rand(N, Cin, generator=g),
                t=(2.0 + torch.rand(N, Cin, generator=g)) * sign((N, Cin), g), res=torch.randn(out, generator=g),
                dy=torch.randn(out, generator=g))


def run_conv(d, c, shape, pro=False, res=False, stats=False):
    """The forward of one CONV_SHAPES entry as the module runs it: 27 taps on oniris_disc3d_conv, 1 tap on oniris_disc_conv over the
    N T planes."""
    N, T, H, W, Cin, Cout, taps = shape
    if taps == 27:
        pr = (c["s"].to(DEV), c["t"].to(DEV)) if pro else None
        return d.conv3(cl(c["x"]), d.pack_weight3(c["w"].to(DEV)), c["b"].to(DEV), Cout, pro=pr, res=cl(c["res"]) if res else None,
                       res_scale=d._SCALE if res else 1.0, stats=stats)
    out, part = d.conv(d._planes(cl(c["x"])), d.pack_weight(c["w"][..., 0].to(DEV)), c["b"].to(DEV), Cout, 1,
                       res=d._planes(cl(c["res"])) if res else None, res_scale=d._SCALE if res else 1.0, stats=stats)
    return out.view(N, T, H, W, Cout), part


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=ident)
def test_conv_stage(shape):
    """Forward (bias) with and without the per-sample prologue, the residual epilogue and the data gradient of every shape; element
    bound (K + 4) u sum|terms|, K = taps Cin + 1 (data gradient: taps Cout + 1).  A halo filled with lrelu(t) instead of 0 shows
    at every border voxel, one sample's s, t applied to another everywhere."""
    d = D()
    N, T, H, W, Cin, Cout, taps = shape
    c = conv_case(shape)
    x64, w64, b64 = c["x"].double(), c["w"].double(), c["b"].double()
    for pro in ((False, True) if taps == 27 else (False,)):
        a64 = R3.act(x64, c["s"].double(), c["t"].double()) if pro else x64
        out, _ = run_conv(d, c, shape, pro)
        want, mag = R3.conv_terms(a64, w64, b64)
        check_elements(f"conv3d {shape} prologue={pro}", ncthw(out), want, mag, taps * Cin + 1)
        out, _ = run_conv(d, c, shape, pro, res=True)
        want, mag = R3.conv_terms(a64, w64, b64, c["res"].double(), float(np.float32(d._SCALE)))
        check_elements(f"conv3d {shape} prologue={pro} residual", ncthw(out), want, mag, taps * Cin + 1)
    if taps == 27:
        dx, _ = d.conv3(cl(c["dy"]), d.pack_weight3_dgrad(c["w"].to(DEV)), None, Cin)
    else:
        dx = d.conv(d._planes(cl(c["dy"])), d.pack_weight_dgrad(c["w"][..., 0].to(DEV)), None, Cin, 1)[0].view(N, T, H, W, Cin)
    want, mag, _ = R3.dgrad_terms(c["dy"].double(), w64, (T, H, W))
    check_elements(f"dgrad3d {shape}", ncthw(dx), want, mag, taps * Cout + 1)


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=ident)
def test_stem_stage(shape):
    """conv_in at stride 2: output extents (n - 1) // 2 + 1; forward to K = 27 Cin + 1, the gathered data gradient to K = (pairs that
    reach the element) Cout, counted per element by the transposed conv of ones."""
    d = D()
    N, T, H, W, Cin, Cout = shape
    c = conv_case(shape, stride=2)
    wp = d.pack_weight3(c["w"].to(DEV))
    out, part = d.conv3(cl(c["x"]), wp, c["b"].to(DEV), Cout, stride=2, stats=True)
    half = lambda n: (n - 1) // 2 + 1
    assert tuple(out.shape) == (N, half(T), half(H), half(W), Cout)
    assert tuple(part.shape) == (N, half(T) * -(-half(H) // 16) * -(-half(W) // 16), 4, Cout)
    want, mag = R3.conv_terms(c["x"].double(), c["w"].double(), c["b"].double(), stride=2)
    check_elements(f"stem {shape}", ncthw(out), want, mag, 27 * Cin + 1)
    dx = d.stem_dgrad3(cl(c["dy"]), wp, T, H, W, Cin)
    want, mag, pairs = R3.dgrad_terms(c["dy"].double(), c["w"].double(), (T, H, W), stride=2)
    assert 1 <= pairs.max() <= 8
    check_elements(f"stem dgrad {shape} (1..{int(pairs.max())} pairs)", ncthw(dx), want, mag, pairs * Cout)


STAT_CASES = [("conv",) + s for s in CONV_SHAPES if s[5] % 32 == 0 and s[6] == 27] + [("stem",) + s for s in STEM_SHAPES] + ["mean50"]


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda s: s if isinstance(s, str) else s[0] + "-" + ident(s[1:]))
def test_statistics(case):
    """The per-tile (count, centre, S2, S1) of what a conv or the stem stored, combined per (sample, group) by the finalize launch,
    against float64 statistics of the stored tensor itself; `mean50`: values of mean 50, std 1 through an identity conv, where
    sum x^2 - (sum x)^2 / n would lose 2500 x 2 u and the tile-centred combination does not."""
    d = D()
    g = gen(7)
    if case == "mean50":
        N, T, H, W, C = 3, 2, 17, 5, 64
        x = 50.0 + torch.randn(N, C, T, H, W, generator=g)
        w = torch.zeros(C, C, 3, 3, 3)
        w[:, :, 1, 1, 1] = torch.eye(C)
        out, part = d.conv3(cl(x), d.pack_weight3(w.to(DEV)), None, C, stats=True)
        assert torch.equal(out.cpu(), cl(x).cpu())
    elif case[0] == "conv":
        shape = case[1:]
        C = shape[5]
        out, part = run_conv(d, conv_case(shape), shape, pro=True, stats=True)
    else:
        shape = case[1:]
        C = shape[5]
        c = conv_case(shape, stride=2)
        out, part = d.conv3(cl(c["x"]), d.pack_weight3(c["w"].to(DEV)), c["b"].to(DEV), C, stride=2, stats=True)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    st = d.gn_finalize(part, gamma.to(DEV), beta.to(DEV)).double().cpu()
    assert tuple(st.shape) == (5, out.shape[0], C)
    o = ncthw(out)
    mean, var, s, t, rstd = R3.gn_vectors(o, gamma.double(), beta.double())
    std = var.sqrt()
    rows = [("mean", st[0], mean, 4 * U * (mean.abs() + std)), ("var", st[1], var, 8 * U * var), ("s", st[2], s, 8 * U * s.abs()),
            ("t", st[3], t, 16 * U * (beta.abs()[None] + (mean * s).abs() + (std * s).abs())), ("rstd", st[4], rstd, 8 * U * rstd)]
    for name, got, want, bound in rows:
        print(f"stats {case} {name}: worst |err| / bound = {((got - want).abs() / bound).max().item():.3f}")
    for name, got, want, bound in rows:
        assert bool(((got - want).abs() <= bound).all()), name


@pytest.mark.parametrize("shape", [(2, 1, 7, 5, 32), (2, 3, 9, 11, 64), (1, 2, 6, 6, 96)], ids=ident)
def test_gn_lrelu_backward(shape):
    """dx element by element at (K + 4) u sum|terms|, K = 160 as counted in the module docstring, with the add / add_scale input;
    d gamma and d beta by the margin rule, the yardstick being the float32 run of the expectation on the CPU; want_dx=False gives
    the same sums and no dx.  The kernel and the oracle read the same fp32 statistics.  Pre-activations within 1e-3 of the kink
    are moved off it: there lrelu' is a coin toss in any arithmetic."""
    d = D()
    N, T, H, W, C = shape
    g = gen(13)
    z = 0.5 + 1.5 * torch.randn(N, C, T, H, W, generator=g)
    da = torch.randn(N, C, T, H, W, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    for _ in range(3):
        mean, var, s, t, rstd = R3.gn_vectors(z.double(), gamma.double(), beta.double())
        pre = z.double() * R3._c(s) + R3._c(t)
        z = torch.where(pre.abs() < 1e-3, z + R3._c(0.02 / s).float(), z)
    st32 = torch.stack(R3.gn_vectors(z.double(), gamma.double(), beta.double())).float()
    pre = z.double() * R3._c(st32[2].double()) + R3._c(st32[3].double())
    assert float(pre.abs().min()) > 5e-4
    add = torch.randn(N, C, T, H, W, generator=g)
    dx, sums = d.gn_bwd(cl(da), cl(z), st32.to(DEV), gamma.to(DEV), cl(add), 0.5)
    mean, rstd = st32[0].double(), st32[4].double()
    want, dgamma, dbeta, mag = R3.gn_backward(da.double(), z.double(), gamma.double(), beta.double(), mean, rstd)
    check_elements(f"gn backward dx {shape}", ncthw(dx), want + 0.5 * add.double(), mag + 0.5 * add.abs().double(), K_GN)
    _, dg32, db32, _ = R3.gn_backward(da, z, gamma, beta, st32[0], st32[4])
    check_margin(f"gn backward d gamma {shape}", sums[1], dgamma, R.rel(dg32, dgamma))
    check_margin(f"gn backward d beta {shape}", sums[0], dbeta, R.rel(db32, dbeta))
    none, sums2 = d.gn_bwd(cl(da), cl(z), st32.to(DEV), gamma.to(DEV), want_dx=False)
    assert none is None and torch.equal(sums2, sums)


@pytest.mark.parametrize("thw", [(1, 7, 5), (4, 24, 40), (2, 2, 2), (1, 1, 1)], ids=ident)
def test_blur_pool(thw):
    """3-D blur pool with and without the per-sample prologue, and its transpose: (K + 4) u sum|terms| with K = 26."""
    d = D()
    T, H, W = thw
    g = gen(11)
    N, C = 2, 32
    x = torch.randn(N, C, T, H, W, generator=g)
    s = 0.5 + torch.rand(N, C, generator=g)
    t = (2.0 + torch.rand(N, C, generator=g)) * sign((N, C), g)
    half = lambda n: (n - 1) // 2 + 1
    for pro in (False, True):
        a64 = R3.act(x.double(), s.double(), t.double()) if pro else x.double()
        out = d.blur3(cl(x), (s.to(DEV), t.to(DEV)) if pro else None)
        want, mag = R3.blur(a64, terms=True)
        assert tuple(out.shape) == (N, half(T), half(H), half(W), C)
        check_elements(f"blur3d {thw} prologue={pro}", ncthw(out), want, mag, 26)
    dy = torch.randn(N, C, half(T), half(H), half(W), generator=g)
    want, mag = R3.blur_t(dy.double(), thw, terms=True)
    check_elements(f"blur3d transpose {thw}", ncthw(d.blur3_bwd(cl(dy), T, H, W)), want, mag, 26)


WGRAD_CASES = [("conv",) + s for s in CONV_SHAPES] + [("stem",) + s for s in STEM_SHAPES]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda s: s[0] + "-" + ident(s[1:]))
def test_weight_and_bias_gradient(case, monkeypatch):
    """d weight and d bias of every conv and stem shape against float64 by the margin rule (yardstick: the expectation in float32 on
    the CPU), once with one slab per work item and once with _MAX_SLABS lowered to 2 so that the work items wrap; the two runs
    agree to the same bound."""
    d = D()
    stem, shape = case[0] == "stem", case[1:]
    N, T, H, W, Cin, Cout = shape[:6]
    taps = 27 if stem else shape[6]
    stride = 2 if stem else 1
    c = conv_case(shape, stride)
    pro = taps == 27 and not stem and Cout != 2
    a64 = R3.act(c["x"].double(), c["s"].double(), c["t"].double()) if pro else c["x"].double()
    if taps == 27:
        ref = lambda a, dy: R3.wgrad(a, dy, stride)
    else:
        ref = lambda a, dy: (torch.einsum("ncthw,nothw->oc", a, dy)[:, :, None, None, None], dy.sum((0, 2, 3, 4)))
    dw64, db64 = ref(a64, c["dy"].double())
    dw32, db32 = ref(a64.float(), c["dy"])
    pr = (c["s"].to(DEV), c["t"].to(DEV)) if pro else None

    def run():
        if taps == 27:
            return d.wgrad3(cl(c["x"]), cl(c["dy"]), stride, pro=pr)
        dw, db = d.wgrad(d._planes(cl(c["x"])), d._planes(cl(c["dy"])), 1)
        return dw[..., None], db
    dw, db = run()
    assert tuple(dw.shape) == tuple(c["w"].shape)
    check_margin(f"wgrad3d {case} d weight", dw, dw64, R.rel(dw32, dw64))
    check_margin(f"wgrad3d {case} d bias", db, db64, R.rel(db32, db64))
    dw, db = dw.double().cpu(), db.double().cpu()
    monkeypatch.setattr(d, "_MAX_SLABS", 2)
    o = lambda n: (n - 1) // stride + 1
    work = N * o(T) * -(-o(H) // 16) * -(-o(W) // 16) if taps == 27 else N * T * -(-H // 16) * -(-W // 16)
    assert (d._nslab3 if taps == 27 else d._nslab)(work, dw.numel() + Cout) == min(work, 2)
    dw2, db2 = run()
    check_margin(f"wgrad3d {case} d weight, {min(work, 2)} slabs for {work} items", dw2, dw64, R.rel(dw32, dw64))
    check_margin(f"wgrad3d {case} d bias, {min(work, 2)} slabs for {work} items", db2, db64, R.rel(db32, db64))
    check_margin(f"wgrad3d {case} wrapped vs unwrapped", dw2, dw, R.rel(dw32, dw64))
    check_margin(f"wgrad3d {case} d bias wrapped vs unwrapped", db2, db, R.rel(db32, db64))


# ---- whole nets

_runs = {}


def native_run(name, frozen=False, fresh=False):
    """Train-mode logits, input gradient and every parameter gradient in full from the native module."""
    key = (name, frozen)
    if key in _runs and not fresh:
        return _runs[key]
    d = D()
    cin, widths, shape, seed = G3.G20_NETS[name]
    net = d.Discriminator3D(cin, widths)
    net.load_state_dict(G.fill(G.disc3d_shapes(cin, widths), seed), strict=True)
    net = net.to(DEV).train()
    if frozen:
        net.requires_grad_(False)
    x = G.inputs(shape, seed).to(DEV).requires_grad_(True)
    logits = net(x)
    assert logits.grad_fn is not None
    (logits * G.cot(logits.shape, G3.PHI, torch.float32).to(DEV)).sum().backward()
    out = {"logits": logits.detach(), "dx": x.grad}
    for k, v in net.named_parameters():
        if v.grad is not None:
            assert tuple(v.grad.shape) == tuple(v.shape), k
            out["grad/" + k] = v.grad
    out = {k: v.cpu() for k, v in out.items()}
    if not fresh:
        _runs[key] = out
    return out


@pytest.mark.parametrize("name", list(G3.G20_NETS))
def test_whole_net(name):
    """Logits, input gradient and every parameter gradient by the margin rule: first against fixture G20 (the reference in float64)
    on everything it stores -- small gradients in full, of the large 27-tap weights the norm, the 27 per-tap norms and output
    channels 0..3 --, then against the float64 restatement in full.  The zero-bias keys are exactly zero, conv_norm_out has no
    gradient, and the set of compared keys equals the set produced."""
    cin, widths, shape, seed = G3.G20_NETS[name]
    got = native_run(name)
    assert tuple(got["logits"].shape) == G3.G20_LOGITS[name]
    zero = ["grad/" + k for k in G3.G20_ZERO_BIAS[name]]
    assert not any("conv_norm_out" in k for k in got)
    for k in zero:
        assert not bool(got[k].any()), k
    fx = R.fixture("g20_disc3d.npz", name)
    derived = {}
    for k, v in got.items():
        derived.update(G3.grad_entries(k[len("grad/"):], v) if k.startswith("grad/") else {k: v})
    stored = [k for k in fx if not k.startswith("ref32_rel/") and k not in ("keys", "shapes")]
    assert set(stored) == set(derived), set(stored) ^ set(derived)
    for k in stored:
        if k not in zero:
            assert tuple(derived[k].shape) == tuple(fx[k].shape), k
            check_margin(f"net {name} {widths} G20 {k}", derived[k], fx[k], fx["ref32_rel/" + k])
    params, x = G.fill(G.disc3d_shapes(cin, widths), seed), G.inputs(shape, seed)
    want = R3.full_grads(params, x, len(widths), torch.float64)
    o32 = R3.full_grads(params, x, len(widths), torch.float32)
    assert set(want) == set(got), set(want) ^ set(got)
    for k, v in want.items():
        if k not in zero:
            check_margin(f"net {name} {widths} float64 {k}", got[k], v, R.rel(o32[k], v))


def _no_torch_3d(monkeypatch):
    def gone(*a, **k):
        raise AssertionError("the torch 3-D path ran on the GPU")
    monkeypatch.setattr(torch.nn.functional, "conv3d", gone)
    monkeypatch.setattr(torch.nn.functional, "group_norm", gone)


def _mixed(name):
    d = D()
    cin, shape, seed = G.G19_NETS[name]
    net = d.MixedDiscriminator(cin)
    net.load_state_dict(G.fill(G.mixed_shapes(cin), seed), strict=True)
    return net.to(DEV).train(), R.fixture("g19_disc_mixed.npz", name), G.inputs(shape, seed)


def test_torch_path_is_gone_on_the_gpu(monkeypatch):
    """With torch's conv3d and group_norm raising, MixedDiscriminator(3) forward + backward on the G19 input still runs, meets G19
    (logits, dx, and d3_logits through discriminator3d alone), and the census shows launches of the 3-D kernels."""
    from autoregressive_diffusion_amd import ops
    _no_torch_3d(monkeypatch)
    with pytest.raises(AssertionError, match="torch 3-D path"):
        torch.nn.GroupNorm(32, 32)(torch.zeros(2, 32, 1, 1, 1))
    net, fx, x = _mixed("m3")
    before = ops.census_peek()
    xg = x.to(DEV).requires_grad_(True)
    logits = net(xg)
    (logits * G.cot(logits.shape, 0.3, torch.float32).to(DEV)).sum().backward()
    after = ops.census_peek()
    launched = {k.split("(")[0]: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)}
    print("mixed forward + backward launches:", launched)
    for kern in ("disc3d_conv_kernel", "disc3d_wgrad_kernel", "disc3d_stem_dgrad_kernel", "disc3d_gn_finalize_kernel",
                 "disc3d_gn_bwd_reduce_kernel", "disc3d_gn_bwd_finalize_kernel", "disc3d_gn_bwd_dx_kernel", "disc3d_blur_kernel",
                 "disc3d_blur_bwd_kernel"):
        assert any(kern in k for k in launched), kern
    check_margin("mixed m3 logits (no torch 3-D ops)", logits, fx["logits"], fx["ref32_rel/logits"])
    check_margin("mixed m3 dx (no torch 3-D ops)", xg.grad, fx["dx"], fx["ref32_rel/dx"])
    with torch.no_grad():
        y3 = net.discriminator3d(x.to(DEV))
    assert tuple(y3.shape) == (2, 2, 1, 8, 8)
    check_margin("mixed m3 d3_logits (no torch 3-D ops)", y3, fx["d3_logits"], fx["ref32_rel/d3_logits"])


def test_determinism_and_frozen_critic():
    """Two identical runs of net b3 give the same bits in every output and gradient.  With every parameter frozen, logits and dx
    have the same bits and no weight-gradient kernel (nor a slab sum) is launched."""
    from autoregressive_diffusion_amd import ops
    a, b = native_run("b3"), native_run("b3", fresh=True)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    before = ops.census_peek()
    f = native_run("b3", frozen=True, fresh=True)
    after = ops.census_peek()
    launched = {k: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)}
    print("frozen critic launches:", {k.split("(")[0]: n for k, n in launched.items()})
    assert any("disc3d_conv_kernel" in k for k in launched) and any("disc3d_stem_dgrad_kernel" in k for k in launched)
    assert not any("wgrad" in k or "slab_sum" in k for k in launched), launched
    assert torch.equal(f["dx"], a["dx"]) and torch.equal(f["logits"], a["logits"])
    assert not any(k.startswith("grad/") for k in f)


@pytest.mark.parametrize("name", list(G.G19_NETS))
def test_losses_of_the_native_mixed(name, monkeypatch):
    """vae_loss / discriminator_loss of the all-native MixedDiscriminator against G19 by the margin rule, torch's conv3d and
    group_norm raising; discriminator_loss leaves recon.grad None, vae_loss fills it with finite values."""
    _no_torch_3d(monkeypatch)
    net, fx, _ = _mixed(name)
    frames = fx["frames"].to(DEV)
    for loss in ("discriminator_loss", "vae_loss"):
        recon = fx["recon"].to(DEV).requires_grad_(True)
        net.zero_grad(set_to_none=True)
        val = getattr(net, loss)(frames, recon)
        val.backward()
        e, m = abs(val.item() - float(fx[loss])) / abs(float(fx[loss])), R.margin(fx["ref32_rel/" + loss])
        print(f"mixed {name} {loss}: {val.item():.7f} vs {float(fx[loss]):.7f}, rel {e:.2e} (bound {m:.2e})")
        assert e <= m, (loss, e, m)
        grads = {k: p.grad for k, p in net.named_parameters() if "conv_norm_out" not in k}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
        if loss == "vae_loss":
            assert recon.grad is not None and bool(torch.isfinite(recon.grad).all()) and bool(recon.grad.any())
        else:
            assert recon.grad is None

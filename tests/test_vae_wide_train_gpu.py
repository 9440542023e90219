"""Wide VAE training on the GPU (csrc/vae_wide_train.hip, csrc/vae_wide_train.h; autoregressive_diffusion_amd/vae_train.py:
Res, Down, Up, Out on a wide packed block; VAE.wide_training()) against tests/vae_train_cpu_restatement.py in float64.

Stages, through the autograd Functions with operands packed by vae.py's own pack functions, on Gaussian operands: outputs, input
gradient, parameter gradients and d emb under the two metrics and bounds of tests/vae_stage_oracle.py (5 x the distance of the
restatement's own float32 evaluation from float64, the rel L2 bound capped at 1e-5 / 5e-5).  The data and weight gradients of the
convs and the 1x1 stages through the C entry points on integers in [-3, 3], every sum below 2^24: EQUAL to float64.  Slab wrap:
3 slabs against 16 work items and 1 slab, exact and run twice.  Whole models with the switch on (G24's and [3,16,96,160,8]): per
parameter rel L2 <= max(5e-5, 4 x the float32 restatement's distance from float64); bit identities; frozen parameters by the
dispatch census; a narrow model with the switch on and off.  Every figure is printed as `vae_wide_train: <case> <figure>`
(profiles/vae_wide_training_tests.txt)."""
import copy

import pytest
import torch

import vae_stage_oracle as S
import vae_train_cpu_restatement as RT
import vae_wide_oracle as O
import vae_wide_encoder_oracle as E
import vae_wide_train_oracle as WT
from test_vae_wide_train import g24_vae, g24_grad_error

DEV = "cuda"
pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
F32 = dict(device=DEV, dtype=torch.float32)
GRAD_TOL = 5e-5
_IDS = lambda c: "-".join(str(int(v)) for v in c)

#            C,  g,  H,  W, emb      B = 2, T = 2g: the first group feeds the detached prefix, the last has a single reader
RES_CASES = [(72, 1, 20, 28, 1),    # ragged width (CP = 96, NB = 1), four tiles, three partial
             (72, 2, 5, 7, 0),
             (72, 4, 16, 16, 1),
             (128, 2, 20, 28, 0),   # NB = 2
             (128, 4, 5, 7, 1),
             (160, 2, 16, 16, 1),
             (160, 1, 5, 7, 0)]
#             Cin, tc, sc,  C,  H,  W    the coarse grid; K = Cin tc sc^2
DOWN_CASES = [(8, 2, 1, 72, 20, 28), (72, 2, 2, 160, 5, 7), (160, 1, 2, 8, 16, 16), (3, 1, 2, 128, 5, 7), (96, 1, 1, 160, 5, 7)]
UP_CASES = [(72, 2, 1, 20, 28), (128, 2, 2, 5, 7), (160, 1, 2, 16, 16), (72, 1, 1, 5, 7)]
#            C, Cout, H,  W, split
OUT_CASES = [(72, 8, 20, 28, 0), (160, 96, 5, 7, 0), (128, 6, 16, 16, 1), (72, 6, 5, 7, 1)]


def _note(case, **figs):
    print("vae_wide_train:", case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


def _cl(x):
    """channels-first (B, C, T, H, W) -> a contiguous channels-last tensor on the GPU."""
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def _cf(x):
    return x.detach().permute(0, 4, 1, 2, 3).cpu()


def _res_block(C, g, gen):
    from autoregressive_diffusion_amd.vae import ResBlock
    rb = ResBlock(C, (2 * g, 3, 3), g, t_cond=False)
    with torch.no_grad():
        for p in (rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias):
            p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else p[0].numel() ** -0.5))
    return rb


def _judge(what, got, ref64, ref32):
    bad = S.compare(what, got, ref64, ref32)
    assert not bad, "\n".join(bad)


# ---- every stage alone, Gaussian operands

@pytest.mark.parametrize("case", RES_CASES, ids=_IDS)
def test_res_stage(case):
    from autoregressive_diffusion_amd import vae as V, vae_train
    C, g, H, W, with_emb = case
    B, T = 2, 2 * g
    gen = torch.Generator().manual_seed(2500 + C + 7 * g + H)
    rb = _res_block(C, g, gen)
    x, dout = torch.randn(B, C, T, H, W, generator=gen), torch.randn(B, C, T, H, W, generator=gen)
    emb = 0.5 * torch.randn(B, 2 * C, generator=gen) if with_emb else None
    w = [rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias]
    ref64, ref32 = (WT.res_ref(x, emb, *w, g, dout, dt) for dt in (torch.float64, torch.float32))
    rb = rb.to(DEV)
    w = [rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias]
    pk = V._pack_res_wide(rb, C, g, F32)
    xd = _cl(x).requires_grad_()
    embd = None if emb is None else emb.to(DEV).requires_grad_()
    out = vae_train.Res.apply(xd, embd, *w, dict(g=g, wide=True), pk)
    assert out.grad_fn is not None
    out.backward(_cl(dout))
    grads = dict(dx=_cf(xd.grad), dwa=w[0].grad.cpu(), dba=w[1].grad.cpu(), dwb=w[2].grad.cpu(), dbb=w[3].grad.cpu())
    if with_emb:
        grads["demb"] = embd.grad.cpu()
    _judge(f"res {_IDS(case)}", (dict(out=_cf(out)), grads), ref64, ref32)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_res_where_only_conv_b_trains(wide):
    """Res with only conv B's weight and bias requiring grad: backward ends after conv B's weight gradient.  dwb and dbb are the
    bits of the all-trainable run on the same operands, and every other .grad stays None.  Narrow: the smallest case of
    S.RES_CASES; wide: (C, g, H, W) = (72, 2, 5, 7) with B = 2, T = 2g."""
    from autoregressive_diffusion_amd import vae as V, vae_train
    gen = torch.Generator().manual_seed(2550)
    if wide:
        (C, g, H, W), B = (72, 2, 5, 7), 2
        T = 2 * g
        rb, x, emb = _res_block(C, g, gen), torch.randn(B, C, T, H, W, generator=gen), None
        pk, bk = V._pack_res_wide(rb.to(DEV), C, g, F32), dict(g=g, wide=True)
    else:
        case = min((c for c, _ in S.RES_CASES.values()), key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4])
        B, T, H, W, C, g, _ = case
        rb, x, emb = S.res_operands(case)
        pk, bk = V._pack_res(rb.to(DEV), C, g, F32), dict(g=g, nch=V._nch(C), gpt=V._gpt(C, g))
    w = [rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias]
    xd, doutd = _cl(x), _cl(torch.randn(B, C, T, H, W, generator=gen))

    def run(everything):
        for p in w:
            p.grad = None
        w[0].requires_grad_(everything), w[1].requires_grad_(everything)
        xg = xd.clone().requires_grad_(everything)
        eg = None if emb is None else emb.to(DEV).requires_grad_(everything)
        vae_train.Res.apply(xg, eg, *w, bk, pk).backward(doutd)
        return [p.grad for p in w], [xg.grad, None if eg is None else eg.grad]
    full, full_in = run(True)
    only, only_in = run(False)
    assert all(v is not None for v in full) and full_in[0] is not None
    assert torch.equal(only[2], full[2]) and torch.equal(only[3], full[3])
    assert only[0] is None and only[1] is None and only_in == [None, None]


def _lin_module(cin, cout, gen):
    conv = torch.nn.Conv3d(cin, cout, kernel_size=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / cin ** 0.5)
        conv.bias.copy_(0.1 * torch.randn(cout, generator=gen))
    return conv


@pytest.mark.parametrize("case", DOWN_CASES, ids=_IDS)
def test_down_stage(case):
    """The first case's x is a permuted view of a channels-first tensor, as the first encoder block sees the frames."""
    from autoregressive_diffusion_amd import vae as V, vae_train
    Cin, tc, sc, C, H, W = case
    B, T, npos = 2, 2, tc * sc * sc
    gen = torch.Generator().manual_seed(2600 + Cin + C)
    conv = _lin_module(Cin * npos, C, gen)
    x, dy = torch.randn(B, Cin, T * tc, H * sc, W * sc, generator=gen), torch.randn(B, C, T, H, W, generator=gen)
    ref64, ref32 = (WT.lin_ref("down", x, conv.weight, conv.bias, tc, sc, (dy,), dt) for dt in (torch.float64, torch.float32))
    conv = conv.to(DEV)
    wd, bd = V._pack_down_wide(conv.weight, conv.bias, Cin, C, npos, F32)
    bk = dict(Cin=Cin, C=C, tc=tc, sc=sc, wd=wd, bd=bd, wide_down=True)
    xd = (x.to(DEV).permute(0, 2, 3, 4, 1) if case == DOWN_CASES[0] else _cl(x)).requires_grad_()
    y = vae_train.Down.apply(xd, conv.weight, conv.bias, bk)
    y.backward(_cl(dy))
    _judge(f"down {_IDS(case)}", (dict(y=_cf(y)), dict(dx=_cf(xd.grad), dw=conv.weight.grad.cpu(), db=conv.bias.grad.cpu())), ref64, ref32)


@pytest.mark.parametrize("case", UP_CASES, ids=_IDS)
def test_up_stage(case):
    from autoregressive_diffusion_amd import vae as V, vae_train
    C, tc, sc, H, W = case
    B, T, npos = 2, 2, tc * sc * sc
    gen = torch.Generator().manual_seed(2700 + C + tc + sc)
    conv = _lin_module(C, C * npos, gen)
    x, dup = torch.randn(B, C, T, H, W, generator=gen), torch.randn(B, C, T * tc, H * sc, W * sc, generator=gen)
    ref64, ref32 = (WT.lin_ref("up", x, conv.weight, conv.bias, tc, sc, (dup,), dt) for dt in (torch.float64, torch.float32))
    conv = conv.to(DEV)
    wu, bu = V._pack_lin_wide(conv.weight, conv.bias, C, C, npos, F32)
    xd = _cl(x).requires_grad_()
    y = vae_train.Up.apply(xd, conv.weight, conv.bias, dict(C=C, tc=tc, sc=sc, wu=wu, bu=bu, wide=True))
    y.backward(_cl(dup))
    _judge(f"up {_IDS(case)}", (dict(y=_cf(y)), dict(dx=_cf(xd.grad), dw=conv.weight.grad.cpu(), db=conv.bias.grad.cpu())), ref64, ref32)


@pytest.mark.parametrize("case", OUT_CASES, ids=_IDS)
def test_out_stage(case):
    from autoregressive_diffusion_amd import vae as V, vae_train
    C, Cout, H, W, split = case
    B, T = 2, 2
    gen = torch.Generator().manual_seed(2800 + C + Cout)
    conv = _lin_module(C, Cout, gen)
    x = torch.randn(B, C, T, H, W, generator=gen)
    lvm = torch.nn.Parameter(torch.tensor(-1.7)) if split else None
    douts = [torch.randn(B, Cout // 2 if split else Cout, T, H, W, generator=gen) for _ in range(2 if split else 1)]
    ref64, ref32 = (WT.lin_ref("out", x, conv.weight, conv.bias, 1, 1, douts, dt, lvm) for dt in (torch.float64, torch.float32))
    conv = conv.to(DEV)
    wo, bo = V._pack_lin_wide(conv.weight, conv.bias, C, Cout, 1, F32)
    bk = dict(C=C, Cout=Cout, wo=wo, bo=bo, wide=True)
    xd = _cl(x).requires_grad_()
    grads = lambda: dict(dx=_cf(xd.grad), dw=conv.weight.grad.cpu(), db=conv.bias.grad.cpu())
    if split:
        lvmd = torch.nn.Parameter(lvm.detach().to(DEV))
        mean, logvar = vae_train.Out.apply(xd, conv.weight, conv.bias, lvmd, bk, lvmd.detach().float().reshape(1).contiguous())
        torch.autograd.backward((mean, logvar), [d.to(DEV) for d in douts])
        got = (dict(mean=mean.detach().cpu(), logvar=logvar.detach().cpu()), dict(grads(), dlvm=lvmd.grad.cpu()))
    else:
        y = vae_train.Out.apply(xd, conv.weight, conv.bias, None, bk, None)
        y.backward(_cl(douts[0]))
        got = (dict(y=_cf(y)), grads())
    _judge(f"out {_IDS(case)}", got, ref64, ref32)


# ---- integers: the conv data and weight gradients equal float64, at every slab count and twice

def _exact(name, got, want):
    want = want.detach()
    assert want.abs().max() < 2 ** 24
    _note(name, mismatches=int((got.cpu().double() != want).sum()), absmax=float(want.abs().max()))
    assert torch.equal(got.cpu().double(), want), name


@pytest.mark.parametrize("case", [(72, 1, 20, 28), (72, 2, 5, 7), (128, 2, 20, 28), (128, 4, 5, 7), (160, 4, 16, 16)], ids=_IDS)
def test_conv_gradients_exact(case):
    """du = convB^T(dout), dy = convA^T(da) through D, and both weight gradients at the default slab count, at 3 slabs (16 work
    items at 20x28: workgroup s takes s, s + 3, ...) and at 1, each twice."""
    from autoregressive_diffusion_amd import _lib as L, vae as V, vae_train
    C, g, H, W = case
    B, T = 2, 2 * g
    gen = torch.Generator().manual_seed(2900 + C + g)
    wa, wb = _ints(gen, C * g, C, 2 * g, 3, 3), _ints(gen, C, C, 1, 3, 3)
    y, u, da, dout = (_ints(gen, B, T, H, W, C) for _ in range(4))
    y64, u64, wa64, wb64 = (t.double().requires_grad_() for t in (y, u, wa, wb))
    ba64, bb64 = torch.zeros(C * g, dtype=torch.float64, requires_grad=True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    S64 = torch.cat((y64[:, :g].detach(), y64), dim=1)
    (O.conv_a(S64, wa64, ba64, g) * da.double()).sum().backward()
    (O.conv_b(u64, torch.zeros_like(u64), wb64, bb64) * dout.double()).sum().backward()
    wda, wdb, zb = vae_train._pack_dgrad_wide(wa.to(DEV), wb.to(DEV), C, g)
    s, p = V._stream(), V._p
    doutd, ud, Sd = dout.to(DEV), u.to(DEV), S64.detach().float().to(DEV)
    du = torch.full((B, T, H, W, C), float("nan"), device=DEV)
    L.check(L.lib.oniris_vae_wide_conv_b_bwd(p(doutd), p(wdb), p(du), B, T, H, W, C, s), "vae_wide_conv_b_bwd")
    _exact(f"conv B dgrad {_IDS(case)}", du, u64.grad)
    D = torch.cat((da, torch.zeros(B, g, H, W, C)), dim=1).to(DEV)
    _exact(f"conv A dgrad {_IDS(case)}", V.wide_conv_a(D, dict(wa=wda, ba=zb), g, s), y64.grad)
    items = B * (T // g) * -(-H // 16) * -(-W // 16)
    for nslab in (None, 3, 1):
        runs = []
        for _ in range(2):
            ra, rba = vae_train._wide_conv3_dw(Sd, D, B, T, H, W, C, g, True, nslab)
            rb_, rbb = vae_train._wide_conv3_dw(ud, doutd, B, T, H, W, C, 1, False, nslab)
            runs.append((ra.clone(), rba.clone(), rb_.clone(), rbb.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), (case, nslab)
        ra, rba, rb_, rbb = runs[0]
        tag = f"{_IDS(case)} nslab={nslab} items={items}"
        _exact(f"conv A wgrad {tag}", ra.view(2 * g, g, 3, 3, C, C).permute(5, 1, 4, 0, 2, 3).reshape(wa.shape), wa64.grad)
        _exact(f"conv A bgrad {tag}", rba.view(g, C).t().reshape(-1), ba64.grad)
        _exact(f"conv B wgrad {tag}", rb_.view(3, 3, C, C).permute(3, 2, 0, 1).reshape(wb.shape), wb64.grad)
        _exact(f"conv B bgrad {tag}", rbb, bb64.grad)


@pytest.mark.parametrize("case", [(72, 2, 1, 160, 20, 28), (72, 2, 2, 128, 5, 7), (160, 1, 2, 8, 20, 28), (3, 1, 1, 72, 5, 7)], ids=_IDS)
def test_lin_gradients_exact(case):
    """The 1x1 stages without the (fractional) area matrix: the adjoint of `down` / `out` (an `up` on W^T), the adjoint of `up`
    (a `down` on W^T without residual) and the weight gradient over both rearranged views, at three slab counts, each twice."""
    from autoregressive_diffusion_amd import _lib as L, vae as V, vae_train
    Cin, tc, sc, C, H, W = case
    B, T, npos = 2, 2, tc * sc * sc
    gen = torch.Generator().manual_seed(3000 + Cin + C)
    w, x, dy = _ints(gen, C, Cin * npos), _ints(gen, B, T * tc, H * sc, W * sc, Cin), _ints(gen, B, T, H, W, C)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    r = E.rearrange_down(x64, tc, sc)
    ((r @ w64.T + b64) * dy.double()).sum().backward()
    s, p = V._stream(), V._p
    xd, dyd = x.to(DEV), dy.to(DEV)
    pack = V._pack_lin_wide(w.t().to(DEV), torch.zeros(Cin * npos, device=DEV), C, Cin, npos, F32)
    _exact(f"down dgrad {_IDS(case)}", vae_train._wide_down_dx(dyd, pack, (B, T, H, W), C, Cin, tc, sc), x64.grad)
    for nslab in (None, 3, 1):
        runs = [tuple(t.clone() for t in vae_train._wide_lin_dw(xd, (Cin, tc, sc), dyd, (C, 1, 1), (B, T, H, W), nslab)) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*runs)), (case, nslab)
        _exact(f"down wgrad {_IDS(case)} nslab={nslab}", runs[0][0][:, 0].permute(2, 0, 1).reshape(C, -1), w64.grad)
        _exact(f"down bgrad {_IDS(case)} nslab={nslab}", runs[0][1].reshape(-1), b64.grad)
    if Cin < 65:
        return
    # `up` at width Cin: x2 (B, T, H, W, Cin) -> dup (B, T tc, H sc, W sc, Cin)
    wu, x2, dup = _ints(gen, Cin * npos, Cin), _ints(gen, B, T, H, W, Cin), x
    x264, wu64, bu64 = x2.double().requires_grad_(), wu.double().requires_grad_(), torch.zeros(Cin * npos, dtype=torch.float64, requires_grad=True)
    (O.up(x264, wu64, bu64, tc, sc) * dup.double()).sum().backward()
    pack = vae_train._pack_up_dgrad(wu.to(DEV), Cin, tc, sc)
    dx = torch.full((B, T, H, W, Cin), float("nan"), device=DEV)
    L.check(L.lib.oniris_vae_wide_up_bwd(p(xd), p(pack[0]), p(pack[1]), p(dx), B, T, H, W, Cin, tc, sc, s), "vae_wide_up_bwd")
    _exact(f"up dgrad {_IDS(case)}", dx, x264.grad)
    for nslab in (None, 3, 1):
        dw, db = vae_train._wide_lin_dw(x2.to(DEV), (Cin, 1, 1), xd, (Cin, tc, sc), (B, T, H, W), nslab)
        _exact(f"up wgrad {_IDS(case)} nslab={nslab}", dw[0].permute(0, 2, 1).reshape(Cin * npos, Cin), wu64.grad)
        _exact(f"up bgrad {_IDS(case)} nslab={nslab}", db.reshape(-1), bu64.grad)


# ---- whole models

CS_KW = dict(channels=[3, 16, 96, 160, 8], n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
_models = {}


def _model(name):
    """(vae on the GPU in training mode with the switch on, kwargs, x, t_sample, noise, float64 outputs and gradients, float32
    gradients of the restatement), computed once per process and left unchanged."""
    if name not in _models:
        from autoregressive_diffusion_amd.vae import VAE
        if name == "g24":
            z, kw, vae = g24_vae()
            x = (torch.from_numpy(z["frames"]).double() / 127.5 - 1).permute(0, 4, 1, 2, 3).float()
            t_sample, noise = torch.from_numpy(z["t_sample"]), torch.from_numpy(z["noise"])
        else:
            kw, gen = CS_KW, torch.Generator().manual_seed(3100)
            vae = O.seed_params(VAE(**kw), 3101)
            x = torch.rand(2, 3, 8, 16, 24, generator=gen) * 2 - 1
            t_sample, noise = torch.rand(2, generator=gen) * 0.1, torch.randn(2, 8, 2, 2, 3, generator=gen)
        sd = vae.state_dict()
        o64, g64 = RT.grads(sd, kw, x, t_sample, noise)
        _, g32 = RT.grads(sd, kw, x, t_sample, noise, dtype=torch.float32)
        _models[name] = (vae.to(DEV).train().wide_training(), kw, x, t_sample, noise, o64, g64, g32)
    return _models[name]


def _train(vae, x, t_sample, noise):
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, mean, cache = vae(x.to(DEV), t_sample=t_sample.to(DEV), noise=noise.to(DEV))
    RT.loss(r_mean, r_logvar, mean).backward()
    return (r_mean, r_logvar, mean, cache), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in vae.named_parameters()}


@pytest.mark.parametrize("name", ["g24", "cs"])
def test_model_gradients(name):
    vae, kw, x, t_sample, noise, o64, g64, g32 = _model(name)
    (r_mean, r_logvar, mean, cache), grads = _train(vae, x, t_sample, noise)
    assert all(o.grad_fn is not None for o in (r_mean, r_logvar, mean))
    assert all(v is None for side in cache.values() for blk in side.values() for rb in blk.values() for v in rb.values())
    for k, o in (("r_mean", r_mean), ("r_logvar", r_logvar), ("mean", mean)):
        e = O.rel_l2(o.detach(), o64[k])
        _note(f"model {name} output {k}", rel_l2=e)
        assert e <= 1e-5, k
    bad = []
    for n in g64:
        e32, e = O.rel_l2(g32[n], g64[n]), O.rel_l2(grads[n], g64[n])
        bound = max(GRAD_TOL, 4 * e32)
        _note(f"model {name} grad {n}", rel_l2=e, float32_restatement=e32, bound=bound)
        if not e <= bound:
            bad.append((n, e, bound))
    assert not bad, bad
    if name == "g24":                                            # and against the reference itself, through the fixture
        z = g24_vae()[0]
        assert max(g24_grad_error(z, n, grads[n]) for n in g64) <= 1e-4
    # clip_grad_norm_ and torch's AdamW work as they are
    vae2 = copy.deepcopy(vae)
    assert vae2._wide_training
    opt = torch.optim.AdamW(vae2.parameters(), lr=1e-4)
    _train(vae2, x, t_sample, noise)
    assert torch.isfinite(torch.nn.utils.clip_grad_norm_(vae2.parameters(), 1.0))
    opt.step()
    _, g2 = _train(vae2, x, t_sample, noise)                      # the packs follow the parameters' versions
    assert not torch.equal(g2["encoder.encoder_blocks.1.res_blocks.0.conv3d1.weight"], grads["encoder.encoder_blocks.1.res_blocks.0.conv3d1.weight"])


@pytest.mark.parametrize("name", ["g24", "cs"])
def test_model_bit_identities(name):
    vae, kw, x, t_sample, noise = _model(name)[:5]
    (r_mean, r_logvar, mean, _), grads = _train(vae, x, t_sample, noise)
    with torch.no_grad():
        assert torch.equal(mean, vae.encode(x.to(DEV))[0])
    vae.eval()
    try:
        e_mean, e_logvar, e_m, _ = vae(x.to(DEV), t_sample=t_sample.to(DEV), noise=noise.to(DEV))
    finally:
        vae.train()
    assert torch.equal(r_mean, e_mean) and torch.equal(r_logvar, e_logvar) and torch.equal(mean, e_m)
    (_, _, _, _), again = _train(vae, x, t_sample, noise)
    assert all(torch.equal(grads[n], again[n]) for n in grads)
    # a sample's activation path does not depend on B: outputs, and the gradient that reaches the latents, of row 0 alone
    def latent_grad(xs, ts, ns):
        got = {}
        out = vae(xs.to(DEV), t_sample=ts.to(DEV), noise=ns.to(DEV))
        out[2].register_hook(lambda g_: got.setdefault("dmean", g_.detach().clone()))
        vae.zero_grad(set_to_none=True)
        (out[0] * RT.cotangents(out[0].shape[1:], 0.1, torch.float32).to(DEV)).sum().backward()
        return out[0].detach(), out[1].detach(), out[2].detach(), got["dmean"]
    both, one = latent_grad(x, t_sample, noise), latent_grad(x[:1], t_sample[:1], noise[:1])
    assert all(torch.equal(a[:1], b) for a, b in zip(both, one))


def test_frozen_encoder():
    """cs_vae_adversarial.py's commented lines: the encoder frozen.  Its .grad stays None and no weight-gradient launch is issued
    for it: the census counts one per 1x1 stage and two per ResBlock of the decoder alone."""
    from autoregressive_diffusion_amd import ops
    vae, kw, x, t_sample, noise = _model("cs")[:5]
    vae = copy.deepcopy(vae)

    def wgrad_launches():
        before = ops.census_peek()                               # the suite's own census is running: the difference of two peeks
        grads = _train(vae, x, t_sample, noise)[1]
        torch.cuda.synchronize()
        c = {k: v - before.get(k, 0) for k, v in ops.census_peek().items() if v != before.get(k, 0)}
        return grads, sum(v for k, v in c.items() if "wgrad" in k or "lin_dw" in k), c
    nblk, nres = len(kw["channels"]) - 1, kw["n_res_blocks"]
    grads, n, c = wgrad_launches()
    _note("frozen: all trainable", wgrad_launches=n)
    assert n == 2 * nblk * (2 + 2 * nres) - nblk and all(v is not None for v in grads.values()), c     # down | up + out, 2 per ResBlock
    for p in vae.encoder.parameters():
        p.requires_grad_(False)
    grads, n, c = wgrad_launches()
    _note("frozen: encoder frozen", wgrad_launches=n)
    assert n == nblk * (2 + 2 * nres), c
    assert all((v is None) == k.startswith("encoder.") for k, v in grads.items())


def test_narrow_model_is_untouched():
    """channels=[3,8,8,8] trained with the switch off and on: the same output and gradient bits (none of its packed blocks is
    wide, so every Function takes the narrow kernels either way)."""
    from autoregressive_diffusion_amd.vae import VAE
    gen = torch.Generator().manual_seed(3200)
    vae = O.seed_params(VAE(channels=[3, 8, 8, 8], n_res_blocks=1), 3201).to(DEV).train()
    x, t_sample, noise = torch.rand(2, 3, 4, 16, 24, generator=gen) * 2 - 1, torch.rand(2, generator=gen) * 0.1, torch.randn(2, 8, 1, 4, 6, generator=gen)
    assert vae._wide_training is False
    outs_off, grads_off = _train(vae, x, t_sample, noise)
    outs_on, grads_on = _train(vae.wide_training(), x, t_sample, noise)
    assert all(torch.equal(a, b) for a, b in zip(outs_off[:3], outs_on[:3]))
    assert all(torch.equal(grads_off[n], grads_on[n]) for n in grads_off)


def test_refusals_with_the_switch_on():
    vae, kw, x, t_sample, noise = _model("g24")[:5]
    xd = x.to(DEV)
    with pytest.raises(ValueError, match="requires grad"):
        vae(xd.clone().requires_grad_())
    with torch.no_grad():
        cache = vae(xd)[3]
    with pytest.raises(ValueError, match="non-empty cache"):
        vae(xd, cache=cache)
    off = copy.deepcopy(vae).wide_training(False)
    with pytest.raises(NotImplementedError, match=r"72 channels.*edm2\.vae"):
        off(xd)

"""`VAE.bf16_inference()` on the GPU: the bf16-operand kernels of csrc/vae_wide_bf16.hip against tests/vae_bf16_oracle.py.

Stages, one launch each through the wrappers of vae.py on operands packed by its own pack functions (bf16=True): on integers in
[-3, 3] (exact in bf16, every sum below 2^24) the result EQUALS float64; on Gaussian operands it is held, under the two metrics of
tests/vae_stage_oracle.py, to max(1e-5, 5 x the distance of a float32 evaluation of the same rounded operands from float64) of the
bf16-faithful float64 oracle, it is farther than 1e-4 from the unrounded float64 oracle, and it is not bit-equal to the fp32 launch.
Widths 72 (CP = 96, CinP = 80: ragged against the 32-channel chunk and the 16-channel K step), 128, 264 (CP = 288, NB = 1; CinP =
272: a last chunk of one K step) and 512; g = 1, 2, and 4 at 512; 5x7 is one partial
tile, 20x28 four tiles of which three are partial; T = 2g; B = 2, and B = 1 at C = 512, g = 4.

Whole models ([3,16,96,160,8] and the Counter-Strike shape [3,32,128,512,8] under VAE512) with the switch on: encode, decode and the
eval-mode forward within 2 E of the UNROUNDED float64 oracle, E = the distance of the bf16-faithful oracle from it (a model cannot
be held tightly to the faithful oracle: every rounding turns an fp32-level difference into a bf16-level one); the bit identities of
chunked decoding and encoding, of batch rows and of repeated runs; the dispatch census; and that nothing changes while the switch is
off: on-then-off gives the bits and the census of a model never switched, the training path ignores it, and caches pass between
the modes.  Every figure is printed as `vae_bf16: <case> <figure>` (profiles/vae_bf16_tests.txt)."""
import copy
import re

import pytest
import torch

import vae_bf16_oracle as BO
import vae_train_cpu_restatement as RT
import vae_wide_encoder_oracle as E
import vae_wide_oracle as O
from test_vae_512 import CS512_KW

DEV = "cuda"
pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
F32 = dict(device=DEV, dtype=torch.float32)
_IDS = lambda c: "-".join(str(int(v)) for v in c)

#            C,  g,  H,  W
RES_CASES = [(72, 1, 5, 7), (72, 2, 20, 28), (128, 2, 5, 7), (128, 1, 20, 28), (264, 1, 5, 7), (264, 2, 20, 28), (512, 1, 20, 28),
             (512, 2, 5, 7), (512, 4, 5, 7)]
#             Cin, tc, sc,  C,  H,  W, uint8    the coarse grid; K = Cin tc sc^2.  The last: uint8 frames normalised on load, CinP = 16
DOWN_CASES = [(512, 1, 2, 8, 20, 28, 0), (128, 2, 2, 512, 5, 7, 0), (32, 2, 2, 128, 20, 28, 0), (3, 1, 2, 96, 5, 7, 1)]
UP_CASES = [(512, 2, 2, 5, 7), (512, 1, 2, 16, 16), (128, 2, 2, 20, 28)]
#            C, Cout, H,  W, split
OUT_CASES = [(512, 8, 20, 28, 0), (512, 6, 5, 7, 1), (512, 6, 20, 28, 1), (512, 8, 5, 7, 0)]


def _note(case, **figs):
    print("vae_bf16:", case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _batch(C, g):
    return 1 if (C, g) == (512, 4) else 2


def _res_block(C, g, wa, ba, wb, bb):
    from autoregressive_diffusion_amd.vae import ResBlock
    rb = ResBlock(C, (2 * g, 3, 3), g, t_cond=False)
    with torch.no_grad():
        for p, v in zip((rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias), (wa, ba, wb, bb)):
            p.copy_(v)
    return rb.to(DEV)


def _draw(gen, ints, *shape, scale=1.0):
    return torch.randint(-3, 4, shape, generator=gen).float() if ints else scale * torch.randn(*shape, generator=gen)


def _exact(name, got, want):
    want = want.detach()
    assert want.abs().max() < 2 ** 24
    _note(name, mismatches=int((got.cpu().double() != want).sum()), absmax=float(want.abs().max()))
    assert torch.equal(got.cpu().double(), want), name


def _judge(name, kind, got, fp32_launch, args):
    """Items 2 and 3 for one Gaussian launch."""
    got = got.cpu()
    ref, bnd, f32 = BO.bound(kind, *args)
    m, bad = BO.outside(got, ref, bnd)
    far = O.rel_l2(got, BO.unrounded(kind, *args))
    same = int((got == fp32_launch.cpu()).sum())
    _note(name, rel=m[0], max_rms=m[1], float32_rel=f32[0], float32_max_rms=f32[1], bound_rel=bnd[0], bound_max_rms=bnd[1],
          from_unrounded=far, elements_equal_to_fp32_launch=f"{same}/{got.numel()}")
    assert not bad, (name, m, bnd)
    assert far > 1e-4, (name, far)
    assert not torch.equal(got, fp32_launch.cpu()), name


# ---- the ResBlock's convs

def _res_run(case, ints):
    """One conv A and one conv B launch on bf16 packs, and on fp32 packs: (the CPU operands of each, the four results)."""
    from autoregressive_diffusion_amd import vae as V
    C, g, H, W = case
    B, T = _batch(C, g), 2 * g
    gen = torch.Generator().manual_seed(7500 + C + 7 * g + H + ints)
    wa = _draw(gen, ints, C * g, C, 2 * g, 3, 3, scale=(C * 2 * g * 9) ** -0.5)
    wb = _draw(gen, ints, C, C, 1, 3, 3, scale=(C * 9) ** -0.5)
    ba, bb = _draw(gen, ints, C * g, scale=0.1), _draw(gen, ints, C, scale=0.1)
    Sq, u, x = _draw(gen, ints, B, g + T, H, W, C), _draw(gen, ints, B, T, H, W, C), _draw(gen, ints, B, T, H, W, C)
    rb = _res_block(C, g, wa, ba, wb, bb)
    pk, pk32 = V._pack_res_wide(rb, C, g, F32, bf16=True), V._pack_res_wide(rb, C, g, F32)
    assert pk["bf16"] and pk["wa"].dtype == torch.bfloat16
    s, Sd, ud, xd = V._stream(), Sq.to(DEV), u.to(DEV), x.to(DEV)
    a, o = V.wide_conv_a(Sd, pk, g, s), V.wide_conv_b(ud, xd, pk, s)
    a32, o32 = V.wide_conv_a(Sd, pk32, g, s), V.wide_conv_b(ud, xd, pk32, s)
    return (Sq, wa, ba, g), (u, x, wb, bb), a, o, a32, o32


@pytest.mark.parametrize("case", RES_CASES, ids=_IDS)
def test_convs_exact(case):
    args_a, args_b, a, o, a32, o32 = _res_run(case, 1)
    _exact(f"conv A exact {_IDS(case)}", a, O.conv_a(*args_a))
    _exact(f"conv B exact {_IDS(case)}", o, O.conv_b(*args_b))
    assert torch.equal(a, a32) and torch.equal(o, o32)           # on integers the fp32 launch is exact too


@pytest.mark.parametrize("case", RES_CASES, ids=_IDS)
def test_convs_gaussian(case):
    args_a, args_b, a, o, a32, o32 = _res_run(case, 0)
    _judge(f"conv A {_IDS(case)} K={2 * case[1] * 9 * case[0]}", "conv_a", a, a32, args_a)
    _judge(f"conv B {_IDS(case)} K={9 * case[0]}", "conv_b", o, o32, args_b)


# ---- the 1x1 stages

def _lin(gen, ints, cout, cin):
    return _draw(gen, ints, cout, cin, 1, 1, 1, scale=cin ** -0.5), _draw(gen, ints, cout, scale=0.1)


def _up_run(case, ints):
    from autoregressive_diffusion_amd import vae as V
    C, tc, sc, H, W = case
    B, T, npos = 2, 2, tc * sc * sc
    gen = torch.Generator().manual_seed(7600 + C + tc + sc + ints)
    (w, b), x = _lin(gen, ints, C * npos, C), _draw(gen, ints, B, T, H, W, C)
    res = []
    for bf16 in (True, False):
        wu, bu = V._pack_lin_wide(w.to(DEV), b.to(DEV), C, C, npos, F32, bf16)
        bk = dict(C=C, tc=tc, sc=sc, wu=wu, bu=bu, wide=True, bf16=bf16)
        res.append(V.up(x.to(DEV), None, (B, T, H, W), bk, V._stream()))
    return (x, w, b, tc, sc), res[0], res[1]


@pytest.mark.parametrize("case", UP_CASES, ids=_IDS)
def test_up(case):
    args, y, y32 = _up_run(case, 1)
    _exact(f"up exact {_IDS(case)}", y, O.up(*args))
    args, y, y32 = _up_run(case, 0)
    _judge(f"up {_IDS(case)}", "up", y, y32, args)


def _area_fp32(r, cout):
    """The area term as the kernels form it on integers: the window's sum (exact) divided by its length, one fp32 division."""
    return torch.stack([r[..., s0:s1].sum(dim=-1).float() / float(s1 - s0) for s0, s1 in O.area_windows(r.shape[-1], cout)], dim=-1)


def _pow2_windows(K, cout):
    return all((s1 - s0) & (s1 - s0 - 1) == 0 for s0, s1 in O.area_windows(K, cout))


def _out_run(case, ints):
    from autoregressive_diffusion_amd import vae as V
    C, Cout, H, W, split = case
    B, T = 2, 2
    gen = torch.Generator().manual_seed(7700 + C + Cout + H + ints)
    (w, b), x = _lin(gen, ints, Cout, C), _draw(gen, ints, B, T, H, W, C)
    lvm = torch.tensor([0.0 if ints else -1.7], device=DEV) if split else None         # exp(0) = 1: the integers stay integers
    res = []
    for bf16 in (True, False):
        wo, bo = V._pack_lin_wide(w.to(DEV), b.to(DEV), C, Cout, 1, F32, bf16)
        bk = dict(C=C, Cout=Cout, wo=wo, bo=bo, wide=True, bf16=bf16)
        y = V.out(x.to(DEV), bk, V._stream(), lvm, "moments" if split else "next")
        if split:                                                # (mean, logvar) (B, half, T, H, W) -> channels-last, logvar unscaled
            y = torch.cat([v.permute(0, 2, 3, 4, 1) for v in y], dim=-1)
            y[..., Cout // 2:] /= torch.exp(lvm)
        res.append(y)
    return (x, w, b), res[0], res[1], lvm


@pytest.mark.parametrize("case", OUT_CASES, ids=_IDS)
def test_out(case):
    """Integers: the product and the bias are exact, the area term is the window's integer sum over its length -- exact too where
    the length is a power of two (512 -> 8: 64), and otherwise (512 -> 6: 86) one correctly rounded fp32 division and one fp32
    addition, which the test forms with the same two IEEE operations.  Gaussian: the logvar half is compared before its scale
    exp(logvar_multiplier) (divided out again in fp32: two roundings of 6e-8, far below the bound)."""
    C, Cout = case[0], case[1]
    (x, w, b), y, y32, _ = _out_run(case, 1)
    want = (BO.out(x, w, b, area=False).float() + _area_fp32(x, Cout)).double()
    if _pow2_windows(C, Cout):
        assert torch.equal(want, O.out(x, w, b))                 # float64 itself
    _exact(f"out exact {_IDS(case)}", y, want)
    args, y, y32, lvm = _out_run(case, 0)
    _judge(f"out {_IDS(case)}", "out", y, y32, args)


def _down_run(case, ints):
    from autoregressive_diffusion_amd import vae as V
    Cin, tc, sc, C, H, W, u8 = case
    B, T, npos = 2, 2, tc * sc * sc
    gen = torch.Generator().manual_seed(7800 + Cin + C + ints)
    w, b = _lin(gen, ints, C, Cin * npos)
    shape = (B, T * tc, H * sc, W * sc, Cin)
    if u8:
        xd = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8).to(DEV)
        x = xd.cpu().float() / 127.5 - 1                         # the two fp32 operations of the load
    else:
        x = _draw(gen, ints, *shape)
        xd = x.to(DEV)
    res = []
    for bf16 in (True, False):
        wd, bd = V._pack_down_wide(w.to(DEV), b.to(DEV), Cin, C, npos, F32, bf16)
        bk = dict(Cin=Cin, C=C, tc=tc, sc=sc, wd=wd, bd=bd, wide_down=True, bf16=bf16)
        res.append(V.down(xd, xd.stride(), (B, T, H, W), bool(u8), bk, V._stream()))
    return (x, w, b, tc, sc), res[0], res[1]


@pytest.mark.parametrize("case", DOWN_CASES, ids=_IDS)
def test_down(case):
    """Integers (not for the uint8 case, whose normalised input is no integer): every area window of these cases has a power-of-two
    length, so the whole result, area term included, equals float64."""
    Cin, tc, sc, C = case[:4]
    if not case[6]:
        args, y, y32 = _down_run(case, 1)
        assert _pow2_windows(Cin * tc * sc * sc, C)
        _exact(f"down exact {_IDS(case)}", y, E.down(*args))
    args, y, y32 = _down_run(case, 0)
    _judge(f"down {_IDS(case)}", "down", y, y32, args)


# ---- whole models

M160_KW = dict(channels=[3, 16, 96, 160, 8], n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
_models = {}


def _model(name):
    """(the model on the GPU in eval mode with mean / std, the switch OFF; kwargs; x, t_sample, noise), built once and left as it
    is: a test that switches works on a deep copy."""
    if name not in _models:
        from autoregressive_diffusion_amd.vae import VAE, VAE512
        stats = dict(mean=[0.05 * i for i in range(8)], std=[1 + 0.1 * i for i in range(8)])
        if name == "m160":
            kw, gen = M160_KW, torch.Generator().manual_seed(6000)
            vae = O.seed_params(VAE(**kw, **stats), 6001)
            x = torch.rand(2, 3, 8, 16, 24, generator=gen) * 2 - 1
            t_sample, noise = torch.rand(2, generator=gen) * 0.1, torch.randn(2, 8, 2, 2, 3, generator=gen)
        else:                                                    # the inputs of test_vae_512_gpu._model("cs512")
            kw, gen = CS512_KW, torch.Generator().manual_seed(5800)
            vae = O.seed_params(VAE512(**kw, **stats), 5801)
            x = torch.rand(1, 3, 8, 16, 16, generator=gen) * 2 - 1
            t_sample, noise = torch.rand(1, generator=gen) * 0.1, torch.randn(1, 8, 2, 2, 2, generator=gen)
        _models[name] = (vae.to(DEV).eval(), kw, x, t_sample, noise)
    return _models[name]


def _switched(name):
    vae = copy.deepcopy(_model(name)[0]).bf16_inference()
    assert vae._bf16_inference is True and _model(name)[0]._bf16_inference is False
    return vae


def _census_delta(fn):
    from autoregressive_diffusion_amd import ops
    before = ops.census_peek()                                   # the suite's own census is running: the difference of two peeks
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v - before.get(k, 0) for k, v in ops.census_peek().items() if v != before.get(k, 0)}


def _inference(vae, x, t_sample, noise):
    xd, td, nd = x.to(DEV), t_sample.to(DEV), noise.to(DEV)
    with torch.no_grad():
        mean = vae.encode(xd)[0]
        r_mean, r_logvar, _ = vae.decode(nd, td)
        f_mean, f_logvar, f_m, _ = vae(xd, t_sample=td, noise=nd)
    return {"encode": mean, "decode mean": r_mean, "decode logvar": r_logvar, "forward mean": f_m, "forward r_mean": f_mean,
            "forward r_logvar": f_logvar}


def _levels(mean):
    return ((mean.float() + 1) * 127.5).clamp(0, 255).to(torch.uint8).int()


@pytest.mark.parametrize("name", ["m160", "cs512"])
def test_model_accuracy(name):
    off, kw, x, t_sample, noise = _model(name)
    sd = {k: v.cpu() for k, v in off.state_dict().items()}
    want, faithful = {}, {}
    for tag, dst in ((False, want), (True, faithful)):
        d = BO.decode(sd, kw, noise, t_sample, faithful=tag)
        f = BO.forward(sd, kw, x, t_sample, noise, faithful=tag)
        dst.update({"encode": f[2], "decode mean": d[0], "decode logvar": d[1], "forward mean": f[2], "forward r_mean": f[0],
                    "forward r_logvar": f[1]})
    got, got32 = _inference(_switched(name), x, t_sample, noise), _inference(off, x, t_sample, noise)
    for k in want:
        Ek, e, e32 = O.rel_l2(faithful[k], want[k]), O.rel_l2(got[k], want[k]), O.rel_l2(got32[k], want[k])
        _note(f"model {name} {k}", E=Ek, rel_l2=e, bound=2 * Ek, fp32_path=e32)
        assert Ek < 2e-2 and e <= 2 * Ek, (k, e, Ek)
    a, b = _levels(got["decode mean"]), _levels(got32["decode mean"])
    _note(f"model {name} uint8 frame bytes", share_beyond_one_level=float(((a - b).abs() > 1).float().mean()), max_levels=int((a - b).abs().max()))


def _smallest_chunk(vae, T):
    tc = int(vae.time_compression)
    for n in range(tc, T + 1, tc):
        try:
            vae._check_groups(n)
            return n
        except ValueError:
            pass
    raise AssertionError("no chunk size")


@pytest.mark.parametrize("name", ["m160", "cs512"])
def test_model_bit_identities(name):
    vae = _switched(name)
    _, kw, x, t_sample, noise = _model(name)
    gen = torch.Generator().manual_seed(7900)
    B, T, H, W = 2, 2 * x.shape[2], x.shape[3], x.shape[4]
    frames = torch.randint(0, 256, (B, T, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)
    whole, _ = vae.encode_frames(frames)
    n, cache, parts = _smallest_chunk(vae, T), None, []
    assert n < T
    for t0 in range(0, T, n):
        part, cache = vae.encode_frames(frames[:, t0:t0 + n], cache)
        parts.append(part)
    assert torch.equal(torch.cat(parts, dim=1), whole)
    lat = torch.randn(B, whole.shape[1], 8, whole.shape[3], whole.shape[4], generator=gen).to(DEV)
    whole_f, _ = vae.decode_frames(lat)
    cache, parts = None, []
    for t0 in range(lat.shape[1]):
        part, cache = vae.decode_frames(lat[:, t0:t0 + 1], cache=cache)
        parts.append(part)
    assert whole_f.dtype == torch.uint8 and torch.equal(torch.cat(parts, dim=1), whole_f)
    # row 0 of the batch of 2 is the same sequence at B = 1; and a second run gives the same bits
    assert torch.equal(vae.encode_frames(frames[:1])[0], whole[:1]) and torch.equal(vae.decode_frames(lat[:1])[0], whole_f[:1])
    assert torch.equal(vae.encode_frames(frames)[0], whole) and torch.equal(vae.decode_frames(lat)[0], whole_f)
    off = _model(name)[0]
    assert not torch.equal(off.decode_frames(lat)[0], whole_f) or not torch.equal(off.encode_frames(frames)[0], whole)     # it is on
    _note(f"model {name} streaming", encoder_chunk_frames=n, latent_frames=lat.shape[1])


FP32_WIDE = ("vae_wide_kernel", "vae_wide_down_kernel", "disc_conv_kernel")
BF16_WIDE = ("vae_wide_bf16_kernel", "vae_wide_down_bf16_kernel")


def _split_census(c, names):
    return {k: v for k, v in c.items() if any(n in k for n in names)}, {k: v for k, v in c.items() if not any(n in k for n in names)}


@pytest.mark.parametrize("name", ["m160", "cs512"])
def test_dispatch_census(name):
    off, kw, x, t_sample, noise = _model(name)
    on = _switched(name)
    run = lambda vae: _inference(vae, x, t_sample, noise)
    run(off), run(on)                                            # packs built, LDS limits raised
    _, c_off = _census_delta(lambda: run(off))
    _, c_on = _census_delta(lambda: run(on))
    wide_off, rest_off = _split_census(c_off, FP32_WIDE + BF16_WIDE)
    wide_on, rest_on = _split_census(c_on, FP32_WIDE + BF16_WIDE)
    assert wide_on and all(any(n in k for n in BF16_WIDE) for k in wide_on), wide_on          # no fp32 matrix kernel with it on
    assert wide_off and all(any(n in k for n in FP32_WIDE) and "bf16" not in k for k in wide_off), wide_off
    assert sum(wide_on.values()) == sum(wide_off.values())       # launch for launch
    assert rest_on == rest_off and sum(rest_on.values()) > 0     # the narrow kernels, the activation pass, the t-embedding
    modes = {int(m) for k in wide_on for m in re.findall(r"vae_wide_bf16_kernel<\d+, ?(\d)>", k)}
    assert modes == {0, 1, 2, 3}, wide_on                        # conv A, up, out, conv B
    assert any("vae_wide_down_bf16_kernel" in k for k in wide_on), wide_on
    _note(f"model {name} census", bf16_launches=sum(wide_on.values()), other_launches=sum(rest_on.values()))


def _train(vae, x, t_sample, noise):
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, mean, _ = vae(x.to(DEV), t_sample=t_sample.to(DEV), noise=noise.to(DEV))
    RT.loss(r_mean, r_logvar, mean).backward()
    return (r_mean, r_logvar, mean), {n: p.grad.detach().clone() for n, p in vae.named_parameters() if p.grad is not None}


def test_off_means_unchanged():
    """On and off again: the bits and the census of a model that was never switched.  The training path: outputs and gradients of
    the switch off, bit for bit, with it on.  Caches: written in one mode, accepted in the other."""
    never, kw, x, t_sample, noise = _model("m160")
    back = copy.deepcopy(never).bf16_inference()
    on = _inference(back, x, t_sample, noise)
    back.bf16_inference(False)
    ref, c_ref = _census_delta(lambda: _inference(never, x, t_sample, noise))
    got, c_got = _census_delta(lambda: _inference(back, x, t_sample, noise))
    assert all(torch.equal(got[k], ref[k]) for k in ref) and c_got == c_ref
    assert not all(torch.equal(on[k], ref[k]) for k in ref)
    # training (a wide model trains once wide_training() says so)
    a, b = copy.deepcopy(never).train().wide_training(), copy.deepcopy(never).train().wide_training().bf16_inference()
    (outs_a, grads_a), ca = _census_delta(lambda: _train(a, x, t_sample, noise))
    (outs_b, grads_b), cb = _census_delta(lambda: _train(b, x, t_sample, noise))
    assert all(o.grad_fn is not None for o in outs_b)
    assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_b))
    assert sorted(grads_a) == sorted(grads_b) and all(torch.equal(grads_a[n], grads_b[n]) for n in grads_a)
    assert ca == cb and not any("bf16_kernel" in k for k in cb), cb
    # caches across the modes: the first half in one mode, the second in the other
    on_m = _switched("m160")
    gen = torch.Generator().manual_seed(7950)
    lat = torch.randn(2, 4, 8, 2, 3, generator=gen).to(DEV)
    frames = torch.randint(0, 256, (2, 16, 16, 24, 3), generator=gen, dtype=torch.uint8).to(DEV)
    for first, second in ((never, on_m), (on_m, never)):
        _, cache = first.decode_frames(lat[:, :2])
        assert all(c["conv3d_res0"].dtype == torch.float32 for blk in cache.values() for c in blk.values())
        part, _ = second.decode_frames(lat[:, 2:], cache=cache)
        assert part.shape == (2, 8, 16, 24, 3) and part.dtype == torch.uint8
        _, cache = first.encode_frames(frames[:, :8])
        part, _ = second.encode_frames(frames[:, 8:], cache)
        assert torch.isfinite(part).all() and part.shape[1] == 2

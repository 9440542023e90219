"""The review of tests/step_edge_oracle.py, on the CPU (thresholds of tests/test_glue_oracle.py):
  1. pin: every restatement equals float64 autograd through the reference formulas (edm2.utils, edm2.conv.Gating,
     edm2.loss_weight, tests/torch_prelude.py, torch.lerp) to 1e-12 relative -- dF, d out_gain, d mse, dparams, dc_all, dgain, de1, de2
     included.  MPFourier casts to float32 itself: its two lines are restated in float64 (and the module checked against that).
  2. not too tight: the same formulas in float32, the reductions in the kernels' summation shape, on the very inputs of the GPU
     cases (tests/step_edge_cases.py) use at most 0.25 of every bound.
  3. not too loose: each deliberate defect, one at a time, moves every element it touches by at least 8 x the bound (where the
     bound is 0 -- exact outputs --: by anything at all).
The figures of 2. and 3. are printed (pytest -s) and recorded in profiles/step_edge_tests.txt."""
import math
import types

import pytest
import torch

import step_edge_cases as SC
import step_edge_oracle as SO
from glue_oracle import bound_bf16, bound_f32, U_F32_64
import torch_prelude

D = torch.float64
SD = SC.SD
torch.set_num_threads(min(16, torch.get_num_threads()))


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(tuple(shape), generator=g, dtype=D)


def _floored(g, *shape, lo=0.5, hi=1.0, signed=True):
    mag = lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=D)
    return mag * (torch.randint(0, 2, shape, generator=g).to(D) * 2 - 1) if signed else mag


def _bfr(t):
    return t.to(torch.bfloat16).to(D)


# ---------------------------------------------------------------------------------------------------------------------
# 1. pin
def _precond_reference(F, images, noise, sigma, og, S):
    """loss.py:17-47 with Precond.forward (networks_edm2.py:278-297) in float64 torch: the packed input, D and the per-frame loss
    of the noised slots.  F (B, S*T, C, HW) plays the raw UNet output."""
    B, T, C = images.shape[:3]
    img = images.reshape(B, T, C, -1)
    x = torch.cat([img] * S, 1) + sigma[:, :, None, None] * noise.reshape(B, S * T, C, -1)
    sg = sigma[:, :, None, None]
    c_skip, c_out, c_in = SD ** 2 / (sg ** 2 + SD ** 2), sg * SD / (sg ** 2 + SD ** 2).sqrt(), 1 / (SD ** 2 + sg ** 2).sqrt()
    Dx = c_skip * x + c_out * (F * og)
    losses = ((Dx[:, -T:] - img) ** 2).mean((2, 3))
    return c_in * x, sigma.log() / 4, losses


@pytest.mark.parametrize("S", [1, 2])
def test_pin_dart_input_loss_and_bwd(S):
    g = _gen(1)
    B, T, C, H, W = 2, 3, 4, 3, 5
    images, noise, sigma = _randn(g, B, T, C, H, W), _randn(g, B, S * T, C, H, W), _randn(g, B, S * T).exp()
    F = _randn(g, B, S * T, C, H * W).requires_grad_()
    og = torch.tensor(0.7, dtype=D, requires_grad=True)
    dl = _randn(g, B, T)
    xin, cn, losses = _precond_reference(F, images, noise, sigma, og, S)
    (losses * dl).sum().backward()
    (xcl, _), (rcn, _) = SO.dart_input(images, noise, sigma, S, SD, 32)
    assert _rel(xcl[..., :C], xin.reshape(B * S * T, C, H * W).transpose(1, 2)) < 1e-12 and _rel(rcn, cn.reshape(-1)) < 1e-12
    assert bool((xcl[..., C] == 1).all()) and float(xcl[..., C + 1:].abs().max()) == 0.0
    Fcl = torch.zeros(B * S * T, H * W, 8, dtype=D)
    Fcl[..., :C] = F.detach().reshape(B * S * T, C, H * W).transpose(1, 2)
    assert _rel(SO.dart_loss(Fcl, images, noise, sigma, 0.7, S, SD)[0], losses.detach()) < 1e-12
    (dF, _), _, (dgain, _) = SO.dart_loss_bwd(Fcl, images, noise, sigma, 0.7, dl, S, SD)
    assert _rel(dF[..., :C], F.grad.reshape(B * S * T, C, H * W).transpose(1, 2)) < 1e-12 and float(dF[..., C:].abs().max()) == 0.0
    assert _rel(dgain, og.grad) < 1e-12
    # the pair rows: the same packed input twice, source row n % (B*T)
    (pair, _), (pcn, _) = SO.dart_input_pair(images, sigma[:, :T], SD, 32)
    one = SO.dart_input(images, None, sigma[:, :T], 1, SD, 32)[0][0]
    assert torch.equal(pair, torch.cat([one, one])) and pcn.numel() == B * T


@pytest.mark.parametrize("nterms", [1, 4])
def test_pin_loss_tail(nterms):
    from edm2.loss_weight import MultiNoiseLoss, FourierSeriesFit
    g = _gen(2)
    B, T, S = 3, 5, 2
    mse, sigma, coef = (torch.rand(B, T, generator=g, dtype=D) + 0.1).requires_grad_(), _randn(g, B, S * T).exp(), _randn(g, 2 * nterms - 1) * 0.3
    mnl = MultiNoiseLoss()
    if nterms != 4:
        mnl.fourier_approximator = FourierSeriesFit(-math.pi, math.pi, num_terms=nterms)
    mnl = mnl.double()
    mnl.fourier_approximator.coefficients.data.copy_(coef.reshape(-1, 1))
    sg = sigma[:, -T:]
    l = mse * (sg ** 2 + SD ** 2) / (sg * SD) ** 2                    # loss.py:34-38
    loss = (l / mnl.calculate_mean_loss(sg)).mean()
    loss.backward()
    (out, _), (dcoef, _) = SO.loss_tail(mse, sigma, (S - 1) * T, coef, nterms, SD)[:2]
    assert _rel(out[0], loss.detach()) < 1e-12 and _rel(out[1], l.detach().mean()) < 1e-12 and _rel(dcoef, mse.grad) < 1e-12


def test_pin_loss_tail_history_is_add_data():
    """Three launches into rings of 7 (n = 15 > cap, starting count 5): read back in chronological order, the rings hold what
    MultiNoiseLoss.add_data's concatenate-and-truncate lists hold (loss_weight.py:30-39)."""
    from edm2.loss_weight import MultiNoiseLoss
    g = _gen(3)
    B, T, cap = 3, 5, 7
    mnl = MultiNoiseLoss()
    mnl.history_size = cap
    rings, count = (torch.zeros(cap), torch.zeros(cap), torch.zeros(cap, dtype=torch.int32)), 0
    for launch in range(3):
        mse, sigma = torch.rand(B, T, generator=g) + 0.1, torch.randn(B, T, generator=g).exp()
        r = SO.loss_tail(mse, sigma, 0, torch.zeros(1), 1, SD, rings, count)
        rings, count = (r[3], r[2][0].float(), r[4]), r[5]
        mnl.add_data(sigma, (mse.double() * (sigma.double() ** 2 + SD ** 2) / (sigma.double() * SD) ** 2).float())
        order = (torch.arange(cap) + count) % cap if count > cap else torch.arange(count)
        assert torch.equal(rings[0][order], mnl.sigmas) and torch.equal(rings[2][order].long(), mnl.positions)
        assert _rel(rings[1][order].double(), mnl.losses.double()) < 1e-6
    assert count == 45


def test_pin_precond_out_and_lerp():
    g = _gen(4)
    N, C, HW = 3, 4, 11
    F, x, sigma = _randn(g, 2 * N, HW, 8), _randn(g, N, C, HW), _randn(g, N).exp()
    sg = sigma.reshape(N, 1, 1)

    def Dref(Fh):
        return SD ** 2 / (sg ** 2 + SD ** 2) * x + sg * SD / (sg ** 2 + SD ** 2).sqrt() * (Fh[..., :C].transpose(1, 2) * 0.7)
    assert _rel(SO.precond_out(F[:N], x, sigma, 0.7, SD)[0], Dref(F[:N])) < 1e-12
    for gw in SC.GUIDANCE:
        want = torch.lerp(Dref(F[N:]), Dref(F[:N]), gw)               # sampler.py:32
        assert _rel(SO.precond_out_guided(F, x, sigma, 0.7, SD, gw)[0], want) < 1e-12


@pytest.mark.parametrize("training", [False, True])
def test_pin_gates_and_bwd(training):
    """edm2.conv.Gating per layer (eval: T = tt; training: T = tt / 2) and tests/torch_prelude.batched_gates for all layers at once."""
    from edm2.conv import Gating
    from autoregressive_diffusion_amd import ops
    g = _gen(5)
    B, tt, L = 2, 6, 3
    T = tt // 2 if training else tt
    nctx = [0, 3, 7]
    mods = [Gating().double().train(training) for _ in range(L)]
    for m in mods:
        for p in m.parameters():
            p.data.add_(_randn(g, *p.shape) * 0.5)
    c_noise = _randn(g, B, tt)
    ra, rb = _randn(g, L, B * tt), _randn(g, L, B * tt)
    gate = torch.stack([m(c_noise, n)[0].reshape(-1) for m, n in zip(mods, nctx)])
    ca, cb = ops.gate_coefs(gate)
    (ca * ra + cb * rb).sum().backward()
    params = torch.stack([torch.cat([m.mult, m.offset, m.min_gating.reshape(1), m.max_gating.reshape(1)]) for m in mods]).detach()
    want = torch.stack([torch.cat([m.mult.grad, m.offset.grad, m.min_gating.grad.reshape(1), m.max_gating.grad.reshape(1)]) for m in mods])
    nc = torch.tensor(nctx, dtype=torch.int32)
    (gca, _), (gcb, _) = SO.gates(c_noise.reshape(-1), params, nc, T)
    assert _rel(gca, ca.detach()) < 1e-12 and _rel(gcb, cb.detach()) < 1e-12
    assert _rel(SO.gates_bwd(c_noise.reshape(-1), params, nc, ra, rb, T)[0], want) < 1e-12
    if not training:
        convs = [types.SimpleNamespace(gating=m) for m in mods]
        res = torch_prelude.batched_gates(convs, c_noise, None, False, nctx, T, lambda n, dev: torch.tensor(n).reshape(-1, 1, 1))
        assert _rel(gca, torch.stack([r[0] for r in res]).detach()) < 1e-12
    assert _rel(SO.gates(c_noise.reshape(-1), params, None, T)[0][0], SO.gates(c_noise.reshape(-1), params, nc * 0, T)[0][0]) == 0.0


def _what(w):
    fan = w.shape[1]
    return w / (1e-4 + w.norm(dim=1, keepdim=True) / fan ** 0.5) / fan ** 0.5          # MPConv in eval, conv.py:14-21,36-42


def test_pin_embed_eval_pre_post():
    from edm2.utils import MPFourier, mp_sum, mp_silu
    g = _gen(6)
    N, cn, cemb, L = 6, 12, 20, 4
    four = MPFourier(cn)
    freqs, phases = four.freqs.double(), four.phases.double()
    c_noise, lab = _randn(g, N), torch.tensor([0, 3, 1, 3, 2, 0])
    wn, wl = _randn(g, cemb, cn), _randn(g, cemb, L)
    f64 = (torch.outer(c_noise, freqs) + phases).cos() * math.sqrt(2)            # utils.py:139-150 in float64
    assert _rel(four(c_noise.float()).double(), f64) < 1e-5
    assert _rel(SO.fourier(c_noise, freqs, phases)[0], f64) < 1e-12
    e = f64 @ _what(wn).t()
    oh = torch.nn.functional.one_hot(lab, L).to(D) * math.sqrt(L)
    want = mp_silu(mp_sum(e, oh @ _what(wl).t(), t=1 / 3))
    assert _rel(SO.embed_eval(c_noise, lab, freqs, phases, wn, wl, L, t=1 / 3)[0], want) < 1e-12
    unl = SO.embed_eval(c_noise, None, freqs, phases, wn, None, L)[0]
    assert _rel(unl, mp_silu(e)) < 1e-12
    for bad in (L, -1):                                                          # out of range: the unlabeled embedding
        assert torch.equal(SO.embed_eval(c_noise, torch.full((N,), bad), freqs, phases, wn, wl, L)[0], unl)
    (pre, _), onehot = SO.embed_pre(c_noise, lab, freqs, phases, 16, L, 8)
    assert _rel(pre[:, :cn], f64) < 1e-12 and float(pre[:, cn:].abs().max()) == 0.0
    assert torch.equal(onehot[:, :L].double(), oh) and float(onehot[:, L:].abs().max()) == 0.0       # (sqrt(4) = 2 is a bf16 value)
    for t in (1 / 3, 0.5, None):
        e1, e2, demb = _randn(g, 50).requires_grad_(), (_randn(g, 50).requires_grad_() if t is not None else None), _randn(g, 50)
        emb = mp_silu(mp_sum(e1, e2, t=t)) if t is not None else mp_silu(e1)
        (emb * demb).sum().backward()
        tt = 1 / 3 if t is None else t
        assert _rel(SO.embed_post(e1, e2, tt)[0], emb.detach()) < 1e-12
        d1, d2 = SO.embed_post_bwd(demb, e1, e2, tt)
        assert _rel(d1[0], e1.grad) < 1e-12 and (t is None or _rel(d2[0], e2.grad) < 1e-12)


def test_pin_emb_scale_and_bwd():
    g = _gen(7)
    N, widths = 9, [5, 8, 3]
    seg = torch.tensor([k for k, w in enumerate(widths) for _ in range(w)], dtype=torch.int32)
    start = torch.tensor([0, 5, 13, 16], dtype=torch.int32)
    c_all, gain, dc = _randn(g, N, 16).requires_grad_(), _randn(g, 3).requires_grad_(), _randn(g, N, 16)
    c = 1 + c_all * gain[seg.long()][None]                                       # networks_edm2.py:78
    (c * dc).sum().backward()
    assert _rel(SO.emb_scale(c_all, gain, seg)[0], c.detach()) < 1e-12
    (dall, _), (part, _), (dgain, _) = SO.emb_scale_bwd(dc, c_all, gain, start)
    assert _rel(dall, c_all.grad) < 1e-12 and _rel(dgain, gain.grad) < 1e-12 and part.shape == (3, 16)
    assert int((part != 0).sum()) == 3 * 9                                       # N = 9 < 16: seven empty row chunks per Block


# ---------------------------------------------------------------------------------------------------------------------
# 2. not too tight: the same formulas in float32, reductions in the kernels' summation shape, on the GPU cases' inputs
def _in_float32(fn):
    SO.DTYPE, SO.KSUM = torch.float32, True
    try:
        return fn()
    finally:
        SO.DTYPE, SO.KSUM = torch.float64, False


def _usage(name, got32, pair, kind):
    ref, mag = pair[0].to(D), pair[1].to(D)
    got32 = got32.to(D).reshape(ref.shape)
    term = {"bf16": U_F32_64, "elem": U_F32_64, "f32": 2 * U_F32_64}[kind] * mag
    live = term > 0
    assert bool(((got32 - ref).abs()[~live] == 0).all()), name
    use = ((got32 - ref).abs()[live] / term[live]).max().item() if bool(live.any()) else 0.0
    line = f"float32-emulation {name}: fp32 term used {use:.3f}"
    assert use <= 0.25, line
    if kind == "bf16":
        whole = bound_bf16(ref, mag)
        useb = ((_bfr(got32) - ref).abs()[live] / whole[live]).max().item() if bool(live.any()) else 0.0
        line += f", bf16 result / whole bound {useb:.3f}"
        assert useb <= 1.0, line
    print(line)


def _both(fn):
    return fn(), _in_float32(fn)


@pytest.mark.parametrize("case", SC.DART_INPUT)
def test_float32_fits_dart_input(case):
    B, S, T, C, H, W, cpad = case
    images, noise, sigma = SC.dart_input_inputs(case)
    for nz in (noise, None):
        r, r32 = _both(lambda: SO.dart_input(images, nz, sigma, S, SD, cpad))
        _usage(f"dart_input{case}[noise={int(nz is not None)}] xcl", r32[0][0], r[0], "bf16")
        _usage(f"dart_input{case} c_noise", r32[1][0], r[1], "elem")


@pytest.mark.parametrize("case", SC.DART_PAIR)
def test_float32_fits_dart_input_pair(case):
    x, sigma = SC.dart_pair_inputs(case)
    r, r32 = _both(lambda: SO.dart_input_pair(x, sigma, SD, 32))
    _usage(f"dart_input_pair{case} xcl", r32[0][0], r[0], "bf16")
    _usage(f"dart_input_pair{case} c_noise", r32[1][0], r[1], "elem")


@pytest.mark.parametrize("case", SC.DART_LOSS)
def test_float32_fits_dart_loss(case):
    B, S, T, C, H, W = case
    F, images, noise, sigma, dl = SC.dart_loss_inputs(case)
    F = torch.nan_to_num(F.float(), nan=0.0)                # (the pad channels are never read)
    r, r32 = _both(lambda: SO.dart_loss(F, images, noise, sigma, 0.7, S, SD))
    _usage(f"dart_loss{case} losses", r32[0], r, "f32")
    b, b32 = _both(lambda: SO.dart_loss_bwd(F, images, noise, sigma, 0.7, dl, S, SD))
    _usage(f"dart_loss{case} dF", b32[0][0], b[0], "bf16")
    _usage(f"dart_loss{case} dgain_part", b32[1][0], b[1], "f32")


@pytest.mark.parametrize("case", SC.LOSS_TAIL)
def test_float32_fits_loss_tail(case):
    B, T, S, nterms, cap, count = case
    mse, sigma, coef, rings = SC.loss_tail_inputs(case)
    r, r32 = _both(lambda: SO.loss_tail(mse, sigma, (S - 1) * T, coef, nterms, SD, rings, count))
    _usage(f"loss_tail{case} out", r32[0][0], r[0], "f32")
    _usage(f"loss_tail{case} dcoef", r32[1][0], r[1], "elem")
    _usage(f"loss_tail{case} ring_loss", r32[2][0], r[2], "elem")
    assert torch.equal(r[3], r32[3]) and torch.equal(r[4], r32[4]) and r[5] == r32[5] == count + B * T


@pytest.mark.parametrize("case", SC.PRECOND)
def test_float32_fits_precond(case):
    F, x, sigma = SC.precond_inputs(case)
    F = torch.nan_to_num(F.float(), nan=0.0)
    N = case[0]
    r, r32 = _both(lambda: SO.precond_out(F[:N], x, sigma, 0.7, SD))
    _usage(f"precond_out{case}", r32[0], r, "elem")
    for gw in SC.GUIDANCE:
        r, r32 = _both(lambda: SO.precond_out_guided(F, x, sigma, 0.7, SD, gw))
        _usage(f"precond_out_guided{case}[g={gw}]", r32[0], r, "elem")


@pytest.mark.parametrize("nctx_kind", SC.NCTX)
@pytest.mark.parametrize("case", SC.GATES + [(4, 294, 7)])
def test_float32_fits_gates(case, nctx_kind):
    sat = case[0] == 4
    if sat and nctx_kind != "mixed":
        return
    c_noise, params, nctx, dca, dcb = SC.gates_inputs(case, nctx_kind, saturated=sat)
    T = case[2]
    r, r32 = _both(lambda: SO.gates(c_noise, params, nctx, T))
    _usage(f"gates{case}[{nctx_kind}] ca", r32[0][0], r[0], "elem")
    _usage(f"gates{case}[{nctx_kind}] cb", r32[1][0], r[1], "elem")
    b, b32 = _both(lambda: SO.gates_bwd(c_noise, params, nctx, dca, dcb, T))
    _usage(f"gates{case}[{nctx_kind}] dparams", b32[0], b, "f32")


@pytest.mark.parametrize("label_kind", ["none", "in-range"])
@pytest.mark.parametrize("case", SC.EMBED_EVAL)
def test_float32_fits_embed_eval(case, label_kind):
    args = SC.embed_eval_inputs(case, label_kind)
    r, r32 = _both(lambda: SO.embed_eval(*args, case[3]))
    _usage(f"embed_eval{case}[{label_kind}] emb", r32[0], r, "bf16")


@pytest.mark.parametrize("t", SC.EMBED_POST_T)
@pytest.mark.parametrize("n", SC.EMBED_POST_N)
def test_float32_fits_embed_post(n, t):
    e1, e2, demb = SC.embed_post_inputs(n, t)
    tt = float(torch.tensor(1 / 3 if t is None else t, dtype=torch.float32))
    r, r32 = _both(lambda: SO.embed_post(e1, e2, tt))
    _usage(f"embed_post(n={n},t={t}) emb", r32[0], r, "bf16")
    b, b32 = _both(lambda: SO.embed_post_bwd(demb, e1, e2, tt))
    _usage(f"embed_post(n={n},t={t}) de1", b32[0][0], b[0], "bf16")
    if e2 is not None:
        _usage(f"embed_post(n={n},t={t}) de2", b32[1][0], b[1], "bf16")


@pytest.mark.parametrize("case", SC.EMBED_PRE)
def test_float32_fits_embed_pre(case):
    N, cn, cnP, L, LP = case
    c_noise, labels, freqs, phases = SC.embed_pre_inputs(case)
    r, r32 = _both(lambda: SO.embed_pre(c_noise, labels, freqs, phases, cnP, L, LP))
    _usage(f"embed_pre{case} four", r32[0][0], r[0], "bf16")


@pytest.mark.parametrize("case", SC.EMB_SCALE)
def test_float32_fits_emb_scale(case):
    c_all, gain, seg, start, dc = SC.emb_scale_inputs(case)
    r, r32 = _both(lambda: SO.emb_scale(c_all, gain, seg))
    _usage(f"emb_scale{case} c", r32[0], r, "elem")
    b, b32 = _both(lambda: SO.emb_scale_bwd(dc, c_all, gain, start))
    _usage(f"emb_scale{case} dc_all", b32[0][0], b[0], "bf16")
    _usage(f"emb_scale{case} dgain_part", b32[1][0], b[1], "f32")
    _usage(f"emb_scale{case} dgain", b32[2][0], b[2], "f32")


# ---------------------------------------------------------------------------------------------------------------------
# 3. not too loose: deliberate defects
def _stands_out(name, bad, pair, kind, touched=None, unit=None):
    ref, mag = pair
    bound = {"bf16": bound_bf16(ref, mag), "f32": bound_f32(mag), "elem": U_F32_64 * mag, "exact": torch.zeros_like(ref)}[kind]
    moved = (bad.to(D) - ref).abs()
    if touched is None:
        touched = moved > 0
    n = int(touched.sum())
    assert n > 0, f"{name}: the defect touches nothing"
    seen = (moved >= 8 * bound) & (moved > 0)
    assert bool(seen[touched].all()), f"{name}: {int((~seen & touched).sum())} of {n} touched elements move by less than 8 x the bound"
    assert bool((moved[~touched] == 0).all()), f"{name}: an element outside the touched set moved"
    live = touched & (bound > 0)
    ratio = (moved[live] / bound[live]).min().item() if bool(live.any()) else float("inf")
    extra = f" = {ratio * unit:.0f} fp32 units of mag (allowed: {unit})" if unit and ratio != float("inf") else ""
    print(f"defect {name}: {n} elements touched, each moves by >= {ratio:.0f} x its bound{extra}")


def _every(t):
    return torch.ones_like(t, dtype=torch.bool)


def _aligned_loss_inputs(g, B, S, T, C, H, W):
    """images > 0, noise < 0, F < 0, all floored: c_skip x - images and c_out out_gain F are both negative, so no e cancels and the
    terms of every sum share a sign.  Sigmas 1, 2, 4, ...: neighbours differ by a factor of two."""
    images = _floored(g, B, T, C, H, W, signed=False)
    noise = -_floored(g, B, S * T, C, H, W, signed=False)
    F = torch.zeros(B * S * T, H * W, 8, dtype=D)
    F[..., :C] = -_bfr(_floored(g, B * S * T, H * W, C, signed=False))
    sigma = (2.0 ** torch.arange(B * S * T, dtype=D)).reshape(B, S * T)
    return F, images, noise, sigma, _floored(g, B, T, signed=False)


def test_defects_of_dart_loss():
    g = _gen(20)
    B, S, T, C, H, W = 1, 2, 3, 4, 5, 7
    F, images, noise, sigma, dl = _aligned_loss_inputs(g, B, S, T, C, H, W)
    args = (F, images, noise, sigma, 0.7)
    loss = SO.dart_loss(*args, S, SD)
    dF, part, _ = SO.dart_loss_bwd(*args, dl, S, SD)
    _stands_out("one pixel missing from a frame's loss", SO.dart_loss(*args, S, SD, _defect="pixel")[0], loss, "f32", _every(loss[0]), 128)
    _stands_out("one pixel missing from d out_gain", SO.dart_loss_bwd(*args, dl, S, SD, _defect="pixel")[1][0], part, "f32",
                _every(part[0]), 128)
    noised = torch.zeros(B, S, T, H * W, 8, dtype=torch.bool)
    noised[:, S - 1, :, :, :C] = True
    noised = noised.reshape(dF[0].shape)
    _stands_out("out_gain applied twice in dF", SO.dart_loss_bwd(*args, dl, S, SD, _defect="gain_twice")[0][0], dF, "bf16", noised)
    clean = torch.zeros(B, S, T, H * W, 8, dtype=torch.bool)
    clean[:, :S - 1, :, :, :C] = True
    _stands_out("the clean slots' dF not zeroed", SO.dart_loss_bwd(*args, dl, S, SD, _defect="clean_not_zeroed")[0][0], dF, "bf16",
                clean.reshape(dF[0].shape))
    _stands_out("the neighbouring frame's sigma (losses)", SO.dart_loss(*args, S, SD, _defect="sigma_next")[0], loss, "f32", _every(loss[0]))


def test_defects_of_dart_input():
    g = _gen(21)
    B, S, T, C, H, W = 2, 2, 3, 4, 3, 5
    images = _floored(g, B, T, C, H, W)
    sigma = (2.0 ** torch.arange(B * S * T, dtype=D)).reshape(B, S * T) / 8
    ref, cn = SO.dart_input(images, None, sigma, S, SD, 32)
    img_ch = torch.zeros_like(ref[0], dtype=torch.bool)
    img_ch[..., :C] = True
    bad, bcn = SO.dart_input(images, None, sigma, S, SD, 32, _defect="sigma_next")
    _stands_out("the neighbouring frame's sigma (xcl)", bad[0], ref, "bf16", img_ch)
    _stands_out("the neighbouring frame's sigma (c_noise)", bcn[0], cn, "elem", _every(cn[0]))
    ones = torch.zeros_like(img_ch)
    ones[..., C:C + 2] = True
    _stands_out("the ones channel at c = C + 1", SO.dart_input(images, None, sigma, S, SD, 32, _defect="ones_at_C+1")[0][0], ref, "bf16", ones)
    # s*T + t read as t: the two slots of a frame share sigma here and their noise has opposite signs everywhere
    n1 = _floored(g, B, 1, T, C, H, W)
    noise = torch.cat([-n1.sign() * _floored(g, B, 1, T, C, H, W, signed=False), n1], 1).reshape(B, S * T, C, H, W)
    sig2 = (2.0 ** torch.arange(B * T, dtype=D)).reshape(B, 1, T).expand(B, S, T).reshape(B, S * T) / 4
    ref2 = SO.dart_input(images, noise, sig2, S, SD, 32)[0]
    second = torch.zeros(B, S, T, H * W, 32, dtype=torch.bool)
    second[:, 1, :, :, :C] = True
    _stands_out("s*T + t read as t", SO.dart_input(images, noise, sig2, S, SD, 32, _defect="st_as_t")[0][0], ref2, "bf16",
                second.reshape(ref2[0].shape))
    # the pair rows taken from n / nsrc: source rows at scales 1, 2, 4, ... under one sigma
    Bp, Tp = 2, 3
    x = _floored(g, Bp, Tp, C, H, W, lo=0.75, signed=False) * (2.0 ** torch.arange(Bp * Tp, dtype=D)).reshape(Bp, Tp, 1, 1, 1)
    sp = torch.full((Bp, Tp), 1.5, dtype=D)
    refp = SO.dart_input_pair(x, sp, SD, 32)[0]
    rows = torch.zeros_like(refp[0], dtype=torch.bool)
    wrong = (torch.arange(2 * Bp * Tp) % (Bp * Tp)) != (torch.arange(2 * Bp * Tp) // (Bp * Tp))
    rows[wrong, :, :C] = True
    _stands_out("the pair rows taken from n / nsrc", SO.dart_input_pair(x, sp, SD, 32, _defect="n_div_nsrc")[0][0], refp, "bf16", rows)


def test_defects_of_gates():
    g = _gen(22)
    L, N, T = 3, 6, 3
    c_noise = _randn(g, N) * 0.3
    params = torch.stack([_floored(g, L), _floored(g, L), _randn(g, L) * 0.2, _randn(g, L) * 0.2, _randn(g, L) * 0.3 - 1, _randn(g, L) * 0.3 + 1], 1)
    nctx = torch.tensor([0, 3, 12], dtype=torch.int32)
    ca, cb = SO.gates(c_noise, params, nctx, T)
    n = torch.arange(N)
    moved_pos = ((n % T) != (n // T)).reshape(1, N).expand(L, N)
    bad = SO.gates(c_noise, params, nctx, T, _defect="n_div_T")
    _stands_out("gate position n / T (ca)", bad[0][0], ca, "elem", moved_pos)
    _stands_out("gate position n / T (cb)", bad[1][0], cb, "elem", moved_pos)
    bad = SO.gates(c_noise, params, nctx, T, _defect="nctx_next")
    _stands_out("nctx of the neighbouring layer (ca)", bad[0][0], ca, "elem", _every(ca[0]))
    _stands_out("nctx of the neighbouring layer (cb)", bad[1][0], cb, "elem", _every(cb[0]))
    dca, dcb = -_floored(g, L, N, signed=False), _floored(g, L, N, signed=False)       # dg > 0 everywhere: the offset sum cannot cancel
    dp = SO.gates_bwd(c_noise, params, nctx, dca, dcb, T)
    col3 = torch.zeros(L, 6, dtype=torch.bool)
    col3[:, 3] = True
    _stands_out("o[3] of gates_bwd not set to the offset sum", SO.gates_bwd(c_noise, params, nctx, dca, dcb, T, _defect="o3_not_set")[0], dp,
                "f32", col3, 128)
    assert torch.equal(dp[0][:, 2], dp[0][:, 3])


def test_defect_lerp_ends_and_branches():
    """Ends swapped (lerp(D3, D2, g)): stands out at every g but 0.5, where lerp is symmetric.  The two BRANCHES of torch.lerp are the
    same polynomial in exact arithmetic: swapping them at g = 0.5 (or anywhere) changes only fp32 roundings, which no bound that a
    float32 evaluation must fit into can tell apart.  That listed defect therefore cannot stand out; what is asserted here is that it
    does not (so nobody mistakes the GPU test for a check of the branch) -- the GPU test pins value and magnitude at both forms."""
    g = _gen(23)
    N, C, HW = 3, 4, 11
    F = torch.zeros(2 * N, HW, 8, dtype=D)
    F[:N, :, :C], F[N:, :, :C] = _bfr(_floored(g, N, HW, C, signed=False)), -_bfr(_floored(g, N, HW, C, signed=False))
    x, sigma = _floored(g, N, C, HW), torch.tensor([0.5, 1.0, 2.0], dtype=D)
    for gw in (0.3, -0.3, 1.7, -2.0, 0.0, 1.0):
        ref = SO.precond_out_guided(F, x, sigma, 0.7, SD, gw)
        _stands_out(f"lerp ends swapped at g = {gw}", SO.precond_out_guided(F, x, sigma, 0.7, SD, gw, _defect="ends_swapped")[0], ref, "elem",
                    _every(ref[0]))
    d3, d2 = SO.precond_out(F[:N], x, sigma, 0.7, SD)[0], SO.precond_out(F[N:], x, sigma, 0.7, SD)[0]
    worst = 0.0
    for gw in SC.GUIDANCE:
        ref, mag = SO.precond_out_guided(F, x, sigma, 0.7, SD, gw)
        other = d2 + gw * (d3 - d2) if abs(gw) >= 0.5 else d3 - (d3 - d2) * (1 - gw)
        worst = max(worst, ((other - ref).abs() / (U_F32_64 * mag)).max().item())
    print(f"defect lerp branches swapped: moves the float64 value by at most {worst:.1e} x the bound (the two forms are one polynomial)")
    assert worst < 1e-6


def test_defects_of_embedding():
    g = _gen(24)
    N, cn, cemb, L = 8, 2, 24, 4
    c_noise, freqs, phases = _randn(g, N), torch.zeros(cn, dtype=D), torch.zeros(cn, dtype=D)      # features = sqrt(2): e ~ 2 > 0
    w_noise = _floored(g, cemb, cn, signed=False)
    w_label = _floored(g, cemb, L, signed=False) * torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=D)    # neighbouring columns differ by >= 1
    labels = torch.arange(N) % L
    args = (c_noise, labels, freqs, phases, w_noise, w_label, L)
    ref = SO.embed_eval(*args)
    for d_ in ("label_off_by_one", "sqrt_L_dropped", "t_swapped"):
        _stands_out(f"embed_eval {d_}", SO.embed_eval(*args, _defect=d_)[0], ref, "bf16", _every(ref[0]))
    # (e1 in [5, 6], e2 in [2, 3]: both mixtures lie where silu' ~ 1, so the swapped weights show in de1 and de2 as the factor 2 they are)
    e1, e2, demb = _bfr(_floored(g, 300, lo=5.0, hi=6.0, signed=False)), _bfr(_floored(g, 300, lo=2.0, hi=3.0, signed=False)), _bfr(_floored(g, 300))
    t = 1 / 3
    ref = SO.embed_post(e1, e2, t)
    _stands_out("mp_sum with t and 1 - t swapped (emb)", SO.embed_post(e1, e2, t, _defect="t_swapped")[0], ref, "bf16", _every(ref[0]))
    r1, r2 = SO.embed_post_bwd(demb, e1, e2, t)
    b1, b2 = SO.embed_post_bwd(demb, e1, e2, t, _defect="t_swapped")
    _stands_out("mp_sum with t and 1 - t swapped (de1)", b1[0], r1, "bf16", _every(r1[0]))
    _stands_out("mp_sum with t and 1 - t swapped (de2)", b2[0], r2, "bf16", _every(r2[0]))


def test_defects_of_emb_scale():
    g = _gen(25)
    N, widths = 40, [8, 16, 8]
    seg = torch.tensor([k for k, w in enumerate(widths) for _ in range(w)], dtype=torch.int32)
    start = torch.tensor([0, 8, 24, 32], dtype=torch.int32)
    c_all, dc = _bfr(_floored(g, N, 32, signed=False)), _floored(g, N, 32, signed=False)        # positive products: no sum cancels
    gain = torch.tensor([0.75, -1.5, 3.0], dtype=D)
    c = SO.emb_scale(c_all, gain, seg)
    border = torch.zeros(N, 32, dtype=torch.bool)
    border[:, [8, 24]] = True
    _stands_out("seg shifted by one column at a block border", SO.emb_scale(c_all, gain, seg, _defect="seg_shifted")[0], c, "elem", border)
    _, part, _ = SO.emb_scale_bwd(dc, c_all, gain, start)
    _stands_out("a row chunk's last row missing from dgain_part", SO.emb_scale_bwd(dc, c_all, gain, start, _defect="last_row")[1][0], part,
                "f32", _every(part[0]), 128)


def test_defects_of_the_history_rings():
    case = (3, 5, 1, 1, 7, 5)
    B, T, S, nterms, cap, count = case
    mse, sigma, coef, rings = SC.loss_tail_inputs(case)
    ref = SO.loss_tail(mse, sigma, 0, coef, nterms, SD, rings, count)
    for d_ in ("slot_off_by_one", "first_entries"):
        bad = SO.loss_tail(mse, sigma, 0, coef, nterms, SD, rings, count, _defect=d_)
        _stands_out(f"{d_} (ring_sigma)", bad[3].double(), (ref[3].double(), ref[3].double().abs()), "exact")
        _stands_out(f"{d_} (ring_loss)", bad[2][0], ref[2], "elem")
        assert int((bad[3] != ref[3]).sum()) == cap and int((bad[2][0] != ref[2][0]).sum()) == cap

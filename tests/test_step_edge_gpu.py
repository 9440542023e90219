"""The step-edge kernels (lower half of csrc/elementwise.hip: dart_input[_pair], dart_loss[_bwd], loss_tail, precond_out[_guided],
gates[_bwd], embed_eval, embed_pre, embed_post[_bwd], emb_scale[_bwd], sampler_update) element by element against their float64
restatements (tests/step_edge_oracle.py, reviewed by tests/test_step_edge_oracle.py).  The C-ABI entry points are called directly,
one call against one restatement fed with exactly the tensors the kernel read; the `ops` wrappers are used only where their plumbing
is under test (the part.sum() of _DartLoss and _EmbScaleFn, the T_off / sigma.stride(0) arguments of loss_tail).

Bounds (derived in tests/step_edge_oracle.py; no element is left out anywhere):
  bf16 outputs               2^-8 |ref| + 2^-18 mag
  fp32 elementwise outputs   2^-18 mag          (D, ca, cb, c, dcoef, c_noise, ring_loss)
  fp32 reductions            2^-17 mag          (losses, dgain_part, out, dparams)
  exact                      ones / pad channels, one-hot, rings, counters, the sampler update, the integer-exact probes
Every output buffer starts as NaN and has 64 guard elements behind it that must come back untouched (tests/step_edge_cases.py has
the shapes, each with the loop or edge it is there for, and the inputs).

Longest chain of fp32 additions behind each reduction (sequential per thread + butterfly + waves):
  dart_loss / dgain_part   C * ceil(HW / 1024) + 6 + 16:  (2,2,3,4,5,7) 26; (1,2,2,8,33,32) 38; (1,1,2,3,64,64) 34; (2,2,1,1,16,16) 23
  loss_tail out            ceil(n / 256) + 6 + 4:  n = 512: 12; n = 15: 11; n = 128: 11
  gates_bwd dparams        ceil(N / 256) + 6 + 2:  N = 6: 9; 1024: 12; 294: 10; 16390: 65 + 8 = 73
  emb_scale_bwd parts      ceil(rows * width / 256) + 6 + 2:  at most 32 + 8 = 40 ((1024, [64, 128]): 64 rows of 128); dgain + 16
  embed_eval               cn <= 512 sequential additions per dot product inside a bf16 output: the fp32 part of that bound is 64
                           roundoffs, so a 512-term chain holds only because rounding errors do not all point the same way; the
                           bf16 rounding itself (2^-8 |ref|) is 2^10 times larger than the whole fp32 part unless the dot product cancels
Every figure is printed as `EDGE <case> <tensor> <worst error / bound>` (pytest -s); profiles/step_edge_tests.txt has them."""
import functools
import math

import pytest
import torch

import oracle_hold as OH
import step_edge_cases as SC
import step_edge_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
SD = SC.SD
GUARD = 64
OG = float(torch.tensor(0.7, dtype=torch.float32))       # out_gain as the kernels read it
torch.set_num_threads(min(16, torch.get_num_threads()))

hold_bf16 = functools.partial(OH.hold_bf16, tag="EDGE")
hold_f32 = functools.partial(OH.hold_f32, tag="EDGE")
hold_f32_elem = functools.partial(OH.hold_f32_elem, tag="EDGE")
hold_exact = functools.partial(OH.hold_exact, tag="EDGE")


def _api():
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    return ops, lib, check


def _g(t):
    return None if t is None else t.to(DEV).contiguous()


class Buf:
    """An output buffer pre-filled with NaN (`init`: with those values) and 64 guard elements behind it."""

    def __init__(self, *shape, dtype=BF16, init=None):
        self.n = math.prod(shape)
        floating = dtype.is_floating_point
        self.flat = OH.out(self.n + GUARD, dtype=dtype, fill=OH.NAN if floating else 0)
        self.mark = 777.0 if floating else 777
        self.flat[self.n:] = self.mark
        self.t = self.flat[:self.n].view(*shape)
        if init is not None:
            self.t.copy_(init.to(dtype))

    def guards_ok(self, case, name):
        assert bool((self.flat[self.n:] == self.mark).all()), f"{case} {name}: the guard elements behind the buffer were written"


def _ptr(ops, x):
    return ops._p(x.t if isinstance(x, Buf) else x)


def _first(pair, C):
    return pair[0][..., :C], pair[1][..., :C]


# ---------------------------------------------------------------------------------------------------------------------
# dart_input / dart_input_pair
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("case", SC.DART_INPUT)
def test_dart_input(case, with_noise):
    """Every shape with noise and with noise = NULL; c_noise requested and with a NULL pointer.  The image channels to the bf16
    bound, the ones channel and every pad channel exactly."""
    ops, lib, check = _api()
    B, S, T, C, H, W, cpad = case
    images, noise, sigma = SC.dart_input_inputs(case)
    if not with_noise:
        noise = None
    name = f"dart_input{case}[noise={int(with_noise)}]"
    ig, ng, sg = _g(images), _g(noise), _g(sigma)
    ref, rcn = SO.dart_input(images, noise, sigma, S, SD, cpad)
    for want_cn in (True, False):
        xcl, cn = Buf(B * S * T, H * W, cpad), (Buf(B * S * T, dtype=F32) if want_cn else None)
        check(lib.oniris_dart_input(ops._p(ig), ops._p(ng), ops._p(sg), _ptr(ops, xcl), B, S, T, C, H, W, SD,
                                    _ptr(ops, cn) if want_cn else None, cpad, ops._stream()), "dart_input")
        torch.cuda.synchronize()
        hold_bf16(name, f"xcl[c<C,cn={int(want_cn)}]", xcl.t[..., :C], _first(ref, C))
        hold_exact(name, f"xcl[c>=C,cn={int(want_cn)}]", xcl.t[..., C:].float(), ref[0][..., C:])
        xcl.guards_ok(name, "xcl")
        if want_cn:
            hold_f32_elem(name, "c_noise", cn.t, rcn)
            cn.guards_ok(name, "c_noise")


def test_dart_input_exact_probe():
    """Small-integer images and noise, power-of-two sigmas and sigma_data = 0: c_in = 1 / sigma and every product are exact."""
    ops, lib, check = _api()
    B, S, T, C, H, W, cpad = 2, 2, 3, 4, 5, 7, 32
    g = SC.gen(7)
    images = torch.randint(-4, 5, (B, T, C, H, W), generator=g).float()
    noise = torch.randint(-4, 5, (B, S * T, C, H, W), generator=g).float()
    sigma = 2.0 ** (torch.arange(B * S * T) % 3 - 1).float().reshape(B, S * T)
    xcl = Buf(B * S * T, H * W, cpad)
    ig, ng, sg = _g(images), _g(noise), _g(sigma)
    check(lib.oniris_dart_input(ops._p(ig), ops._p(ng), ops._p(sg), _ptr(ops, xcl), B, S, T, C, H, W, 0.0, None, cpad, ops._stream()),
          "dart_input")
    torch.cuda.synchronize()
    hold_exact("dart_input exact probe", "xcl", xcl.t.float(), SO.dart_input(images, noise, sigma, S, 0.0, cpad)[0][0])
    xcl.guards_ok("dart_input exact probe", "xcl")


@pytest.mark.parametrize("case", SC.DART_PAIR)
def test_dart_input_pair(case):
    """Both halves of the 2 * B * T rows; c_noise in B * T entries only (the guard behind them stays)."""
    ops, lib, check = _api()
    B, T, C, H, W = case
    x, sigma = SC.dart_pair_inputs(case)
    name = f"dart_input_pair{case}"
    xg, sg = _g(x), _g(sigma)
    xcl, cn = Buf(2 * B * T, H * W, 32), Buf(B * T, dtype=F32)
    check(lib.oniris_dart_input_pair(ops._p(xg), ops._p(sg), _ptr(ops, xcl), B, T, C, H, W, SD, _ptr(ops, cn), 32, ops._stream()),
          "dart_input_pair")
    torch.cuda.synchronize()
    ref, rcn = SO.dart_input_pair(x, sigma, SD, 32)
    hold_bf16(name, "xcl[c<C]", xcl.t[..., :C], _first(ref, C))
    hold_exact(name, "xcl[c>=C]", xcl.t[..., C:].float(), ref[0][..., C:])
    hold_f32_elem(name, "c_noise", cn.t, rcn)
    xcl.guards_ok(name, "xcl")
    cn.guards_ok(name, "c_noise")
    assert torch.equal(xcl.t[:B * T], xcl.t[B * T:])


# ---------------------------------------------------------------------------------------------------------------------
# dart_loss / dart_loss_bwd
@pytest.mark.parametrize("case,og", [(c, OG) for c in SC.DART_LOSS] + [(SC.DART_LOSS[0], 0.0)],
                         ids=[f"case{i}-og0.7" for i in range(len(SC.DART_LOSS))] + ["case0-og0"])
def test_dart_loss_and_bwd(case, og):
    """The losses, dF elementwise (the clean slots and the pad channels have bound 0: exactly 0), dgain_part per frame, and
    out_gain.grad through ops.dart_loss (part.sum()).  out_gain = 0: dF is exactly 0 while dgain is not."""
    ops, lib, check = _api()
    B, S, T, C, H, W = case
    F, images, noise, sigma, dl = SC.dart_loss_inputs(case)
    name = f"dart_loss{case}[og={og:.1f}]"
    Fg, ig, ng, sg, dlg = (_g(t) for t in (F, images, noise, sigma, dl))
    ogg = torch.tensor([og], dtype=F32, device=DEV)
    losses = Buf(B, T, dtype=F32)
    check(lib.oniris_dart_loss(ops._p(Fg), ops._p(ig), ops._p(ng), ops._p(sg), ops._p(ogg), _ptr(ops, losses), B, S, T, C, H, W, SD,
                               ops._stream()), "dart_loss")
    dF, part = Buf(B * S * T, H * W, 8), Buf(B, T, dtype=F32)
    check(lib.oniris_dart_loss_bwd(ops._p(Fg), ops._p(ig), ops._p(ng), ops._p(sg), ops._p(ogg), ops._p(dlg), _ptr(ops, dF),
                                   _ptr(ops, part), B, S, T, C, H, W, SD, ops._stream()), "dart_loss_bwd")
    torch.cuda.synchronize()
    hold_f32(name, "losses", losses.t, SO.dart_loss(F, images, noise, sigma, og, S, SD))
    rdF, rpart, rgain = SO.dart_loss_bwd(F, images, noise, sigma, og, dl, S, SD)
    hold_bf16(name, "dF", dF.t, rdF)
    hold_f32(name, "dgain_part", part.t, rpart)
    for b_, n_ in ((losses, "losses"), (dF, "dF"), (part, "dgain_part")):
        b_.guards_ok(name, n_)
    clean = dF.t.reshape(B, S, T, -1)[:, :S - 1]
    assert float(clean.abs().sum()) == 0.0 and float(dF.t[..., C:].abs().sum()) == 0.0
    if og == 0.0:
        assert float(dF.t.abs().sum()) == 0.0 and bool((part.t != 0).all())
    gain = torch.tensor(og, dtype=F32, device=DEV, requires_grad=True)
    lw = ops.dart_loss(Fg, gain, ig, ng, sg, S, SD)
    lw.backward(dlg)
    torch.cuda.synchronize()
    hold_f32(name, "ops losses", lw, SO.dart_loss(F, images, noise, sigma, og, S, SD))
    hold_f32(name, "out_gain.grad", gain.grad, rgain)


# ---------------------------------------------------------------------------------------------------------------------
# loss_tail
def _launch_loss_tail(mse, sigma, coef, nterms, rings, count, T_off):
    ops, lib, check = _api()
    B, T = mse.shape
    out, dcoef = Buf(2, dtype=F32), Buf(B, T, dtype=F32)
    bufs = None
    if rings is not None:
        cap = rings[0].numel()
        bufs = (Buf(cap, dtype=F32, init=rings[0]), Buf(cap, dtype=F32, init=rings[1]), Buf(cap, dtype=torch.int32, init=rings[2]))
    cnt = Buf(1, dtype=torch.int64, init=torch.tensor([count]))
    mg, sg, cg = _g(mse), _g(sigma), _g(coef)
    check(lib.oniris_loss_tail(ops._p(mg), ops._p(sg), ops._p(cg), _ptr(ops, out), _ptr(ops, dcoef),
                               *([_ptr(ops, b) for b in bufs] if bufs else [None, None, None]), _ptr(ops, cnt),
                               bufs[0].n if bufs else 0, B, T, sigma.shape[1], T_off, nterms, SD, ops._stream()), "loss_tail")
    torch.cuda.synchronize()
    return out, dcoef, bufs, cnt


@pytest.mark.parametrize("case", SC.LOSS_TAIL)
def test_loss_tail(case):
    """out[0], out[1] and dcoef elementwise; ring_sigma, ring_pos and count exactly, ring_loss to its fp32 bound; the slots the
    launch must not touch keep their previous contents (their bound is 0)."""
    B, T, S, nterms, cap, count = case
    mse, sigma, coef, rings = SC.loss_tail_inputs(case)
    name = f"loss_tail{case}"
    out, dcoef, bufs, cnt = _launch_loss_tail(mse, sigma, coef, nterms, rings, count, (S - 1) * T)
    rout, rdcoef, rrl, rrs, rrp, rcount, slots = SO.loss_tail(mse, sigma, (S - 1) * T, coef, nterms, SD, rings, count)
    hold_f32(name, "out", out.t, rout)
    hold_f32_elem(name, "dcoef", dcoef.t, rdcoef)
    hold_exact(name, "ring_sigma", bufs[0].t, rrs)
    hold_f32_elem(name, "ring_loss", bufs[1].t, rrl)
    hold_exact(name, "ring_pos", bufs[2].t, rrp)
    assert int(cnt.t[0]) == rcount == count + B * T
    assert slots.numel() == min(cap, B * T) == slots.unique().numel()
    for b_, n_ in ((out, "out"), (dcoef, "dcoef"), (bufs[0], "ring_sigma"), (bufs[1], "ring_loss"), (bufs[2], "ring_pos"), (cnt, "count")):
        b_.guards_ok(name, n_)


def test_loss_tail_without_history_leaves_count_alone():
    case = (2, 64, 2, 4, 300, 41)
    mse, sigma, coef, _ = SC.loss_tail_inputs(case)
    out, dcoef, _, cnt = _launch_loss_tail(mse, sigma, coef, 4, None, 41, 64)
    rout, rdcoef = SO.loss_tail(mse, sigma, 64, coef, 4, SD)[:2]
    hold_f32("loss_tail no history", "out", out.t, rout)
    hold_f32_elem("loss_tail no history", "dcoef", dcoef.t, rdcoef)
    assert int(cnt.t[0]) == 41
    cnt.guards_ok("loss_tail no history", "count")


def test_loss_tail_wrapper_passes_row_stride_and_offset():
    """ops.loss_tail on sigma as a row-strided view (stride(0) = S*T + 5, three columns in): the wrapper's sig_pitch and T_off."""
    ops, lib, check = _api()
    case = (3, 5, 2, 4, 50, 0)
    B, T, S = case[:3]
    mse, sigma, coef, rings = SC.loss_tail_inputs(case)
    wide = torch.full((B, S * T + 5), OH.NAN, device=DEV)
    wide[:, 3:3 + S * T] = sigma.to(DEV)
    view = wide[:, 3:3 + S * T]
    hist = tuple(_g(r) for r in rings) + (torch.zeros(1, dtype=torch.int64, device=DEV),)
    mg = _g(mse).requires_grad_()
    loss, unweighted = ops.loss_tail(mg, view, _g(coef), hist, SD)
    loss.backward()
    torch.cuda.synchronize()
    rout, rdcoef, rrl, rrs, rrp, rcount, _ = SO.loss_tail(mse, sigma, (S - 1) * T, coef, 4, SD, rings, 0)
    name = "ops.loss_tail strided"
    hold_f32(name, "out", torch.stack([loss.detach(), unweighted]), rout)
    hold_f32_elem(name, "mse.grad", mg.grad, rdcoef)
    hold_exact(name, "ring_sigma", hist[0], rrs)
    hold_f32_elem(name, "ring_loss", hist[1], rrl)
    hold_exact(name, "ring_pos", hist[2], rrp)
    assert int(hist[3][0]) == rcount


# ---------------------------------------------------------------------------------------------------------------------
# precond_out / precond_out_guided
@pytest.mark.parametrize("case", SC.PRECOND)
def test_precond_out_and_guided(case):
    """The plain output of either half, and the guided one at every guidance weight (both lerp forms, their switch at 0.5, weights
    beyond 1 and negative); at g = 0 and g = 1 additionally against the plain restatement of the 2-D / the 3-D half under ITS bound."""
    ops, lib, check = _api()
    N, C, H, W = case
    F, x, sigma = SC.precond_inputs(case)
    name = f"precond_out{case}"
    Fg, xg, sg = _g(F), _g(x), _g(sigma)
    og = torch.tensor([OG], dtype=F32, device=DEV)
    plain = {}
    for half, rows in (("3d", slice(0, N)), ("2d", slice(N, 2 * N))):
        D = Buf(N, C, H * W, dtype=F32)
        Fh = Fg[rows].contiguous()
        check(lib.oniris_precond_out(ops._p(Fh), ops._p(xg), ops._p(sg), ops._p(og), _ptr(ops, D), N, C, H, W, SD, ops._stream()),
              "precond_out")
        torch.cuda.synchronize()
        plain[half] = SO.precond_out(F[rows], x, sigma, OG, SD)
        hold_f32_elem(name, f"D[{half}]", D.t, plain[half])
        D.guards_ok(name, "D")
    for gw in SC.GUIDANCE:
        D = Buf(N, C, H * W, dtype=F32)
        check(lib.oniris_precond_out_guided(ops._p(Fg), ops._p(xg), ops._p(sg), ops._p(og), _ptr(ops, D), N, C, H, W, SD, gw,
                                            ops._stream()), "precond_out_guided")
        torch.cuda.synchronize()
        hold_f32_elem(name, f"D[g={gw}]", D.t, SO.precond_out_guided(F, x, sigma, OG, SD, float(torch.tensor(gw, dtype=F32))))
        D.guards_ok(name, "D guided")
        if gw in (0.0, 1.0):
            hold_f32_elem(name, f"D[g={gw}] vs plain", D.t, plain["2d" if gw == 0.0 else "3d"])


# ---------------------------------------------------------------------------------------------------------------------
# gates / gates_bwd
def _run_gates(name, case, c_noise, params, nctx, dca, dcb):
    ops, lib, check = _api()
    L, N, T = case
    cg, pg, ng, dag, dbg = (_g(t) for t in (c_noise, params, nctx, dca, dcb))
    ca, cb, dparams = Buf(L, N, dtype=F32), Buf(L, N, dtype=F32), Buf(L, 6, dtype=F32)
    check(lib.oniris_gates(ops._p(cg), ops._p(pg), ops._p(ng), _ptr(ops, ca), _ptr(ops, cb), L, N, T, ops._stream()), "gates")
    check(lib.oniris_gates_bwd(ops._p(cg), ops._p(pg), ops._p(ng), ops._p(dag), ops._p(dbg), _ptr(ops, dparams), L, N, T,
                               ops._stream()), "gates_bwd")
    torch.cuda.synchronize()
    rca, rcb = SO.gates(c_noise, params, nctx, T)
    hold_f32_elem(name, "ca", ca.t, rca)
    hold_f32_elem(name, "cb", cb.t, rcb)
    rdp = SO.gates_bwd(c_noise, params, nctx, dca, dcb, T)
    hold_f32(name, "dparams", dparams.t, rdp)
    for b_, n_ in ((ca, "ca"), (cb, "cb"), (dparams, "dparams")):
        b_.guards_ok(name, n_)
    return ca.t.double().cpu(), cb.t.double().cpu(), rca, rcb, dparams.t.double().cpu(), rdp


@pytest.mark.parametrize("nctx_kind", SC.NCTX)
@pytest.mark.parametrize("case", SC.GATES)
def test_gates_and_bwd(case, nctx_kind):
    c_noise, params, nctx, dca, dcb = SC.gates_inputs(case, nctx_kind)
    _run_gates(f"gates{case}[nctx={nctx_kind}]", case, c_noise, params, nctx, dca, dcb)


def test_gates_saturated():
    """Four layers saturated four ways (sv ~ +60, sv ~ -60, lo ~ 1, lo ~ 0 with hi ~ 1): everything stays finite, ca^2 + cb^2 = 1
    within the coefficients' bounds, and the parameter gradients are 0 within theirs where the saturation kills them: d mult, d offset
    of layers 0 and 1 (s (1 - s) ~ e^-60), all six of layer 2 (1 - lo ~ 1e-13)."""
    case = (4, 294, 7)
    c_noise, params, nctx, dca, dcb = SC.gates_inputs(case, "mixed", saturated=True)
    ca, cb, rca, rcb, dp, rdp = _run_gates("gates saturated", case, c_noise, params, nctx, dca, dcb)
    assert bool(torch.isfinite(ca).all() and torch.isfinite(cb).all() and torch.isfinite(dp).all())
    slack = 2 * (ca.abs() * SO.bound_f32_elem(rca[1]) + cb.abs() * SO.bound_f32_elem(rcb[1]))
    assert bool(((ca * ca + cb * cb - 1).abs() <= slack).all())
    zero = torch.zeros(4, 6, dtype=torch.bool)
    zero[:2, :4], zero[2] = True, True
    assert float(rdp[0][zero].abs().max()) < 1e-9 and bool((dp[zero].abs() <= SO.bound_f32(rdp[1][zero]) + 1e-9).all())


# ---------------------------------------------------------------------------------------------------------------------
# embed_eval / embed_pre / embed_post
@pytest.mark.parametrize("label_kind", SC.LABELS)
@pytest.mark.parametrize("case", SC.EMBED_EVAL)
def test_embed_eval(case, label_kind):
    """labels NULL; w_label NULL; labels in range (L - 1 among them); labels L and -1, which give the unlabeled result.  Row 1 of
    w_noise is all zero: unlabeled, emb = 0 there exactly (its bound is 0)."""
    ops, lib, check = _api()
    N, cn, cemb, L = case
    c_noise, labels, freqs, phases, w_noise, w_label = SC.embed_eval_inputs(case, label_kind)
    name = f"embed_eval{case}[labels={label_kind}]"
    dev = [_g(t) for t in (c_noise, labels, freqs, phases, w_noise, w_label)]
    emb = Buf(N, cemb)
    check(lib.oniris_embed_eval(*[ops._p(t) for t in dev], _ptr(ops, emb), N, cn, cemb, L, ops._stream()), "embed_eval")
    torch.cuda.synchronize()
    hold_bf16(name, "emb", emb.t, SO.embed_eval(c_noise, labels, freqs, phases, w_noise, w_label, L))
    emb.guards_ok(name, "emb")
    if label_kind != "in-range":
        assert float(emb.t[:, 1].abs().max()) == 0.0
        unl = SO.embed_eval(c_noise, None, freqs, phases, w_noise, None, L)
        hold_bf16(name, "emb vs unlabeled", emb.t, unl)


@pytest.mark.parametrize("case", SC.EMBED_PRE)
def test_embed_pre(case):
    """The Fourier features to the bf16 bound, their padding exactly; the one-hot rows exactly: bf16(float32 sqrt(L)) at the label."""
    ops, lib, check = _api()
    N, cn, cnP, L, LP = case
    c_noise, labels, freqs, phases = SC.embed_pre_inputs(case)
    name = f"embed_pre{case}"
    cg, lg, fg, pg = (_g(t) for t in (c_noise, labels, freqs, phases))
    four, oh = Buf(N, cnP), (Buf(N, LP) if L else None)
    check(lib.oniris_embed_pre(ops._p(cg), ops._p(lg), ops._p(fg), ops._p(pg), _ptr(ops, four), _ptr(ops, oh) if L else None, N, cn,
                               cnP, L or 0, LP or 0, ops._stream()), "embed_pre")
    torch.cuda.synchronize()
    rfour, roh = SO.embed_pre(c_noise, labels, freqs, phases, cnP, L, LP)
    hold_bf16(name, "four", four.t, rfour)
    four.guards_ok(name, "four")
    if cnP > cn:
        assert float(four.t[:, cn:].abs().max()) == 0.0
    if L:
        hold_exact(name, "onehot", oh.t.float(), roh)
        oh.guards_ok(name, "onehot")


@pytest.mark.parametrize("t", SC.EMBED_POST_T)
@pytest.mark.parametrize("n", SC.EMBED_POST_N)
def test_embed_post_and_bwd(n, t):
    ops, lib, check = _api()
    e1, e2, demb = SC.embed_post_inputs(n, t)
    tt = 1 / 3 if t is None else t
    tf = float(torch.tensor(tt, dtype=F32))               # the C ABI takes a float
    name = f"embed_post(n={n},t={'null' if t is None else round(t, 3)})"
    e1g, e2g, dg = _g(e1), _g(e2), _g(demb)
    emb, de1, de2 = Buf(n), Buf(n), (Buf(n) if e2 is not None else None)
    check(lib.oniris_embed_post(ops._p(e1g), ops._p(e2g), _ptr(ops, emb), n, tf, ops._stream()), "embed_post")
    check(lib.oniris_embed_post_bwd(ops._p(dg), ops._p(e1g), ops._p(e2g), _ptr(ops, de1), _ptr(ops, de2) if de2 else None, n, tf,
                                    ops._stream()), "embed_post_bwd")
    torch.cuda.synchronize()
    hold_bf16(name, "emb", emb.t, SO.embed_post(e1, e2, tf))
    r1, r2 = SO.embed_post_bwd(demb, e1, e2, tf)
    hold_bf16(name, "de1", de1.t, r1)
    emb.guards_ok(name, "emb")
    de1.guards_ok(name, "de1")
    if e2 is not None:
        hold_bf16(name, "de2", de2.t, r2)
        de2.guards_ok(name, "de2")


# ---------------------------------------------------------------------------------------------------------------------
# emb_scale / emb_scale_bwd
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("case", SC.EMB_SCALE)
def test_emb_scale_and_bwd(case, exact):
    """c, dc_all and every one of the K * 16 partial sums (an empty row chunk's must be WRITTEN 0: the buffer starts as NaN);
    gain.grad through ops._EmbScaleFn (part.sum(1)).  `exact`: the integer-exact probe."""
    ops, lib, check = _api()
    N, widths = case
    c_all, gain, seg, start, dc = SC.emb_scale_inputs(case, exact)
    Ct, K = sum(widths), len(widths)
    name = f"emb_scale({N},{widths})" + ("[exact]" if exact else "")
    cag, gg, sgg, stg, dcg = (_g(t) for t in (c_all, gain, seg, start, dc))
    c, dall, part = Buf(N, Ct, dtype=F32), Buf(N, Ct), Buf(K, SO.EMB_BWD_CHUNKS, dtype=F32)
    check(lib.oniris_emb_scale(ops._p(cag), ops._p(gg), ops._p(sgg), _ptr(ops, c), N, Ct, ops._stream()), "emb_scale")
    check(lib.oniris_emb_scale_bwd(ops._p(dcg), ops._p(cag), ops._p(gg), ops._p(stg), _ptr(ops, dall), _ptr(ops, part), N, Ct, K,
                                   ops._stream()), "emb_scale_bwd")
    torch.cuda.synchronize()
    rc = SO.emb_scale(c_all, gain, seg)
    rall, rpart, rgain = SO.emb_scale_bwd(dc, c_all, gain, start)
    cagr, ggr = cag.clone().requires_grad_(), gg.clone().requires_grad_()
    ops._EmbScaleFn.apply(cagr, ggr, sgg, stg).backward(dcg)
    torch.cuda.synchronize()
    if exact:
        hold_exact(name, "c", c.t, rc[0])
        hold_exact(name, "dc_all", dall.t.float(), rall[0])
        hold_exact(name, "dgain_part", part.t, rpart[0])
        hold_exact(name, "gain.grad", ggr.grad, rgain[0])
    else:
        hold_f32_elem(name, "c", c.t, rc)
        hold_bf16(name, "dc_all", dall.t, rall)
        hold_f32(name, "dgain_part", part.t, rpart)
        hold_f32(name, "gain.grad", ggr.grad, rgain)
        hold_bf16(name, "c_all.grad", cagr.grad, rall)
    for b_, n_ in ((c, "c"), (dall, "dc_all"), (part, "dgain_part")):
        b_.guards_ok(name, n_)


# ---------------------------------------------------------------------------------------------------------------------
# sampler_update
@pytest.mark.parametrize("nsig", [0, 7, 1000])
@pytest.mark.parametrize("mode,aliased", [(0, False), (1, False), (1, True)])
def test_sampler_update(mode, aliased, nsig):
    """n = 1000 (a ragged fourth block); sigma_buf of 0, 7 and n entries; mode 1 with x_out distinct from x_hat and with the two one
    buffer.  Bit-exact against the reference's float32 tensor expressions."""
    ops, lib, check = _api()
    n, t_a, dt, s_next = 1000, 37.25, -16.125, 21.125
    g = SC.gen(1100 + mode)
    x_hat, x_pred, d_in, x_aux = SC.rn(g, n, scale=40.0), SC.rn(g, n), SC.rn(g, n), SC.rn(g, n, scale=30.0)
    want_x, want_d = SO.sampler_update(mode, x_hat, x_pred, d_in, x_aux, t_a, dt)
    name = f"sampler_update(mode={mode},aliased={int(aliased)},nsig={nsig})"
    xh, d_io = Buf(n, dtype=F32, init=x_hat), Buf(n, dtype=F32, init=d_in)
    xo = xh if aliased else Buf(n, dtype=F32)
    sig = Buf(max(nsig, 1), dtype=F32)
    xpg, xag = _g(x_pred), _g(x_aux)
    check(lib.oniris_sampler_update(mode, _ptr(ops, xh), ops._p(xpg), _ptr(ops, d_io), ops._p(xag) if mode == 1 else None,
                                    _ptr(ops, xo), n, t_a, dt, _ptr(ops, sig) if nsig else None, nsig, s_next, ops._stream()),
          "sampler_update")
    torch.cuda.synchronize()
    hold_exact(name, "x_out", xo.t, want_x)
    hold_exact(name, "d_io", d_io.t, want_d)
    hold_exact(name, "x_hat", xh.t, x_hat if mode == 0 else want_x)
    if nsig:
        hold_exact(name, "sigma_buf", sig.t, torch.full((nsig,), s_next))
    else:
        assert bool(torch.isnan(sig.t).all())
    for b_, n_ in ((xh, "x_hat"), (d_io, "d_io"), (xo, "x_out"), (sig, "sigma_buf")):
        b_.guards_ok(name, n_)

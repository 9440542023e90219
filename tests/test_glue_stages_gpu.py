"""The magnitude-preserving glue kernels (csrc/elementwise.hip: act_fwd / act_bwd, emb_silu_bwd, mpsum_bwd, mpsum_mask, resample,
resample_filter; csrc/weights.hip: gconv_bwd_prep, gconv_bwd_fused modes 1 and 2) element by element against their float64
restatements (tests/glue_oracle.py, reviewed by tests/test_glue_oracle.py).  The C-ABI entry points are called directly, one call
against one restatement fed with exactly the tensors the kernel read; ops.act / ops.resample are used where their autograd plumbing
(GradSlot, the resampled input) is what is under test.  Kernels with an <NT> template run under both `nt_policy` settings.

Bounds (derived, not fitted; no element is left out anywhere):
  bf16 outputs      |got - ref| <= 2^-8 |ref| + 2^-18 mag     one bf16 rounding + 64 fp32 unit roundoffs (<= ~20 fp32 operations
                                                               per element and the ~1 ulp hardware exp2 / rcp)
  fp32 reductions   |got - ref| <= 2^-17 mag                   128 fp32 unit roundoffs
  linear kernels    additionally torch.equal on integer-exact probes (sparse ternary tensors times small integers, power-of-two
                    coefficients: every output and every sum is exactly representable)
`mag` is the reference expression with every addend replaced by its absolute value.  Inputs keep |z| <= 8.  A bf16 intermediate that
a later expression reads (xo for a, dout for the gate sums) is taken from the kernel's own output, itself held to its bound, so that
a rounding tie cannot leak from one tensor into the next.

Longest chain of fp32 additions behind each reduction (sequential per thread + butterfly + waves + slices):
  sden                 8 + log2(C / 8) <= 14
  emb_silu_bwd dc      (3,37,8) 11; (2,2049,64) 33 + 3 + 4 + 1 = 41; (2,300,40) 6 + 51 = 57; (1,64,512) 16 + 4 = 20; (5,130,96) 7 + 21 = 28
  gconv_bwd_fused dcs  the same scheme: at most 17 + 3 + 4 + 1 = 25 ((2,2,1025,64))
  gconv_bwd_fused dca / dcb   8 per pixel: (1,3,37,8) 18; (1,2,300,40) 35; (1,1,64,512) 75; (2,2,1025,64) 8 * 17 + 6 + 4 + 1 = 147 --
                       that one is longer than the 128 the bound is made of: it holds there only because rounding errors do not
                       all point the same way (measured: profiles/glue_stage_tests.txt)
                       (2^-17 mag of a sum over P * C elements is many times one element's term: what a single lost element
                       does to these sums is the integer-exact probes' part, a lost pixel or slice the bound's)
  gconv_bwd_prep       (1,2,3,296) 18; (2,2,2,8200) 35; (1,1,4,4096) 26

Out of scope: the 1024-thread form of gconv_bwd_fused mode 1 is chosen only by an environment knob (ONIRIS_GCONV_BWD_THREADS) that
is read once per process; the default never launches it.
Every figure is printed as `GLUE <case> <tensor> <worst error / bound>` (pytest -s); profiles/glue_stage_tests.txt has them."""
import ctypes

import pytest
import torch

import glue_oracle as GO
from oracle_hold import out as _out, ratio as _ratio, hold_bf16, hold_f32, hold_exact

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
torch.set_num_threads(min(16, torch.get_num_threads()))


def _api():
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    return ops, lib, check


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape, scale=1.0, lim=8.0):
    """bf16 normal values on the CPU, |v| <= lim."""
    return (torch.randn(*shape, generator=gen) * scale).clamp(-lim, lim).to(BF16)


def _probe(gen, *shape, density=0.3, top=4):
    """Integer-exact probe: sparse ternary times small integers."""
    sign = torch.randint(-1, 2, shape, generator=gen)
    keep = torch.rand(*shape, generator=gen) < density
    return (sign * keep * torch.randint(1, top + 1, shape, generator=gen)).to(BF16)


def _pow2(gen, *shape, signed=False):
    v = 2.0 ** torch.randint(-1, 2, shape, generator=gen).float()
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return v


def _g(t):
    return None if t is None else t.to(DEV).contiguous()


# (the NaN-prefilled buffers and the three kinds of comparison are shared with test_step_edge_gpu.py: tests/oracle_hold.py)


# ---------------------------------------------------------------------------------------------------------------------
# act_fwd -> act_bwd
ACT_CASES = [(8, 0, True, 77), (512, 0, True, 50), (24, 8, True, 203), (40, 0, False, 103), (64, 32, False, 129)]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("C1,C2,norm,npix", ACT_CASES)
def test_act_fwd_bwd(C1, C2, norm, npix):
    """C = 8: one thread per pixel; C = 512: the full 64-lane butterfly, 12.5 blocks; (24, 8): pixel norm together with mp_cat;
    C = 40: five threads per pixel, pixels straddle waves and blocks (515 threads); every pixel-norm case holds an all-zero pixel
    (xo = a = 0, sden = 1e-4, dx = g * w1 / 1e-4: the zero-subgradient convention).  Backward with and without dxo (dxo_scale = 0.75)
    and with and without dadd."""
    ops, lib, check = _api()
    gen = _gen(1000 + C1 + C2)
    C = C1 + C2
    case = f"act({C1},{C2},norm={int(norm)},{npix})"
    x, skip = _rn(gen, npix, C1, scale=2.0), (_rn(gen, npix, C2) if C2 else None)
    w1, w2 = (0.75, 1.25) if C2 else (1.0, 1.0)
    if norm:
        x[5] = 0
        if C2:
            skip[5] = 0
    xg, sg = _g(x), _g(skip)
    xo, a, sden = _out(npix, C), _out(npix, C), (_out(npix, dtype=torch.float32) if norm else None)
    check(lib.oniris_act_fwd(ops._p(xg), ops._p(sg), ops._p(xo), ops._p(a), ops._p(sden), npix, C1, C2, w1, w2, int(norm), 0, 0, 0,
                             ops._stream()), "act_fwd")
    torch.cuda.synchronize()
    _, rxo, ra, rs = GO.act_fwd(x, skip, w1, w2, norm, xo_bf16=xo)
    hold_bf16(case, "xo", xo, rxo)
    hold_bf16(case, "a", a, ra)
    if norm:
        hold_f32(case, "sden", sden, rs)
        assert float(xo[5].abs().max()) == 0.0 and float(a[5].abs().max()) == 0.0 and abs(float(sden[5]) - 1e-4) < 1e-9
    da, dxo, dadd = _rn(gen, npix, C), _rn(gen, npix, C), _rn(gen, npix, C1)
    for with_dxo in (True, False):
        for with_dadd in (True, False):
            dx, dskip = _out(npix, C1), (_out(npix, C2) if C2 else None)
            dxo_, dadd_ = (dxo if with_dxo else None), (dadd if with_dadd else None)
            dag, dxog, daddg = _g(da), _g(dxo_), _g(dadd_)
            check(lib.oniris_act_bwd(ops._p(dag), ops._p(dxog), ops._p(xo), ops._p(sden), ops._p(dx), ops._p(dskip),
                                     ops._p(daddg), npix, C1, C2, w1, w2, int(norm), 0.75, ops._stream()), "act_bwd")
            torch.cuda.synchronize()
            rdx, rdskip = GO.act_bwd(da, dxo_, xo, sden, dadd_, C1, C2, w1, w2, norm, 0.75)
            tag = f"dxo={int(with_dxo)},dadd={int(with_dadd)}"
            hold_bf16(case, f"dx[{tag}]", dx, rdx)
            if C2:
                hold_bf16(case, f"dskip[{tag}]", dskip, rdskip)
            if norm and not with_dxo and not with_dadd:   # the all-zero pixel: dx = g * w1 / 1e-4
                want = (da[5, :C1].double() * 0.5 / GO.SILU_DIV) * w1 / float(sden[5])
                assert bool(((dx[5].double().cpu() - want).abs() <= GO.U_BF16 * want.abs() * 1.001).all())


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("with_dxo,with_dadd", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("rs,norm,C1,C2", [(1, True, 16, 16), (2, False, 24, 8)])
def test_act_resampled_input_and_parked_gradients(rs, norm, C1, C2, with_dxo, with_dadd):
    """ops.act(..., resample=...): rs = 1 at N = 2 on an output grid of 3 x 5, rs = 2 at N = 2 on an output grid of 4 x 6.  with_dadd: a
    gradient of the un-resampled input is parked in its GradSlot; with_dxo: the gradient of xo is parked in xo's slot as (g, 0.75), which
    reaches act_bwd as dxo_scale.  Forward: xo and a against the restatement on the bf16-resampled input.  Backward: x.grad =
    resample^T(dx) + parked, two kernels with the bf16 dx between them -- the act_bwd bound of dx is carried through the resampling
    adjoint (a linear map with positive weights) and added to that stage's own bound."""
    ops, lib, check = _api()
    gen = _gen(2000 + rs)
    N, Ho, Wo = (2, 3, 5) if rs == 1 else (2, 4, 6)
    Hi, Wi = (2 * Ho, 2 * Wo) if rs == 1 else (Ho // 2, Wo // 2)
    case = f"ops.act(rs={rs},norm={int(norm)},{C1}+{C2},dxo={int(with_dxo)},dadd={int(with_dadd)})"
    x, skip = _rn(gen, N, Hi, Wi, C1, scale=2.0), _rn(gen, N, Ho, Wo, C2)
    parked, da, dxo = _rn(gen, N, Hi, Wi, C1), _rn(gen, N, Ho, Wo, C1 + C2), _rn(gen, N, Ho, Wo, C1 + C2)
    if not with_dadd:
        parked = None
    if not with_dxo:
        dxo = None
    w1, w2 = 0.75, 1.25
    xg, sg = _g(x).requires_grad_(), _g(skip).requires_grad_()
    in_slot, xo_slot = ops.GradSlot(), (ops.GradSlot() if with_dxo else None)
    if with_dadd:
        in_slot.put(_g(parked))
    xo, a = ops.act(xg, sg, w1, w2, norm=norm, want_xo=True, in_slot=in_slot, resample="down" if rs == 1 else "up", xo_slot=xo_slot)
    if with_dxo:
        xo_slot.put(_g(dxo), 0.75)
    a.backward(_g(da))
    torch.cuda.synchronize()
    left = [s_ for s_ in (in_slot, xo_slot) if s_ is not None and s_.g is not None]
    ops.GradSlot.live.clear()
    assert not left, "a parked gradient was not taken"
    assert tuple(xo.shape) == (N, Ho, Wo, C1 + C2) and tuple(xg.grad.shape) == tuple(x.shape)
    _, rxo, ra, rsd = GO.act_fwd(x, skip, w1, w2, norm, rs, Ho, Wo, xo_bf16=xo)
    hold_bf16(case, "xo", xo, rxo)
    hold_bf16(case, "a", a, ra)
    sden = rsd[0].float() if norm else None                # (the kernel's own sden stays inside ops.act: the restatement's, as fp32)
    (dx, mdx), rdskip = GO.act_bwd(da, dxo, xo, sden, None, C1, C2, w1, w2, norm, 0.75)
    hold_bf16(case, "dskip", sg.grad, rdskip)
    mode, scale = (1, 0.25) if rs == 1 else (0, 4.0)
    shape = (N, Ho, Wo, C1)
    ref, mag = GO.resample(dx.reshape(shape), mode, (0.5, 0.5), scale, parked)
    carried = GO.resample(GO.bound_bf16(dx, mdx).reshape(shape), mode, (0.5, 0.5), scale)[0]
    _ratio(case, "dx", xg.grad, ref, GO.bound_bf16(ref, mag) + carried)


# ---------------------------------------------------------------------------------------------------------------------
# emb_silu_bwd
@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("N,P,C,pitch,dc_is_zero", [(3, 37, 8, 0, 1), (2, 2049, 64, 0, 1), (2, 300, 40, 0, 1), (1, 64, 512, 520, 1),
                                                    (5, 130, 96, 0, 0)])
def test_emb_silu_bwd(N, P, C, pitch, dc_is_zero):
    """(2,2049,64): two pixel slices of 1025; (2,300,40): the sequential branch (five channel groups, an idle tail thread);
    (1,64,512): c_pitch = 520 > C, the padding is NaN; (5,130,96): dc_is_zero = 0 with dc pre-filled with NaN."""
    ops, lib, check = _api()
    gen = _gen(3000 + C)
    case = f"emb_silu_bwd({N},{P},{C},pitch={pitch},zero={dc_is_zero})"
    du, y = _rn(gen, N, P, C), _rn(gen, N, P, C, scale=2.0, lim=5.0)
    c = torch.rand(N, C, generator=gen) + 0.5
    cfull = torch.full((N, pitch or C), NAN)
    cfull[:, :C] = c
    dy, dc = _out(N, P, C), _out(N, C, dtype=torch.float32, fill=0.0 if dc_is_zero else NAN)
    dug, yg, cg = _g(du), _g(y), _g(cfull)
    check(lib.oniris_emb_silu_bwd(ops._p(dug), ops._p(yg), ops._p(cg), ops._p(dy), ops._p(dc), N, P, C, pitch, dc_is_zero,
                                  ops._stream()), "emb_silu_bwd")
    torch.cuda.synchronize()
    rdy, rdc = GO.emb_silu_bwd(du, y, c)
    hold_bf16(case, "dy", dy, rdy)
    hold_f32(case, "dc", dc, rdc)


# ---------------------------------------------------------------------------------------------------------------------
# mpsum_bwd / mpsum_mask
def _clipped_out(gen, n, clip=256.0):
    """A forward output with elements at exactly +-clip and one bf16 step inside it (255 for clip 256)."""
    out = _rn(gen, n, scale=100.0, lim=clip)
    out[::7], out[1::7], out[2::7], out[3::7] = clip, -clip, clip - 1, -(clip - 1)
    return out


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("clip", [0.0, 256.0])
@pytest.mark.parametrize("with_dv", [True, False])
@pytest.mark.parametrize("exact", [False, True])
def test_mpsum_bwd(clip, with_dv, exact):
    ops, lib, check = _api()
    gen = _gen(4000)
    n = 8 * (3 * 256 + 5)
    ta, tb = (0.5, 2.0) if exact else (0.8, 0.6)
    g, out = (_probe(gen, n) if exact else _rn(gen, n)), _clipped_out(gen, n)
    dres, dv = _out(n), (_out(n) if with_dv else None)
    gg, og = _g(g), _g(out)
    check(lib.oniris_mpsum_bwd(ops._p(gg), ops._p(og) if clip > 0 else None, ops._p(dres), ops._p(dv), n, ta, tb, clip,
                               ops._stream()), "mpsum_bwd")
    torch.cuda.synchronize()
    rres, rv = GO.mpsum_bwd(g, out, ta, tb, clip)
    case = f"mpsum_bwd(clip={clip},dv={int(with_dv)})"
    if exact:
        hold_exact(case, "dres", dres, rres[0])
        if with_dv:
            hold_exact(case, "dv", dv, rv[0])
    else:
        hold_bf16(case, "dres", dres, rres)
        if with_dv:
            hold_bf16(case, "dv", dv, rv)
    if clip > 0:
        assert float(dres[out.abs().to(DEV) == clip].abs().max()) == 0.0
        inside = (out.abs() == clip - 1) & (g != 0)
        assert bool((dres.cpu()[inside] != 0).all())


@pytest.mark.parametrize("flag", [0, 1])
def test_mpsum_mask(flag):
    ops, lib, check = _api()
    gen = _gen(4100)
    n = 8 * (3 * 256 + 5)
    g, out = _rn(gen, n), _clipped_out(gen, n)
    gg, og, fl = _g(g).clone(), _g(out), torch.tensor([flag], dtype=torch.int32, device=DEV)
    check(lib.oniris_mpsum_mask(ops._p(gg), ops._p(og), n, 256.0, ops._p(fl), ops._stream()), "mpsum_mask")
    torch.cuda.synchronize()
    hold_exact(f"mpsum_mask(flag={flag})", "g", gg, GO.mpsum_mask(g, out, 256.0, flag)[0])


_BIG = {}


def _big_mpsum(n):
    if n not in _BIG:
        gen = _gen(n)
        g, out = _probe(gen, n), _clipped_out(gen, n)
        keep = (out.float().abs() < 256.0)
        _BIG[n] = (g, out, (g.float() * keep * 0.5).to(BF16), (g.float() * keep * 2.0).to(BF16), (g.float() * keep).to(BF16))
    return _BIG[n]


@pytest.mark.usefixtures("nt_policy")
def test_mpsum_bwd_second_grid_trip():
    """numel = 8 * (2 097 152 + 1000): the grid is capped at 8192 blocks, the last 1000 vectors are a second trip of the loop."""
    ops, lib, check = _api()
    n = 8 * (2097152 + 1000)
    g, out, wres, wv, _ = _big_mpsum(n)
    dres, dv = _out(n), _out(n)
    gg, og = _g(g), _g(out)
    check(lib.oniris_mpsum_bwd(ops._p(gg), ops._p(og), ops._p(dres), ops._p(dv), n, 0.5, 2.0, 256.0, ops._stream()), "mpsum_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dres.cpu(), wres) and torch.equal(dv.cpu(), wv)


def test_mpsum_mask_second_grid_trip():
    """numel = 8 * (524 288 + 777) with the flag set: the grid is capped at 2048 blocks."""
    ops, lib, check = _api()
    n = 8 * (524288 + 777)
    g, out, _, _, wg = _big_mpsum(n)
    gg, og, fl = _g(g).clone(), _g(out), torch.ones(1, dtype=torch.int32, device=DEV)
    check(lib.oniris_mpsum_mask(ops._p(gg), ops._p(og), n, 256.0, ops._p(fl), ops._stream()), "mpsum_mask")
    torch.cuda.synchronize()
    assert torch.equal(gg.cpu(), wg)


# ---------------------------------------------------------------------------------------------------------------------
# gconv_bwd_prep
@pytest.mark.parametrize("B,S,T,fe", [(1, 2, 3, 296), (2, 2, 2, 8200), (1, 1, 4, 4096)])
@pytest.mark.parametrize("exact", [False, True])
def test_gconv_bwd_prep(B, S, T, fe, exact):
    """(2,2,2,8200): two slices over an odd count of 16-byte vectors (1025); (1,1,4,4096): S = 1 (the 2-D steps)."""
    ops, lib, check = _api()
    gen = _gen(5000 + fe)
    case = f"gconv_bwd_prep({B},{S},{T},{fe})"
    if exact:
        dout, out, y3 = _probe(gen, B, S, T, fe), _probe(gen, B, S, T, fe), _probe(gen, B, T, fe)
        ca, cb = _pow2(gen, B, S, T), _pow2(gen, B, S, T, signed=True)
    else:
        dout, out, y3 = _rn(gen, B, S, T, fe), _rn(gen, B, S, T, fe), _rn(gen, B, T, fe)
        ca, cb = torch.rand(B, S, T, generator=gen) * 0.5 + 0.5, torch.rand(B, S, T, generator=gen) - 0.5
    dca, dcb = _out(B, S, T, dtype=torch.float32, fill=0.0), _out(B, S, T, dtype=torch.float32, fill=0.0)
    dy3 = _out(B, T, fe)
    dev = [_g(t) for t in (dout, out, y3, ca, cb)]
    check(lib.oniris_gconv_bwd_prep(*[ops._p(t) for t in dev], ops._p(dca), ops._p(dcb), ops._p(dy3), B, S, T, fe, ops._stream()),
          "gconv_bwd_prep")
    torch.cuda.synchronize()
    rca, rcb, ry3 = GO.gconv_prep(dout, out, y3, ca, cb, S)
    if exact:
        hold_exact(case, "dca", dca, rca[0])
        hold_exact(case, "dcb", dcb, rcb[0])
        hold_exact(case, "dy3", dy3, ry3[0])
    else:
        hold_f32(case, "dca", dca, rca)
        hold_f32(case, "dcb", dcb, rcb)
        hold_bf16(case, "dy3", dy3, ry3)


# ---------------------------------------------------------------------------------------------------------------------
# gconv_bwd_fused
FUSED_SHAPES = [(1, 3, 37, 8, 0), (2, 2, 1025, 64, 0), (1, 2, 300, 40, 0), (1, 1, 64, 512, 520)]


def _gate_inputs(gen, B, T, P, C, exact):
    if exact:
        return (_probe(gen, B, 2, T, P, C), _probe(gen, B, 2, T, P, C), _probe(gen, B, T, P, C), _pow2(gen, B, 2, T),
                _pow2(gen, B, 2, T, signed=True))
    return (_rn(gen, B, 2, T, P, C), _rn(gen, B, 2, T, P, C, scale=2.0, lim=5.0), _rn(gen, B, T, P, C),
            torch.rand(B, 2, T, generator=gen) * 0.5 + 0.5, torch.rand(B, 2, T, generator=gen) - 0.5)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("B,T,P,C,pitch", FUSED_SHAPES)
def test_gconv_bwd_fused_mode1(B, T, P, C, pitch):
    """(2,2,1025,64): two pixel slices; (1,2,300,40): channel groups that are no power of two; (1,1,64,512): cscale_pitch = 520 with
    NaN in the padding.  The 256-thread form only (see the module docstring)."""
    ops, lib, check = _api()
    gen = _gen(6000 + C)
    case = f"gconv_bwd_fused1({B},{T},{P},{C},pitch={pitch})"
    g, raw, y3, ca, cb = _gate_inputs(gen, B, T, P, C, False)
    cs = torch.rand(B, 2, T, C, generator=gen) + 0.5
    csfull = torch.full((B, 2, T, pitch or C), NAN)
    csfull[..., :C] = cs
    dout, dy3 = _out(B, 2, T, P, C), _out(B, T, P, C)
    dca, dcb, dcs = (_out(B, 2, T, dtype=torch.float32, fill=0.0), _out(B, 2, T, dtype=torch.float32, fill=0.0),
                     _out(B, 2, T, C, dtype=torch.float32, fill=0.0))
    dev = [_g(t) for t in (g, raw, y3, ca, cb, csfull)]
    check(lib.oniris_gconv_bwd_fused(1, *[ops._p(t) for t in dev], None, ops._p(dout), None, ops._p(dy3), ops._p(dca), ops._p(dcb),
                                     ops._p(dcs), B, T, P, C, 1.0, 1.0, 0.0, pitch, None, None, ops._stream()), "gconv_bwd_fused")
    torch.cuda.synchronize()
    rdout, _, rdy3, rca, rcb, rcs, _ = GO.gconv_fused(1, g, raw, y3, ca, cb, cs, None, 1.0, 1.0, 0.0, False, 0, dout_bf16=dout)
    hold_bf16(case, "dout", dout, rdout)
    hold_bf16(case, "dy3", dy3, rdy3)
    hold_f32(case, "dca", dca, rca)
    hold_f32(case, "dcb", dcb, rcb)
    hold_f32(case, "dcs", dcs, rcs)


MODE2_VARIANTS = ["plain", "clip", "alias-flag0", "alias-flag1", "alias-noclip", "alias-flag1-nodres", "exact", "exact-alias"]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("variant", MODE2_VARIANTS)
@pytest.mark.parametrize("B,T,P,C,pitch", FUSED_SHAPES)
def test_gconv_bwd_fused_mode2(B, T, P, C, pitch, variant):
    """The aliasing protocol driven directly: not alias with clip 0 / 256; alias with the flag clear and xo full of values >= clip
    (g must come back untouched), with the flag set (g masked in place, with dres given and with dres NULL), and with clip <= 0 and
    no flag.  xo holds elements at exactly +-256 and at +-255.  ca_scaled is checked on every alias variant.  `exact`: the
    integer-exact probes, not alias and alias with the flag set."""
    ops, lib, check = _api()
    gen = _gen(7000 + C)
    case = f"gconv_bwd_fused2({B},{T},{P},{C}) {variant}"
    exact = variant.startswith("exact")
    alias = "alias" in variant
    clip = 0.0 if variant in ("plain", "alias-noclip") else 256.0
    flag = None if (not alias or clip <= 0) else (0 if variant == "alias-flag0" else 1)
    with_dres = variant != "alias-flag1-nodres"
    ta, tb = (0.5, 2.0) if exact else (0.8, 0.6)
    g, raw, y3, ca, cb = _gate_inputs(gen, B, T, P, C, exact)
    if variant == "alias-flag0":
        xo = torch.full((B, 2, T, P, C), 300.0).to(BF16)
    else:
        xo = _clipped_out(gen, B * 2 * T * P * C).reshape(B, 2, T, P, C)
    gg = _g(g).clone()
    dout = gg if alias else _out(B, 2, T, P, C)
    dres, dy3 = (_out(B, 2, T, P, C) if with_dres else None), _out(B, T, P, C)
    dca, dcb = _out(B, 2, T, dtype=torch.float32, fill=0.0), _out(B, 2, T, dtype=torch.float32, fill=0.0)
    cas = _out(B, 2, T, dtype=torch.float32) if alias else None
    fl = torch.tensor([flag], dtype=torch.int32, device=DEV) if flag is not None else None
    dev = [_g(t) for t in (raw, y3, ca, cb)]
    xog = _g(xo)
    check(lib.oniris_gconv_bwd_fused(2, ops._p(gg), *[ops._p(t) for t in dev], None,
                                     ops._p(xog) if clip > 0 else None, ops._p(dout), ops._p(dres), ops._p(dy3), ops._p(dca),
                                     ops._p(dcb), None, B, T, P, C, ta, tb, clip, 0, ops._p(fl), ops._p(cas), ops._stream()),
          "gconv_bwd_fused")
    torch.cuda.synchronize()
    rfirst, rres, rdy3, rca, rcb, _, rcas = GO.gconv_fused(2, g, raw, y3, ca, cb, None, xo, ta, tb, clip, alias, flag or 0,
                                                           dout_bf16=None if alias else dout)
    if alias:
        hold_exact(case, "g'", gg, rfirst[0])              # masking is exact: g itself, or g with zeros
        if variant == "alias-flag0":
            assert torch.equal(gg.cpu(), g), "flag = 0: g must come back untouched"
        hold_f32(case, "ca_scaled", cas, rcas)
        if exact:
            hold_exact(case, "ca_scaled", cas, rcas[0])
    elif exact:
        hold_exact(case, "dout", dout, rfirst[0])
    else:
        hold_bf16(case, "dout", dout, rfirst)
    if exact:
        hold_exact(case, "dres", dres, rres[0])
        hold_exact(case, "dy3", dy3, rdy3[0])
        hold_exact(case, "dca", dca, rca[0])
        hold_exact(case, "dcb", dcb, rcb[0])
    else:
        if with_dres:
            hold_bf16(case, "dres", dres, rres)
        hold_bf16(case, "dy3", dy3, rdy3)
        hold_f32(case, "dca", dca, rca)
        hold_f32(case, "dcb", dcb, rcb)


# ---------------------------------------------------------------------------------------------------------------------
# resample / resample_filter
def _taps(f):
    return None if f is None else [v / sum(f) for v in f]


def _launch_resample(x, add, mode, taps, scale, shape_out):
    ops, lib, check = _api()
    N, H, W, C = x.shape
    out = _out(*shape_out)
    if taps is None:
        check(lib.oniris_resample(ops._p(x), ops._p(out), ops._p(add), N, H, W, C, mode, scale, ops._stream()), "resample")
    else:
        arr = (ctypes.c_float * len(taps))(*taps)
        check(lib.oniris_resample_filter(ops._p(x), ops._p(out), ops._p(add), N, H, W, C, mode, arr, len(taps), scale, ops._stream()),
              "resample_filter")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("f", [None, (1, 1), (1, 3, 3, 1), (1, 2, 3, 3, 2, 1), (2, 5)])
@pytest.mark.parametrize("mode,shape", [(0, (2, 6, 10, 8)), (1, (3, 5, 7, 24))])
def test_resample(f, mode, shape):
    """Down at (2,6,10,8), up at (3,5,7,24), each plain, with `add`, and with the adjoints' scale (0.25 for up, 4 for down); f = None:
    oniris_resample, else oniris_resample_filter ([1,1] included).  Every element is compared, every border row and column among
    them; the [1,1] cases also with an integer-exact probe."""
    gen = _gen(8000 + mode)
    N, H, W, C = shape
    so = (N, H // 2, W // 2, C) if mode == 0 else (N, 2 * H, 2 * W, C)
    x, add = _rn(gen, *shape), _rn(gen, *so)
    taps = _taps(f)
    for with_add in (False, True):
        for scale in (1.0, 4.0 if mode == 0 else 0.25):
            got = _launch_resample(_g(x), _g(add) if with_add else None, mode, taps, scale, so)
            hold_bf16(f"resample(f={f},mode={mode})", f"out[add={int(with_add)},scale={scale}]", got,
                      GO.resample(x, mode, taps or (0.5, 0.5), scale, add if with_add else None))
    if f is None or f == (1, 1):
        xp, ap = _probe(gen, *shape), _probe(gen, *so)
        for scale in (1.0, 4.0 if mode == 0 else 0.25):
            got = _launch_resample(_g(xp), _g(ap), mode, taps, scale, so)
            hold_exact(f"resample(f={f},mode={mode})", f"probe[scale={scale}]", got, GO.resample(xp, mode, (0.5, 0.5), scale, ap)[0])


@pytest.mark.parametrize("f", [None, (1, 3, 3, 1)])
@pytest.mark.parametrize("mode", ["down", "up"])
def test_ops_resample_backward_takes_the_parked_gradient(f, mode):
    """ops.resample's autograd plumbing: the backward is the other mode with the adjoint's scale plus the gradient parked in the
    input's GradSlot."""
    ops, lib, check = _api()
    gen = _gen(8100)
    shape = (2, 6, 10, 8) if mode == "down" else (3, 5, 7, 24)
    x, parked = _rn(gen, *shape), _rn(gen, *shape)
    taps = ops.resample_taps(f) if f else None
    xg, slot = _g(x).requires_grad_(), ops.GradSlot()
    slot.put(_g(parked))
    y = ops.resample(xg, mode, in_slot=slot, taps=taps)
    gy = _rn(gen, *y.shape)
    y.backward(_g(gy))
    torch.cuda.synchronize()
    assert slot.g is None
    ops.GradSlot.live.clear()
    m = 0 if mode == "down" else 1
    case = f"ops.resample({mode},f={f})"
    hold_bf16(case, "out", y, GO.resample(x, m, taps or (0.5, 0.5)))
    hold_bf16(case, "dx", xg.grad, GO.resample(gy, 1 - m, taps or (0.5, 0.5), 0.25 if m == 0 else 4.0, parked))


@pytest.mark.parametrize("f", [None, (1, 3, 3, 1)])
def test_resample_second_grid_trip(f):
    """Up at N = 3, 256 x 256, C = 64: 6.3 M threads' worth of work on a grid capped at 16384 blocks.  Integer-exact probe; the
    reference is two separable 1-D passes in float32, exact on these values (numerators <= 64 over 16)."""
    gen = _gen(8200)
    shape = (3, 256, 256, 64)
    x = _probe(gen, *shape)
    got = _launch_resample(_g(x), None, 1, _taps(f), 1.0, (3, 512, 512, 64)).cpu()
    want = GO.resample(x, 1, _taps(f) or (0.5, 0.5), dtype=torch.float32, want_mag=False)[0].to(BF16)
    assert torch.equal(got, want)

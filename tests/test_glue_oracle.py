"""The review of tests/glue_oracle.py, on the CPU:
  1. pin: fed the unrounded float64 intermediates, every restatement equals float64 autograd through oracle.oniris_oracle's
     normalize / mp_cat / mp_silu / mp_sum / resample and torch's clamp to 1e-12 relative;
  2. the bounds are not too tight: the same formulas in torch float32 use less than a quarter of the fp32 term, and their bf16
     rounding stays inside the whole bound;
  3. the bounds are not too loose: deliberate defects, one at a time, move the value by at least 8 x the bound at every element
     they touch (the norm backward's projection term: at >= 40 % of the elements).
The figures of 2. are printed (pytest -s) and recorded in profiles/glue_stage_tests.txt."""
import math

import pytest
import torch

import glue_oracle as GO
from oracle import oniris_oracle as O

D = torch.float64


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=D)


def _floored(gen, *shape, lo=0.5, hi=1.0):
    """Random signs times magnitudes in [lo, hi]: no element is small, so a defect shows at EVERY element it touches."""
    sign = torch.randint(0, 2, shape, generator=gen).to(D) * 2 - 1
    return sign * (lo + (hi - lo) * torch.rand(*shape, generator=gen, dtype=D))


def _bfr(t):
    return t.to(torch.bfloat16).to(D)


def _cat_weights(C1, C2, t=0.5):
    c = math.sqrt((C1 + C2) / ((1 - t) ** 2 + t ** 2))
    return c / math.sqrt(C1) * (1 - t), c / math.sqrt(C2) * t


# ---------------------------------------------------------------------------------------------------------------------
# 1. pin
@pytest.mark.parametrize("C1,C2,norm", [(8, 0, True), (24, 8, True), (512, 0, True), (40, 0, False), (64, 32, False)])
@pytest.mark.parametrize("with_dxo,with_dadd", [(True, True), (False, False)])
def test_pin_act(C1, C2, norm, with_dxo, with_dadd):
    gen = _gen(C1 + C2)
    npix, C = 13, C1 + C2
    x = _randn(gen, npix, C1).requires_grad_()
    skip = _randn(gen, npix, C2).requires_grad_() if C2 else None
    w1, w2 = _cat_weights(C1, C2) if C2 else (1.0, 1.0)
    v = O.mp_cat(x, skip) if C2 else x
    xo = O.normalize(v, dim=1) if norm else v
    a = O.mp_silu(xo)
    da, dxo, dadd = _randn(gen, npix, C), _randn(gen, npix, C), _randn(gen, npix, C1)
    loss = (a * da).sum() + (0.75 * (xo * dxo).sum() if with_dxo else 0)
    loss.backward()
    (gv, _), (gxo, _), (ga, _), sden = GO.act_fwd(x, skip, w1, w2, norm, xo_bf16=xo)
    assert _rel(gv, v.detach()) < 1e-12 and _rel(gxo, xo.detach()) < 1e-12 and _rel(ga, a.detach()) < 1e-12
    s = sden[0] if norm else None
    if norm:
        assert _rel(s, GO.EPS + v.detach().norm(dim=1) / math.sqrt(C)) < 1e-12
    (dx, _), dskip = GO.act_bwd(da, dxo if with_dxo else None, xo, s, dadd if with_dadd else None, C1, C2, w1, w2, norm, 0.75)
    assert _rel(dx, x.grad + (dadd if with_dadd else 0)) < 1e-12
    if C2:
        assert _rel(dskip[0], skip.grad) < 1e-12


def test_pin_act_resampled_input():
    gen = _gen(5)
    x = _bfr(_randn(gen, 2, 6, 10, 8))
    down = O.resample(x.permute(0, 3, 1, 2), "down").permute(0, 2, 3, 1)
    up = O.resample(x.permute(0, 3, 1, 2), "up").permute(0, 2, 3, 1)
    assert torch.equal(GO.resample_in(x, 1, 3, 5), _bfr(down)) and torch.equal(GO.resample_in(x, 2, 12, 20), up)


def test_pin_emb_silu_bwd():
    gen = _gen(1)
    y, c, du = _randn(gen, 3, 11, 16).requires_grad_(), (_randn(gen, 3, 16) * 0.5 + 1).requires_grad_(), _randn(gen, 3, 11, 16)
    (O.mp_silu(y * c[:, None, :]) * du).sum().backward()
    (dy, _), (dc, _) = GO.emb_silu_bwd(du, y, c)
    assert _rel(dy, y.grad) < 1e-12 and _rel(dc, c.grad) < 1e-12


@pytest.mark.parametrize("clip", [0.0, 1.5])
def test_pin_mpsum(clip):
    gen = _gen(2)
    t = 0.3
    ta, tb = (1 - t) / math.sqrt((1 - t) ** 2 + t ** 2), t / math.sqrt((1 - t) ** 2 + t ** 2)
    res, v, g = _randn(gen, 500).requires_grad_(), _randn(gen, 500).requires_grad_(), _randn(gen, 500)
    out = O.mp_sum(res, v, t)
    if clip > 0:
        out = out.clamp(-clip, clip)
        assert int((out.detach().abs() == clip).sum()) > 20
    (out * g).sum().backward()
    (dres, _), (dv, _) = GO.mpsum_bwd(g, out, ta, tb, clip)
    assert _rel(dres, res.grad) < 1e-12 and _rel(dv, v.grad) < 1e-12
    if clip > 0:
        assert _rel(GO.mpsum_mask(g, out, clip, 1)[0] * tb, v.grad) < 1e-12
        assert torch.equal(GO.mpsum_mask(g, out, clip, 0)[0], g)


def _gated(gen, B, S, T, P, C):
    y2, y3 = _randn(gen, B, S, T, P, C).requires_grad_(), _randn(gen, B, T, P, C).requires_grad_()
    ca = (_randn(gen, B, S, T) * 0.3 + 1).requires_grad_()
    cb = (_randn(gen, B, S, T) * 0.5).requires_grad_()
    out = ca[..., None, None] * y2 + cb[..., None, None] * y3[:, None]
    out.retain_grad()
    return y2, y3, ca, cb, out


@pytest.mark.parametrize("S", [1, 2])
def test_pin_gconv_prep(S):
    gen = _gen(3)
    y2, y3, ca, cb, out = _gated(gen, 2, S, 3, 7, 8)
    dout = _randn(gen, *out.shape)
    (out * dout).sum().backward()
    (dca, _), (dcb, _), (dy3, _) = GO.gconv_prep(dout, out, y3, ca, cb, S)
    assert _rel(dca, ca.grad) < 1e-12 and _rel(dcb, cb.grad) < 1e-12 and _rel(dy3, y3.grad) < 1e-12


def test_pin_gconv_fused_mode1():
    gen = _gen(4)
    y2, y3, ca, cb, out = _gated(gen, 2, 2, 3, 7, 8)
    cs = (_randn(gen, 2, 2, 3, 8) * 0.3 + 1).requires_grad_()
    g = _randn(gen, *out.shape)
    (O.mp_silu(out * cs[:, :, :, None, :]) * g).sum().backward()
    first, dres, dy3, dca, dcb, dcs, cas = GO.gconv_fused(1, g, out, y3, ca, cb, cs, None, 1.0, 1.0, 0.0, False, 0,
                                                          dout_bf16=out.grad)
    assert dres is None and cas is None
    assert _rel(first[0], out.grad) < 1e-12 and _rel(dy3[0], y3.grad) < 1e-12 and _rel(dca[0], ca.grad) < 1e-12
    assert _rel(dcb[0], cb.grad) < 1e-12 and _rel(dcs[0], cs.grad) < 1e-12


@pytest.mark.parametrize("alias,clip,flag", [(False, 0.0, 0), (False, 1.5, 0), (True, 1.5, 1), (True, 0.0, 0)])
def test_pin_gconv_fused_mode2(alias, clip, flag):
    gen = _gen(6)
    t = 0.3
    ta, tb = (1 - t) / math.sqrt((1 - t) ** 2 + t ** 2), t / math.sqrt((1 - t) ** 2 + t ** 2)
    y2, y3, ca, cb, v = _gated(gen, 2, 2, 3, 7, 8)
    res = _randn(gen, *v.shape).requires_grad_()
    xo = O.mp_sum(res, v, t)
    if clip > 0:
        xo = xo.clamp(-clip, clip)
    g = _randn(gen, *v.shape)
    (xo * g).sum().backward()
    first, dres, dy3, dca, dcb, dcs, cas = GO.gconv_fused(2, g, v, y3, ca, cb, None, xo, ta, tb, clip, alias, flag, dout_bf16=v.grad)
    assert dcs is None
    if alias:                                            # g' = the masked gradient; dgrad / wgrad read it with tb * ca
        assert _rel(first[0] * tb, v.grad) < 1e-12 and _rel(cas[0], tb * ca.detach()) < 1e-12
    else:
        assert cas is None and _rel(first[0], v.grad) < 1e-12
    assert _rel(dres[0], res.grad) < 1e-12 and _rel(dy3[0], y3.grad) < 1e-12
    assert _rel(dca[0], ca.grad) < 1e-12 and _rel(dcb[0], cb.grad) < 1e-12


def test_gconv_fused_alias_without_flag_leaves_g_alone():
    gen = _gen(7)
    y2, y3, ca, cb, v = _gated(gen, 1, 2, 2, 5, 8)
    g = _randn(gen, *v.shape)
    xo = torch.full_like(g, 3.0)                          # everything at or beyond the clip: flag = 0 must not look
    first = GO.gconv_fused(2, g, v, y3, ca, cb, None, xo, 0.5, 2.0, 2.0, True, 0)[0]
    assert torch.equal(first[0], g)
    first = GO.gconv_fused(2, g, v, y3, ca, cb, None, xo, 0.5, 2.0, 2.0, True, 1)[0]
    assert float(first[0].abs().max()) == 0.0


@pytest.mark.parametrize("f", [(1, 1), (1, 3, 3, 1), (2, 5)])
@pytest.mark.parametrize("mode", ["down", "up"])
def test_pin_resample(f, mode):
    gen = _gen(8)
    x, taps = _randn(gen, 2, 6, 10, 8), [v / sum(f) for v in f]
    want = O.resample(x.permute(0, 3, 1, 2), mode, f).permute(0, 2, 3, 1)
    got, mag = GO.resample(x, 0 if mode == "down" else 1, taps)
    assert got.shape == want.shape and _rel(got, want) < 1e-12 and bool((mag >= got.abs() * (1 - 1e-12)).all())
    add = _randn(gen, *want.shape)
    got2, mag2 = GO.resample(x, 0 if mode == "down" else 1, taps, scale=0.25, add=add)
    assert _rel(got2, 0.25 * want + add) < 1e-12 and _rel(mag2, 0.25 * mag + add.abs()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 2. not too tight: the same formulas in float32
def _in_float32(fn):
    GO.DTYPE = torch.float32
    try:
        return fn()
    finally:
        GO.DTYPE = torch.float64


def _usage(name, got32, ref, mag, kind):
    """Fraction of the fp32 term that the float32 evaluation uses, and of the whole bound that its bf16 rounding uses."""
    ref, mag, got32 = ref.to(D), mag.to(D), got32.to(D)
    fp32_term = (GO.U_F32_64 if kind == "bf16" else GO.U_F32_128) * mag
    live = fp32_term > 0
    assert bool(((got32 - ref).abs()[~live] == 0).all())
    use32 = ((got32 - ref).abs()[live] / fp32_term[live]).max().item()
    line = f"float32-emulation {name}: fp32 term used {use32:.3f}"
    assert use32 <= 0.25, line
    if kind == "bf16":
        whole = GO.bound_bf16(ref, mag)
        useb = ((_bfr(got32) - ref).abs()[live] / whole[live]).max().item()
        line += f", bf16 result / whole bound {useb:.3f}"
        assert useb <= 1.0, line
    print(line)


@pytest.mark.parametrize("C1,C2,norm", [(8, 0, True), (64, 0, True), (512, 0, True), (24, 8, True), (40, 0, False)])
def test_float32_fits_act(C1, C2, norm):
    gen = _gen(100 + C1)
    npix, C = 200, C1 + C2
    x, skip = _bfr(_randn(gen, npix, C1) * 2), (_bfr(_randn(gen, npix, C2)) if C2 else None)
    w1, w2 = _cat_weights(C1, C2) if C2 else (1.0, 1.0)
    r = GO.act_fwd(x, skip, w1, w2, norm)
    r32 = _in_float32(lambda: GO.act_fwd(x, skip, w1, w2, norm))
    xo = _bfr(r32[1][0])                                 # the bf16 xo both backward evaluations read
    _usage(f"act_fwd C={C} xo", r32[1][0], *r[1], "bf16")
    a = GO.act_fwd(x, skip, w1, w2, norm, xo_bf16=xo)[2]
    a32 = _in_float32(lambda: GO.act_fwd(x, skip, w1, w2, norm, xo_bf16=xo))[2]
    _usage(f"act_fwd C={C} a", a32[0], *a, "bf16")
    sden32 = None
    if norm:
        _usage(f"act_fwd C={C} sden", r32[3][0], *r[3], "f32")
        sden32 = r32[3][0]
    da, dxo, dadd = _bfr(_randn(gen, npix, C)), _bfr(_randn(gen, npix, C)), _bfr(_randn(gen, npix, C1))
    args = (da, dxo, xo, sden32, dadd, C1, C2, w1, w2, norm, 0.75)
    b, b32 = GO.act_bwd(*args), _in_float32(lambda: GO.act_bwd(*args))
    _usage(f"act_bwd C={C} norm={int(norm)} dx", b32[0][0], *b[0], "bf16")
    if C2:
        _usage(f"act_bwd C={C} norm={int(norm)} dskip", b32[1][0], *b[1], "bf16")


def test_float32_fits_emb_silu_and_gate_sums():
    gen = _gen(200)
    du, y, c = _bfr(_randn(gen, 2, 300, 40)), _bfr(_randn(gen, 2, 300, 40) * 2), (torch.rand(2, 40, generator=gen) + 0.5).to(D)
    r, r32 = GO.emb_silu_bwd(du, y, c), _in_float32(lambda: GO.emb_silu_bwd(du, y, c))
    _usage("emb_silu_bwd dy", r32[0][0], *r[0], "bf16")
    _usage("emb_silu_bwd dc", r32[1][0], *r[1], "f32")
    dout, out, y3 = _bfr(_randn(gen, 1, 2, 3, 296)), _bfr(_randn(gen, 1, 2, 3, 296)), _bfr(_randn(gen, 1, 3, 296))
    ca, cb = (torch.rand(1, 2, 3, generator=gen) + 0.5).to(D), (torch.rand(1, 2, 3, generator=gen) - 0.5).to(D)
    r, r32 = GO.gconv_prep(dout, out, y3, ca, cb, 2), _in_float32(lambda: GO.gconv_prep(dout, out, y3, ca, cb, 2))
    _usage("gconv_prep dca", r32[0][0], *r[0], "f32")
    _usage("gconv_prep dcb", r32[1][0], *r[1], "f32")
    _usage("gconv_prep dy3", r32[2][0], *r[2], "bf16")


def test_float32_fits_resample_filter():
    gen = _gen(300)
    x, add = _bfr(_randn(gen, 2, 6, 10, 8)), _bfr(_randn(gen, 2, 12, 20, 8))
    taps = [v / 12 for v in (1, 2, 3, 3, 2, 1)]
    r, r32 = GO.resample(x, 1, taps, 0.25, add), _in_float32(lambda: GO.resample(x, 1, taps, 0.25, add))
    _usage("resample_filter up [1,2,3,3,2,1]", r32[0], *r, "bf16")


# ---------------------------------------------------------------------------------------------------------------------
# 3. not too loose: deliberate defects
def _stands_out(name, bad, ref, mag, kind, touched=None, min_fraction=None):
    bound = GO.bound_bf16(ref, mag) if kind == "bf16" else GO.bound_f32(mag)
    moved = (bad - ref).abs()
    if touched is None:
        touched = moved > 0
    n = int(touched.sum())
    assert n > 0, f"{name}: the defect touches nothing"
    seen = moved >= 8 * bound
    if min_fraction is None:
        assert bool(seen[touched].all()), f"{name}: {int((~seen & touched).sum())} of {n} touched elements move by less than 8 x the bound"
    else:
        frac = float(seen.sum()) / seen.numel()
        print(f"defect {name}: {100 * frac:.0f} % of the elements move by >= 8 x the bound")
        assert frac >= min_fraction, (name, frac)
    return (moved[touched] / bound[touched].clamp_min(1e-300)).min().item()


def _norm_case(gen, C1, C2, npix=64, floored=True):
    x, skip = _bfr(_randn(gen, npix, C1)), (_bfr(_randn(gen, npix, C2)) if C2 else None)
    w1, w2 = (0.5, 1.5) if C2 else (1.25, 1.0)
    _, (xo, _), _, sden = GO.act_fwd(x, skip, w1, w2, True)
    mk = (lambda *s: _bfr(_floored(gen, *s))) if floored else (lambda *s: _bfr(_randn(gen, *s)))
    return _bfr(xo), sden[0].float(), mk(npix, C1 + C2), mk(npix, C1 + C2), mk(npix, C1), w1, w2


@pytest.mark.parametrize("C,min_fraction", [(512, 0.4), (64, 0.4), (8, 0.4)])
def test_defect_projection_term_dropped(C, min_fraction):
    xo, sden, da, dxo, dadd, w1, w2 = _norm_case(_gen(C), C, 0, floored=False)
    (ref, mag), _ = GO.act_bwd(da, None, xo, sden, None, C, 0, w1, w2, True)
    (bad, _), _ = GO.act_bwd(da, None, xo, sden, None, C, 0, w1, w2, True, _no_projection=True)
    _stands_out(f"projection dropped, C = {C}", bad, ref, mag, "bf16", min_fraction=min_fraction)


@pytest.mark.parametrize("norm", [True, False])
def test_defects_of_act_bwd(norm):
    gen = _gen(11)
    C1, C2 = 24, 8
    xo, sden, da, dxo, dadd, w1, w2 = _norm_case(gen, C1, C2)
    if not norm:
        sden = None
    (dx, mdx), (dsk, mdsk) = GO.act_bwd(da, dxo, xo, sden, dadd, C1, C2, w1, w2, norm, 0.75)
    (bad, _), _ = GO.act_bwd(da, dxo, xo, sden, None, C1, C2, w1, w2, norm, 0.75)
    _stands_out("dadd dropped", bad, dx, mdx, "bf16", touched=torch.ones_like(dx, dtype=torch.bool))
    (bad, _), (bads, _) = GO.act_bwd(da, dxo, xo, sden, dadd, C1, C2, w1, w2, norm, 1.0)
    if not norm:                                         # (under the norm the projection mixes channels: some elements move less)
        _stands_out("dxo_scale ignored", bad, dx, mdx, "bf16", touched=torch.ones_like(dx, dtype=torch.bool))
        _stands_out("dxo_scale ignored (dskip)", bads, dsk, mdsk, "bf16", touched=torch.ones_like(dsk, dtype=torch.bool))
    else:
        _stands_out("dxo_scale ignored", bad, dx, mdx, "bf16", min_fraction=0.9)
    (dx0, mdx0), _ = GO.act_bwd(da, dxo, xo, sden, None, C1, C2, w1, w2, norm, 0.75)
    (bad, _), (bads, _) = GO.act_bwd(da, dxo, xo, sden, None, C1, C2, w2, w1, norm, 0.75)
    _stands_out("w1 / w2 swapped", bad, dx0, mdx0, "bf16")
    _stands_out("w1 / w2 swapped (dskip)", bads, dsk, mdsk, "bf16")


def test_defect_one_pixel_missing_from_the_sums():
    gen = _gen(12)
    N, P, C = 2, 300, 40
    # (y * c > 0: silu' >= 1/2 there -- it crosses zero near z = -1.28, where the missing term itself would vanish)
    du, y, c = _bfr(_floored(gen, N, P, C)), _bfr(_floored(gen, N, P, C)).abs(), (torch.rand(N, C, generator=gen) + 0.5).to(D)
    _, (dc, mdc) = GO.emb_silu_bwd(du, y, c)
    du2 = du.clone()
    du2[:, 123] = 0
    ratio = _stands_out("pixel missing from dc", GO.emb_silu_bwd(du2, y, c)[1][0], dc, mdc, "f32",
                        touched=torch.ones_like(dc, dtype=torch.bool))
    print(f"defect pixel missing from dc: moved by {ratio * 128:.0f} fp32 units of mag (allowed: 128)")
    B, T = 1, 3
    dout, out, y3 = _bfr(_floored(gen, B, 2, T, P, C)), _bfr(_floored(gen, B, 2, T, P, C)), _bfr(_floored(gen, B, T, P, C))
    ca, cb = (torch.rand(B, 2, T, generator=gen) + 0.5).to(D), (torch.rand(B, 2, T, generator=gen) * 0.5 + 0.25).to(D)
    # (at the pixel that goes missing y3 = y2 = dout, so that its terms sum(d * y3), sum(d * y2) are sums of squares and cannot cancel)
    dout[:, 1, :, 123] = dout[:, 0, :, 123]
    y3[:, :, 123] = dout[:, 0, :, 123]
    out[:, :, :, 123] = _bfr((ca + cb)[..., None] * dout[:, :, :, 123])
    dca, dcb, _ = GO.gconv_prep(dout, out, y3, ca, cb, 2)
    d2 = dout.clone()
    d2[:, :, :, 123] = 0
    bca, bcb, _ = GO.gconv_prep(d2, out, y3, ca, cb, 2)
    every = torch.ones_like(dcb[0], dtype=torch.bool)
    _stands_out("pixel missing from dcb", bcb[0], *dcb, "f32", touched=every)
    _stands_out("pixel missing from dca", bca[0], *dca, "f32", touched=every)


def test_defect_slots_cb_swapped():
    gen = _gen(13)
    B, T, PC = 1, 3, 296
    d0 = _bfr(_floored(gen, B, 1, T, PC))
    dout = torch.cat([d0, -d0.sign() * _bfr(_floored(gen, B, 1, T, PC)).abs()], 1)       # the slots' gradients differ by >= 1 everywhere
    out, y3 = _bfr(_floored(gen, B, 2, T, PC)), _bfr(_floored(gen, B, T, PC))
    ca = torch.ones(B, 2, T, dtype=D)
    cb = torch.tensor([0.25, 1.0], dtype=D).reshape(1, 2, 1).expand(B, 2, T).contiguous()
    dca, _, dy3 = GO.gconv_prep(dout, out, y3, ca, cb, 2)
    bca, _, by3 = GO.gconv_prep(dout, out, y3, ca, cb.flip(1), 2)
    _stands_out("cb swapped: dy3", by3[0], *dy3, "bf16", touched=torch.ones_like(dy3[0], dtype=torch.bool))
    _stands_out("cb swapped: dca", bca[0], *dca, "f32", touched=torch.ones_like(dca[0], dtype=torch.bool))


def test_defect_mask_at_le_and_ca_scaled():
    gen = _gen(14)
    g = _bfr(_floored(gen, 4096))
    out = _bfr(_randn(gen, 4096) * 100)
    out[::7], out[1::7], out[2::7], out[3::7] = 256.0, -256.0, 255.0, -255.0         # at the clip, and one bf16 step inside it
    at_clip = out.abs() == 256.0
    (dres, mres), (dv, mdv) = GO.mpsum_bwd(g, out, 0.5, 2.0, 256.0)
    assert float(dres[at_clip].abs().max()) == 0.0 and bool((dres[out.abs() == 255.0] != 0).all())
    (bres, _), (bv, _) = GO.mpsum_bwd(g, out, 0.5, 2.0, 258.0)         # `<= 256` on bf16 data is `< 258`, the next bf16 value
    assert torch.equal((bres != dres), at_clip)
    _stands_out("mask at <=: dres", bres, dres, mres, "bf16", touched=at_clip)
    _stands_out("mask at <=: dv", bv, dv, mdv, "bf16", touched=at_clip)
    bm, (m, mm) = GO.mpsum_mask(g, out, 258.0, 1)[0], GO.mpsum_mask(g, out, 256.0, 1)
    _stands_out("mask at <=: mpsum_mask", bm, m, mm, "bf16", touched=at_clip)
    ca = (torch.rand(6, generator=gen) + 0.5).to(D)
    for tb in (0.7, 2.0):
        _stands_out("ca_scaled = ca", ca, tb * ca, (tb * ca).abs(), "f32", touched=torch.ones(6, dtype=torch.bool))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", [(1, 1), (1, 3, 3, 1)])
def test_defect_resample_tap_shifted_at_a_border(mode, f):
    gen = _gen(15)
    H = 6
    rows = torch.arange(H, dtype=D).reshape(1, H, 1, 1)
    x = _bfr(_floored(gen, 2, H, 10, 8).abs() * (1 + rows))             # rows differ by >= 0.5: a shifted tap reads another value
    taps = [v / sum(f) for v in f]
    ref, mag = GO.resample(x, mode, taps)
    shifted = GO.resample(torch.roll(x, -1, 1), mode, taps)[0]          # every tap one input row further down ...
    bad = ref.clone()
    bad[:, 0] = shifted[:, 0]                                           # ... at the top border row only
    touched = torch.zeros_like(ref, dtype=torch.bool)
    touched[:, 0] = True
    _stands_out(f"resample tap shifted, mode {mode}, f = {f}", bad, ref, mag, "bf16", touched=touched)

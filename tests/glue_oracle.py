"""Float64 restatements of the magnitude-preserving glue kernels (csrc/elementwise.hip, lower half of csrc/weights.hip)  --
TEST INFRASTRUCTURE.  One function per kernel, written as a function of exactly the tensors that kernel reads, so that one call
is compared with one stage.  Plain channels-last torch tensors on the CPU in, float64 out.

Every result is a pair (value, mag): `mag` is the same expression with every addend replaced by its absolute value (for silu'
it is (1 + |z|) * |da| / 0.596), i.e. the scale against which a float32 evaluation's rounding errors are measured:

  bf16 outputs      |got - value| <= 2^-8 * |value| + 2^-18 * mag      (bound_bf16: one bf16 rounding + 64 fp32 unit roundoffs)
  fp32 reductions   |got - value| <= 2^-17 * mag                        (bound_f32: 128 fp32 unit roundoffs)

tests/test_glue_oracle.py pins every function to float64 autograd through oracle.oniris_oracle and checks that the bounds are
neither too tight (a float32 evaluation of the same formulas fits with room) nor too loose (deliberate defects stand out)."""
import math

import torch

EPS = 1e-4
SILU_DIV = 0.596
U_BF16 = 2.0 ** -8       # worst-case relative error of one round-to-nearest bf16 rounding
U_F32_64 = 2.0 ** -18    # 64 fp32 unit roundoffs: <= ~20 fp32 operations per element + the ~1 ulp hardware exp2 / rcp
U_F32_128 = 2.0 ** -17   # 128 fp32 unit roundoffs: the reductions' chains of additions


DTYPE = torch.float64    # (test_glue_oracle evaluates the same formulas in float32 to see how much of a bound float32 uses)


def _d(t, dtype=None):
    return None if t is None else t.detach().to("cpu", dtype or DTYPE)


def bf(t):
    """Round to bf16 and back (what a kernel's store does to a value)."""
    return t.to(torch.bfloat16).to(t.dtype)


def bound_bf16(ref, mag):
    return U_BF16 * ref.abs() + U_F32_64 * mag


def bound_f32(mag):
    return U_F32_128 * mag


def dsilu(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def _eps_of(sden):
    """The kernel's eps is the float32 1e-4f: an fp32 `sden` of an all-zero pixel is exactly that value, and s - eps must then be
    exactly 0 as it is in the kernel.  A float64 `sden` (the pin) carries the exact 1e-4."""
    return float(torch.tensor(EPS, dtype=torch.float32)) if sden.dtype == torch.float32 else EPS


# ---------------------------------------------------------------------------------------------------------------------
def resample_in(x, rs, Ho, Wo):
    """act_fwd's resampling of x on the way in (rs = 1: 2x2 mean, rs = 2: nearest x2; Ho x Wo = the OUTPUT grid), rounded to bf16
    as the kernel does before anything else.  x (N, Hi, Wi, C) -> (N, Ho, Wo, C)."""
    x = _d(x)
    if rs == 0:
        return x
    N, Hi, Wi, C = x.shape
    if rs == 1:
        assert (Hi, Wi) == (2 * Ho, 2 * Wo)
        return bf(x.reshape(N, Ho, 2, Wo, 2, C).sum((2, 4)) * 0.25)
    assert (2 * Hi, 2 * Wi) == (Ho, Wo)
    yy, xx = torch.arange(Ho) // 2, torch.arange(Wo) // 2
    return x[:, yy][:, :, xx]


def act_fwd(x, skip, w1, w2, norm, rs=0, Ho=0, Wo=0, xo_bf16=None):
    """v = cat(w1 * x, w2 * skip);  norm: s = eps + |v| / sqrt(C), xo = v / s, else xo = v;  a = silu(xo_bf16) / 0.596.
    `xo_bf16`: the bf16 xo that `a` is computed from (the kernel's own output, so that a tie in rounding xo cannot leak into a);
    None: the rounded value of this function's xo.  Returns v, xo, a, sden as (value, mag) pairs over (npix, C) / (npix,);
    sden is None without the norm."""
    x = resample_in(x, rs, Ho, Wo)
    C1 = x.shape[-1]
    parts = [w1 * x.reshape(-1, C1)]
    if skip is not None:
        parts.append(w2 * _d(skip).reshape(-1, skip.shape[-1]))
    v = torch.cat(parts, -1)
    C = v.shape[-1]
    mv = v.abs()
    sden = None
    xo, mxo = v, mv
    if norm:
        s = EPS + (v * v).sum(-1).sqrt() / math.sqrt(C)
        sden = (s, s.clone())                            # (every addend is positive already)
        xo, mxo = v / s[:, None], mv / s[:, None]
    xb = bf(xo) if xo_bf16 is None else _d(xo_bf16).reshape(-1, C)
    a = xb * torch.sigmoid(xb) / SILU_DIV
    return (v, mv), (xo, mxo), (a, a.abs()), sden


def act_bwd(da, dxo, xo, sden, dadd, C1, C2, w1, w2, norm, dxo_scale=1.0, _no_projection=False):
    """g = dxo_scale * dxo + da * silu'(xo) / 0.596;  norm: g <- (g - xo * sum(g * xo) * s / (C * (s - eps))) / s  (0 for the second
    term where s - eps <= 0: the zero-subgradient convention of an all-zero pixel);  dx = w1 * g[:C1] + dadd,  dskip = w2 * g[C1:].
    `_no_projection` is the defect of test_glue_oracle (the norm backward without its projection term)."""
    C = C1 + C2
    z = _d(xo).reshape(-1, C)
    da = _d(da).reshape(-1, C)
    g = da * dsilu(z) / SILU_DIV
    mg = (1 + z.abs()) * da.abs() / SILU_DIV
    if dxo is not None:
        t = dxo_scale * _d(dxo).reshape(-1, C)
        g, mg = g + t, mg + t.abs()
    if norm:
        eps = _eps_of(sden)
        s = _d(sden).reshape(-1, 1)
        nsc = (s - eps) * C
        ok = nsc > 0
        safe = torch.where(ok, nsc, torch.ones_like(nsc))
        k = torch.where(ok, (g * z).sum(-1, keepdim=True) * s / safe, torch.zeros_like(s))
        mk = torch.where(ok, (mg * z.abs()).sum(-1, keepdim=True) * s / safe, torch.zeros_like(s))
        if _no_projection:
            k, mk = torch.zeros_like(k), torch.zeros_like(mk)
        g, mg = (g - z * k) / s, (mg + z.abs() * mk) / s
    dx, mdx = w1 * g[:, :C1], abs(w1) * mg[:, :C1]
    if dadd is not None:
        t = _d(dadd).reshape(-1, C1)
        dx, mdx = dx + t, mdx + t.abs()
    dskip = (w2 * g[:, C1:], abs(w2) * mg[:, C1:]) if C2 else None
    return (dx, mdx), dskip


def emb_silu_bwd(du, y, c):
    """u = silu(y * c[n]) / 0.596:  dz = du * silu'(y * c) / 0.596;  dy = dz * c;  dc[n] = sum_pixels dz * y.
    du, y (N, P, C); c (N, C)."""
    du, y, c = _d(du), _d(y), _d(c)[:, None, :]
    z = y * c
    dz = du * dsilu(z) / SILU_DIV
    mdz = (1 + z.abs()) * du.abs() / SILU_DIV
    return (dz * c, mdz * c.abs()), ((dz * y).sum(1), (mdz * y.abs()).sum(1))


def _mask(out, clip):
    return (_d(out).abs() < clip).to(DTYPE)


def mpsum_bwd(g, out, ta, tb, clip):
    """out = clip(ta * res + tb * v):  dres = ta * g * [|out| < clip],  dv = tb * g * [|out| < clip]  (clip <= 0: no mask)."""
    g = _d(g)
    if clip > 0:
        g = g * _mask(out, clip)
    return (ta * g, (ta * g).abs()), (tb * g, (tb * g).abs())


def mpsum_mask(g, out, clip, flag):
    """g * [|out| < clip] if the forward's clip flag is set, else g itself."""
    g = _d(g)
    if flag:
        g = g * _mask(out, clip)
    return g, g.abs()


def _gate_sums(dr, raw, y3, ca, cb):
    """S1 = sum dr * raw, S2 = sum dr * y3 per frame slot;  dca = (S1 - cb * S2) / ca,  dcb = S2,  dy3 = sum_s cb * dr.
    dr, raw (B, S, T, ...); y3 (B, T, ...); ca, cb (B, S, T)."""
    red = tuple(range(3, dr.ndim))
    y3 = y3[:, None]
    S1, mS1 = (dr * raw).sum(red), (dr * raw).abs().sum(red)
    S2, mS2 = (dr * y3).sum(red), (dr * y3).abs().sum(red)
    cbx = cb.reshape(*cb.shape, *([1] * len(red)))
    dy3, mdy3 = (cbx * dr).sum(1), (cbx * dr).abs().sum(1)
    dca = ((S1 - cb * S2) / ca, (mS1 + cb.abs() * mS2) / ca.abs())
    return dca, (S2, mS2), (dy3, mdy3)


def gconv_prep(dout, out, y3, ca, cb, S):
    """oniris_gconv_bwd_prep: dout, out (B, S, T, ...), y3 (B, T, ...), ca, cb (B, S, T)  ->  dca, dcb, dy3."""
    assert dout.shape[1] == S
    return _gate_sums(_d(dout), _d(out), _d(y3), _d(ca), _d(cb))


def gconv_fused(mode, g, raw, y3, ca, cb, cs, xo, ta, tb, clip, alias, flag, dout_bf16=None):
    """oniris_gconv_bwd_fused.  g, raw, xo (B, 2, T, P, C); y3 (B, T, P, C); ca, cb (B, 2, T); cs (B, 2, T, C).
      mode 1: dz = g * silu'(raw * cs) / 0.596, dcs = sum_pixels dz * raw, d = dz * cs
      mode 2: gg = g * [|xo| < clip] (masked when clip > 0 and (not alias or flag)), dres = ta * gg, d = tb * gg
    Not alias: dout = d, and the sums use the bf16-ROUNDED dout (`dout_bf16`: the kernel's own output, so that a rounding tie cannot
    leak into the sums; None: this function's rounding).  Alias: the first result is g' = gg (g masked in place, or g itself), the
    sums use the unrounded tb * gg, and ca_scaled = tb * ca.
    Returns dout or g', dres, dy3, dca, dcb, dcs, ca_scaled -- (value, mag) pairs, None where the mode has no such output."""
    g, raw, y3, ca, cb = _d(g), _d(raw), _d(y3), _d(ca), _d(cb)
    dres = dcs = ca_scaled = None
    if mode == 1:
        assert not alias
        c = _d(cs)[:, :, :, None, :]
        z = raw * c
        dz = g * dsilu(z) / SILU_DIV
        mdz = (1 + z.abs()) * g.abs() / SILU_DIV
        dcs = ((dz * raw).sum(3), (mdz * raw.abs()).sum(3))
        d, md = dz * c, mdz * c.abs()
    else:
        gg = g
        if clip > 0 and (not alias or flag):
            gg = g * _mask(xo, clip)
        dres = (ta * gg, (ta * gg).abs())
        d, md = tb * gg, (tb * gg).abs()
    if alias:
        first, dr = (gg, gg.abs()), d
        ca_scaled = (tb * ca, (tb * ca).abs())
    else:
        first = (d, md)
        dr = bf(d) if dout_bf16 is None else _d(dout_bf16)
    dca, dcb, dy3 = _gate_sums(dr, raw, y3, ca, cb)
    return first, dres, dy3, dca, dcb, dcs, ca_scaled


# ---------------------------------------------------------------------------------------------------------------------
def _pass1d(x, dim, mode, f, size_in):
    """One 1-D pass of the resampling filter along `dim`, by index arithmetic (pad = (L - 1) // 2, zero padding):
      mode 0 (down): out[o] = sum_a f[a] * x[2 o + a - pad]
      mode 1 (up):   out[O] = sum_{a : O + pad - a even} 2 f[a] * x[(O + pad - a) / 2]
    Returns (value, mag)."""
    L = len(f)
    pad = (L - 1) // 2
    n_out = size_in // 2 if mode == 0 else size_in * 2
    o = torch.arange(n_out)
    val = mag = None
    shape = [1] * x.ndim
    shape[dim] = n_out
    for a in range(L):
        if mode == 0:
            i = 2 * o + a - pad
            ok = (i >= 0) & (i < size_in)
            w = f[a]
        else:
            num = o + pad - a
            i = torch.div(num, 2, rounding_mode="floor")
            ok = (num % 2 == 0) & (num >= 0) & (i < size_in)
            w = 2 * f[a]
        if not bool(ok.any()):
            continue
        t = x.index_select(dim, i.clamp(0, size_in - 1)) * (w * ok.to(x.dtype)).reshape(shape)
        val = t if val is None else val + t
        mag = t.abs() if mag is None else mag + t.abs()
    return val, mag


def resample(x, mode, taps, scale=1.0, add=None, dtype=None, want_mag=True):
    """oniris_resample / oniris_resample_filter: x (N, H, W, C); mode 0 = down (depthwise outer(f, f), stride 2), 1 = up (the
    transposed one with 4 * outer(f, f)); `taps` = the 1-D filter normalised to sum 1 ((0.5, 0.5) = 2x2 mean / nearest x2);
    out = scale * filtered + add.  Two separable 1-D passes written by index arithmetic (_pass1d).  `dtype` / `want_mag`: the
    integer-exact probes of the large grids are evaluated in float32 (exact there) without the magnitude."""
    x = _d(x, dtype)
    f = [float(t) for t in taps]
    N, H, W, C = x.shape
    v = _pass1d(_pass1d(x, 1, mode, f, H)[0], 2, mode, f, W)[0] * scale
    m = None
    if want_mag:
        fa = [abs(t) for t in f]
        m = _pass1d(_pass1d(x.abs(), 1, mode, fa, H)[1], 2, mode, fa, W)[1] * abs(scale)
    if add is not None:
        t = _d(add, dtype)
        v = v + t
        m = m + t.abs() if want_mag else None
    return v, m

"""Float64 restatements of the step-edge kernels (lower half of csrc/elementwise.hip)  --  TEST INFRASTRUCTURE.  These kernels turn
images, noise and sigma into the UNet's input and conditioning and its raw output into a loss, a gradient or a denoised frame.
One function per kernel, a function of exactly the tensors and scalars that kernel reads; CPU tensors in, float64 (value, mag) pairs
out.  `mag` is the same expression with every addend replaced by its absolute value (see tests/glue_oracle.py); the bounds are

  bf16 outputs               |got - value| <= 2^-8 |value| + 2^-18 mag     (glue_oracle.bound_bf16)
  fp32 elementwise outputs   |got - value| <= 2^-18 mag                      (64 fp32 unit roundoffs: D, ca, cb, c, dcoef, c_noise)
  fp32 reductions            |got - value| <= 2^-17 mag                      (glue_oracle.bound_f32: chains of <= 128 additions)

Transcendentals.  Where a kernel evaluates f(a) with an argument `a` that it computed in fp32 itself, the rounding of `a` (a few
units of 2^-24 * mag_a) reaches the result as |f'(a)| * mag_a; that product is added to `mag`, once per kernel, derived in the
function's docstring.  An argument that is an input (sigma under logf / log10f, min_gating under expf) carries no such term: the
functions themselves are accurate to a few ulp of their result, which `|value|` in `mag` covers.

Layout conventions (spelled out where they are used):
  * slot n = (b, s, t) of a training step, s = 0 clean | 1 noised (S = 1: only noised).  sigma and noise are indexed [b, s*T + t],
    images [b, t].  Only slot s = S - 1 enters the loss; the clean slots get dF = 0.
  * dart_input writes C image channels, the ones channel at c = C and zeros behind it up to cpad.
  * dart_input_pair: output row n packs source row n % (B*T); c_noise has B*T entries (the source rows only).
  * gate position of frame slot n of layer l = n % T + nctx[l].
  * a label outside [0, L) yields the unlabeled embedding (embed_eval guards the read).
  * history entry i of a launch goes to ring slot (count + i) % cap; only the last `cap` entries of a launch are logged; then
    count += n.
  * precond_out_guided uses torch.lerp's two forms, which switch at |g| < 0.5.

`_defect=...` arguments are the deliberate defects of tests/test_step_edge_oracle.py (one wrong index or factor each).
`DTYPE` / `KSUM`: that file also evaluates the same formulas in float32, with the reductions in the kernels' summation shape."""
import math

import torch

from glue_oracle import bound_f32, U_F32_64, dsilu, SILU_DIV   # noqa: F401  (bound_f32: used by the GPU test next to bound_f32_elem)

DTYPE = torch.float64
KSUM = False             # True: reductions in the kernel's summation shape (per-thread sequences, butterfly, waves)
LN10 = math.log(10.0)
SQRT2 = 1.4142135623730951
T_LABEL = float(torch.tensor(1.0, dtype=torch.float32) / 3)        # embed_eval's `1.f / 3.f`


def bound_f32_elem(mag):
    return U_F32_64 * mag


def _d(t):
    return None if t is None else t.detach().to("cpu", DTYPE)


def ksum(seq, waves="seq"):
    """Sum of `seq` (..., steps, threads) over its last two dims.  KSUM: every thread adds its `steps` terms in order, the 64
    lanes of a wave meet in a butterfly, the waves sequentially (block_sum) or pairwise ('tree': gates_bwd, emb_scale_bwd)."""
    if not KSUM:
        return seq.sum((-2, -1))
    acc = torch.zeros_like(seq[..., 0, :])
    for i in range(seq.shape[-2]):
        acc = acc + seq[..., i, :]
    nw = acc.shape[-1] // 64
    acc = acc.reshape(*acc.shape[:-1], nw, 64)
    o = 32
    while o:
        acc = acc[..., :o] + acc[..., o:2 * o]
        o //= 2
    acc = acc[..., 0]
    if waves == "tree":
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
        return acc[..., 0]
    tot = torch.zeros_like(acc[..., 0])
    for i in range(nw):
        tot = tot + acc[..., i]
    return tot


def lay(x, threads):
    """(..., n) -> (..., steps, threads): element i belongs to thread i % threads, step i // threads (zero padded)."""
    n = x.shape[-1]
    steps = -(-n // threads)
    x = torch.nn.functional.pad(x, (0, steps * threads - n))
    return x.reshape(*x.shape[:-1], steps, threads)


# ---------------------------------------------------------------------------------------------------------------------
# Preconditioning coefficients (networks_edm2.py:286-291)
def _coefs(sg, sd):
    den = sg * sg + sd * sd
    return sd * sd / den, sg * sd / den.sqrt(), 1 / den.sqrt()           # c_skip, c_out, c_in


def _noised(images, noise, sigma, S, _defect=None):
    """x[b, s, t] = images[b, t] + sigma[b, s*T + t] * noise[b, s*T + t] and its magnitude; (B, S, T, C, HW) each, with the
    slot's sigma (B, S, T)."""
    images, noise, sigma = _d(images), _d(noise), _d(sigma)
    B, T, C = images.shape[:3]
    img = images.reshape(B, 1, T, C, -1)
    sg = sigma.reshape(B, S, T)
    if _defect == "sigma_next":                      # the neighbouring frame's sigma
        sg = torch.roll(sigma.reshape(B, S * T), -1, 1).reshape(B, S, T)
    if _defect == "st_as_t":                         # s*T + t read as t
        sg = sigma.reshape(B, S, T)[:, :1].expand(B, S, T)
    if noise is None:
        x, mx = img.expand(B, S, T, C, img.shape[-1]), img.abs().expand(B, S, T, C, img.shape[-1])
    else:
        nz = noise.reshape(B, S, T, C, -1)
        if _defect == "st_as_t":
            nz = nz[:, :1].expand_as(nz)
        t = sg[..., None, None] * nz
        x, mx = img + t, img.abs() + t.abs()
    return x, mx, sg, img


def dart_input(images, noise, sigma, S, sd, cpad, _defect=None):
    """oniris_dart_input (loss.py:17-31 + networks_edm2.py:286-292).  images (B,T,C,H,W), noise (B,S*T,C,H,W) or None, sigma (B,S*T).
      xcl[n = (b,s,t)][p][c] = c_in * x[b,s,t][c][p] for c < C,  1 for c = C,  0 for C < c < cpad        (bf16, channels last)
      c_noise[n] = log(sigma) / 4        (sigma is an input: no argument term; mag = |value|)
    Returns xcl (B*S*T, HW, cpad) and c_noise (B*S*T) as (value, mag) pairs; mag of the ones / pad channels is 0 (they are exact)."""
    x, mx, sg, _ = _noised(images, noise, sigma, S, _defect)
    B, _, T, C, HW = x.shape
    cin = _coefs(sg, sd)[2][..., None, None]
    v = torch.zeros(B, S, T, HW, cpad, dtype=x.dtype)
    m = torch.zeros_like(v)
    v[..., :C] = (cin * x).transpose(-1, -2)
    m[..., :C] = (cin * mx).transpose(-1, -2)
    v[..., C + 1 if _defect == "ones_at_C+1" else C] = 1.0
    cn = sg.log() / 4
    return (v.reshape(B * S * T, HW, cpad), m.reshape(B * S * T, HW, cpad)), (cn.reshape(-1), cn.abs().reshape(-1))


def dart_input_pair(x, sigma, sd, cpad, _defect=None):
    """oniris_dart_input_pair (sampler.py:25-32: the 3-D and the 2-D evaluation of one x in one batch).  x (B,T,C,H,W), sigma (B,T):
    output row n of 2*B*T packs SOURCE row n % (B*T), without noise; c_noise has B*T entries."""
    B, T = x.shape[:2]
    (v, m), cn = dart_input(x, None, sigma, 1, sd, cpad)
    nsrc = B * T
    src = torch.arange(2 * nsrc) % nsrc
    if _defect == "n_div_nsrc":
        src = torch.arange(2 * nsrc) // nsrc
    return (v[src], m[src]), cn


def _loss_terms(F, images, noise, sigma, out_gain, S, sd, _defect=None):
    """e = c_skip * x + c_out * (out_gain * F) - images per slot (B, S, T, C, HW), its magnitude, c_out (B,S,T,1,1) and F (fp)."""
    x, mx, sg, img = _noised(images, noise, sigma, S, _defect)
    B, _, T, C, HW = x.shape
    Fd = _d(F).reshape(B, S, T, HW, 8)[..., :C].transpose(-1, -2)
    cskip, cout, _ = (c[..., None, None] for c in _coefs(sg, sd))
    og = float(out_gain)
    e = cskip * x + cout * (Fd * og) - img
    me = cskip * mx + (cout * Fd * og).abs() + img.abs()
    return e, me, cout, Fd


def dart_loss(F, images, noise, sigma, out_gain, S, sd, _defect=None):
    """oniris_dart_loss (loss.py:32-38 with Precond's output side, networks_edm2.py:293-297).  F (B*S*T, H, W, 8) bf16 raw UNet
    output (channels >= C are never read).  losses[b, t] = mean_{c,p} e^2 of slot (b, S-1, t); mag = mean mag_e^2 (an error of
    k units in e is one of 2k units of mag_e^2 in e^2).  Chain: 1024 threads, thread p % 1024 adds its C * ceil(HW / 1024) terms in
    order, + 6 butterfly + 16 waves."""
    e, me, _, _ = _loss_terms(F, images, noise, sigma, out_gain, S, sd, _defect)
    B, _, T, C, HW = e.shape
    e, me = e[:, S - 1], me[:, S - 1]
    sq, msq = e * e, me * me
    if _defect == "pixel":
        sq = sq.clone()
        sq[..., HW // 2] = 0
    seq = lay(sq, 1024).permute(0, 1, 3, 2, 4).reshape(B, T, -1, 1024)        # (b, t, pass * C + c, thread)
    return ksum(seq) / (C * HW), msq.sum((-2, -1)) / (C * HW)


def dart_loss_bwd(F, images, noise, sigma, out_gain, dlosses, S, sd, _defect=None):
    """oniris_dart_loss_bwd: with gl = dlosses[b,t] * 2 / (C * HW) and d = gl * e * c_out,
      dF[n][p][c] = d * out_gain  (bf16; 0 for the clean slots s < S-1 and for the pad channels c >= C)
      dgain_part[b, t] = sum_{c,p} d * F          (d out_gain = their sum over the frames)
    Returns dF (B*S*T, HW, 8), dgain_part (B, T), dgain () as (value, mag) pairs.  Chain of dgain_part: as dart_loss."""
    e, me, cout, Fd = _loss_terms(F, images, noise, sigma, out_gain, S, sd, _defect)
    B, _, T, C, HW = e.shape
    og = float(out_gain)
    gl = (_d(dlosses).reshape(B, 1, T, 1, 1) * 2 / (C * HW)).expand(B, S, T, 1, 1)
    d, md = gl * e * cout, (gl * cout).abs() * me
    dF = torch.zeros(B, S, T, HW, 8, dtype=e.dtype)
    mF = torch.zeros_like(dF)
    lo = 0 if _defect == "clean_not_zeroed" else S - 1
    k = og * og if _defect == "gain_twice" else og
    dF[:, lo:, :, :, :C] = (d * k).transpose(-1, -2)[:, lo:]
    mF[:, lo:, :, :, :C] = (md * abs(k)).transpose(-1, -2)[:, lo:]
    term, mterm = (d * Fd)[:, S - 1], (md * Fd.abs())[:, S - 1]
    if _defect == "pixel":
        term = term.clone()
        term[..., HW // 2] = 0
    seq = lay(term, 1024).permute(0, 1, 3, 2, 4).reshape(B, T, -1, 1024)
    part, mpart = ksum(seq), mterm.sum((-2, -1))
    return (dF.reshape(B * S * T, HW, 8), mF.reshape(B * S * T, HW, 8)), (part, mpart), (part.sum(), mpart.sum())


# ---------------------------------------------------------------------------------------------------------------------
def loss_tail(mse, sigma, T_off, coef, nterms, sd, rings=None, count=0, _defect=None):
    """oniris_loss_tail (loss.py:32-46, loss_weight.py:30-39,104-131).  mse (B,T); sigma (B, >= T_off + T): columns T_off .. T_off+T-1
    are read; coef: 2 * nterms - 1 Fourier coefficients.  Per entry i = b * T + t:
      w = (sg^2 + sd^2) / (sg sd)^2,  l = mse w,  xl = log10 sg,  e = c0 / 2 + sum_k c[2k-1] cos(k xl) + c[2k] sin(k xl),  1/m = 10^-e
      out[0] = mean(l / m), out[1] = mean(l), dcoef[i] = w / (m n)
    Transcendental term: e is computed in fp32, mag_e = |c0| / 2 + sum_k (|c[2k-1]| + |c[2k]|) (1 + k |xl|)  (the products' own
    roundings and the arguments k * xl through |cos'|, |sin'| <= 1); it reaches 10^-e as ln 10 * mag_e relative, so every quantity
    with the factor 1/m has mag = |value| * (1 + ln 10 * mag_e).
    History (rings = (ring_sigma, ring_loss, ring_pos) of length cap, or None): entry i goes to slot (count + i) % cap if i >= n - cap,
    with pos = t; count += n.  Chain of out: thread i % 256 adds ceil(n / 256) terms, + 6 + 4.
    Returns out (2,), dcoef (B,T), ring_loss -- (value, mag) pairs --, ring_sigma, ring_pos, count (exact), and the slots written."""
    mse, sigma, coef = _d(mse), _d(sigma), _d(coef).reshape(-1)
    B, T = mse.shape
    n = B * T
    sg = sigma[:, T_off:T_off + T]
    w = (sg * sg + sd * sd) / ((sg * sd) * (sg * sd))
    l = mse * w
    xl = sg.log10()
    e, me = 0.5 * coef[0] + 0 * xl, 0.5 * coef[0].abs() + 0 * xl
    for k in range(1, nterms):
        e = e + coef[2 * k - 1] * (k * xl).cos() + coef[2 * k] * (k * xl).sin()
        me = me + (coef[2 * k - 1].abs() + coef[2 * k].abs()) * (1 + k * xl.abs())
    inv_m = 10.0 ** (-e)
    rel = 1 + LN10 * me
    t0, t1 = (l * inv_m).reshape(-1), l.reshape(-1)
    out = torch.stack([ksum(lay(t0, 256)), ksum(lay(t1, 256))]) / n
    mout = torch.stack([(t0.abs() * rel.reshape(-1)).sum(), t1.abs().sum()]) / n
    dcoef = w * inv_m / n
    res = [(out, mout), (dcoef, dcoef.abs() * rel)]
    if rings is None:
        return res + [None, None, None, count, None]
    rs, rl, rp = (r.detach().cpu().clone() for r in rings)
    cap = rs.numel()
    i = torch.arange(n)
    keep = i >= n - cap
    if _defect == "first_entries":                   # the first n - cap ... entries logged in place of the last cap
        keep = i < cap
    slot = (count + i) % cap
    if _defect == "slot_off_by_one":
        slot = (count + i + 1) % cap
    i, slot = i[keep], slot[keep]
    rs[slot] = sigma[:, T_off:T_off + T].reshape(-1)[i].to(rs.dtype)
    rl = rl.to(DTYPE)
    mrl = torch.zeros_like(rl)                       # untouched slots: compared exactly (bound 0)
    rl[slot] = l.reshape(-1)[i]
    mrl[slot] = l.reshape(-1)[i].abs()
    rp[slot] = (i % T).to(rp.dtype)
    return res + [(rl, mrl), rs, rp, count + n, slot]


# ---------------------------------------------------------------------------------------------------------------------
def precond_out(F, x, sigma, out_gain, sd):
    """oniris_precond_out (networks_edm2.py:293-297, eval): D[n][c][p] = c_skip[n] x + c_out[n] out_gain F[n][p][c], fp32.
    F (N, HW, 8) bf16, x (N, C, HW), sigma (N)."""
    F, x, sg = _d(F), _d(x), _d(sigma).reshape(-1, 1, 1)
    C = x.shape[1]
    cskip, cout, _ = _coefs(sg, sd)
    t = cout * float(out_gain) * F[..., :C].transpose(1, 2)
    return cskip * x + t, (cskip * x).abs() + t.abs()


def precond_out_guided(F, x, sigma, out_gain, sd, g, _defect=None):
    """oniris_precond_out_guided (sampler.py:25-32): F (2N, HW, 8): rows [0, N) the 3-D evaluation, [N, 2N) the 2-D one;
    D = lerp(D2, D3, g) in torch.lerp's two forms:  |g| < 0.5: D2 + g (D3 - D2);  else D3 - (D3 - D2) (1 - g)."""
    N = x.shape[0]
    d3, m3 = precond_out(F[:N], x, sigma, out_gain, sd)
    d2, m2 = precond_out(F[N:], x, sigma, out_gain, sd)
    small = abs(g) < 0.5
    if _defect == "ends_swapped":
        d2, m2, d3, m3 = d3, m3, d2, m2
    if small:
        return d2 + g * (d3 - d2), m2 + abs(g) * (m3 + m2)
    return d3 - (d3 - d2) * (1 - g), m3 + (m3 + m2) * abs(1 - g)


def sampler_update(mode, x_hat, x_pred, d_io, x_aux, t_a, dt):
    """oniris_sampler_update (sampler.py:66-76): the reference's float32 tensor expressions themselves, operation by operation
    (every product and sum rounded on its own), so the comparison is bit-exact.  Returns (x_out, d_io')."""
    t_a, dt = torch.tensor(t_a, dtype=torch.float32), torch.tensor(dt, dtype=torch.float32)      # 0-dim tensors, as the reference has them
    if mode == 0:
        d = (x_hat - x_pred) / t_a
        return x_hat + dt * d, d
    dp = (x_aux - x_pred) / t_a
    return x_hat + dt * (0.5 * d_io + 0.5 * dp), d_io


# ---------------------------------------------------------------------------------------------------------------------
class _Gate:
    """The gate of every (layer, frame slot) with the first-order error scale E_q (in fp32 unit roundoffs) of every intermediate q:
      E(a b) = E_a |b| + |a| E_b + |a b|,   E(a +- b) = E_a + E_b + |a +- b|,   E(f(a)) = |f'(a)| E_a + |f(a)|,   E(input) = 0
    -- the rule `every addend by its absolute value` applied to the kernel's own sequence of operations (1 - lo, 1 - g, 1 - s and
    1 - hi s are differences the kernel forms in fp32: a saturated lo = 1 - 1e-13 rounds to 1 and 1 - lo to 0), with the
    transcendental term of sv: E_sv = |c_noise m0| + |o0| + |pos m1| + |o1| reaches s through sigmoid' = s (1 - s)."""

    def __init__(self, c_noise, params, nctx, T, _defect=None):
        cn, p = _d(c_noise).reshape(1, -1), _d(params)
        L, N = p.shape[0], cn.shape[1]
        n = torch.arange(N)
        base = (n // T if _defect == "n_div_T" else n % T).to(DTYPE).reshape(1, N)
        nc = torch.zeros(L, 1, dtype=DTYPE) if nctx is None else nctx.detach().cpu().to(DTYPE).reshape(L, 1)
        if _defect == "nctx_next":
            nc = torch.roll(nc, -1, 0)
        pos = (base + nc).log1p()
        m0, m1, o0, o1 = (p[:, i:i + 1] for i in range(4))
        lo, hi = torch.sigmoid(p[:, 4:5]), torch.sigmoid(p[:, 5:6])
        sv = cn * m0 + o0 + pos * m1 + o1
        E_sv = (cn * m0).abs() + o0.abs() + (pos * m1).abs() + o1.abs()
        s = torch.sigmoid(sv)
        E_lo, E_hi, E_s = lo, hi, s * (1 - s) * E_sv + s
        a1 = 1 - lo
        E_a1 = E_lo + a1
        k = a1 * hi
        E_k = E_a1 * hi + a1 * E_hi + k
        g = lo + k * s
        E_g = E_lo + E_k * s + k * E_s + g
        r = ((1 - g) ** 2 + g ** 2) ** -0.5
        self.__dict__.update(cn=cn, pos=pos, lo=lo, hi=hi, s=s, a1=a1, k=k, g=g, r=r, E_lo=E_lo, E_hi=E_hi, E_s=E_s, E_a1=E_a1, E_k=E_k,
                             E_g=E_g)


def gates(c_noise, params, nctx, T, _defect=None):
    """oniris_gates (conv.py:113-127): params (L, 6) = mult0, mult1, off0, off1, min_gating, max_gating; c_noise (N); nctx (L) or None.
      sv = c_noise m0 + o0 + log1p(n % T + nctx[l]) m1 + o1,  g = lo + (1 - lo) hi sigmoid(sv),  r = ((1-g)^2 + g^2)^-1/2,
      ca = (1 - g) r,  cb = g r                                                          (fp32, (L, N) each)
    mag (see _Gate for E_g, which holds sv's transcendental term): with d ca / d g = -g r^3 and d cb / d g = (1 - g) r^3,
      mag_ca = |ca| + g r^3 E_g,   mag_cb = |cb| + (1 - g) r^3 E_g."""
    q = _Gate(c_noise, params, nctx, T, _defect)
    g, r = q.g, q.r
    ca, cb = (1 - g) * r, g * r
    return (ca, ca.abs() + g * r ** 3 * q.E_g), (cb, cb.abs() + (1 - g) * r ** 3 * q.E_g)


def gates_bwd(c_noise, params, nctx, dca, dcb, T, _defect=None):
    """oniris_gates_bwd: dparams (L, 6) from dca, dcb (L, N).  Per frame slot
      dg = r^3 ((1 - g) dcb - g dca),  dsv = dg (1 - lo) hi s (1 - s)
      d mult0 = sum dsv c_noise,  d mult1 = sum dsv pos,  d off0 = d off1 = sum dsv,
      d min_gating = lo (1 - lo) sum dg (1 - hi s),  d max_gating = hi (1 - hi) sum dg (1 - lo) s
    mag by _Gate's rules: dg = f(g) with |f'| <= 3 r^5 |2g - 1| (|(1-g) dcb| + |g dca|) + r^3 (|dcb| + |dca|), so
    E_dg = r^3 (|(1-g) dcb| + |g dca|) + |f'| E_g; the products dsv, dg (1 - hi s), dg (1 - lo) s and the two factors behind the
    sums follow the product rule.  Chain: thread n % 256 adds ceil(N / 256) terms, + 6 butterfly + 2 (four waves pairwise)."""
    q = _Gate(c_noise, params, nctx, T, _defect)
    cn, pos, lo, hi, s, g, r, k, a1 = q.cn, q.pos, q.lo, q.hi, q.s, q.g, q.r, q.k, q.a1
    dca, dcb = _d(dca), _d(dcb)
    a = ((1 - g) * dcb).abs() + (g * dca).abs()
    dg = r ** 3 * ((1 - g) * dcb - g * dca)
    E_dg = r ** 3 * a + (3 * r ** 5 * (2 * g - 1).abs() * a + r ** 3 * (dcb.abs() + dca.abs())) * q.E_g
    b1 = 1 - s
    E_b1 = q.E_s + b1
    dsv = dg * k * s * b1
    E_dsv = E_dg * k * s * b1 + dg.abs() * (q.E_k * s * b1 + k * q.E_s * b1 + k * s * E_b1) + dsv.abs()
    c4 = 1 - hi * s
    t4, t5 = dg * c4, dg * a1 * s
    E_t4 = E_dg * c4 + dg.abs() * (q.E_hi * s + hi * q.E_s + c4) + t4.abs()
    E_t5 = E_dg * a1 * s + dg.abs() * (q.E_a1 * s + a1 * q.E_s) + t5.abs()
    terms = [dsv * cn, dsv * pos, dsv, dsv, t4, t5]
    mags = [E_dsv * cn.abs(), E_dsv * pos.abs(), E_dsv, E_dsv, E_t4, E_t5]
    val = torch.stack([ksum(lay(t, 256), "tree") for t in terms], 1)
    mag = torch.stack([m.sum(1) for m in mags], 1)
    absum = torch.stack([t.abs().sum(1) for t in terms], 1)
    f4, f5 = lo * a1, hi * (1 - hi)
    E_f4, E_f5 = q.E_lo * a1 + lo * q.E_a1 + f4, q.E_hi * (1 - hi) + hi * (q.E_hi + 1 - hi) + f5
    one = torch.ones(lo.shape[0], 4, dtype=lo.dtype)
    post, E_post = torch.cat([one, f4, f5], 1), torch.cat([0 * one, E_f4, E_f5], 1)
    val, mag = val * post, mag * post + absum * E_post
    if _defect == "o3_not_set":
        val = val.clone()
        val[:, 3] = 0
    return val, mag


# ---------------------------------------------------------------------------------------------------------------------
def fourier(c_noise, freqs, phases):
    """MPFourier (utils.py:139-150): sqrt(2) cos(x f + phi), (N, cn).  The argument is computed in fp32: |cos'| <= 1 carries its
    rounding, mag = sqrt(2) (|cos| + |x f| + |phi|)."""
    x, f, ph = _d(c_noise).reshape(-1, 1), _d(freqs).reshape(1, -1), _d(phases).reshape(1, -1)
    arg = x * f + ph
    return SQRT2 * arg.cos(), SQRT2 * (arg.cos().abs() + (x * f).abs() + ph.abs())


def _mp_weight_dot(w, col, mcol):
    """MPConv in eval (conv.py:14-21,36-42) applied to a vector: sum_i w[co][i] col[n][i] / sqrt(fan) / (eps + |w[co]| / sqrt(fan)),
    (N, cout).  KSUM: the kernel's thread adds the fan-in terms in order."""
    fan = w.shape[1]
    rs = fan ** -0.5
    if KSUM:
        dot = torch.zeros(col.shape[0], w.shape[0], dtype=w.dtype)
        ss = torch.zeros(w.shape[0], dtype=w.dtype)
        for i in range(fan):
            dot = dot + col[:, i:i + 1] * w[:, i].reshape(1, -1)
            ss = ss + w[:, i] * w[:, i]
    else:
        dot, ss = col @ w.t(), (w * w).sum(1)
    den = 1e-4 + ss.sqrt() * rs
    return dot * rs / den, (mcol @ w.abs().t()) * rs / den


def silu_out(e, me):
    """mp_silu (utils.py:112) of a pre-activation known to mag `me`: silu(e) / 0.596; mag = |value| + (|silu'(e)| me + e^2 s (1 - s))
    / 0.596  (the second term: sigmoid_fast's own argument -1.4427 e is rounded, |e| units, times |e| s (1 - s))."""
    s = torch.sigmoid(e)
    v = e * s / SILU_DIV
    return v, v.abs() + (dsilu(e).abs() * me + e * e * s * (1 - s)) / SILU_DIV


def embed_eval(c_noise, labels, freqs, phases, w_noise, w_label, L, t=T_LABEL, _defect=None):
    """oniris_embed_eval (networks_edm2.py:204-216, eval).  e = What_noise . fourier(c_noise); with labels and a label weight:
    el = What_label[:, label] * sqrt(L) (the scaled one-hot input), e <- mp_sum(e, el, t) = (e + (el - e) t) / sqrt((1-t)^2 + t^2) --
    only where 0 <= label < L, the unlabeled embedding otherwise;  emb = silu(e) / 0.596 -> bf16 (N, cemb).
    mag: the dot product's with the Fourier features' mag (their argument term), carried through mp_sum and silu'.
    Chain: one thread adds the cn <= 512 terms of a dot product in order -- longer than the 64 roundoffs of the fp32 part of a bf16
    bound; it holds because that part is 2^-10 of the bf16 rounding itself (see tests/test_step_edge_gpu.py)."""
    four, mfour = fourier(c_noise, freqs, phases)
    e, me = _mp_weight_dot(_d(w_noise), four, mfour)
    if labels is not None and w_label is not None:
        wl = _d(w_label)
        lab = labels.detach().cpu().reshape(-1)
        ok = (lab >= 0) & (lab < L)
        col = lab.clamp(0, L - 1)
        if _defect == "label_off_by_one":
            col = (col + 1) % L
        rl = L ** -0.5
        scale = 1.0 if _defect == "sqrt_L_dropped" else math.sqrt(L)
        el = wl[:, col].t() * scale * rl / (1e-4 + (wl * wl).sum(1).sqrt() * rl)
        tt = 1 - t if _defect == "t_swapped" else t
        c = ((1 - tt) ** 2 + tt ** 2) ** -0.5
        e2, me2 = (e + (el - e) * tt) * c, (me + (el.abs() + me) * tt) * c
        okc = ok.reshape(-1, 1)
        e, me = torch.where(okc, e2, e), torch.where(okc, me2, me)
    return silu_out(e, me)


def embed_pre(c_noise, labels, freqs, phases, cnP, L, LP):
    """oniris_embed_pre (networks_edm2.py:204-212): four (N, cnP) bf16 = the Fourier features, zero-padded from cn to cnP;
    onehot (N, LP) bf16 = bf16(float32 sqrt(L)) at the label's column, 0 elsewhere (exact; None without labels)."""
    v, m = fourier(c_noise, freqs, phases)
    N, cn = v.shape
    pad = torch.zeros(N, cnP - cn, dtype=v.dtype)
    oh = None
    if labels is not None:
        lab = labels.detach().cpu().reshape(-1)
        oh = torch.zeros(N, LP, dtype=torch.float32)
        oh[torch.arange(N), lab] = torch.tensor(float(L), dtype=torch.float32).sqrt().to(torch.bfloat16).float()
    return (torch.cat([v, pad], 1), torch.cat([m, pad], 1)), oh


def _mp_sum(e1, e2, t, _defect=None):
    e1 = _d(e1)
    if e2 is None:
        return e1, e1.abs()
    e2 = _d(e2)
    if _defect == "t_swapped":
        t = 1 - t
    den = ((1 - t) ** 2 + t ** 2) ** -0.5
    return (e1 + (e2 - e1) * t) * den, (e1.abs() + (e2.abs() + e1.abs()) * t) * den


def embed_post(e1, e2, t, _defect=None):
    """oniris_embed_post (utils.py:118-123, :112): emb = silu(mp_sum(e1, e2, t)) / 0.596, bf16; e2 None: silu(e1) / 0.596."""
    return silu_out(*_mp_sum(e1, e2, t, _defect))


def embed_post_bwd(demb, e1, e2, t, _defect=None):
    """oniris_embed_post_bwd: de = demb silu'(e) / 0.596 with e recomputed;  de1 = de (1 - t) den,  de2 = de t den  (e2 None: de1 = de).
    mag: |de| plus e's mag through silu'' = s (1 - s) (2 + e (1 - 2 s)) and sigmoid_fast's argument rounding |e| through
    d silu' / d s * s (1 - s) = (1 + e (1 - 2 s)) s (1 - s)."""
    e, me = _mp_sum(e1, e2, t, _defect)
    demb = _d(demb)
    s = torch.sigmoid(e)
    de = demb * dsilu(e) / SILU_DIV
    d2 = s * (1 - s) * (2 + e * (1 - 2 * s))
    mde = de.abs() + demb.abs() * (d2.abs() * me + e.abs() * (s * (1 - s) * (1 + e * (1 - 2 * s))).abs()) / SILU_DIV
    if e2 is None:
        return (de, mde), None
    if _defect == "t_swapped":
        t = 1 - t
    den = ((1 - t) ** 2 + t ** 2) ** -0.5
    return (de * (1 - t) * den, mde * (1 - t) * den), (de * t * den, mde * t * den)


# ---------------------------------------------------------------------------------------------------------------------
EMB_BWD_CHUNKS = 16


def emb_scale(c_all, gain, seg, _defect=None):
    """oniris_emb_scale (networks_edm2.py:78, every Block at once): c[n][j] = 1 + c_all[n][j] gain[seg[j]], fp32 (N, Ctot)."""
    c_all, gain = _d(c_all), _d(gain)
    seg = seg.detach().cpu().long()
    if _defect == "seg_shifted":                     # column j reads the Block of column j - 1: wrong at every Block's first column
        seg = torch.cat([seg[:1], seg[:-1]])
    t = c_all * gain[seg][None]
    return 1 + t, 1 + t.abs()


def emb_scale_bwd(dc, c_all, gain, start, _defect=None):
    """oniris_emb_scale_bwd: dc_all = dc gain[k] (bf16) over Block k's columns [start[k], start[k+1]);
    dgain_part[k][ch] = sum over rows [N ch / 16, N (ch + 1) / 16) and those columns of dc c_all (0 for an empty row chunk);
    d gain[k] = the sum of its 16 parts.  Chain: thread i % 256 adds ceil(rows * width / 256) terms, + 6 butterfly + 2.
    Returns dc_all (N, Ctot), dgain_part (K, 16), dgain (K) as (value, mag) pairs."""
    dc, c_all, gain = _d(dc), _d(c_all), _d(gain)
    st = [int(v) for v in start.detach().cpu()]
    N, K = dc.shape[0], len(st) - 1
    dall, part, mpart = torch.zeros_like(dc), torch.zeros(K, EMB_BWD_CHUNKS, dtype=dc.dtype), torch.zeros(K, EMB_BWD_CHUNKS, dtype=dc.dtype)
    for k in range(K):
        j0, j1 = st[k], st[k + 1]
        dall[:, j0:j1] = dc[:, j0:j1] * gain[k]
        for ch in range(EMB_BWD_CHUNKS):
            n0, n1 = N * ch // EMB_BWD_CHUNKS, N * (ch + 1) // EMB_BWD_CHUNKS
            if _defect == "last_row" and n1 > n0:
                n1 -= 1
            if n1 > n0:
                t = (dc[n0:n1, j0:j1] * c_all[n0:n1, j0:j1]).reshape(-1)
                part[k, ch], mpart[k, ch] = ksum(lay(t, 256), "tree"), t.abs().sum()
    return (dall, dall.abs()), (part, mpart), (part.sum(1), mpart.sum(1))

"""Float64 restatements of the UNet conv entry points, written from include/oniris.h  --  TEST INFRASTRUCTURE.

  conv_fwd    oniris_conv_fwd (forward AND data gradient: the data gradient is the same entry point with coff = (+2, +1),
              ctx_fill = 0 and the `wb` packing, pack_wb)
  conv_wgrad  one group of oniris_conv_wgrad_group: the full sum over positions, as deep as the weight's slabs (taps_total)

Plain channels-last CPU tensors in, float64 out.  The weights are the PACKED buffers the kernel reads, [taps][CoutP][CinP]; rows
co >= Cout and columns ci >= Cin are padding that no result may depend on.  Every result is a pair (value, mag): `mag` is the same
expression with every product replaced by its absolute value, i.e. the scale against which the rounding errors of a float32
accumulation are measured.

What the epilogues read (csrc/conv_parts.h, csrc/conv_kernels.h; the same in every forward family):
  v                    fp32:  coef_own[n] * acc_own + coef_ctx[n] * acc_ctx
  EPI_NONE             out  = bf16(v)
  EPI_EMB_SILU         out  = bf16(v);  out2 = bf16(silu(bf16(v) * escale[n][co]) / 0.596): the activation reads the ROUNDED v, so
                       conv_fwd takes the kernel's own `out` (out_bf16=..., itself held to its bound) for it
  EPI_MPSUM            out  = bf16(clip(ta * res + tb * v)) from the fp32 v;  out2 = bf16(v)
  ctx_out              bf16(acc_ctx), the un-gated context product of frame (b, t)
  ctx_prod             the same product as the FP32 tensor the one-frame launches keep (mode 1 / 3) or read back (mode 2)
  ctx_rows             rows b >= ctx_rows of a guided pair:  v = acc_own, epilogue on escale[b - ctx_rows] and res[b]
  x2 / act_out         taps 1: x is [bf16(cat_w1 x) | bf16(cat_w2 x2)], act_out = bf16(silu(that) / 0.596)
  clip_flag            1 iff the STORED value of some element is not below the clip in magnitude

Bounds (derived from the chain lengths, not fitted).  With round-to-nearest fp32 arithmetic a chain of n operations is off by at
most n * 2^-24 times the sum of the magnitudes it adds up (the products bf16 x bf16 are exact in fp32), and one bf16 store by at
most 2^-8 of the stored value (glue_oracle.U_BF16):

  bf16 outputs    |got - ref| <= 2^-8 |ref| + u * mag,     u = u_fwd(K, splits) = (K + splits + EPI_OPS) * 2^-24
                  K = taps * Cin * (1 or 3 phases) products behind one accumulator, `splits` the slices a split-K launch adds up,
                  EPI_OPS = 16 for the two coefficient products, their sum, ta * res + tb * v and the emb-scale product.
                  clip is 1-Lipschitz: the same bound holds through it.  The activation silu(z) / 0.596 with z = bf16(v) * c is an
                  elementwise function of values the kernel itself stored: its magnitude is (1 + |z|) |a| (the exponent z log2(e)
                  is rounded in fp32, which for z << 0 is a RELATIVE error of ~|z| 2^-24 in sigmoid(z)), with u = U_F32_64 of
                  glue_oracle for the ~20 fp32 operations and the ~1 ulp hardware exp2 / rcp, plus 2^-112 absolute for the fp32
                  underflow of sigmoid(z) at z < -87 (the probes reach |z| of a few hundred).
  own-only rows   the same bound with K = 9 Cin: the frames that walk the own taps only (ctx_prod_mode 2, the 2-D rows of a pair)
  fp32 ctx_prod   |got - ref| <= (18 Cin + 4) * 2^-24 * mag  (bound_ctx_prod): 18 Cin exact products summed in fp32 in any order,
                  + 4 for the four partial tiles added in LDS; the store is fp32, so there is no 2^-8 term.
  act_out         glue_oracle.bound_bf16 of (a, |a|), a = silu(xo) / 0.596 of the exact xo: the bound mp_silu has there.
  slab sums       |sum_s slab[s] - ref| <= (2^-8 [+ 2^-8 with scale] + chain * 2^-24) * mag
                  every slab is ONE bf16 rounding of its fp32 partial sum, so 2^-8 * mag covers all slabs together whatever the
                  split; `scale` adds the bf16 rounding wgrad_fold applies to scale[n] * dy; chain = the positions one slab sums
                  (ceil(positions / nsplit) + one 128-position tile).  The slabs are added in float64 by the test.

tests/test_conv_oracle.py pins both functions to float64 torch.nn.functional.conv2d + autograd assembled independently and checks
that the bounds are neither too tight nor too loose."""
import math

import torch

import glue_oracle as GO

EPI_NONE, EPI_EMB_SILU, EPI_MPSUM = 0, 1, 2
SILU_DIV = GO.SILU_DIV
U_BF16 = GO.U_BF16
U1 = 2.0 ** -24          # one round-to-nearest fp32 operation
EPI_OPS = 16


def roundup(a, b):
    return (a + b - 1) // b * b


def u_fwd(K, splits=0):
    return (K + splits + EPI_OPS) * U1


def bound_out(pair, u):
    """bf16 output of a forward launch: 2^-8 |ref| + u mag."""
    return U_BF16 * pair[0].abs() + u * pair[1]


def bound_act(pair):
    """out2 of EPI_EMB_SILU (an elementwise function of the kernel's own bf16 `out`).  The constant is fp32 underflow: from z < -87
    on sigmoid(z) is below 2^-126 and flushes to zero, an absolute error of at most |z| 2^-126 / 0.596 < 2^-112 for |z| < 2^13."""
    return U_BF16 * pair[0].abs() + GO.U_F32_64 * pair[1] + 2.0 ** -112


def bound_ctx_prod(pair, Cin):
    """The FP32 context product a one-frame launch keeps (OnirisConvArgs.ctx_prod): a sum of 18 Cin exact bf16 x bf16 products in
    fp32, in any order, + the four partial tiles added in LDS.  No 2^-8 term: the store is fp32."""
    return (18 * Cin + 4) * U1 * pair[1]


def wgrad_chain(positions, nsplit):
    return -(-positions // nsplit) + 128


def bound_wgrad(pair, chain, scaled):
    return ((2 if scaled else 1) * U_BF16 + chain * U1) * pair[1]


# ---------------------------------------------------------------------------------------------------------------------
# packing (what oniris_weight_prep writes; csrc/weights.hip)

def pack_wf(w, pad_rows=None):
    """w (cout, cin, taps) or (cout, cin, kt, taps) -> the forward packing [kt * taps][CoutP][CinP] (ci contiguous), CoutP =
    roundup(cout, 32), CinP = roundup(cin, 64).  pad_rows: value source for the padded rows co >= cout (a tensor [taps][CoutP][CinP]
    or None = zeros); the padded columns ci >= cin stay zero."""
    if w.ndim == 4:
        w = w.reshape(w.shape[0], w.shape[1], -1)
    cout, cin, taps = w.shape
    CoutP, CinP = roundup(cout, 32), roundup(cin, 64)
    p = torch.zeros(taps, CoutP, CinP, dtype=w.dtype)
    if pad_rows is not None:
        p[:, cout:, :cin] = pad_rows[:, cout:, :cin].to(w.dtype)
    p[:, :cout, :cin] = w.permute(2, 0, 1)
    return p


def pack_wb(w, pad_rows=None, _no_flip=False):
    """The data-gradient packing: wb[j * 9 + (8 - k)][ci][co] = w[co][ci][j * 9 + k] -- spatially flipped tap, same temporal slice,
    transposed -- as [kt * taps][roundup(cin, 32)][roundup(cout, 64)].  `_no_flip` is the defect of test_conv_oracle."""
    if w.ndim == 4:
        w = w.reshape(w.shape[0], w.shape[1], -1)
    cout, cin, tt = w.shape
    per = 9 if tt % 9 == 0 else 1
    idx = torch.arange(tt)
    src = idx if _no_flip else (idx // per) * per + (per - 1 - idx % per)
    return pack_wf(w[:, :, src].permute(1, 0, 2).contiguous(), pad_rows)


# ---------------------------------------------------------------------------------------------------------------------
def _conv_frames(x, w, taps, dtype, drop=None):
    """x (N, H, W, Ci), w (taps, Co, Ci) -> (value, mag) (N, H, W, Co): out[p] = sum_tap x[p + tap] @ w[tap]^T with tap = 3 ky + kx
    reading (y + ky - 1, x + kx - 1), zero outside the image.  drop = (frame, column, tap): that tap's term is left out there."""
    N, H, W, Ci = x.shape
    val = torch.zeros(N, H, W, w.shape[1], dtype=dtype)
    mag = torch.zeros_like(val)
    if taps == 1:
        return x @ w[0].T, x.abs() @ w[0].abs().T
    xp = torch.zeros(N, H + 2, W + 2, Ci, dtype=dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    for k in range(9):
        ky, kx = divmod(k, 3)
        patch = xp[:, ky:ky + H, kx:kx + W]
        t, m = patch @ w[k].T, patch.abs() @ w[k].abs().T
        if drop is not None and drop[2] == k:
            t[drop[0], :, drop[1]] = 0
            m[drop[0], :, drop[1]] = 0
        val += t
        mag += m
    return val, mag


def cat_input(x, x2, cat_w):
    """The two-source input of a 1x1 launch (OnirisConvArgs.x2): xo = [bf16(cat_w1 * x) | bf16(cat_w2 * x2)], every product formed in
    float32 from the float32 cat_w the launch is handed and rounded ONCE to bf16 -- the op's definition, reproduced exactly.
    x (..., C1), x2 (..., C2) -> float32 (..., C1 + C2) holding bf16 values."""
    f = lambda t, w: (t.detach().to("cpu", torch.float32) * torch.tensor(float(w), dtype=torch.float32)).to(torch.bfloat16).float()
    return torch.cat([f(x, cat_w[0]), f(x2, cat_w[1])], -1)


def conv_fwd(x, ctx, w_own, w_ctx, B, S, T, H, W, Cin, Cout, taps, coef_own=None, coef_ctx=None, ctx_bstride=0, ctx_T=0, coff=(0, 0),
             ctx_fill=0.0, epi=EPI_NONE, res=None, escale=None, ta=0.0, tb=0.0, clip=0.0, out_bf16=None, dtype=torch.float64,
             ctx_prod=None, ctx_prod_mode=0, ctx_rows=0, x2=None, x_split=0, cat_w=(1.0, 1.0), _defect=None):
    """oniris_conv_fwd:  v[n] = coef_own[n] * conv(x[n], w_own) + coef_ctx[n] * sum_j conv(ctxframe(b, t + coff[j]), w_ctx[j]),
    n = (b, s, t);  ctxframe(b, f) = ctx[b * ctx_bstride + f] if 0 <= f < ctx_T else a frame of ctx_fill (inside the image only:
    the spatial padding stays zero).  x (B*S*T, H, W, Cin); ctx (rows, H, W, Cin) or None; w_own [taps][CoutP][CinP], w_ctx
    [2 taps][CoutP][CinP] packed; coef_* (B*S*T,) or None (= 1); res (B*S*T, H, W, Cout); escale (B*S*T, Cout) -- pass the logical
    columns, the row pitch is the launch's business.  out_bf16: the kernel's own `out` for EPI_EMB_SILU (None: this function's
    rounding).  Returns a dict of (value, mag) pairs: 'v', 'out', and where they exist 'out2', 'ctx_out'; 'clip_hit' (bool: some
    |bf16(out)| >= clip) and 'clip_margin' (min over elements of | |q| - clip |, the distance of the unclipped sum from the clip).

    The evaluation-path options (include/oniris.h; all off by default):
      ctx_prod_mode   0 / 1: as above, and the entry 'ctx_prod' = the un-gated context product (y3, m3) that the launch keeps as an
                      FP32 tensor (mode 1; the same pair as 'ctx_out', which is its bf16 store);  3: that entry ALONE (x, coef_*, the
                      epilogue are not read);  2: `ctx_prod` is an INPUT, v = coef_own * y2 + coef_ctx * ctx_prod with magnitude
                      |coef_own| m2 + |coef_ctx| |ctx_prod| -- ctx and w_ctx are not read (None will do).
      ctx_rows        R > 0 with B = 2 R, S = T = 1 (a guided pair): ctx, coef_*, escale and ctx_prod hold R rows; rows b >= R are
                      v = y2 alone -- no coefficient, no context -- with the epilogue on escale[b - R] and res[b]; 'ctx_prod' (and
                      'ctx_out') have R rows.
      x2, x_split,    taps 1 without a context: the input is xo = cat_input(x (.., x_split), x2 (.., Cin - x_split), cat_w), the conv
      cat_w           is taken of that xo in float64, and 'act_out' = (silu(xo) / 0.596, its magnitude): an elementwise function
                      of the exact xo, the pair glue_oracle.act_fwd gives mp_silu.
    `_defect`: the deliberate defects of test_conv_oracle (None: the restatement)."""
    N = B * S * T
    R = ctx_rows
    assert R == 0 or (B == 2 * R and S == 1 and T == 1)
    Bc = R if R else B                                # the sequences that have a context
    Nc = Bc * S * T
    d = lambda t: None if t is None else t.detach().to("cpu", dtype)
    r = {}
    if x2 is not None:
        assert taps == 1 and ctx is None and 0 < x_split < Cin
        if _defect == "cat_swap":
            cat_w = (cat_w[1], cat_w[0])
        x2 = x2.reshape(N, H, W, Cin - x_split)
        xo = cat_input(x.reshape(N, H, W, x_split), x2, cat_w)
        if _defect == "split_off8":                   # the scale changes 8 channels late: x2's first 8 channels times cat_w1
            xo[..., x_split:x_split + 8] = cat_input(x2[..., :8], x2[..., :0], cat_w)
        x = xo
        a = xo.double() * torch.sigmoid(xo.double()) / SILU_DIV
        r["act_out"] = (a.to(dtype), a.abs().to(dtype))
    has_ctx = ctx is not None or ctx_prod_mode == 2
    y3 = m3 = None
    if has_ctx:
        if ctx_prod_mode == 2:
            y3 = d(ctx_prod).reshape(Bc * T, H, W, Cout)
            m3 = y3.abs()
        else:
            ctx = d(ctx).reshape(-1, H, W, Cin)
            wc = d(w_ctx)[:, :Cout, :Cin]
            if _defect == "coff_swap":
                coff = (coff[1], coff[0])
            if _defect == "append_bstride":
                ctx_bstride = T
            fill = 0.0 if _defect == "fill0" else ctx_fill
            y3 = torch.zeros(Bc * T, H, W, Cout, dtype=dtype)
            m3 = torch.zeros_like(y3)
            for j in range(2):
                fr = torch.full((Bc * T, H, W, Cin), fill, dtype=dtype)
                for b in range(Bc):
                    for t in range(T):
                        f = t + coff[j]
                        if 0 <= f < ctx_T:
                            fr[b * T + t] = ctx[b * ctx_bstride + f]
                        elif _defect == "cross_sequence" and coff[j] == -1 and b > 0:
                            fr[b * T + t] = ctx[b * ctx_bstride + f]            # the frame in front of row b's first: row b - 1's
                t_, m_ = _conv_frames(fr, wc[j * taps:(j + 1) * taps], taps, dtype)
                y3 += t_
                m3 += m_
            r["ctx_out"] = (y3, m3)
            r["ctx_prod"] = (GO.bf(y3), m3) if _defect == "ctx_prod_bf16" else (y3, m3)
            if ctx_prod_mode == 3:
                return {"ctx_prod": r["ctx_prod"]}
    x = d(x).reshape(N, H, W, Cin)
    wo = d(w_own)[:, :Cout, :Cin]
    drop = (1, 0, 4) if _defect == "tap_drop" else None
    y2, m2 = _conv_frames(x, wo, taps, dtype, drop)
    co = torch.ones(N, dtype=dtype)                   # (rows b >= ctx_rows: no coefficient)
    if coef_own is not None:
        co[:Nc] = d(coef_own).reshape(Nc)
    if _defect == "pair_twin_coef":
        co[R:] = co[:R]
    v, mag = co.reshape(N, 1, 1, 1) * y2, co.abs().reshape(N, 1, 1, 1) * m2
    if has_ctx:
        cc = torch.zeros(N, dtype=dtype)              # (rows b >= ctx_rows: no context)
        cc[:Nc] = 1.0 if coef_ctx is None else d(coef_ctx).reshape(Nc)
        if _defect == "coef_neighbour":
            cc[1] = cc[2]
        if _defect == "pair_ctx_added":
            cc[R:] = cc[:R]
        if _defect == "mode2_scaled":
            cc = cc * co
        e3 = lambda t: t.reshape(Bc, 1, T, H, W, Cout).expand(Bc, S, T, H, W, Cout).reshape(Nc, H, W, Cout)
        y3n, m3n = e3(y3), e3(m3)
        if R:                                         # the twin's product, which only a defect's coefficient lets through
            y3n, m3n = torch.cat([y3n, y3n]), torch.cat([m3n, m3n])
        v = v + cc.reshape(N, 1, 1, 1) * y3n
        mag = mag + cc.abs().reshape(N, 1, 1, 1) * m3n
    if _defect == "ragged_cout":
        # ONE 16-byte store -- the last 8-channel block of one pixel -- filled from the padded weight rows behind it
        lo = Cout - 8
        alt = _conv_frames(x[3:4], d(w_own)[:, lo + 8:lo + 16, :Cin], taps, dtype)[0]
        v = v.clone()
        v[3, H // 2, W // 2, lo:] = co[3] * alt[0, H // 2, W // 2]
    r["v"] = (v, mag)
    r["clip_hit"], r["clip_margin"] = False, math.inf
    if epi == EPI_NONE:
        r["out"] = (v, mag)
    elif epi == EPI_EMB_SILU:
        r["out"] = (v, mag)
        vb = GO.bf(v) if out_bf16 is None else d(out_bf16).reshape(N, H, W, Cout)
        es = d(escale).reshape(Nc, 1, 1, Cout)
        if R:                                         # a 2-D row reads the emb-scale row of its twin
            es = torch.cat([es, es[:1].expand(R, 1, 1, Cout) if _defect == "pair_escale0" else es])
        z = vb * es
        a = z * torch.sigmoid(z) / SILU_DIV
        r["out2"] = (a, (1 + z.abs()) * a.abs())
    else:
        assert epi == EPI_MPSUM
        tr = ta * d(res).reshape(N, H, W, Cout)
        q, mq = tr + tb * v, tr.abs() + abs(tb) * mag
        r["out2"] = (v, mag)
        if clip > 0:
            r["clip_margin"] = float((q.abs() - clip).abs().min())
            q = q.clamp(-clip, clip)
            r["clip_hit"] = bool((GO.bf(q).abs() >= clip).any())
        r["out"] = (q, mq)
    return r


def conv_wgrad(x, dy, scale, B, T, H, W, Cin, Cout, taps, xb_stride, x_T, coff, fill, tap0, taps_total, dtype=torch.float64,
               _defect=None):
    """One group of oniris_conv_wgrad_group, all slabs together:
      dw[co][tap0 + tap][ci] = sum_{n = (b, t), p} scale[n] * dy[n][p][co] * xframe(n)[p + tap][ci]
    xframe(b, t) = x[b * xb_stride + t + coff] if 0 <= t + coff < x_T else a frame of `fill` (zero outside the image).
    x (rows, H, W, Cin); dy (B*T, H, W, Cout); scale (B*T,) or None.  Returns (value, mag) of shape (Cout, taps_total, Cin), zero
    outside [tap0, tap0 + taps).  With `scale` the kernel rounds scale[n] * dy to bf16 first (wgrad_fold): that rounding is part
    of the bound, not of this function."""
    d = lambda t: None if t is None else t.detach().to("cpu", dtype)
    x = d(x).reshape(-1, H, W, Cin)
    g = d(dy).reshape(B * T, H, W, Cout)
    if scale is not None:
        g = g * d(scale).reshape(B * T, 1, 1, 1)
    fr = torch.full((B * T, H, W, Cin), fill, dtype=dtype)
    for b in range(B):
        for t in range(T):
            f = t + coff
            if 0 <= f < x_T:
                fr[b * T + t] = x[b * xb_stride + f]
    if _defect == "tap0_off":
        tap0 = (tap0 + taps) % taps_total if taps_total > taps else tap0 + 1
    val = torch.zeros(Cout, taps_total + (1 if _defect == "tap0_off" else 0), Cin, dtype=dtype)
    mag = torch.zeros_like(val)
    g2, ga = g.reshape(-1, Cout), g.abs().reshape(-1, Cout)
    if taps == 1:
        val[:, tap0], mag[:, tap0] = g2.T @ fr.reshape(-1, Cin), ga.T @ fr.abs().reshape(-1, Cin)
    else:
        xp = torch.zeros(B * T, H + 2, W + 2, Cin, dtype=dtype)
        xp[:, 1:H + 1, 1:W + 1] = fr
        for k in range(9):
            ky, kx = divmod(k, 3)
            patch = xp[:, ky:ky + H, kx:kx + W]
            val[:, tap0 + k] = g2.T @ patch.reshape(-1, Cin)
            mag[:, tap0 + k] = ga.T @ patch.abs().reshape(-1, Cin)
            if _defect == "tile_missing" and k == 4:
                # one 32 x 32 (co, ci) block of the centre tap without one 8 x 16-pixel position tile of frame 1
                gt, pt = g[1, :8, :16].reshape(-1, Cout), patch[1, :8, :16].reshape(-1, Cin)
                val[:32, tap0 + k, :32] -= (gt.T @ pt)[:32, :32]
    return val[:, :taps_total], mag[:, :taps_total]

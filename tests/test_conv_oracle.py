"""Review of tests/conv_oracle.py (the float64 restatements test_conv_stages_gpu.py holds the conv kernels to)  --  CPU only.

  pinned         every restatement against float64 torch.nn.functional.conv2d + autograd assembled independently (the context
                 concatenation of test_ops_gpu._gated_conv_train_case, oracle.oniris_oracle.mp_sum / mp_silu): forward, data gradient
                 through the flipped and transposed `wb` packing, weight gradient; 1e-12 relative.  The evaluation-path options
                 likewise: the append against ONE F.conv3d over [cached pair | new frames], ctx_prod_mode 1 / 2 / 3, the rows of a
                 guided pair (ctx_rows), the two-source 1x1 conv with its activation
  not too tight  the same formulas with bf16 operands, fp32 accumulation and one bf16 store fit every bound
  not too loose  deliberate defects injected into the restatement exceed the bound on at least one element -- while the starred ones
                 change the tensor's relative L2 norm by less than the 5e-3 the aggregate tests (test_ops_gpu.py) allow.  For the
                 evaluation path: a 2-D row of a pair with its twin's gate coefficient, with the context added, with emb-scale row 0;
                 a kept product scaled by coef_own or stored through bf16; an append with the row stride of its frames alone; the
                 cat weights swapped; the split 8 channels late
  exact probes   for every case of test_conv_stages_gpu.py: all values integers and mag <= 256 for every output element and every
                 weight-gradient element, the condition under which any summation order and any split is exact

The weight-gradient defect (a lost position tile) is shown on same-sign data (post-activation-like: mag = |ref|), the regime in
which the slab bound is sharpest.  On signed Gaussian data a lost tile is far below 2^-8 mag: there it is the integer-exact probes'
part, as a lost element is for the glue reductions (test_glue_stages_gpu.py)."""
import math

import pytest
import torch

import conv_oracle as CO
import test_conv_stages_gpu as CS
from oracle import oniris_oracle as O

F = torch.nn.functional
F64 = torch.float64
torch.set_num_threads(min(16, torch.get_num_threads()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def close(a, b, what):
    err = float((a - b).abs().max() / b.abs().max())
    assert err <= 1e-12, (what, err)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def _gated_problem(B, T, H, W, cin, cout, seed, pos=False):
    """Inputs of a gated conv in the DART training layout + its float64 autograd graph, assembled as _gated_conv_train_case does."""
    gen = _gen(seed)
    N = B * 2 * T
    r = (lambda *s: torch.rand(*s, generator=gen, dtype=F64)) if pos else (lambda *s: torch.randn(*s, generator=gen, dtype=F64))
    x = r(N, cin, H, W).requires_grad_(True)
    w2 = (r(cout, cin, 3, 3) / math.sqrt(9 * cin)).requires_grad_(True)
    w3 = (r(cout, cin, 2, 3, 3) / math.sqrt(18 * cin)).requires_grad_(True)
    g = (torch.rand(N, generator=gen, dtype=F64) * 0.6 + 0.05)
    y2 = F.conv2d(x, w2, padding=1)
    clean = x.reshape(B, 2, T, cin, H, W)[:, 0]
    ctx = torch.cat([torch.ones(B, 2, cin, H, W, dtype=F64), clean], 1)
    y3 = F.conv2d(ctx[:, 0:T].reshape(B * T, cin, H, W), w3[:, :, 0], padding=1) + \
        F.conv2d(ctx[:, 1:T + 1].reshape(B * T, cin, H, W), w3[:, :, 1], padding=1)
    y3e = y3.reshape(B, 1, T, cout, H, W).expand(B, 2, T, cout, H, W).reshape(N, cout, H, W)
    v = O.mp_sum(y2, y3e, g)
    norm = ((1 - g) ** 2 + g ** 2) ** -0.5
    return dict(x=x, w2=w2, w3=w3, ca=(1 - g) * norm, cb=g * norm, v=v, y3=y3, gen=gen, N=N)


def _train_kw(B, T, H, W, cin, cout):
    return dict(B=B, S=2, T=T, H=H, W=W, Cin=cin, Cout=cout, taps=9, ctx_bstride=2 * T, ctx_T=T, coff=(-2, -1), ctx_fill=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# pinned

@pytest.mark.parametrize("B,T,H,W,cin,cout", [(2, 3, 4, 6, 8, 16), (1, 1, 5, 3, 16, 8)])
def test_forward_is_pinned(B, T, H, W, cin, cout):
    p = _gated_problem(B, T, H, W, cin, cout, 5)
    gen, N = p["gen"], p["N"]
    xl = nhwc(p["x"].detach())
    wf2, wf3 = CO.pack_wf(p["w2"].detach().reshape(cout, cin, 9)), CO.pack_wf(p["w3"].detach().reshape(cout, cin, 2, 9))
    kw = _train_kw(B, T, H, W, cin, cout)
    r = CO.conv_fwd(xl, xl, wf2, wf3, coef_own=p["ca"], coef_ctx=p["cb"], **kw)
    close(r["out"][0], nhwc(p["v"].detach()), "v")
    close(r["ctx_out"][0], nhwc(p["y3"].detach()), "y3")
    assert bool((r["out"][1] >= r["out"][0].abs() * (1 - 1e-12)).all())
    # EPI_MPSUM = mp_sum(res, v, t) clipped; EPI_EMB_SILU = mp_silu(v * c)
    t = 0.3
    res = torch.randn(N, cout, H, W, generator=gen, dtype=F64)
    nrm = math.sqrt((1 - t) ** 2 + t ** 2)
    for clip in (0.0, 0.75):       # (bf16-representable: the flag tests the STORED value)
        want = O.mp_sum(res, p["v"].detach(), t)
        if clip > 0:
            want = want.clamp(-clip, clip)
        r = CO.conv_fwd(xl, xl, wf2, wf3, coef_own=p["ca"], coef_ctx=p["cb"], epi=CO.EPI_MPSUM, res=nhwc(res), ta=(1 - t) / nrm, tb=t / nrm,
                        clip=clip, **kw)
        close(r["out"][0], nhwc(want), f"mpsum clip={clip}")
        close(r["out2"][0], nhwc(p["v"].detach()), "raw")
        assert r["clip_hit"] == (clip > 0)
    c = 1 + 0.3 * torch.randn(N, cout, generator=gen, dtype=F64)
    r = CO.conv_fwd(xl, xl, wf2, wf3, coef_own=p["ca"], coef_ctx=p["cb"], epi=CO.EPI_EMB_SILU, escale=c, out_bf16=nhwc(p["v"].detach()), **kw)
    close(r["out2"][0], nhwc(O.mp_silu(p["v"].detach() * c[:, :, None, None])), "emb_silu")


def test_plain_and_1x1_are_pinned():
    gen = _gen(9)
    x = torch.randn(3, 16, 5, 7, generator=gen, dtype=F64)
    for taps in (9, 1):
        k = 3 if taps == 9 else 1
        w = torch.randn(24, 16, k, k, generator=gen, dtype=F64)
        r = CO.conv_fwd(nhwc(x), None, CO.pack_wf(w.reshape(24, 16, taps)), None, 1, 1, 3, 5, 7, 16, 24, taps)
        close(r["out"][0], nhwc(F.conv2d(x, w, padding=k // 2)), f"plain taps={taps}")


def _cached_problem(B, T, H, W, cin, cout, seed):
    """A cached evaluation assembled with torch: T new frames per sequence behind a cached pair, the context product as ONE
    F.conv3d over [pair | frames] (edm2/conv.py:84-86), NCHW float64."""
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    x, pair = r(B, T, cin, H, W), r(B, 2, cin, H, W)
    w2, w3 = r(cout, cin, 3, 3) / math.sqrt(9 * cin), r(cout, cin, 2, 3, 3) / math.sqrt(18 * cin)
    ca, cb = torch.rand(B * T, generator=gen, dtype=F64) + 0.2, torch.rand(B * T, generator=gen, dtype=F64) - 0.5
    y2 = F.conv2d(x.reshape(B * T, cin, H, W), w2, padding=1)
    m2 = F.conv2d(x.reshape(B * T, cin, H, W).abs(), w2.abs(), padding=1)
    seq = torch.cat([pair, x], 1).permute(0, 2, 1, 3, 4)                                  # (B, cin, T + 2, H, W)
    y3 = F.conv3d(seq, w3, padding=(0, 1, 1))[:, :, :T].permute(0, 2, 1, 3, 4).reshape(B * T, cout, H, W)
    m3 = F.conv3d(seq.abs(), w3.abs(), padding=(0, 1, 1))[:, :, :T].permute(0, 2, 1, 3, 4).reshape(B * T, cout, H, W)
    flat = lambda t: nhwc(t.reshape(-1, *t.shape[2:]))
    return dict(x=x, pair=pair, xl=flat(x), pairl=flat(pair), ctxl=flat(torch.cat([pair, x], 1)), wf2=CO.pack_wf(w2.reshape(cout, cin, 9)),
                wf3=CO.pack_wf(w3.reshape(cout, cin, 2, 9)), w2=w2, ca=ca, cb=cb, y2=y2, m2=m2, y3=y3, m3=m3, gen=gen)


def test_append_is_pinned():
    """S = 1, ctx = [cached pair | the T new frames] with row stride T + 2 and coff (0, 1)."""
    B, T, H, W, cin, cout = 2, 3, 4, 6, 8, 16
    p = _cached_problem(B, T, H, W, cin, cout, 21)
    r = CO.conv_fwd(p["xl"], p["ctxl"], p["wf2"], p["wf3"], B, 1, T, H, W, cin, cout, 9, coef_own=p["ca"], coef_ctx=p["cb"],
                    ctx_bstride=T + 2, ctx_T=T + 2, coff=(0, 1))
    e = lambda c: c.reshape(-1, 1, 1, 1)
    close(r["out"][0], nhwc(e(p["ca"]) * p["y2"] + e(p["cb"]) * p["y3"]), "append v")
    close(r["out"][1], nhwc(e(p["ca"]).abs() * p["m2"] + e(p["cb"]).abs() * p["m3"]), "append mag")
    close(r["ctx_prod"][0], nhwc(p["y3"]), "append y3")


def test_ctx_prod_modes_and_ctx_rows_are_pinned():
    """The one-frame forms: the kept product written (1), alone (3), read back (2); the guided pair with every epilogue."""
    R, H, W, cin, cout = 3, 4, 6, 8, 16
    p = _cached_problem(R, 1, H, W, cin, cout, 22)
    gen = p["gen"]
    e = lambda c: c.reshape(-1, 1, 1, 1)
    v3 = e(p["ca"]) * p["y2"] + e(p["cb"]) * p["y3"]
    geo = dict(B=R, S=1, T=1, H=H, W=W, Cin=cin, Cout=cout, taps=9)
    one = dict(geo, ctx_bstride=2, ctx_T=2, coff=(0, 1), coef_own=p["ca"], coef_ctx=p["cb"])
    for pm in (0, 1):
        r = CO.conv_fwd(p["xl"], p["pairl"], p["wf2"], p["wf3"], ctx_prod_mode=pm, **one)
        close(r["out"][0], nhwc(v3), f"mode {pm} v")
        close(r["ctx_prod"][0], nhwc(p["y3"]), f"mode {pm} y3")
        close(r["ctx_prod"][1], nhwc(p["m3"]), f"mode {pm} m3")
    r = CO.conv_fwd(None, p["pairl"], p["wf2"], p["wf3"], ctx_prod_mode=3, **dict(one, coef_own=None, coef_ctx=None))
    assert set(r) == {"ctx_prod"}
    close(r["ctx_prod"][0], nhwc(p["y3"]), "mode 3 y3")
    kept = torch.randn(R, cout, H, W, generator=gen, dtype=F64)
    r = CO.conv_fwd(p["xl"], None, p["wf2"], None, ctx_prod=nhwc(kept), ctx_prod_mode=2, **one)
    close(r["out"][0], nhwc(e(p["ca"]) * p["y2"] + e(p["cb"]) * kept), "mode 2 v")
    close(r["out"][1], nhwc(e(p["ca"]).abs() * p["m2"] + e(p["cb"]).abs() * kept.abs()), "mode 2 mag")
    assert "ctx_prod" not in r
    # the pair: R more rows of x and res, y2 alone, the emb-scale row of the twin
    x2d = torch.randn(R, cin, H, W, generator=gen, dtype=F64)
    vp = torch.cat([v3, F.conv2d(x2d, p["w2"], padding=1)])
    xp = torch.cat([p["xl"], nhwc(x2d)])
    pk = dict(one, B=2 * R, ctx_rows=R)
    c = 1 + 0.3 * torch.randn(R, cout, generator=gen, dtype=F64)
    res = torch.randn(2 * R, cout, H, W, generator=gen, dtype=F64)
    r = CO.conv_fwd(xp, p["pairl"], p["wf2"], p["wf3"], epi=CO.EPI_EMB_SILU, escale=c, out_bf16=nhwc(vp), ctx_prod_mode=1, **pk)
    close(r["out"][0], nhwc(vp), "pair v")
    close(r["out2"][0], nhwc(O.mp_silu(vp * torch.cat([c, c])[:, :, None, None])), "pair emb_silu")
    close(r["ctx_prod"][0], nhwc(p["y3"]), "pair y3")
    assert r["ctx_prod"][0].shape[0] == R
    t = 0.3
    nrm = math.sqrt((1 - t) ** 2 + t ** 2)
    r = CO.conv_fwd(xp, p["pairl"], p["wf2"], p["wf3"], epi=CO.EPI_MPSUM, res=nhwc(res), ta=(1 - t) / nrm, tb=t / nrm, **pk)
    close(r["out"][0], nhwc(O.mp_sum(res, vp, t)), "pair mpsum")
    r = CO.conv_fwd(xp, None, p["wf2"], None, ctx_prod=nhwc(kept), ctx_prod_mode=2, **pk)
    close(r["out"][0], nhwc(torch.cat([e(p["ca"]) * p["y2"] + e(p["cb"]) * kept, vp[R:]])), "pair mode 2")


def test_two_source_1x1_is_pinned():
    gen = _gen(23)
    N, H, W, C1, C2, cout = 3, 5, 7, 24, 16, 40
    bf = lambda t: t.to(torch.bfloat16)
    x, skip = bf(torch.randn(N, C1, H, W, generator=gen)), bf(torch.randn(N, C2, H, W, generator=gen))
    w = torch.randn(cout, C1 + C2, 1, 1, generator=gen, dtype=F64)
    w1, w2 = 1.2345678, 0.7654321
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    xo = torch.cat([bf(x.float() * f32(w1)), bf(skip.float() * f32(w2))], 1).double()
    r = CO.conv_fwd(nhwc(x), None, CO.pack_wf(w.reshape(cout, C1 + C2, 1)), None, 1, 1, N, H, W, C1 + C2, cout, 1, x2=nhwc(skip), x_split=C1,
                    cat_w=(w1, w2))
    close(r["out"][0], nhwc(F.conv2d(xo, w)), "two-source out")
    close(r["out"][1], nhwc(F.conv2d(xo.abs(), w.abs())), "two-source mag")
    close(r["act_out"][0], nhwc(O.mp_silu(xo)), "act_out")


@pytest.mark.parametrize("B,T,H,W,cin,cout", [(2, 3, 4, 6, 8, 16), (2, 1, 3, 5, 16, 8)])
def test_data_and_weight_gradient_are_pinned(B, T, H, W, cin, cout):
    p = _gated_problem(B, T, H, W, cin, cout, 6)
    N = p["N"]
    gy = torch.randn(N, cout, H, W, generator=p["gen"], dtype=F64)
    (p["v"] * gy).sum().backward()
    w2, w3 = p["w2"].detach().reshape(cout, cin, 9), p["w3"].detach().reshape(cout, cin, 2, 9)
    dout = nhwc(gy)
    dy3 = (p["cb"].reshape(B, 2, T, 1, 1, 1) * dout.reshape(B, 2, T, H, W, cout)).sum(1).reshape(B * T, H, W, cout)
    sel = torch.zeros(B, 2, T, dtype=F64)
    sel[:, 0] = 1
    # data gradient: the same entry point, x = dout, ctx = dy3, coff (+2, +1), fill 0, the wb packing; Cin and Cout change places
    r = CO.conv_fwd(dout, dy3, CO.pack_wb(w2), CO.pack_wb(w3), B, 2, T, H, W, cout, cin, 9, coef_own=p["ca"], coef_ctx=sel.reshape(-1),
                    ctx_bstride=T, ctx_T=T, coff=(2, 1), ctx_fill=0.0)
    close(r["out"][0], nhwc(p["x"].grad), "dx")
    bad = CO.conv_fwd(dout, dy3, CO.pack_wb(w2, _no_flip=True), CO.pack_wb(w3, _no_flip=True), B, 2, T, H, W, cout, cin, 9, coef_own=p["ca"],
                      coef_ctx=sel.reshape(-1), ctx_bstride=T, ctx_T=T, coff=(2, 1), ctx_fill=0.0)
    assert rel_l2(bad["out"][0], nhwc(p["x"].grad)) > 0.1
    # weight gradient: own group over all B 2 T frames with the per-frame coefficient, the context taps into the 18-deep slabs
    xl = nhwc(p["x"].detach())
    dw2 = CO.conv_wgrad(xl, dout, p["ca"], 1, N, H, W, cin, cout, 9, N, N, 0, 0.0, 0, 9)
    close(dw2[0], p["w2"].grad.reshape(cout, cin, 9).permute(0, 2, 1), "dw2")
    want3 = p["w3"].grad.reshape(cout, cin, 18).permute(0, 2, 1)
    got3 = sum(CO.conv_wgrad(xl, dy3, None, B, T, H, W, cin, cout, 9, 2 * T, T, coff, 1.0, 9 * j, 18)[0] for j, coff in enumerate((-2, -1)))
    close(got3, want3, "dw3")
    one = CO.conv_wgrad(xl, dy3, None, B, T, H, W, cin, cout, 9, 2 * T, T, -1, 1.0, 9, 18)
    assert float(one[0][:, :9].abs().max()) == 0.0 and float(one[1][:, :9].abs().max()) == 0.0
    # 1x1
    w1 = torch.randn(cout, cin, 1, 1, generator=p["gen"], dtype=F64).requires_grad_(True)
    xx = p["x"].detach()
    (F.conv2d(xx, w1) * gy).sum().backward()
    close(CO.conv_wgrad(xl, dout, None, 1, N, H, W, cin, cout, 1, N, N, 0, 0.0, 0, 1)[0], w1.grad.reshape(cout, cin, 1).permute(0, 2, 1), "dw 1x1")


# ---------------------------------------------------------------------------------------------------------------------
# not too tight: the GPU cases themselves, evaluated with bf16 operands, fp32 accumulation and one bf16 store

def _usage(what, got, ref, bound):
    err = (got.double() - ref).abs()
    live = bound > 0
    assert bool((err[~live] == 0).all()), what
    use = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"CONV-ORACLE float32 {what}: uses {use:.3f} of the bound")
    assert use <= 1.0, (what, use)


_TIGHT_FWD = [r for r in CS.FWD if r[0] in ("st_8x8", "st_2x2", "st_8x8_dgrad", "st_1x1_36", "g16_64_64", "g8_32_64", "s_alias", "few_2", "ev_8x8", "st_1x1_nt3",
                                                     "ap_8x8", "ap_ones", "e1_store", "e1_ctx_96", "e1_read_160", "pair_silu", "pair_read",
                                                     "cat_few_ragged", "cat_few_512")]


@pytest.mark.parametrize("row", _TIGHT_FWD, ids=lambda r: r[0])
def test_forward_bounds_are_not_too_tight(row):
    name, mode, B, T, H, W, Cin, Cout, taps, epi = row[:10]
    d = CS.fwd_inputs(row, False)
    d["clip"] = CS.pick_clip(d, epi, False)
    kw = {k: d[k] for k in CS._FWD_KW + ("clip",)}
    ctx = d["x"] if isinstance(d["ctx"], str) else d["ctx"]
    lo = CO.conv_fwd(d["x"], ctx, d["w_own"], d["w_ctx"], dtype=torch.float32, **kw)
    if d["ctx_prod_mode"] in (1, 3):                 # the kept product: fp32 sum, fp32 store
        rp = CS.fwd_reference(d)["ctx_prod"]
        _usage(f"{name} ctx_prod", lo["ctx_prod"][0], rp[0], CO.bound_ctx_prod(rp, d["Cin"]))
        if d["ctx_prod_mode"] == 3:
            return
    out = lo["out"][0].to(torch.bfloat16)
    r = CS.fwd_reference(d, out_bf16=out)
    u = CS.fwd_u(row)
    _usage(f"{name} out", out, r["out"][0], CO.bound_out(r["out"], u))
    if "act_out" in r:
        xo = CO.cat_input(d["x"], d["x2"], d["cat_w"])
        a32 = xo * torch.sigmoid(xo) / torch.tensor(CO.SILU_DIV, dtype=torch.float32)
        _usage(f"{name} act_out", a32.to(torch.bfloat16), r["act_out"][0], CS.GO.bound_bf16(*r["act_out"]))
    if "ctx_out" in r:
        u3 = CO.u_fwd(taps * d["Cin"] * CS._ctx_phases(mode), 12)
        _usage(f"{name} ctx_out", lo["ctx_out"][0].to(torch.bfloat16), r["ctx_out"][0], CO.bound_out(r["ctx_out"], u3))
    if d["epi"] == CO.EPI_EMB_SILU:
        lo2 = CO.conv_fwd(d["x"], ctx, d["w_own"], d["w_ctx"], dtype=torch.float32, out_bf16=out, **kw)
        _usage(f"{name} out2", lo2["out2"][0].to(torch.bfloat16), r["out2"][0], CO.bound_act(r["out2"]))
    elif d["epi"] == CO.EPI_MPSUM:
        _usage(f"{name} out2", lo["out2"][0].to(torch.bfloat16), r["out2"][0], CO.bound_out(r["out2"], u))


@pytest.mark.parametrize("row", [r for r in CS.WGRAD if r[0] in ("wr_8", "wr_1x1", "wg_16", "wg_many", "w1_glds")], ids=lambda r: r[0])
def test_wgrad_bounds_are_not_too_tight(row):
    """Four slabs: every quarter of the frames summed in fp32 (scale * dy rounded to bf16 first) and rounded to bf16 once."""
    for g in CS.wgrad_groups(row, False):
        ref, mag = CS.wgrad_reference(g)
        Bq, Tq = g["B"], g["T"]
        dy = g["dy"].float().reshape(Bq * Tq, g["H"], g["W"], g["Cout"])
        if g["scale"] is not None:
            dy = (dy * g["scale"].float().reshape(-1, 1, 1, 1)).to(torch.bfloat16).float()
        total, nslab = torch.zeros_like(ref), 4
        for s in range(nslab):
            part = dy.clone()
            part[[n for n in range(Bq * Tq) if n % nslab != s]] = 0
            total += CO.conv_wgrad(g["x"], part, None, Bq, Tq, g["H"], g["W"], g["Cin"], g["Cout"], g["taps"], g["xb_stride"], g["x_T"],
                                   g["coff"], g["fill"], g["tap0"], g["taps_total"], dtype=torch.float32)[0].to(torch.bfloat16).double()
        chain = CO.wgrad_chain(Bq * Tq * g["H"] * g["W"], nslab)
        _usage(f"{row[0]} dw_{g['key']}", total, ref, CO.bound_wgrad((ref, mag), chain, g["scale"] is not None))


# ---------------------------------------------------------------------------------------------------------------------
# not too loose

def _wide(cout, seed=11):
    """B, T, H, W = 2, 40, 8, 32: wide and long enough that ONE border column of ONE frame is below the aggregate tests' 5e-3."""
    B, T, H, W, cin = 2, 40, 8, 32, 8
    gen = _gen(seed)
    N = B * 2 * T
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(N, H, W, cin, generator=gen))
    pad = bf(torch.randn(18, CO.roundup(cout, 32), 64, generator=gen) / math.sqrt(27 * cin))
    w2 = CO.pack_wf(bf(torch.randn(cout, cin, 9, generator=gen) / math.sqrt(27 * cin)), pad[:9])
    w3 = CO.pack_wf(bf(torch.randn(cout, cin, 2, 9, generator=gen) / math.sqrt(27 * cin)), pad)
    t = (torch.arange(N) % T).float()
    ca, cb = 0.9 - 0.01 * t, 0.3 + 0.02 * t                  # distinct per frame, varying as slowly as a gate does
    kw = dict(_train_kw(B, T, H, W, cin, cout), coef_own=ca, coef_ctx=cb)
    return x, w2, w3, kw


def _defect(what, got, ref, bound, starred):
    err = (got - ref).abs()
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    if bool((err[~live] > 0).any()):
        worst = math.inf
    l2 = rel_l2(got, ref)
    print(f"CONV-ORACLE defect {what}: worst error / bound {worst:.1f}, relative L2 {l2:.2e}{'  *' if starred else ''}")
    assert worst > 1.0, (what, worst)
    if starred:
        assert l2 < 5e-3, (what, l2)


def _eval_defect_problem(defect):
    """The evaluation-path launch a defect is shown on: (positional arguments, keyword arguments, the tensor held, its bound as a
    function of the good pair).  bf16 operands; the coefficients, emb-scales and cat weights differ from row to row as they do in
    a rollout."""
    gen = _gen(31)
    bf = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(torch.bfloat16)
    H = W = 8
    cin = cout = 8
    if defect in ("cat_swap", "split_off8"):
        C1, C2, N = 24, 16, 2
        args = (bf(N, H, W, C1), None, CO.pack_wf(bf(cout, C1 + C2, 1, scale=(C1 + C2) ** -0.5)), None, 1, 1, N, H, W, C1 + C2, cout, 1)
        kw = dict(x2=bf(N, H, W, C2), x_split=C1, cat_w=(1.29, 0.91))
        return args, kw, "out", lambda good: CO.bound_out(good, CO.u_fwd(C1 + C2, 12))
    w2, w3 = CO.pack_wf(bf(cout, cin, 9, scale=(27 * cin) ** -0.5)), CO.pack_wf(bf(cout, cin, 2, 9, scale=(27 * cin) ** -0.5))
    if defect == "append_bstride":
        B, T = 2, 3
        x, pair = bf(B, T, H, W, cin), bf(B, 2, H, W, cin)
        args = (x, torch.cat([pair, x], 1), w2, w3, B, 1, T, H, W, cin, cout, 9)
        kw = dict(coef_own=0.9 - 0.05 * torch.arange(B * T), coef_ctx=0.3 + 0.05 * torch.arange(B * T), ctx_bstride=T + 2, ctx_T=T + 2, coff=(0, 1))
        return args, kw, "out", lambda good: CO.bound_out(good, CO.u_fwd(27 * cin, 12))
    R = 2
    one = dict(coef_own=0.9 - 0.1 * torch.arange(R), coef_ctx=0.3 + 0.1 * torch.arange(R), ctx_bstride=2, ctx_T=2, coff=(0, 1))
    if defect in ("mode2_scaled", "ctx_prod_bf16"):
        pm = 2 if defect == "mode2_scaled" else 1
        args = (bf(R, H, W, cin), bf(R * 2, H, W, cin), w2, w3, R, 1, 1, H, W, cin, cout, 9)
        kw = dict(one, ctx_prod_mode=pm, ctx_prod=torch.randn(R, H, W, cout, generator=gen) if pm == 2 else None)
        if pm == 1:
            return args, kw, "ctx_prod", lambda good: CO.bound_ctx_prod(good, cin)
        return args, kw, "out", lambda good: CO.bound_out(good, CO.u_fwd(9 * cin, 12))
    assert defect in ("pair_twin_coef", "pair_ctx_added", "pair_escale0"), defect
    args = (bf(2 * R, H, W, cin), bf(R * 2, H, W, cin), w2, w3, 2 * R, 1, 1, H, W, cin, cout, 9)
    kw = dict(one, ctx_rows=R, epi=CO.EPI_EMB_SILU, escale=1 + 0.3 * torch.randn(R, cout, generator=gen))
    if defect == "pair_escale0":
        return args, kw, "out2", CO.bound_act
    u = torch.tensor([CO.u_fwd(27 * cin, 12)] * R + [CO.u_fwd(9 * cin, 12)] * R, dtype=F64).reshape(2 * R, 1, 1, 1)
    return args, kw, "out", lambda good: CO.bound_out(good, u)


_EVAL_DEFECTS = ("pair_twin_coef", "pair_ctx_added", "pair_escale0", "mode2_scaled", "ctx_prod_bf16", "append_bstride", "cat_swap", "split_off8")


@pytest.mark.parametrize("defect,starred", [("tap_drop", True), ("fill0", False), ("cross_sequence", False), ("coef_neighbour", True),
                                            ("coff_swap", False), ("ragged_cout", True)] + [(k, False) for k in _EVAL_DEFECTS])
def test_forward_defects_stand_out(defect, starred):
    if defect in _EVAL_DEFECTS:
        args, kw, tensor, bound = _eval_defect_problem(defect)
        good = CO.conv_fwd(*args, **kw)[tensor]
        _defect(defect, CO.conv_fwd(*args, _defect=defect, **kw)[tensor][0], good[0], bound(good), starred)
        return
    cout = 40 if defect == "ragged_cout" else 8
    x, w2, w3, kw = _wide(cout)
    good = CO.conv_fwd(x, x, w2, w3, **kw)["out"]
    bad = CO.conv_fwd(x, x, w2, w3, _defect=defect, **kw)["out"][0]
    _defect(defect, bad, good[0], CO.bound_out(good, CO.u_fwd(27 * 8, 12)), starred)


def test_missing_tap_flip_stands_out():
    gen = _gen(12)
    B, T, H, W, cin, cout = 2, 3, 8, 8, 8, 16
    bf = lambda t: t.to(torch.bfloat16)
    dout, dy3 = bf(torch.randn(B * 2 * T, H, W, cout, generator=gen)), bf(torch.randn(B * T, H, W, cout, generator=gen))
    w2, w3 = bf(torch.randn(cout, cin, 9, generator=gen) / 12), bf(torch.randn(cout, cin, 2, 9, generator=gen) / 12)
    kw = dict(coef_own=torch.rand(B * 2 * T, generator=gen) + 0.3, coef_ctx=torch.rand(B * 2 * T, generator=gen), ctx_bstride=T, ctx_T=T,
              coff=(2, 1), ctx_fill=0.0)
    good = CO.conv_fwd(dout, dy3, CO.pack_wb(w2), CO.pack_wb(w3), B, 2, T, H, W, cout, cin, 9, **kw)["out"]
    bad = CO.conv_fwd(dout, dy3, CO.pack_wb(w2, _no_flip=True), CO.pack_wb(w3, _no_flip=True), B, 2, T, H, W, cout, cin, 9, **kw)["out"][0]
    _defect("no tap flip in the data gradient", bad, good[0], CO.bound_out(good, CO.u_fwd(27 * cout, 12)), False)


def test_weight_gradient_defects_stand_out():
    gen = _gen(13)
    N, H, W, C = 64, 16, 16, 32                                   # 128 position tiles of 8 x 16 pixels
    x = torch.rand(N, H, W, C, generator=gen).to(torch.bfloat16)      # same-sign data: mag = |ref| (module docstring)
    dy = torch.rand(N, H, W, C, generator=gen).to(torch.bfloat16)
    args = (x, dy, None, 1, N, H, W, C, C, 9, N, N, 0, 0.0, 0, 9)
    good = CO.conv_wgrad(*args)
    bound = CO.bound_wgrad(good, CO.wgrad_chain(N * H * W, 128), False)
    _defect("one (co, tap, ci) block without one position tile", CO.conv_wgrad(*args, _defect="tile_missing")[0], good[0], bound, True)
    # a context group written one slab depth off: taps [0, 9) instead of [9, 18)
    B, T = 2, 4
    xs, dy3 = x[:B * 2 * T], dy[:B * T]
    args = (xs, dy3, None, B, T, H, W, C, C, 9, 2 * T, T, -1, 1.0, 9, 18)
    good = CO.conv_wgrad(*args)
    bound = CO.bound_wgrad(good, CO.wgrad_chain(B * T * H * W, 16), False)
    _defect("tap0 off by one slab depth", CO.conv_wgrad(*args, _defect="tap0_off")[0], good[0], bound, False)


# ---------------------------------------------------------------------------------------------------------------------
# exact probes

def _integers_below_256(case, name, pair):
    v, m = pair
    assert bool((v == v.round()).all()) and bool((m == m.round()).all()), (case, name, "not all integers")
    top = float(m.max())
    print(f"CONV-ORACLE probe {case} {name}: mag <= {top:.0f}, {int((v != 0).sum())} of {v.numel()} elements non-zero")
    assert top <= 256, (case, name, top)
    assert int((v != 0).sum()) * 100 >= v.numel(), (case, name, "the probe is all but empty")


@pytest.mark.parametrize("row", CS.FWD + [CS.PAIR_FALLBACK], ids=lambda r: r[0])
def test_forward_probes_are_exact(row):
    d = CS.fwd_inputs(row, True)
    d["clip"] = CS.pick_clip(d, row[9], True)
    for k in ("x", "x2", "w_own", "w_ctx", "res", "coef_own", "coef_ctx", "ctx_prod"):
        if isinstance(d[k], torch.Tensor):
            assert bool((d[k].double() == d[k].double().round()).all()), (row[0], k)
    assert d["ta"] == round(d["ta"]) and d["tb"] == round(d["tb"]) and d["clip"] == round(d["clip"])
    assert all(math.log2(w) == round(math.log2(w)) for w in d["cat_w"]), (row[0], "cat_w")
    if row[0] == "ap_ones":
        assert bool((d["ctx"].reshape(d["B"], d["T"] + 2, -1)[:, :2] == 1).all())
    r = CS.fwd_reference(d)
    for name in ("v", "out", "ctx_out", "ctx_prod"):
        if name in r:
            _integers_below_256(row[0], name, r[name])
    if row[9] == "mpsum_hit":
        assert r["clip_hit"]
    elif row[9] == "mpsum_far":
        assert not r["clip_hit"]


@pytest.mark.parametrize("row", CS.WGRAD, ids=lambda r: r[0])
def test_wgrad_probes_are_exact(row):
    for g in CS.wgrad_groups(row, True):
        _integers_below_256(row[0], "dw_" + g["key"], CS.wgrad_reference(g))

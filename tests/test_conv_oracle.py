"""Review of tests/conv_oracle.py (the float64 restatements test_conv_stages_gpu.py holds the conv kernels to)  --  CPU only.

  pinned         every restatement against float64 torch.nn.functional.conv2d + autograd assembled independently (the context
                 concatenation of test_ops_gpu._gated_conv_train_case, oracle.oniris_oracle.mp_sum / mp_silu): forward, data gradient
                 through the flipped and transposed `wb` packing, weight gradient; 1e-12 relative
  not too tight  the same formulas with bf16 operands, fp32 accumulation and one bf16 store fit every bound
  not too loose  deliberate defects injected into the restatement exceed the bound on at least one element -- while the starred ones
                 change the tensor's relative L2 norm by less than the 5e-3 the aggregate tests (test_ops_gpu.py) allow
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


_TIGHT_FWD = [r for r in CS.FWD if r[0] in ("st_8x8", "st_2x2", "st_8x8_dgrad", "st_1x1_36", "g16_64_64", "g8_32_64", "s_alias", "few_2", "ev_8x8", "st_1x1_nt3")]


@pytest.mark.parametrize("row", _TIGHT_FWD, ids=lambda r: r[0])
def test_forward_bounds_are_not_too_tight(row):
    name, mode, B, T, H, W, Cin, Cout, taps, epi = row[:10]
    d = CS.fwd_inputs(row, False)
    d["clip"] = CS.pick_clip(d, epi, False)
    kw = {k: d[k] for k in ("B", "S", "T", "H", "W", "Cin", "Cout", "taps", "coef_own", "coef_ctx", "ctx_bstride", "ctx_T", "coff",
                            "ctx_fill", "epi", "res", "escale", "ta", "tb", "clip")}
    ctx = d["x"] if isinstance(d["ctx"], str) else d["ctx"]
    lo = CO.conv_fwd(d["x"], ctx, d["w_own"], d["w_ctx"], dtype=torch.float32, **kw)
    out = lo["out"][0].to(torch.bfloat16)
    r = CS.fwd_reference(d, out_bf16=out)
    u = CO.u_fwd(taps * Cin * CS._ctx_phases(mode), 12)
    _usage(f"{name} out", out, r["out"][0], CO.bound_out(r["out"], u))
    if "ctx_out" in r:
        _usage(f"{name} ctx_out", lo["ctx_out"][0].to(torch.bfloat16), r["ctx_out"][0], CO.bound_out(r["ctx_out"], u))
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


@pytest.mark.parametrize("defect,starred", [("tap_drop", True), ("fill0", False), ("cross_sequence", False), ("coef_neighbour", True),
                                            ("coff_swap", False), ("ragged_cout", True)])
def test_forward_defects_stand_out(defect, starred):
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


@pytest.mark.parametrize("row", CS.FWD, ids=lambda r: r[0])
def test_forward_probes_are_exact(row):
    d = CS.fwd_inputs(row, True)
    d["clip"] = CS.pick_clip(d, row[9], True)
    for k in ("x", "w_own", "w_ctx", "res", "coef_own", "coef_ctx"):
        if isinstance(d[k], torch.Tensor):
            assert bool((d[k].double() == d[k].double().round()).all()), (row[0], k)
    assert d["ta"] == round(d["ta"]) and d["tb"] == round(d["tb"]) and d["clip"] == round(d["clip"])
    r = CS.fwd_reference(d)
    for name in ("v", "out", "ctx_out"):
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

"""The reference's own numerical criterion -- std(diff) <= 3e-4 on unit-scale activations, edm2/consistency_test.py:32 -- at the
level of single HIP ops, against a "bf16-faithful" evaluation of the fp32 oracle: the oracle formula on EXACTLY the operands the
kernel multiplies (activations rounded to bf16, the packed weights read back from the device) with the result rounded to bf16
where the kernel stores bf16.  What is left is the summation order of the fp32 accumulators, the fast sigmoid / exp2, and an
occasional flip of the final rounding -- i.e. this checks the ARITHMETIC of each kernel two orders of magnitude below the 1e-2
the fp32-vs-bf16 comparisons of test_ops_gpu.py can state.  (SURVEY 8c names the criterion for "an fp32 verification mode"; the
kernels have no fp32 storage mode -- every activation between kernels is bf16 by design -- so the criterion is applied where it
is meaningful for bf16 kernels: with the operand rounding taken out of the comparison.)
The flash kernels also round P to bf16 in front of the P V product; the attention test states both figures: against the exact
softmax (2.5e-3, all of it that rounding) and with the rounding replayed (the criterion holds)."""
import math
import pytest
import torch

from oracle import oniris_oracle as O
from test_ops_gpu import DEV, nhwc, nchw, bfr, make_bank

pytestmark = pytest.mark.gpu
TIGHT = 3e-4                # consistency_test.py:32
F = torch.nn.functional


def sd(got, ref):
    """std(diff) in units of the reference's own standard deviation (the reference's tests run on unit-variance tensors)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return ((got - ref).std() / ref.std()).item()


def packed_weight(pw, cout, cin, kshape):
    """The bf16 weight the kernels multiply with, (cout, cin, *kshape) fp32, from the packed [tap][CoutP][CinP] image."""
    taps = pw.taps
    wf = pw.wf.float().cpu().reshape(taps, pw.CoutP, pw.CinP)[:, :cout, :cin]
    return wf.permute(1, 2, 0).reshape(cout, cin, *kshape).contiguous()


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("N,H,cin,cout,k", [(6, 16, 64, 64, 3), (4, 32, 32, 96, 3), (8, 8, 256, 128, 3), (9, 32, 128, 136, 1), (6, 32, 32, 96, 1)])
def test_conv_plain_bf16_faithful(N, H, cin, cout, k):
    _conv_plain_bf16_faithful_case(N, H, H, cin, cout, k)


def _conv_plain_bf16_faithful_case(N, H, W, cin, cout, k):
    """Body of test_conv_plain_bf16_faithful on an H x W image; returns (got, ref) for element-wise checks (tests/test_nonsquare_gpu.py)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(3)
    p = torch.nn.Parameter(torch.randn(cout, cin, k, k).to(DEV))
    bank, (pw,) = make_bank([p])
    bank.prepare(training=False)
    w = packed_weight(pw, cout, cin, (k, k))
    x0 = bfr(torch.randn(N, cin, H, W))
    with torch.no_grad():
        y = ops.conv(nhwc(x0), pw)
    ref = bfr(F.conv2d(x0.double(), w.double(), padding=k // 2).float())
    e = sd(nchw(y)[:, :cout], ref)
    print("conv_plain bf16-faithful", (N, H, cin, cout, k) if H == W else (N, H, W, cin, cout, k), e)
    assert e <= TIGHT
    return nchw(y)[:, :cout], ref


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("B,T,H,cin,cout,epi", [(2, 4, 16, 64, 64, "none"), (1, 6, 32, 32, 32, "mpsum"), (2, 3, 8, 128, 128, "silu"),
                                                (1, 4, 16, 256, 128, "mpsum"), (1, 5, 32, 96, 32, "none"),
                                                # several tiles per persistent workgroup (1024 tiles on 256 CUs) / the streaming kernel
                                                # over whole 16-frame segments
                                                (6, 16, 16, 128, 128, "mpsum"), (2, 16, 64, 32, 32, "silu"),
                                                # Counter-Strike net shapes (cs_train.py:35-45: 512 channels on 8x8 and 4x4 images)
                                                (2, 4, 4, 512, 512, "silu"), (1, 3, 8, 512, 512, "mpsum"), (1, 4, 4, 1024, 512, "none")])
def test_gated_conv_train_forward_bf16_faithful(B, T, H, cin, cout, epi):
    """DART training layout (edm2/conv.py:59-95): own 3x3 product + the two context taps over the CLEAN frames t-2, t-1 (padding
    frames of ones, :68), gated sum in fp32, fused epilogue -- every output the launch writes."""
    _gated_forward_bf16_faithful_case(B, T, H, H, cin, cout, epi)


def _gated_forward_bf16_faithful_case(B, T, H, W, cin, cout, epi):
    """Body of test_gated_conv_train_forward_bf16_faithful on an H x W image; returns (got, ref)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(4 + cin)
    p2 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)); p3 = torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=False)
    w2, w3 = packed_weight(pw2, cout, cin, (3, 3)).double(), packed_weight(pw3, cout, cin, (2, 3, 3)).double()
    N = B * 2 * T
    x0 = bfr(torch.randn(N, cin, H, W))
    ca, cb = torch.rand(N) * 0.5 + 0.5, torch.rand(N) * 0.5
    kw = {}
    if epi == "silu":
        cs = torch.rand(N, cout) + 0.5
        kw = dict(cscale=cs.to(DEV))
    elif epi == "mpsum":
        r0 = bfr(torch.randn(N, cout, H, W))
        kw = dict(res=nhwc(r0), ta=0.7, tb=0.5, clip=2.5)
    with torch.no_grad():
        y = ops.gated_conv_train(nhwc(x0), None, pw2, pw3, B, T, coefs=(ca.to(DEV), cb.to(DEV)), **kw)
    xs = x0.double().reshape(B, 2, T, cin, H, W)
    clean = torch.cat([torch.ones(B, 2, cin, H, W, dtype=torch.float64), xs[:, 0]], dim=1)              # frames -2, -1, 0 .. T-1
    y3 = (F.conv2d(clean[:, 0:T].reshape(B * T, cin, H, W), w3[:, :, 0], padding=1) +
          F.conv2d(clean[:, 1:T + 1].reshape(B * T, cin, H, W), w3[:, :, 1], padding=1)).reshape(B, 1, T, cout, H, W)
    y2 = F.conv2d(x0.double(), w2, padding=1).reshape(B, 2, T, cout, H, W)
    v = (ca.double().reshape(B, 2, T, 1, 1, 1) * y2 + cb.double().reshape(B, 2, T, 1, 1, 1) * y3).reshape(N, cout, H, W).float()
    if epi == "silu":
        z = bfr(v) * cs[:, :, None, None]                                  # (the activation sees the bf16-rounded conv output)
        ref = bfr(z * torch.sigmoid(z) / 0.596)
    elif epi == "mpsum":
        ref = bfr((0.7 * r0 + 0.5 * v).clamp(-2.5, 2.5))
    else:
        ref = bfr(v)
    e = sd(nchw(y)[:, :cout], ref)
    print("gated_conv_train bf16-faithful", (B, T, H, cin, cout, epi) if H == W else (B, T, H, W, cin, cout, epi), e)
    assert e <= TIGHT
    return nchw(y)[:, :cout], ref


@pytest.mark.parametrize("B,H,cin,cout", [(2, 16, 128, 128), (1, 8, 256, 256), (3, 32, 64, 64), (1, 64, 32, 32)])
def test_gated_conv_one_frame_bf16_faithful(B, H, cin, cout):
    """The sampler's cached evaluation (edm2/conv.py:69,84-86) through the weight-streaming kernel, with the kept context product."""
    _one_frame_bf16_faithful_case(B, H, H, cin, cout)


def _one_frame_bf16_faithful_case(B, H, W, cin, cout):
    """Body of test_gated_conv_one_frame_bf16_faithful on an H x W image; returns (got, ref)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(5 + cin)
    p2 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)); p3 = torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=False)
    w2, w3 = packed_weight(pw2, cout, cin, (3, 3)).double(), packed_weight(pw3, cout, cin, (2, 3, 3)).double()
    x0, c0 = bfr(torch.randn(B, cin, H, W)), bfr(torch.randn(B, 2, cin, H, W))
    g = torch.rand(B) * 0.6 + 0.05
    pad = c0.permute(0, 1, 3, 4, 2).to(DEV, torch.bfloat16).contiguous()
    y3k = ops.gated_conv_ctx_product(pad, pw2, pw3, B)
    ca, cb = ops.gate_coefs(g)
    y = ops.gated_conv_eval(nhwc(x0), None, pw2, pw3, B, 1, pad, coefs=(ca.to(DEV), cb.to(DEV)), ctx_T=2, ctx_prod=y3k, ctx_prod_mode=2)
    y3 = F.conv2d(c0[:, 0].double(), w3[:, :, 0], padding=1) + F.conv2d(c0[:, 1].double(), w3[:, :, 1], padding=1)
    e3 = sd(y3k.permute(0, 3, 1, 2)[:, :cout], y3)
    ref = bfr((ca.double().reshape(B, 1, 1, 1) * F.conv2d(x0.double(), w2, padding=1) + cb.double().reshape(B, 1, 1, 1) * y3).float())
    e = sd(nchw(y)[:, :cout], ref)
    print("one-frame gated conv bf16-faithful", (B, H, cin, cout) if H == W else (B, H, W, cin, cout), "context product (fp32 store)", e3, "output", e)
    assert e3 <= 2e-6 and e <= TIGHT
    return nchw(y)[:, :cout], ref


@pytest.mark.parametrize("kind,B,T,H,m", [("video", 2, 4, 8, 2), ("video", 1, 8, 16, 1), ("frame", 6, 1, 16, 2), ("video", 1, 16, 8, 4)])
def test_attention_core_bf16_faithful(kind, B, T, H, m):
    """The flash kernels on prepared q, k, v (what the qkv kernels hand them: unit-RMS vectors, q carrying 1/8 log2 e): dense
    masked softmax(q k) v in fp64 on the same bf16 values.  The kernels round P to bf16 in front of the P V product (relative
    to no row maximum at all): against the exact softmax that rounding is the whole difference; with it replayed the reference's
    criterion holds."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(6)
    P = H * H
    frames = 2 * T if kind == "video" else 1
    N, C = B * frames, 64 * m
    unit = lambda: O.normalize(torch.randn(N, P, m, 64), dim=-1)
    q0, k0, v0 = bfr(unit() * (0.125 * 1.4426950408889634)), bfr(unit()), bfr(unit())
    dev = lambda z: z.reshape(N, P, C).to(DEV, torch.bfloat16).contiguous()
    out, *_ = ops._attn_core_fwd(dev(q0), dev(k0), dev(v0), kind, B, T, m, P)
    seq = lambda z: z.double().reshape(B if kind == "video" else N, frames * P, m, 64).permute(0, 2, 1, 3)   # (b, m, L, 64)
    q, k, v = seq(q0), seq(k0), seq(v0)
    s = q @ k.transpose(-1, -2) * math.log(2.0)                                       # the kernel's exponent is base 2
    if kind == "video":
        s = s.masked_fill(~torch.from_numpy(O.train_allowed_tokens(T, P)), float("-inf"))
    ref = bfr((torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(N, P, C).float())
    e = sd(out, ref)
    # replayed: the kernels exponentiate without a row maximum (unit vectors: |score| <= 11.6 in the log2 domain) and round
    # P = 2^s to bf16 for the P V product; the persistent training kernel forms the row sum from the ROUNDED values on the matrix
    # pipe (csrc/attention_ws.h: the header and `pv` of attn_fwd_ws_kernel), the grid kernel from the fp32 ones (`softmax` of attn_fwd_kernel)
    p32 = torch.exp2((q.float() @ k.float().transpose(-1, -2)).masked_fill(torch.isinf(s), float("-inf")))
    pr = bfr(p32).double()
    den = pr.sum(-1, keepdim=True) if kind == "video" else p32.double().sum(-1, keepdim=True)
    ref_p = bfr(((pr @ v) / den).permute(0, 2, 1, 3).reshape(N, P, C).float())
    ep = sd(out, ref_p)
    print("attention core bf16-faithful", (kind, B, T, H, m), "exact softmax", e, "bf16 P replayed", ep)
    assert e <= 4e-3            # measured 2.3e-3 ... 2.6e-3: bf16 P (8 mantissa bits, 2^-9 relative each); the fp32-oracle tests allow 1e-2
    assert ep <= TIGHT


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("N,H,C", [(6, 16, 64), (3, 32, 32), (10, 8, 256)])
def test_act_bf16_faithful(N, H, C):
    """Pixel norm + mp_silu (networks_edm2.py:70-77 with utils.py normalize / mp_silu): both outputs of the fused pass."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(7)
    x0 = bfr(torch.randn(N, C, H, H) * 1.7)
    with torch.no_grad():
        xn, a = ops.act(nhwc(x0), norm=True)
    r = O.normalize(x0.double(), dim=1).float()
    rn = bfr(r)
    ra = bfr(bfr(r) * torch.sigmoid(bfr(r)) / 0.596)
    e = (sd(nchw(xn), rn), sd(nchw(a), ra))
    print("act bf16-faithful (pixel norm, silu)", (N, H, C), e)
    assert e[0] <= TIGHT and e[1] <= 2 * TIGHT        # (silu of the ROUNDED norm or of the fp32 one: whichever the kernel does, within a flip)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("B,T,H,cin,cout", [(2, 4, 16, 64, 64), (1, 6, 32, 32, 32), (2, 3, 8, 128, 256), (1, 5, 16, 128, 64),
                                            (2, 4, 4, 512, 512), (1, 3, 8, 512, 512)])
def test_gated_conv_train_backward_bf16_faithful(B, T, H, cin, cout):
    """Data gradient and gate-coefficient gradients of the gated conv (autograd of edm2/conv.py:74-95), replayed on what the
    backward kernels read: the bf16 incoming gradient, the bf16 raw output and context product the forward stored, and the
    bf16 context gradient dy3 = cb0 g[clean] + cb1 g[noised] the pre-pass writes (oniris_gconv_bwd_prep).  The weight gradient
    is not replayed here (its split-K slabs are rounded to bf16 one by one: test_gated_conv_train states its bound)."""
    _gated_backward_bf16_faithful_case(B, T, H, H, cin, cout)


def _gated_backward_bf16_faithful_case(B, T, H, W, cin, cout):
    """Body of test_gated_conv_train_backward_bf16_faithful on an H x W image; returns (dx, dx_ref)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(8 + cin)
    p2 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)); p3 = torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=True)
    w2, w3 = packed_weight(pw2, cout, cin, (3, 3)).double(), packed_weight(pw3, cout, cin, (2, 3, 3)).double()
    N = B * 2 * T
    x0, g0 = bfr(torch.randn(N, cin, H, W)), bfr(torch.randn(N, cout, H, W))
    ca0, cb0 = torch.rand(N) * 0.5 + 0.5, torch.rand(N) * 0.5
    x = nhwc(x0).requires_grad_(True)
    ca, cb = ca0.to(DEV).requires_grad_(True), cb0.to(DEV).requires_grad_(True)
    y = ops.gated_conv_train(x, None, pw2, pw3, B, T, coefs=(ca, cb))
    y.backward(nhwc(g0))
    # forward quantities as stored
    xs = x0.double().reshape(B, 2, T, cin, H, W)
    clean = torch.cat([torch.ones(B, 2, cin, H, W, dtype=torch.float64), xs[:, 0]], dim=1)
    y3 = (F.conv2d(clean[:, 0:T].reshape(B * T, cin, H, W), w3[:, :, 0], padding=1) +
          F.conv2d(clean[:, 1:T + 1].reshape(B * T, cin, H, W), w3[:, :, 1], padding=1)).reshape(B, 1, T, cout, H, W)
    y2 = F.conv2d(x0.double(), w2, padding=1).reshape(B, 2, T, cout, H, W)
    cav, cbv = ca0.double().reshape(B, 2, T, 1, 1, 1), cb0.double().reshape(B, 2, T, 1, 1, 1)
    raw_s, y3_s = bfr((cav * y2 + cbv * y3).float()).double(), bfr(y3.float()).double()       # what the forward wrote (bf16)
    g = g0.double().reshape(B, 2, T, cout, H, W)
    # gate-coefficient gradients: d ca = <g, y2>, d cb = <g, y3> with y2 recovered from the stored pair
    dca_ref = (g * ((raw_s - cbv * y3_s) / cav)).sum(dim=(3, 4, 5)).reshape(N)
    dcb_ref = (g * y3_s).sum(dim=(3, 4, 5)).reshape(N)
    # context gradient as stored (bf16), then the data gradient
    # (B, T, cout, H, W); in the kernel's own fp32 order -- acc = fma(cb[clean], g[clean], 0), acc = fma(cb[noised], g[noised], acc)
    # (gconv_bwd_prep_kernel, csrc/weights.hip) -- so that the rounding to bf16 sees the same fp32 value, element by element
    cbd, gd = cb0.double().reshape(B, 2, T, 1, 1, 1), g0.double().reshape(B, 2, T, cout, H, W)
    dy3 = bfr((cbd[:, 1] * gd[:, 1] + (cbd[:, 0] * gd[:, 0]).float().double()).float()).double()
    own = F.conv_transpose2d((cav * g).reshape(N, cout, H, W), w2, padding=1).reshape(B, 2, T, cin, H, W)
    dpad = torch.cat([dy3, torch.zeros(B, 2, cout, H, W, dtype=torch.float64)], dim=1)                      # frames T, T+1: nothing
    dctx = (F.conv_transpose2d(dpad[:, 2:T + 2].reshape(B * T, cout, H, W), w3[:, :, 0], padding=1) +
            F.conv_transpose2d(dpad[:, 1:T + 1].reshape(B * T, cout, H, W), w3[:, :, 1], padding=1)).reshape(B, T, cin, H, W)
    own[:, 0] += dctx
    dx_ref = bfr(own.reshape(N, cin, H, W).float())
    e = (sd(nchw(x.grad), dx_ref), sd(ca.grad, dca_ref), sd(cb.grad, dcb_ref))
    print("gated_conv_train backward bf16-faithful", (B, T, H, cin, cout) if H == W else (B, T, H, W, cin, cout), "dx, dca, dcb", e)
    assert max(e) <= TIGHT
    return nchw(x.grad), dx_ref


@pytest.mark.parametrize("kind,B,T,H,m", [("video", 2, 4, 8, 2), ("video", 1, 8, 16, 1), ("frame", 6, 1, 16, 2), ("video", 1, 16, 8, 4)])
def test_attention_core_backward_bf16_faithful(kind, B, T, H, m):
    """dQ, dK, dV of the flash backward (persistent dQ and dK/dV kernels for the training table, grid kernels per frame) replayed on
    their own operands: P = 2^(s - lse) from the forward's stored row constants, delta = <dO, O> from the forward's bf16 output,
    P and dS rounded to bf16 in front of their products (`dsoft` of attn_bwd_dq_kernel and attn_bwd_dkv_kernel), the 1/8 of the score scale where
    each kernel applies it."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(9)
    P = H * H
    frames = 2 * T if kind == "video" else 1
    N, C = B * frames, 64 * m
    c = 0.125 * 1.4426950408889634
    unit = lambda: O.normalize(torch.randn(N, P, m, 64), dim=-1)
    q0, k0, v0, g0 = bfr(unit() * c), bfr(unit()), bfr(unit()), bfr(torch.randn(N, P, m, 64))
    dev = lambda z: z.reshape(N, P, C).to(DEV, torch.bfloat16).contiguous()
    qd, kd, vd, gd = dev(q0), dev(k0), dev(v0), dev(g0)
    out, lse, tabs, meta = ops._attn_core_fwd(qd, kd, vd, kind, B, T, m, P)
    dq, dk, dv = ops._attn_core_bwd(qd, kd, vd, out, lse, gd, tabs, meta)
    Bq = B if kind == "video" else N
    seq = lambda z: z.double().reshape(Bq, frames * P, m, 64).permute(0, 2, 1, 3)               # (b, m, L, 64)
    q, k, v, g, o = seq(q0), seq(k0), seq(v0), seq(g0), seq(out.float().cpu().reshape(N, P, m, 64))
    s = (q.float() @ k.float().transpose(-1, -2)).double()
    p = torch.exp2(s - lse.double().cpu().unsqueeze(-1))
    if kind == "video":
        p = p.masked_fill(~torch.from_numpy(O.train_allowed_tokens(T, P)), 0.0)
    delta = (g * o).sum(-1, keepdim=True)
    ds = p * (g @ v.transpose(-1, -2) - delta)
    r = lambda z: bfr(z.float()).double()
    back = lambda z: bfr(z.permute(0, 2, 1, 3).reshape(N, P, C).float())
    dv_ref = back(r(p).transpose(-1, -2) @ g)
    dq_ref = back((r(ds) @ k) * 0.125)
    dk_ref = back((r(ds * 0.125).transpose(-1, -2) @ q) / c)
    e = (sd(dq, dq_ref), sd(dk, dk_ref), sd(dv, dv_ref))
    print("attention backward bf16-faithful", (kind, B, T, H, m), "dq, dk, dv", e)
    assert max(e) <= TIGHT


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("B,T,H,cin,cout,epi", [(2, 4, 16, 64, 64, "silu"), (1, 6, 32, 32, 32, "silu"), (2, 3, 8, 128, 128, "mpsum"),
                                                (1, 5, 16, 128, 64, "mpsum_clipped"), (1, 6, 32, 32, 32, "mpsum_clipped"), (1, 6, 32, 32, 32, "mpsum")])
def test_gated_conv_train_backward_epilogues_bf16_faithful(B, T, H, cin, cout, epi):
    """The backward of the two fused epilogues (oniris_gconv_bwd_fused modes 1 and 2 + dgrad): emb-scale + mp_silu
    (networks_edm2.py:78-79) and mp_sum + clip (:87-93), the latter with the clip never reached (aliasing protocol: no dout is
    written, dgrad reads g with tb * ca) and reached (g masked in place).  Replayed on the stored bf16 tensors: raw conv output,
    context product, clipped output; dout and dy3 rounded to bf16 where the pre-pass stores them."""
    _gated_backward_epilogues_bf16_faithful_case(B, T, H, H, cin, cout, epi)


def _gated_backward_epilogues_bf16_faithful_case(B, T, H, W, cin, cout, epi):
    """Body of test_gated_conv_train_backward_epilogues_bf16_faithful on an H x W image; returns (dx, dx_ref)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(10 + cin + len(epi))
    p2 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)); p3 = torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=True)
    w2, w3 = packed_weight(pw2, cout, cin, (3, 3)).double(), packed_weight(pw3, cout, cin, (2, 3, 3)).double()
    N = B * 2 * T
    x0, g0 = bfr(torch.randn(N, cin, H, W)), bfr(torch.randn(N, cout, H, W))
    ca0, cb0 = torch.rand(N) * 0.5 + 0.5, torch.rand(N) * 0.5
    x = nhwc(x0).requires_grad_(True)
    ca, cb = ca0.to(DEV).requires_grad_(True), cb0.to(DEV).requires_grad_(True)
    ta, tb, clip = 0.7, 0.5, (1.0 if epi == "mpsum_clipped" else 30.0)
    if epi == "silu":
        cs0 = torch.rand(N, cout) + 0.5
        cs = cs0.to(DEV).requires_grad_(True)
        y = ops.gated_conv_train(x, None, pw2, pw3, B, T, coefs=(ca, cb), cscale=cs)
    else:
        r0 = bfr(torch.randn(N, cout, H, W))
        res = nhwc(r0).requires_grad_(True)
        y = ops.gated_conv_train(x, None, pw2, pw3, B, T, coefs=(ca, cb), res=res, ta=ta, tb=tb, clip=clip, grad_private=True)
    y.backward(nhwc(g0).clone())
    # forward quantities as stored
    xs = x0.double().reshape(B, 2, T, cin, H, W)
    clean = torch.cat([torch.ones(B, 2, cin, H, W, dtype=torch.float64), xs[:, 0]], dim=1)
    y3 = (F.conv2d(clean[:, 0:T].reshape(B * T, cin, H, W), w3[:, :, 0], padding=1) +
          F.conv2d(clean[:, 1:T + 1].reshape(B * T, cin, H, W), w3[:, :, 1], padding=1)).reshape(B, 1, T, cout, H, W)
    y2 = F.conv2d(x0.double(), w2, padding=1).reshape(B, 2, T, cout, H, W)
    cav, cbv = ca0.double().reshape(B, 2, T, 1, 1, 1), cb0.double().reshape(B, 2, T, 1, 1, 1)
    v = cav * y2 + cbv * y3
    raw_s, y3_s = bfr(v.float()).double(), bfr(y3.float()).double()
    g = g0.double().reshape(B, 2, T, cout, H, W)
    extra = {}
    if epi == "silu":
        c6 = cs0.double().reshape(B, 2, T, cout, 1, 1)
        z = raw_s * c6
        sig = torch.sigmoid(z)
        dz = g * sig * (1 + z * (1 - sig)) / 0.596
        extra["dcs"] = (sd(cs.grad, (dz * raw_s).sum(dim=(4, 5)).reshape(N, cout)))
        dv = bfr((dz * c6).float()).double()         # dout is stored in bf16, and the ROUNDED value is what the sums below see
    else:
        out_s = bfr((ta * r0.double().reshape(v.shape) + tb * v).clamp(-clip, clip).float()).double()
        mask = (out_s.abs() < clip).double()
        assert (mask.mean().item() < 0.98) == (epi == "mpsum_clipped")
        dv = tb * g * mask
        extra["dres"] = sd(nchw(res.grad), bfr((ta * g * mask).reshape(N, cout, H, W).float()))
    dca_ref = (dv * ((raw_s - cbv * y3_s) / cav)).sum(dim=(3, 4, 5)).reshape(N)
    dcb_ref = (dv * y3_s).sum(dim=(3, 4, 5)).reshape(N)
    # (B, T, cout, H, W), in the kernel's own fp32 order (gconv_bwd_fused_kernel, csrc/weights.hip): dr = fp32(dv), acc = fma(cb[clean],
    # dr[clean], 0), acc = fma(cb[noised], dr[noised], acc) -- so that the rounding to bf16 sees the same fp32 value, element by element
    dr = dv.float().double()
    dy3 = bfr((cbv[:, 1] * dr[:, 1] + (cbv[:, 0] * dr[:, 0]).float().double()).float()).double()
    if epi == "silu" or epi == "mpsum_clipped":
        # dout is a stored bf16 tensor (silu: written by the pre-pass; clipped: g masked in place, scaled by the coefficient)
        dsrc = dv if epi == "silu" else g * mask * tb
    else:
        dsrc = g * tb                                                                                         # read as g with tb * ca
    own = F.conv_transpose2d((cav * dsrc).reshape(N, cout, H, W), w2, padding=1).reshape(B, 2, T, cin, H, W)
    dpad = torch.cat([dy3, torch.zeros(B, 2, cout, H, W, dtype=torch.float64)], dim=1)
    own[:, 0] += (F.conv_transpose2d(dpad[:, 2:T + 2].reshape(B * T, cout, H, W), w3[:, :, 0], padding=1) +
                  F.conv_transpose2d(dpad[:, 1:T + 1].reshape(B * T, cout, H, W), w3[:, :, 1], padding=1)).reshape(B, T, cin, H, W)
    dx_ref = bfr(own.reshape(N, cin, H, W).float())
    e = dict(dx=sd(nchw(x.grad), dx_ref), dca=sd(ca.grad, dca_ref), dcb=sd(cb.grad, dcb_ref), **extra)
    print("gated_conv_train backward epilogue bf16-faithful", (B, T, H, cin, cout, epi) if H == W else (B, T, H, W, cin, cout, epi), e)
    assert max(e.values()) <= TIGHT
    return nchw(x.grad), dx_ref


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("form,N,H,C,Cs", [("enc", 6, 16, 64, 0), ("enc", 3, 32, 32, 0), ("dec", 4, 16, 64, 32), ("dec", 2, 32, 32, 64)])
def test_act_backward_bf16_faithful(form, N, H, C, Cs):
    """Backward of the fused activation pass: pixel norm + mp_silu (encoder blocks, networks_edm2.py:70-77) and mp_cat + mp_silu
    (decoder blocks, :72-77 with utils.py mp_cat): fp64 autograd of the formulas on the bf16 inputs, result rounded to bf16."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(11 + C)
    x0 = bfr(torch.randn(N, C, H, H) * 1.3)
    x = nhwc(x0).requires_grad_(True)
    xr = x0.double().requires_grad_(True)
    if form == "enc":
        o1, o2 = ops.act(x, norm=True)
        r1 = O.normalize(xr, dim=1)
        rq = r1 + (bfr(r1.detach().float()).double() - r1.detach())       # the activation sees the STORED (bf16) first output
        r2 = rq * torch.sigmoid(rq) / 0.596
        ins, rins = [x], [xr]
    else:
        s0 = bfr(torch.randn(N, Cs, H, H))
        sk = nhwc(s0).requires_grad_(True)
        sr = s0.double().requires_grad_(True)
        t = 0.5
        cc = math.sqrt((C + Cs) / ((1 - t) ** 2 + t ** 2))
        w1, w2 = cc / math.sqrt(C) * (1 - t), cc / math.sqrt(Cs) * t                      # utils.py mp_cat
        o1, o2 = ops.act(x, sk, w1, w2, want_xo=True)
        r1 = torch.cat([w1 * xr, w2 * sr], dim=1)
        rq = r1 + (bfr(r1.detach().float()).double() - r1.detach())
        r2 = rq * torch.sigmoid(rq) / 0.596
        ins, rins = [x, sk], [xr, sr]
    g1, g2 = bfr(torch.randn(*r1.shape)), bfr(torch.randn(*r2.shape))
    got = torch.autograd.grad([o1, o2], ins, [nhwc(g1), nhwc(g2)])
    if form == "enc":
        # the kernel differentiates the norm at the STORED normalised tensor and the saved fp32 denominator (elementwise.hip
        # act_bwd_kernel): dx = (g - xn (g . xn) s / (C (s - eps))) / s with xn = bf16(x / s), s = eps + |x| / sqrt(C)
        xq = rq.detach()
        sg = torch.sigmoid(xq)
        gt = g2.double() * sg * (1 + xq * (1 - sg)) / 0.596 + g1.double()
        sden = 1e-4 + x0.double().norm(dim=1, keepdim=True) / math.sqrt(C)
        ref = [(gt - xq * (gt * xq).sum(dim=1, keepdim=True) * sden / (C * (sden - 1e-4))) / sden]
    else:
        ref = torch.autograd.grad([r1, r2], rins, [g1.double(), g2.double()])
    e = [sd(nchw(a), bfr(b.float())) for a, b in zip(got, ref)]
    fe = (sd(nchw(o1), bfr(r1.detach().float())), sd(nchw(o2), bfr(r2.detach().float())))
    print("act backward bf16-faithful", (form, N, H, C, Cs), "forward outputs", fe, "input gradients", e)
    assert max(fe) <= TIGHT and max(e) <= TIGHT


def _ternary(shape, density, gen):
    """Sparse tensor of -1 / 0 / +1: every product and every partial sum of a weight gradient built from two of them is a small
    integer, exactly representable in the bf16 split-K slabs and in the fp32 accumulators -- the kernels must be EXACT."""
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float() * (torch.rand(shape, generator=gen) < density).float()


@pytest.mark.parametrize("B,T,H,cin,cout,dens", [(1, 2, 8, 32, 32, 0.25), (2, 8, 64, 32, 32, 0.05), (2, 4, 16, 128, 128, 0.12),
                                                 (2, 4, 8, 256, 256, 0.2), (1, 6, 32, 64, 64, 0.08), (1, 3, 16, 96, 160, 0.15),
                                                 (2, 16, 64, 32, 32, 0.04), (2, 4, 4, 512, 512, 0.3), (1, 3, 8, 1024, 512, 0.25),
                                                 # more 4x16-pixel tiles than the weights own slabs: the streaming kernel's 8x16-pixel form
                                                 (9, 2, 64, 32, 32, 0.04)])
def test_gated_conv_weight_gradient_integer_exact(B, T, H, cin, cout, dens):
    """Weight gradient of the gated conv -- own 3x3 weight over both slots, the two context taps over the clean frames, split-K
    slabs in bf16, slab reduction + normalisation backward in weight_bwd -- on sparse ternary activations and gradients with
    power-of-two gate coefficients: every slab entry is a small integer, so any lost, doubled or misplaced position, a wrong
    coefficient or a slab rounding shows up at full size.  Compared with fp64 autograd through the reference's forced weight
    normalisation (conv.py:14-21); the bound is fp32 rounding of the normalisation backward alone.  Shapes: the streaming kernel of
    the 32-channel level (several segments), the LDS-DMA kernels for 16x16 and 8x8 tiles, ragged channel counts."""
    _gated_wgrad_integer_exact_case(B, T, H, H, cin, cout, dens)


def _gated_wgrad_integer_exact_case(B, T, H, W, cin, cout, dens, mark=None):
    """Body of test_gated_conv_weight_gradient_integer_exact on an H x W image; mark('fwd') / mark('bwd') after the forward / backward launches."""
    from autoregressive_diffusion_amd import ops
    gen = torch.Generator().manual_seed(12 + cin + H)
    w2, w3 = torch.randn(cout, cin, 3, 3, generator=gen), torch.randn(cout, cin, 2, 3, 3, generator=gen)
    p2, p3 = torch.nn.Parameter(w2.clone().to(DEV)), torch.nn.Parameter(w3.clone().to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=True)
    N = B * 2 * T
    x0, g0 = _ternary((N, cin, H, W), dens, gen), _ternary((N, cout, H, W), dens, gen)
    ca0 = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (N,), generator=gen)]
    cb0 = torch.tensor([1.0, 0.5])[torch.randint(0, 2, (N,), generator=gen)]
    x = nhwc(x0).requires_grad_(True)
    if mark:
        mark("start")
    y = ops.gated_conv_train(x, None, pw2, pw3, B, T, coefs=(ca0.to(DEV), cb0.to(DEV)))
    if mark:
        mark("fwd")
    y.backward(nhwc(g0))
    if mark:
        mark("bwd")
    bank.backward()
    # fp64 reference through the forced normalisation
    r2, r3 = w2.double().requires_grad_(True), w3.double().requires_grad_(True)
    e2, _ = O.weight_effective(r2, 1.0, training=True)
    e3, _ = O.weight_effective(r3, 1.0, training=True)
    xs = x0.double().reshape(B, 2, T, cin, H, W)
    clean = torch.cat([torch.ones(B, 2, cin, H, W, dtype=torch.float64), xs[:, 0]], dim=1)
    y3 = (F.conv2d(clean[:, 0:T].reshape(B * T, cin, H, W), e3[:, :, 0], padding=1) +
          F.conv2d(clean[:, 1:T + 1].reshape(B * T, cin, H, W), e3[:, :, 1], padding=1)).reshape(B, 1, T, cout, H, W)
    y2 = F.conv2d(x0.double(), e2, padding=1).reshape(B, 2, T, cout, H, W)
    v = ca0.double().reshape(B, 2, T, 1, 1, 1) * y2 + cb0.double().reshape(B, 2, T, 1, 1, 1) * y3
    (v * g0.double().reshape(v.shape)).sum().backward()
    rel64 = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    e = (rel64(p2.grad, r2.grad), rel64(p3.grad, r3.grad))
    worst = max(((p2.grad.double().cpu() - r2.grad).abs().max() / r2.grad.abs().max()).item(),
                ((p3.grad.double().cpu() - r3.grad).abs().max() / r3.grad.abs().max()).item())
    print("gated conv weight gradient, integer-exact inputs", (B, T, H, cin, cout) if H == W else (B, T, H, W, cin, cout), "rel L2 dW2, dW3", e, "worst element / max", worst)
    assert max(e) <= 2e-6 and worst <= 1e-5
    return e, worst


@pytest.mark.parametrize("N,H,cin,cout,k,dens", [(16, 32, 128, 256, 1, 0.05), (9, 32, 64, 96, 1, 0.08), (64, 64, 32, 96, 1, 0.03), (12, 16, 64, 64, 3, 0.12),
                                                 (6, 8, 256, 128, 3, 0.2), (32, 64, 32, 32, 3, 0.04), (130, 1, 64, 96, 1, 0.3)])
def test_plain_conv_weight_gradient_integer_exact(N, H, cin, cout, k, dens):
    """The same for MPConv (1x1 through the LDS-DMA GEMM weight-gradient kernel and the small-channel fallback, plain 3x3 of the 2-D
    steps, a linear layer): sparse ternary x and dy, fp64 autograd through the forced normalisation."""
    _plain_wgrad_integer_exact_case(N, H, H, cin, cout, k, dens)


def _plain_wgrad_integer_exact_case(N, H, W, cin, cout, k, dens, mark=None):
    """Body of test_plain_conv_weight_gradient_integer_exact on an H x W image; mark: see _gated_wgrad_integer_exact_case."""
    from autoregressive_diffusion_amd import ops
    gen = torch.Generator().manual_seed(13 + cin + H)
    kk = (k, k) if H > 1 else ()
    w = torch.randn(cout, cin, *kk, generator=gen)
    p = torch.nn.Parameter(w.clone().to(DEV))
    bank, (pw,) = make_bank([p])
    bank.prepare(training=True)
    x0, g0 = _ternary((N, cin, H, W), dens, gen), _ternary((N, cout, H, W), dens, gen)
    x = nhwc(x0).requires_grad_(True)
    if mark:
        mark("start")
    y = ops.conv(x, pw)
    if mark:
        mark("fwd")
    y.backward(nhwc(g0))
    if mark:
        mark("bwd")
    bank.backward()
    r = w.double().requires_grad_(True)
    e_, _ = O.weight_effective(r, 1.0, training=True)
    (F.conv2d(x0.double(), e_.reshape(cout, cin, k, k), padding=k // 2) * g0.double()).sum().backward()
    e = ((p.grad.double().cpu() - r.grad).norm() / r.grad.norm()).item()
    worst = ((p.grad.double().cpu() - r.grad).abs().max() / r.grad.abs().max()).item()
    print("plain conv weight gradient, integer-exact inputs", (N, H, cin, cout, k) if H == W else (N, H, W, cin, cout, k), "rel L2", e, "worst element / max", worst)
    assert e <= 2e-6 and worst <= 1e-5
    return e, worst


@pytest.mark.parametrize("B,P,m,nk,kind", [(1, 64, 4, 10, "decode"), (2, 64, 4, 40, "decode"), (1, 256, 2, 12, "decode"), (2, 64, 2, 6, "prefill"),
                                           # ragged shapes through the four-stream decode kernel: 40 query rows (an 8-row second block),
                                           # 360 keys (a 40-key last tile, streams with unequal tile counts); 16-token frames
                                           (1, 40, 2, 9, "decode"), (3, 16, 1, 20, "decode")])
def test_attention_eval_kernels_bf16_faithful(B, P, m, nk, kind):
    """The sampler's attention launches on prepared q, k, v: one new frame against nk cached frames (dense; from 2048 keys on the key
    tiles are dealt to several workgroups whose un-normalised partials are added: OnirisAttnArgs.kv_splits) and the causal prefill
    over nk frames (infer table, attention_masking.py:56-84).  Replay as for the grid kernel: P = bf16(2^s) without a row maximum in
    front of P V, row sum of the fp32 P."""
    import ctypes
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    torch.manual_seed(14 + nk)
    C = 64 * m
    t = 1 if kind == "decode" else nk
    unit = lambda n: O.normalize(torch.randn(B, n * P, m, 64), dim=-1)
    q0, k0, v0 = bfr(unit(t) * (0.125 * 1.4426950408889634)), bfr(unit(nk)), bfr(unit(nk))
    dev = lambda z: z.reshape(B, -1, C).to(DEV, torch.bfloat16).contiguous()
    qd, kd, vd = dev(q0), dev(k0), dev(v0)
    out = torch.empty((B * t, P, C), dtype=torch.bfloat16, device=DEV)
    Lq, Lk = t * P, nk * P
    tabs = None if kind == "decode" else ops.device_tables("infer", nk, P, DEV)
    a = ops._attn_args(qd, kd, vd, None, None, None, out, None, tabs, B, m, Lq, Lk, C, 0 if kind == "decode" else 1, P, 0)
    if kind == "decode":
        ops._decode_splits(a, B, m, Lq, Lk, DEV)
        assert (a.kv_splits > 1) == (Lk >= ops.DECODE_SPLIT_MIN_KEYS)
    check(lib.oniris_attn_fwd(ctypes.byref(a), ops._stream()), "attn_fwd")
    seq = lambda z: z.double().reshape(B, -1, m, 64).permute(0, 2, 1, 3)
    q, k, v = seq(q0), seq(k0), seq(v0)
    p32 = torch.exp2(q.float() @ k.float().transpose(-1, -2))
    if kind == "prefill":
        p32 = p32.masked_fill(~torch.from_numpy(O.infer_allowed_tokens(nk, P)), 0.0)
    ref = bfr(((bfr(p32).double() @ v) / p32.double().sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B * t, P, C).float())
    e = sd(out, ref)
    print("attention eval kernels bf16-faithful", (B, P, m, nk, kind), "kv_splits", int(a.kv_splits), e)
    assert e <= TIGHT


@pytest.mark.parametrize("B,T,H,m", [(2, 4, 8, 2), (1, 8, 16, 1), (1, 16, 8, 4)])
def test_qkv_norm_rope_bf16_faithful(B, T, H, m):
    """The pass in front of the training attention kernel: split of the qkv conv output, pixel norm per head
    (attention_modules.py:48-49 with utils.normalize), rotary embedding with the fp16-rounded xPos tables (RoPe.py:21-32,43-68,
    positions 0..T-1 for the clean AND the noised half), q scaled by log2(e)/8 for the kernel -- one launch; and its adjoint."""
    import ctypes
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    torch.manual_seed(15 + T)
    P, C, N = H * H, 64 * m, B * 2 * T
    c = 0.125 * 1.4426950408889634
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    sc = (torch.arange(0, 64, 2) + 0.4 * 64) / (1.4 * 64)
    x0 = bfr(torch.randn(N, P, 3, m, 64) * 1.5)                                 # kernel channel order (s m c)
    qkv = x0.reshape(N, P, 3 * C).to(DEV, torch.bfloat16).contiguous()
    q, k, v = (torch.empty((N, P, C), dtype=torch.bfloat16, device=DEV) for _ in range(3))
    cs_, sn_, sc_ = ops.rope_tables(inv.to(DEV), sc.to(DEV), T, DEV)
    check(lib.oniris_qkv_norm_rope(ops._p(qkv), ops._p(q), ops._p(k), ops._p(v), ops._p(cs_), ops._p(sn_), ops._p(sc_), N * P, C, P, T,
                                   ops._stream()), "qkv_norm_rope")
    xr = x0.double().requires_grad_(True)
    y = O.normalize(xr, dim=-1)                                                  # (N, P, 3, m, 64)
    to_seq = lambda z: z.reshape(B, 2 * T, P, m, 64).permute(0, 3, 1, 2, 4)     # (B, m, 2T, P, 64)
    qq, kk = O.rope_apply(to_seq(y[:, :, 0]), to_seq(y[:, :, 1]), inv.double(), sc.double(), True)
    back = lambda z: z.permute(0, 2, 3, 1, 4).reshape(N, P, C)
    rq, rk, rv = back(qq) * c, back(kk), y[:, :, 2].reshape(N, P, C)
    e = (sd(q, bfr(rq.detach().float())), sd(k, bfr(rk.detach().float())), sd(v, bfr(rv.detach().float())))
    # adjoint: bf16 gradients of q (w.r.t. the UNSCALED q: the attention backward hands that over), k, v -> d qkv
    gq, gk, gv = (bfr(torch.randn(N, P, C)) for _ in range(3))
    dqkv = torch.empty_like(qkv)
    gqd, gkd, gvd = (z.to(DEV, torch.bfloat16) for z in (gq, gk, gv))
    check(lib.oniris_qkv_norm_rope_bwd(ops._p(qkv), ops._p(gqd), ops._p(gkd), ops._p(gvd), ops._p(dqkv), ops._p(cs_), ops._p(sn_),
                                       ops._p(sc_), N * P, C, P, T, ops._stream()), "qkv_norm_rope_bwd")
    ((rq / c) * gq.double() + rk * gk.double() + rv * gv.double()).sum().backward()
    eb = sd(dqkv.reshape(N, P, 3, m, 64), bfr(xr.grad.float()))
    print("qkv_norm_rope bf16-faithful", (B, T, H, m), "q, k, v", e, "d qkv", eb)
    assert max(e) <= TIGHT and eb <= TIGHT


@pytest.mark.parametrize("B,T,H,m,d", [(2, 4, 8, 4, 16), (1, 8, 8, 2, 32), (1, 4, 16, 4, 8), (1, 4, 8, 2, 48), (1, 4, 8, 2, 24),
                                       (1, 2, 8, 1, 56), (1, 2, 8, 3, 40)])
def test_qkv_norm_hd_bf16_faithful(B, T, H, m, d):
    """The same pass for heads of 8 / 16 / 32 channels (Block(channels_per_head=), networks_edm2.py:28; the reference's tests use
    16): per-head norm over d channels, rotary embedding with its partner d/2 channels away, q scaled by log2(e)/sqrt(d), heads
    zero-padded to the 64 channels the attention kernels are written for; and the adjoint, which takes dq as the 64-channel
    kernels return it (scaled by 8: the epilogue of attn_bwd_dq_kernel) and the padded dk, dv."""
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    torch.manual_seed(16 + d)
    P, N = H * H, B * 2 * T
    c = 1.4426950408889634 / math.sqrt(d)
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    sc = (torch.arange(0, d, 2) + 0.4 * d) / (1.4 * d)
    x0 = bfr(torch.randn(N, P, 3, m, d) * 1.5)                                  # channel = (s*heads + head)*d + c
    qkv = x0.reshape(N, P, 3 * m * d).to(DEV, torch.bfloat16).contiguous()
    q, k, v = (torch.full((N, P, 64 * m), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(3))
    cs_, sn_, sc_ = ops.rope_tables(inv.to(DEV), sc.to(DEV), T, DEV)
    check(lib.oniris_qkv_norm_hd(ops._p(qkv), ops._p(q), ops._p(k), ops._p(v), ops._p(cs_), ops._p(sn_), ops._p(sc_), N * P, m, d, P, T, 0, 3, T,
                                 ops._stream()), "qkv_norm_hd")
    xr = x0.double().requires_grad_(True)
    y = O.normalize(xr, dim=-1)
    to_seq = lambda z: z.reshape(B, 2 * T, P, m, d).permute(0, 3, 1, 2, 4)
    qq, kk = O.rope_apply(to_seq(y[:, :, 0]), to_seq(y[:, :, 1]), inv.double(), sc.double(), True)
    back = lambda z: z.permute(0, 2, 3, 1, 4).reshape(N, P, m, d)
    rq, rk, rv = back(qq) * c, back(kk), y[:, :, 2]
    heads = lambda z: z.float().cpu().reshape(N, P, m, 64)
    e = [sd(heads(a)[..., :d], bfr(b.detach().float())) for a, b in ((q, rq), (k, rk), (v, rv))]
    pad = max(float(heads(a)[..., d:].abs().max()) for a in (q, k, v))
    gq, gk, gv = (bfr(torch.randn(N, P, m, 64)) for _ in range(3))
    gqd, gkd, gvd = (z.reshape(N, P, 64 * m).to(DEV, torch.bfloat16) for z in (gq, gk, gv))
    dqkv = torch.empty_like(qkv)
    check(lib.oniris_qkv_norm_hd_bwd(ops._p(qkv), ops._p(gqd), ops._p(gkd), ops._p(gvd), ops._p(dqkv), ops._p(cs_), ops._p(sn_), ops._p(sc_),
                                     N * P, m, d, P, T, 0, 3, T, ops._stream()), "qkv_norm_hd_bwd")
    c64 = 0.125 * 1.4426950408889634
    ((rq / c64) * gq[..., :d].double() + rk * gk[..., :d].double() + rv * gv[..., :d].double()).sum().backward()
    eb = sd(dqkv.reshape(N, P, 3, m, d), bfr(xr.grad.float()))
    print("qkv_norm_hd bf16-faithful", (B, T, H, m, d), "q, k, v", e, "padding max", pad, "d qkv", eb)
    assert max(e) <= TIGHT and pad == 0.0 and eb <= TIGHT


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("N,H,cin,cout,k,clip", [(9, 32, 128, 128, 1, 1.0), (6, 16, 256, 256, 1, 0.0), (8, 32, 64, 64, 3, 1.5), (130, 8, 64, 96, 1, 2.0)])
def test_plain_conv_mpsum_bf16_faithful(N, H, cin, cout, k, clip):
    """MPConv with the fused mp_sum (+ clip) epilogue -- the attention projection (attention_modules.py:43,77 + networks_edm2.py
    clip) and conv_res1 of the 2-D steps -- forward, and backward through oniris_mpsum_bwd (both gradients stored in bf16) +
    the data gradient of the ROUNDED dout."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(17 + cin + k)
    p = torch.nn.Parameter(torch.randn(cout, cin, k, k).to(DEV))
    bank, (pw,) = make_bank([p])
    bank.prepare(training=True)
    w = packed_weight(pw, cout, cin, (k, k)).double()
    x0, r0, g0 = bfr(torch.randn(N, cin, H, H)), bfr(torch.randn(N, cout, H, H)), bfr(torch.randn(N, cout, H, H))
    x, res = nhwc(x0).requires_grad_(True), nhwc(r0).requires_grad_(True)
    ta, tb = 0.7 / math.sqrt(0.58), 0.3 / math.sqrt(0.58)
    y = ops.conv(x, pw, res=res, ta=ta, tb=tb, clip=clip)
    y.backward(nhwc(g0))
    v = ta * r0.double() + tb * F.conv2d(x0.double(), w, padding=k // 2)
    out = bfr((v.clamp(-clip, clip) if clip > 0 else v).float())
    mask = (out.double().abs() < clip).double() if clip > 0 else torch.ones_like(v)
    dout = bfr((tb * g0.double() * mask).float()).double()
    e = dict(y=sd(nchw(y)[:, :cout], out), dres=sd(nchw(res.grad), bfr((ta * g0.double() * mask).float())),
             dx=sd(nchw(x.grad), bfr(F.conv_transpose2d(dout, w, padding=k // 2).float())))
    print("plain conv + mp_sum bf16-faithful", (N, H, cin, cout, k, clip), e, "clipped fraction", 1 - mask.mean().item())
    assert max(e.values()) <= TIGHT

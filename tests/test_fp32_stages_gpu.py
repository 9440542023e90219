"""The fp32 verification kernels (csrc/fp32.hip: conv_f32, wgrad_f32, attn_f32_fwd / _dq / _dkv) called directly through
fp32.conv2d / fp32.linear / fp32.attention and held to float64 ELEMENT BY ELEMENT (convs, count probes) or ROW BY ROW (attention on
random inputs), at the shapes the kernels take another path at.  Expectations, probes and bounds: tests/fp32_oracle.py; that they
see the faults they are for: tests/test_fp32_oracle.py.  Every compared figure is printed (profiles/fp32_stage_tests.txt holds a
run); every comparison covers all elements of its tensor.

Bounds (u = 2^-24):
 * conv forward / data gradient: (K + 4) u sum|terms|, K = taps Cin / taps Cout -- any summation order.
 * weight gradient: (K + nz + 4) u sum|terms|, K the element's own number of non-zero terms, nz the number of position chunks whose
   partial sums meet in atomics: any order of the atomics is covered, so nothing here depends on it (two runs are NOT compared bit
   for bit: the order varies).
 * attention count probes: out within 2^-20, dv within 2^-6 (a wrong pair moves them by >= 1 / Lk >= 2^-10 and by 1), dq and dk
   within 2^-6 of the largest |dv|.
 * attention on random inputs: every row within 4 x the worst row of the float32 model of the kernel (model_f32) against float64,
   computed on the CPU.
 * the module check: the margin rule of tests/disc_cpu_restatement.py on the float32 oracle's own error (fp32 mode), 1e-2 (bf16
   path with wide heads, as test_attention_heads_wider_than_64_channels)."""
import math

import pytest
import torch

import disc_cpu_restatement as R
import fp32_oracle as FO
import paramgen
from oracle import oniris_oracle as O

DEV = "cuda"
pytestmark = pytest.mark.gpu


def fp32():
    from autoregressive_diffusion_amd import fp32 as m
    return m


def gen(seed):
    return torch.Generator().manual_seed(seed)


def check_elements(what, got, want, bound):
    """|got - want| <= bound at EVERY element; prints the worst ratio and how many elements were compared."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape), (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"FP32 {what}: worst |err| / bound = {ratio:.3f} (max |err| {float(err.max()):.2e}, {err.numel()} of {err.numel()} elements)")
    assert bool((err <= bound).all()), (what, ratio)


def conv_inputs(N, H, W, Cin, Cout, k, seed):
    g = gen(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    dy = torch.randn(N, Cout, H, W, generator=g)
    return x, w, dy


# ----------------------------------------------------------------------------------------------------------------------
# conv forward, data gradient (and the weight gradient of the same call)

CONV_CASES = [
    # (N, H, W, Cin, Cout): what it reaches
    (3, 5, 7, 5, 7),        # 105 positions: tile 1 holds 41, straddles images 1 / 2 / 3, both upper waves partly dead
    (2, 9, 11, 17, 33),     # one channel past a K chunk of 16, one output row past a wave's 32
    (1, 8, 8, 33, 65),      # a second blockIdx.y block with a single row
    (2, 1, 9, 6, 6),        # all-border images: no row above or below
    (2, 9, 1, 6, 6),        # both x neighbours out
    (3, 4, 2, 6, 6),        # W = 2: one x neighbour out at every pixel
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_forward_and_gradients(case):
    N, H, W, Cin, Cout = case
    tag = "conv3x3 " + "x".join(map(str, case))
    x0, w0, dy0 = conv_inputs(N, H, W, Cin, Cout, 3, 100 + N * H * W + Cin)
    x, w = x0.to(DEV).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    y = fp32().conv2d(x, w)
    y.backward(dy0.to(DEV))
    want, mag = FO.conv_terms(x0.double(), w0.double())
    check_elements(tag + " y", y, want, FO.element_bound(mag, 9 * Cin))
    want, mag = FO.dgrad_terms(dy0.double(), w0.double())
    check_elements(tag + " dx", x.grad, want, FO.element_bound(mag, 9 * Cout))
    want, mag, cnt = FO.wgrad_terms(x0.double(), dy0.double(), 3)
    check_elements(tag + " dw", w.grad, want, FO.element_bound(mag, cnt, extra=FO.wgrad_chunks(N * H * W)))


@pytest.mark.parametrize("N", [65, 1])
def test_linear_forward_and_gradients(N):
    """fp32.linear: the 1x1 kernel over one position per row, 70 -> 130 channels (a tail of one position; three output blocks, the
    last two channels wide; a K tail of 6)."""
    Cin, Cout = 70, 130
    g = gen(200 + N)
    x0, w0, dy0 = torch.randn(N, Cin, generator=g), torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin), torch.randn(N, Cout, generator=g)
    x, w = x0.to(DEV).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    y = fp32().linear(x, w)
    assert y.shape == (N, Cout)
    y.backward(dy0.to(DEV))
    im = lambda t: t.double()[:, :, None, None]
    want, mag = FO.conv_terms(im(x0), im(w0))
    check_elements(f"linear N={N} y", y, want[:, :, 0, 0], FO.element_bound(mag, Cin)[:, :, 0, 0])
    want, mag = FO.dgrad_terms(im(dy0), im(w0))
    check_elements(f"linear N={N} dx", x.grad, want[:, :, 0, 0], FO.element_bound(mag, Cout)[:, :, 0, 0])
    want, mag, cnt = FO.wgrad_terms(im(x0), im(dy0), 1)
    check_elements(f"linear N={N} dw", w.grad, want[:, :, 0, 0], FO.element_bound(mag, cnt, extra=1)[:, :, 0, 0])


# ----------------------------------------------------------------------------------------------------------------------
# weight gradient

WGRAD_CASES = [
    # (N, H, W, Cin, Cout, k, input): what it reaches
    (3, 37, 41, 5, 7, 3, "probes"),      # 4551 positions: the chunk boundary at 4096 inside an image row (row 25 of the third image),
    (3, 37, 41, 5, 7, 3, "dense"),       #   a last chunk of 455 = 28 groups of 16 + 7; blockIdx.z = 1
    (1, 64, 64, 5, 7, 3, "probes"),      # exactly one full chunk
    (2, 6, 6, 65, 70, 1, "dense"),       # 2 x 2 channel blocks, the second ci block one channel wide
    (2, 6, 6, 65, 70, 3, "dense"),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_weight_gradient(case):
    N, H, W, Cin, Cout, k, kind = case
    tag = "wgrad " + "x".join(map(str, case))
    x0, w0, dy0 = conv_inputs(N, H, W, Cin, Cout, k, 300 + N * H * W + Cin + k)
    if kind == "probes":
        x0 = FO.position_probe(N, H, W, Cin, 301)
    w = w0.to(DEV).requires_grad_(True)
    fp32().conv2d(x0.to(DEV), w).backward(dy0.to(DEV))
    want, mag, cnt = FO.wgrad_terms(x0.double(), dy0.double(), k)
    nz = FO.wgrad_chunks(N * H * W)
    npr = len(FO.probe_positions(N, H, W))
    assert int(cnt.max()) <= (npr if kind == "probes" else N * H * W)
    print(f"FP32 {tag}: {nz} chunk(s), terms per element {int(cnt.min())} .. {int(cnt.max())}" + (f", {npr} probe positions" if kind == "probes" else ""))
    check_elements(tag + " dw", w.grad, want, FO.element_bound(mag, cnt, extra=nz))


# ----------------------------------------------------------------------------------------------------------------------
# attention

def run_attention(inp, mask, kw):
    """fp32.attention forward + backward on (BH, L, D) inputs -> dict of out, dq, dk, dv."""
    q, k, v = (z.to(DEV)[None].requires_grad_(True) for z in inp[:3])
    out = fp32().attention(q, k, v, mask, **kw)
    out.backward(inp[3].to(DEV)[None])
    torch.cuda.synchronize()
    return dict(out=out[0], dq=q.grad[0], dk=k.grad[0], dv=v.grad[0])


COUNT_CASES = {cid: (mask, kw, build) for cid, mask, kw, build in FO.count_cases()}


@pytest.mark.parametrize("cid", list(COUNT_CASES))
def test_attention_count_probes(cid):
    """Every element of out, dv, dq and dk of the count probes, BH = 2, D = 64.  train: (P, T) = (1, 256), (4, 64), (16, 16),
    (64, 4), (128, 2) at L = 512 and (256, 2) at L = 1024 -- fpb = 128, 32, 8, 2, 1 and the P >= 128 branch (ops.train_mask_table
    has a table for each of them: none had to be replaced).  causal: 2 frames on 3 cached (Lq 40, Lk 100), 2 on 1 (18, 27), 3 on 0
    (150, 150).  dense: Lq 13, Lk 70.  The masks come from the package's definitions (fp32_oracle.train_allowed / causal_allowed)."""
    mask, kw, build = COUNT_CASES[cid]
    allowed = build()
    inp = FO.count_probe(FO.COUNT_BH, FO.COUNT_D, allowed)
    ref = FO.reference(*inp, allowed)
    got = run_attention(inp, mask, kw)
    top = float(ref["dv"].abs().max())
    for name, tol in (("out", FO.COUNT_OUT_TOL), ("dv", FO.COUNT_DV_TOL), ("dq", FO.COUNT_DV_TOL * top), ("dk", FO.COUNT_DV_TOL * top)):
        check_elements(f"attn count {cid} {name}", got[name], ref[name], torch.full_like(ref[name], tol))


def check_rows(tag, got, ref, bounds):
    for name in FO.NAMES:
        assert bool(torch.isfinite(got[name]).all()), (tag, name)
        m = FO.row_error(got[name], ref[name])
        worst = float(m.max())
        print(f"FP32 {tag} {name}: worst row / bound = {worst / bounds[name]:.3f} (row metric {worst:.2e}, bound {bounds[name]:.2e}, "
              f"{m.numel()} of {m.numel()} rows)")
    for name in FO.NAMES:
        m = FO.row_error(got[name], ref[name])
        assert bool((m <= bounds[name]).all()), (tag, name, float(m.max()), bounds[name])


RANDOM_CASES = [(D, 3, "causal", dict(P=20, q_frame_off=3)) for D in (3, 8, 65, 72, 200, 256)] + [(256, 1, "train", dict(P=64, T=4))]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: f"D{c[0]}-{c[2]}")
def test_attention_random_inputs(case):
    """Head widths 3, 8, 65, 72, 200, 256 (not a multiple of 8, of 64 lanes; the advertised maximum) at BH = 3 under the causal mask
    of 2 frames on 3 cached ones; width 256 under the training mask at L = 512: the largest LDS request (148 480 bytes in the dK /
    dV kernel)."""
    D, BH, mask, kw = case
    allowed = FO.causal_allowed(2, 3, 20) if mask == "causal" else FO.train_allowed(kw["T"], kw["P"])
    inp = FO.random_inputs(BH, *allowed.shape, D, seed=400 + D)
    ref = FO.reference(*inp, allowed)
    bounds = FO.random_bounds(ref, FO.model_f32(*inp, allowed))
    check_rows(f"attn random D={D} {mask} BH={BH}", run_attention(inp, mask, kw), ref, bounds)


# ----------------------------------------------------------------------------------------------------------------------
# the offset branch through the module

def rel(a, b):
    return R.rel(a.detach(), b.detach())


@pytest.mark.parametrize("C,mode", [(128, "fp32"), (256, "bf16")], ids=["d64-fp32-mode", "d128-product-path"])
def test_video_attention_appended_frames(C, mode):
    """VideoAttention(C, 2) in evaluation, B = 2, 8 x 8 tokens: prefill 3 frames, append 2 in ONE call (causal, q_frame_off = 3, two
    query frames), then 1.  By causality every frame's output equals that of a single prefill of all 6 frames, which the oracle
    (oracle.video_attention) evaluates in float64 -- equals up to the fp16 rounding of the xPos scale tables, which are built for the
    key count of each call (3, 5, 6 frames against 6): the ratio of two table entries depends on the frame distance alone only
    before that rounding, which is why the calls with fewer keys sit at 1.4e-5 and the last one at 5e-8 in fp32 mode."""
    from edm2.attention import VideoAttention
    m, B, H, t = 2, 2, 8, 6
    d = C // m
    g = gen(C + m)
    p = {"a.attn_qkv.weight.weight": torch.randn(3 * C, C, 1, 1, generator=g), "a.attn_proj.weight.weight": torch.randn(C, C, 1, 1, generator=g),
         "a.rope.inv_freq": 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d)), "a.rope.scale": (torch.arange(0, d, 2) + 0.4 * d) / (1.4 * d)}
    p = paramgen.prenormalise(p)
    x0 = torch.randn(B * t, C, H, H, generator=g)
    p64 = {k: (v if "rope" in k else v.double()) for k, v in p.items()}          # (the fp16 rope tables are part of the definition)
    want, _ = O.video_attention(p64, "a.", x0.double(), B, m, None, False, False, False)
    own, _ = O.video_attention(p, "a.", x0, B, m, None, False, False, False)
    assert want.dtype == torch.float64
    want, own = want.reshape(B, t, C, H, H), own.reshape(B, t, C, H, H)
    att = VideoAttention(C, m)
    att.load_state_dict({k[2:]: v.clone() for k, v in p.items()}, strict=True)
    att = att.to(DEV).eval()
    xs = x0.reshape(B, t, C, H, H).to(DEV)
    call = lambda a, b, c, upd=True: att(xs[:, a:b].reshape(-1, C, H, H), B, c, update_cache=upd)
    import contextlib
    with torch.no_grad(), (fp32().fp32_arithmetic() if mode == "fp32" else contextlib.nullcontext()):
        y3, c = call(0, 3, None)
        y5, c = call(3, 5, c)
        y6, _ = call(5, 6, c, False)
    for name, y, a, b in (("prefill 0-2", y3, 0, 3), ("appended 3-4", y5, 3, 5), ("appended 5", y6, 5, 6)):
        e = rel(y.reshape(B, b - a, C, H, H).float().cpu(), want[:, a:b])
        own_rel = rel(own[:, a:b], want[:, a:b])
        bound = R.margin(own_rel) if mode == "fp32" else 1e-2
        print(f"FP32 module d={d} {mode} {name}: rel L2 {e:.2e} (bound {bound:.2e}; the float32 oracle's own {own_rel:.2e})")
        assert e <= bound, (name, e, bound)

"""Discriminator2D timing at the gym VAE training shape (gym_vae_train.py:87-119: B = 4 clips of 32 frames of 256x256 = 128 frames,
Discriminator2D(3, (64, 64, 64))): appends a text report to the path given after the mode (e.g. profiles/discriminator.txt).

  python scratch/disc_bench.py native REPORT   the native module: forward alone, forward + backward with all gradients, forward +
                                               backward with the input gradient only (parameters frozen); HIP events, medians of 5;
                                               the FLOPs of its conv / wgrad launches and the bytes its launches read and write
                                               (counted per launch from the operand sizes, not from hardware counters); the largest
                                               conv launch alone against the 157.3 TFLOP/s fp32 roofline
  python scratch/disc_bench.py eager REPORT    the torch restatement of the same net (tests/disc_cpu_restatement.py) eager in fp32
                                               on the same GPU, warmed up once: the same three figures

Run each mode as its own process under its own `timeout -k 10`, with OMP_NUM_THREADS=16."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

import disc_paramgen as G  # noqa: E402

DEV = "cuda"
mode = sys.argv[1]
out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
N, H, W, CIN, WIDTHS = (int(os.environ.get("DISC_BENCH_FRAMES", 128)), 256, 256, 3, (64, 64, 64))
torch.set_num_threads(16)


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


runs = [""]                                     # the last ms() call's range, for the report


def ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    runs[0] = f"({reps} runs {min(ts):.2f} .. {max(ts):.2f})"
    return statistics.median(ts)


params = G.fill(G.disc2d_shapes(CIN, WIDTHS), 7)
x = torch.randn(N, CIN, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)

if mode == "native":
    from autoregressive_diffusion_amd import discriminator as d
    net = d.Discriminator2D(CIN, WIDTHS)
    net.load_state_dict(params, strict=True)
    net = net.to(DEV).train()
    count = dict(flops=0.0, bytes=0.0, on=False)
    nbytes = lambda *ts: sum(4.0 * t.numel() for t in ts if t is not None)

    def wrap(name, flops_of):
        fn = getattr(d, name)

        def w(*a, **k):
            r = fn(*a, **k)
            if count["on"]:
                count["flops"] += flops_of(*a, **k)
                outs = r if isinstance(r, tuple) else (r,)
                count["bytes"] += nbytes(*[t for t in a if torch.is_tensor(t)], *[t for t in k.values() if torch.is_tensor(t)], *outs)
            return r
        setattr(d, name, w)
    wrap("conv", lambda x_, wp, b, Cout, taps, **k: 2.0 * x_.numel() * taps * Cout)
    wrap("wgrad", lambda x_, dy, taps, **k: 2.0 * x_.numel() * taps * dy.shape[-1])
    for name in ("blur", "blur_bwd", "bn_bwd", "finalize"):
        wrap(name, lambda *a, **k: 0.0)

    def fwd():
        with torch.no_grad():
            net(x)

    def step(xin):
        net.zero_grad(set_to_none=True)
        xin.grad = None
        net(xin).square().mean().backward()

    xg = x.clone().requires_grad_(True)
    say(f"device: {torch.cuda.get_device_name(0)}; Discriminator2D({CIN}, {WIDTHS}) native, {N} frames of {H}x{W}, fp32")
    count["on"] = True
    fwd()
    count["on"] = False
    ff, fb = count["flops"], count["bytes"]
    t_f = ms(fwd)
    alg = nbytes(x) + 4.0 * N * 2 * (H // 4) * (W // 4) + 4.0 * sum(v.numel() for v in params.values())
    say(f"forward: median {t_f:.2f} ms {runs[0]}; conv launches {ff / 1e12:.3f} TFLOP -> {ff / t_f / 1e9:.1f} TFLOP/s over the whole pass = "
        f"{100 * ff / t_f / 1e9 / 157.3:.1f} % of 157.3 (the guide's untuned LDS-tiled GEMM on this instruction: 122)")
    say(f"forward: launches read + write {fb / 1e9:.2f} GB (counted from operand sizes) -> {fb / t_f / 1e6:.0f} GB/s; the input, the "
        f"logits and the parameters alone are {alg / 1e9:.3f} GB")
    count.update(flops=0.0, bytes=0.0, on=True)
    step(xg)
    count["on"] = False
    fa = count["flops"]
    t_a = ms(lambda: step(xg))
    say(f"forward + backward, all gradients: median {t_a:.2f} ms {runs[0]}; conv + wgrad launches {fa / 1e12:.3f} TFLOP -> {fa / t_a / 1e9:.1f} TFLOP/s")
    net.requires_grad_(False)
    count.update(flops=0.0, bytes=0.0, on=True)
    step(xg)
    count["on"] = False
    fi = count["flops"]
    t_i = ms(lambda: step(xg))
    say(f"forward + backward, input gradient only (parameters frozen): median {t_i:.2f} ms {runs[0]}; conv launches {fi / 1e12:.3f} TFLOP -> "
        f"{fi / t_i / 1e9:.1f} TFLOP/s")
    # the largest conv launch alone: blocks.0.conv1, 64 -> 64 at full resolution with the prologue and the statistics epilogue
    a = torch.randn(N, H, W, 64, device=DEV)
    wp = d.pack_weight(net.blocks[0].conv1.weight)
    s, t = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV)
    fl = 2.0 * a.numel() * 9 * 64
    t_c = ms(lambda: d.conv(a, wp, None, 64, 9, pro=(s, t), stats=True))
    say(f"blocks.0.conv1 alone (3x3, 64 -> 64, prologue, statistics): {t_c:.2f} ms, {fl / t_c / 1e9:.1f} TFLOP/s = "
        f"{100 * fl / t_c / 1e9 / 157.3:.1f} % of 157.3; reads + writes {2 * nbytes(a) / 1e9:.2f} GB -> {2 * nbytes(a) / t_c / 1e6:.0f} GB/s")
    dy = torch.randn(N, H, W, 64, device=DEV)
    t_w = ms(lambda: d.wgrad(a, dy, 9, pro=(s, t)), reps=3)
    say(f"blocks.0.conv1 weight gradient alone: {t_w:.2f} ms, {fl / t_w / 1e9:.1f} TFLOP/s = {100 * fl / t_w / 1e9 / 157.3:.1f} % of 157.3")
else:
    import disc_cpu_restatement as R
    p = {k: v.to(DEV).requires_grad_(v.is_floating_point() and k.rsplit(".", 1)[1] in ("weight", "bias")) for k, v in params.items()}

    def fwd():
        with torch.no_grad():
            R.disc2d(p, x, len(WIDTHS), True)

    def step(xin):
        for v in p.values():
            v.grad = None
        xin.grad = None
        R.disc2d(p, xin, len(WIDTHS), True)[0].square().mean().backward()

    xg = x.clone().requires_grad_(True)
    say(f"eager baseline: the torch restatement of the same net, fp32, same GPU, {N} frames of {H}x{W}")
    say(f"forward: {ms(fwd, 3):.1f} ms")
    say(f"forward + backward, all gradients: {ms(lambda: step(xg), 3):.1f} ms")
    for v in p.values():
        v.requires_grad_(False)
    say(f"forward + backward, input gradient only: {ms(lambda: step(xg), 3):.1f} ms")
if out:
    out.close()

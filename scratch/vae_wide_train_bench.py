"""Wide VAE training timing ([3,16,64,256,8] with three ResBlocks, time compressions [1,2,2,1], spatial [1,2,2,2], B = 1, 256x256
frames): prints a text report, and also appends it to the path given as argv[1] (e.g. profiles/vae_wide_training.txt).

  (a) forward + backward of VAE.forward with wide_training() on (csrc/vae_wide_train.hip) against the training restatement
      (tests/vae_train_cpu_restatement.py) in eager fp32 PyTorch with autograd on the same GPU in the same process, both warmed
      up, medians of alternating runs, at the largest T of 32, 16, 8 at which both fit, and the rel L2 between the two gradients
      of the 256-wide conv A;
  (b) the backward launches of the 256-wide ResBlock (encoder block 2: g = 2, T / 4 frames of 64x64) alone: kernel time (events
      around back-to-back launches) and FLOP/s against the 157.3 TFLOP/s fp32 matrix roofline, and the 1x1 stages around it;
  (c) where the native step's time goes: the ten kernels with the largest total time under torch's profiler.
Run every GPU step under its own `timeout -k 10`."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import _lib, vae as V, vae_train  # noqa: E402
from autoregressive_diffusion_amd.vae import VAE  # noqa: E402
import vae_train_cpu_restatement as RT  # noqa: E402
from vae_wide_oracle import seed_params  # noqa: E402

DEV = "cuda"
ROOF = 157.3
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
out = open(paths[0], "a") if paths else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_launch_us(fn, n=5):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e3)
    return statistics.median(ts)


KW = dict(channels=[3, 16, 64, 256, 8], n_res_blocks=3, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2])
vae = seed_params(VAE(**KW), 7).to(DEV).train().wide_training()
say(f"device: {torch.cuda.get_device_name(0)}; VAE {KW['channels']}, n_res_blocks {KW['n_res_blocks']}, wide_training() on")
B, H, W = 1, 256, 256
s, p = V._stream(), V._p


def operands(T):
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, T, H, W, generator=g) * 2 - 1).to(DEV)
    ts = (torch.rand(B, generator=g) * 0.1).to(DEV)
    noise = torch.randn(B, 8, T // 4, H // 8, W // 8, generator=g).to(DEV)
    return x, ts, noise


def loss_of(x, r_mean, r_logvar):
    return 0.5 * (r_logvar + (x - r_mean) ** 2 / torch.exp(r_logvar)).mean()


def native(x, ts, noise):
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, _, _ = vae(x, t_sample=ts, noise=noise)
    loss_of(x, r_mean, r_logvar).backward()


def eager(x, ts, noise):
    vae.zero_grad(set_to_none=True)
    sd = dict(vae.named_parameters())
    sd.update(dict(vae.named_buffers()))
    r_mean, r_logvar, _ = RT.forward(sd, vae.kwargs, x, ts, noise)
    loss_of(x, r_mean, r_logvar).backward()


# (b) the backward launches of the 256-wide ResBlock and the 1x1 stages around it, at T = 16 frames
C, g, T4, h = 256, 2, 4, 64
rb = vae.encoder.encoder_blocks[2].res_blocks[0]
wda, wdb, zb = vae_train._pack_dgrad_wide(rb.conv3d0.conv3d.weight, rb.conv3d1.weight, C, g)
S, D = torch.randn(B, g + T4, h, h, C, device=DEV), torch.randn(B, T4 + g, h, h, C, device=DEV)
a, du, dout, dx = (torch.randn(B, T4, h, h, C, device=DEV) for _ in range(4))
emb = 0.1 * torch.randn(B, 2 * C, device=DEV)
part = torch.empty(-(-T4 * h * h // 256), B, 2 * C, device=DEV)
pix = B * T4 * h * h
fa, fb = 2.0 * pix * C * C * 2 * g * 9, 2.0 * pix * C * C * 9


def line(name, us, flops=None, bytes_=None):
    tail = f", {flops / us / 1e6:.1f} TFLOP/s = {100 * flops / us / 1e6 / ROOF:.1f} % of the {ROOF} TFLOP/s fp32 matrix roofline" if flops else ""
    tail += f", {bytes_ / us / 1e3:.0f} GB/s" if bytes_ else ""
    say(f"    {name}: {us:.0f} us per launch{tail}")


say(f"(b) backward launches of the 256-wide ResBlock (C = 256, g = 2, B = {B}, T = {T4}, {h}x{h}):")
line("conv B dgrad (oniris_vae_wide_conv_b_bwd)", per_launch_us(lambda: _lib.check(_lib.lib.oniris_vae_wide_conv_b_bwd(
    p(dout), p(wdb), p(du), B, T4, h, h, C, s), "conv_b_bwd")), fb)
line("act adjoint, plain (oniris_vae_wide_act_bwd)", per_launch_us(lambda: vae_train._wide_act_bwd(a, None, du, None, D, None)),
     bytes_=3.0 * 4 * pix * C)
line("conv A dgrad (oniris_vae_wide_conv_a on D)", per_launch_us(lambda: V.wide_conv_a(D, dict(wa=wda, ba=zb), g, s)), fa)
line("act adjoint, FiLM with partials (oniris_vae_wide_act_bwd)", per_launch_us(lambda: vae_train._wide_act_bwd(a, emb, du, dout, dx, part)),
     bytes_=4.0 * 4 * pix * C)
line("conv A wgrad + slab sum (oniris_vae_wide_conv3_wgrad_bwd)", per_launch_us(lambda: vae_train._wide_conv3_dw(S, D, B, T4, h, h, C, g, True)), fa)
line("conv B wgrad + slab sum (oniris_vae_wide_conv3_wgrad_bwd)", per_launch_us(lambda: vae_train._wide_conv3_dw(a, dout, B, T4, h, h, C, 1, False)), fb)
line("S again (oniris_vae_wide_act)", per_launch_us(lambda: V.wide_act(a, s, p(emb), None, g)), bytes_=2.0 * 4 * pix * C)
# down 64 -> 256 (tc = sc = 2, K = 512) and down 256 -> 8 (sc = 2, K = 1024): the 1x1 stages at the wide block's two ends
x64 = torch.randn(B, 2 * T4, 2 * h, 2 * h, 64, device=DEV)
dy256 = torch.randn(B, T4, h, h, 256, device=DEV)
w = vae.encoder.encoder_blocks[2].compression_block.weight
pack = vae_train._pack_down_dgrad(w, 64, 256, 2, 2)
fl = 2.0 * pix * 512 * 256
line("down 64 -> 256 dgrad (oniris_vae_wide_down_bwd)", per_launch_us(lambda: vae_train._wide_down_dx(dy256, pack, (B, T4, h, h), 256, 64, 2, 2)), fl)
line("down 64 -> 256 wgrad + slab sum (oniris_vae_wide_lin_wgrad_bwd)",
     per_launch_us(lambda: vae_train._wide_lin_dw(x64, (64, 2, 2), dy256, (256, 1, 1), (B, T4, h, h))), fl)
del S, D, a, du, dout, dx, x64, dy256

# (a) the training step at the largest T that fits
for T in (32, 16, 8):
    try:
        ops_ = operands(T)
        native(*ops_)
        key = "encoder.encoder_blocks.2.res_blocks.0.conv3d0.conv3d.weight"
        gn = dict(vae.named_parameters())[key].grad.clone()
        eager(*ops_)
        ge = dict(vae.named_parameters())[key].grad.clone()
    except torch.OutOfMemoryError:
        say(f"(a) T = {T}: out of memory")
        del ops_
        torch.cuda.empty_cache()
        continue
    tn, te = [], []
    for _ in range(3):
        tn.append(timed(lambda: native(*ops_)))
        te.append(timed(lambda: eager(*ops_)))
    mn, me = statistics.median(tn), statistics.median(te)
    say(f"(a) forward + backward, B = {B}, {T} frames {H}x{W}: native median {1e3 * mn:.1f} ms, training restatement (eager fp32 "
        f"PyTorch, autograd, same GPU) median {1e3 * me:.1f} ms; eager / native = {me / mn:.2f}x (3 alternating runs each; native "
        f"{[round(1e3 * v, 1) for v in tn]}, eager {[round(1e3 * v, 1) for v in te]}); rel L2 of d {key}: "
        f"{((gn - ge).norm() / ge.norm()).item():.2e}")
    break

# (c) the native step by kernel: torch's profiler around one step, the ten kernels with the largest total time
from torch.profiler import ProfilerActivity, profile  # noqa: E402
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    native(*ops_)
    torch.cuda.synchronize()
rows = sorted((e for e in prof.key_averages() if e.device_time_total > 0), key=lambda e: -e.device_time_total)
total = sum(e.device_time_total for e in rows)
say(f"(c) kernels of one native step by total time ({total / 1e3:.1f} ms on the device):")
for e in rows[:10]:
    say(f"    {e.key.split('(')[0][:70]:70s} x{e.count:<4d} {e.device_time_total / 1e3:8.2f} ms  {100 * e.device_time_total / total:5.1f} %")
if out:
    out.close()

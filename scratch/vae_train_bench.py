"""VAE training timing (gym VAE, channels [3, 8, 8, 8], the training script's shape: B = 4, 32 frames of 256x256,
gym_vae_train.py:26-27): prints a text report, and also appends it to the path given as argv[1] (e.g. profiles/vae_training.txt).

  (a) forward + backward of VAE.forward on the HIP path (csrc/vae_train.hip) against the training restatement
      (tests/vae_train_cpu_restatement.py) in eager fp32 PyTorch with autograd on the same GPU, both warmed up, medians of
      alternating runs, and the rel L2 between the two gradients of the widest tensor;
  (b) the data-gradient and the weight-gradient launch of res A at the last decoder block (8 channels, g = 4, 256x256, B = 4,
      T = 32) alone: kernel time (events around back-to-back launches) and FLOP/s against the 157.3 TFLOP/s fp32 roofline;
  (w) the worst per-tensor deviations of the HIP path from fixture G16 (the reference's float64 gradients).

`--native-only N` runs N native steps and nothing else (for rocprofv3 --kernel-trace --stats -- python scratch/vae_train_bench.py
--native-only 3).  Run every GPU step under its own `timeout -k 10`.  (c), the headline regression check, is bench.py itself:
bench.py --gpus 1 --steps 8 --warmup 4 --dump-outputs on this tree and on the parent commit's tree, on the same box."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import _lib, vae_train  # noqa: E402
from autoregressive_diffusion_amd.vae import VAE  # noqa: E402
import vae_train_cpu_restatement as RT  # noqa: E402

DEV = "cuda"
native_only = int(sys.argv[sys.argv.index("--native-only") + 1]) if "--native-only" in sys.argv else 0
paths = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()]
out = open(paths[0], "a") if paths else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def per_launch_us(fn, n=10):
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


vae = VAE.from_pretrained(os.path.join(ROOT, "tests", "golden", "g14_vae_gym.pt")).to(DEV).train()
g = torch.Generator().manual_seed(0)
B, T, H, W = 4, 32, 256, 256
x = (torch.rand(B, 3, T, H, W, generator=g) * 2 - 1).to(DEV)
ts = (torch.rand(B, generator=g) * 0.1).to(DEV)
noise = torch.randn(B, 8, T // 4, H // 4, W // 4, generator=g).to(DEV)


def loss_of(r_mean, r_logvar):
    return 0.5 * (r_logvar + (x - r_mean) ** 2 / torch.exp(r_logvar)).mean()


def native():
    vae.zero_grad(set_to_none=True)
    r_mean, r_logvar, _, _ = vae(x, t_sample=ts, noise=noise)
    loss_of(r_mean, r_logvar).backward()


def eager():
    vae.zero_grad(set_to_none=True)
    sd = dict(vae.named_parameters())
    sd.update(dict(vae.named_buffers()))
    r_mean, r_logvar, _ = RT.forward(sd, vae.kwargs, x, ts, noise)
    loss_of(r_mean, r_logvar).backward()


if native_only:
    for _ in range(native_only):
        native()
    torch.cuda.synchronize()
    sys.exit(0)

say(f"device: {torch.cuda.get_device_name(0)}; gym VAE {vae.kwargs['channels']}, n_res_blocks {vae.kwargs['n_res_blocks']}")

# (w) the worst deviations from fixture G16
from test_vae_train import g16  # noqa: E402
from test_vae import rel  # noqa: E402
z, ref_grads, ref32, xg, sdg, kwg = g16()
v16 = VAE(**kwg)
v16.load_state_dict(sdg, strict=True)
v16 = v16.to(DEV).train()
r_mean, r_logvar, mean, _ = v16(xg.to(DEV), t_sample=torch.from_numpy(z["t_sample"]).to(DEV), noise=torch.from_numpy(z["noise"]).to(DEV))
RT.loss(r_mean, r_logvar, mean).backward()
errs = {n: rel(p.grad.cpu(), ref_grads[n]) for n, p in v16.named_parameters()}
say("(w) HIP path vs fixture G16 (rel L2): " + ", ".join(f"{k} {rel(v.detach().cpu(), z[k]):.2e}" for k, v in
                                                        (("mean", mean), ("r_mean", r_mean), ("r_logvar", r_logvar))))
say("    worst parameter gradients (bound 5e-5; the reference's own float32 run in brackets): " +
    "; ".join(f"{k} {errs[k]:.2e} [{ref32[k]:.1e}]" for k in sorted(errs, key=errs.get, reverse=True)[:6]))
del v16, r_mean, r_logvar, mean

# (b) the dgrad and wgrad launches of res A at the last decoder block
C, gsz = 8, 4
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bk = vae._pack(torch.device(DEV))["blocks"][-1]
rb = vae.decoder.encoder_blocks[-1].res_blocks[0]
wda, wdb = vae_train._pack_dgrad(rb.conv3d0.conv3d.weight, rb.conv3d1.weight, C, gsz)
xa = torch.randn(B, T, H, W, C, device=DEV)
da = torch.randn(B, T, H, W, C, device=DEV)
dout = torch.randn(B, T, H, W, C, device=DEV)
dx = torch.empty_like(xa)
emb = 0.1 * torch.randn(B, 2 * C, device=DEV)
tiles = (H // 16) * (W // 16)
part = torch.empty(tiles * (T // bk["gpt"]), B, 2 * C, device=DEV)
flops = 2.0 * B * T * H * W * C * C * 2 * gsz * 9
us = per_launch_us(lambda: _lib.check(_lib.lib.oniris_vae_res_a_bwd(da.data_ptr(), xa.data_ptr(), emb.data_ptr(), dout.data_ptr(),
                                                                     wda.data_ptr(), B, T, H, W, C, gsz, bk["nch"], bk["gpt"],
                                                                     dx.data_ptr(), part.data_ptr(), s), "res_a_bwd"))
say(f"(b) res A dgrad, last decoder block (C = 8, g = 4, B = {B}, T = {T}, {H}x{W}): {us:.0f} us per launch, "
    f"{flops / us / 1e6:.1f} TFLOP/s = {100 * flops / us / 1e6 / 157.3:.1f} % of the 157.3 TFLOP/s fp32 roofline")
n = 2 * gsz * gsz * 9 * C * C + gsz * C
nslab = vae_train._nslab(B * (T // gsz) * tiles, n)
slab = torch.zeros(nslab, n, device=DEV)
us = per_launch_us(lambda: _lib.check(_lib.lib.oniris_vae_conv3_wgrad_bwd(xa.data_ptr(), emb.data_ptr(), da.data_ptr(), B, T, H, W, C,
                                                                           gsz, 1, slab.data_ptr(), nslab, s), "wgrad"), n=5)
say(f"    res A wgrad, the same block ({nslab} slabs of {n} floats): {us:.0f} us per launch, {flops / us / 1e6:.1f} TFLOP/s = "
    f"{100 * flops / us / 1e6 / 157.3:.1f} % of the fp32 roofline")
del xa, da, dout, dx, part, slab

# (a) the training step
native()
key = "decoder.encoder_blocks.2.res_blocks.1.conv3d0.conv3d.weight"
gn = dict(vae.named_parameters())[key].grad.clone()
eager()
ge = dict(vae.named_parameters())[key].grad.clone()
tn, te = [], []
for _ in range(3):
    tn.append(timed(native)[0])
    te.append(timed(eager)[0])
mn, me = statistics.median(tn), statistics.median(te)
say(f"(a) forward + backward, B = {B}, {T} frames {H}x{W}: native median {1e3 * mn:.1f} ms, training restatement (eager fp32 PyTorch, "
    f"autograd, same GPU) median {1e3 * me:.1f} ms; eager / native = {me / mn:.2f}x (3 alternating runs each; native "
    f"{[round(1e3 * v, 1) for v in tn]}, eager {[round(1e3 * v, 1) for v in te]}); rel L2 of d {key}: {((gn - ge).norm() / ge.norm()).item():.2e}")
if out:
    out.close()

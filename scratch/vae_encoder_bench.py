"""VAE encoder timing (gym VAE, channels [3, 8, 8, 8], 256x256 frames, B = 1): prints a text report, and also writes it to the
path given as argv[1] (e.g. profiles/vae_encoder.txt).

  (b) streaming latency per latent frame: encode_frames of 4 uint8 frames through the cache, wall time from the call to the
      latents being complete (synchronised), median over 40 calls;
  (c) the down kernel of the first downsampling block (8 -> 8 channels, tc = sc = 2, 256x256 -> 128x128) alone: kernel time
      (events around 50 back-to-back launches) and achieved bytes/s (input read once + output written once) against the
      achievable HBM rate (about 6.3 TB/s measured, 8 TB/s spec); the first block's down (uint8 in, 3 -> 8 channels) beside it;
  (a) whole-sequence frames_to_latents of 1056 uint8 frames (264 latent frames): the native encoder (csrc/vae_encoder.hip,
      csrc/vae.hip) against the reference's formulation in eager fp32 PyTorch (tests/vae_encoder_cpu_restatement.py run on the
      GPU), both warmed up, medians of alternating runs.
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import _lib  # noqa: E402
from autoregressive_diffusion_amd.vae import VAE  # noqa: E402
import vae_encoder_cpu_restatement as RE  # noqa: E402

DEV = "cuda"
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


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


def per_launch_us(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 50 * 1e3)
    return statistics.median(ts)


vae = VAE.from_pretrained(os.path.join(ROOT, "tests", "golden", "g14_vae_gym.pt")).to(DEV)
sd = {k: v for k, v in vae.state_dict().items()}
g = torch.Generator().manual_seed(0)
say(f"device: {torch.cuda.get_device_name(0)}; gym VAE {vae.kwargs['channels']}, n_res_blocks {vae.kwargs['n_res_blocks']}")

# (b) streaming, 4 RGB frames (one latent frame) per call
frames = torch.randint(0, 256, (1, 4 * 48, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV)
cache, per = None, []
for i in range(48):
    dt, (lat, cache) = timed(lambda: vae.encode_frames(frames[:, 4 * i:4 * i + 4], cache=cache))
    if i >= 8:
        per.append(dt)
say(f"(b) streaming encode_frames, 4 uint8 frames 256x256 (1 latent frame) per call, B = 1: median {1e3 * statistics.median(per):.3f} ms, "
    f"min {1e3 * min(per):.3f}, max {1e3 * max(per):.3f} over {len(per)} calls (wall, call to synchronised latents)")
del frames, cache, lat

# (c) the down kernels alone
pk = vae._pack_encoder(torch.device(DEV))
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
T = 64                                                     # 64 frames in: 134 MB read, 34 MB written
bk = pk["blocks"][1]
x = torch.randn(1, T, 256, 256, 8, device=DEV)
y = torch.empty(1, T // 2, 128, 128, 8, device=DEV)


def down1():
    _lib.check(_lib.lib.oniris_vae_down(x.data_ptr(), 0, *x.stride()[:4], 1, 1, T // 2, 128, 128, 8, 2, 2, 0, bk["wd"].data_ptr(),
                                        bk["bd"].data_ptr(), 8, y.data_ptr(), s), "down")


us = per_launch_us(down1)
nbytes = 4 * (x.numel() + y.numel())
say(f"(c) down, first downsampling block (8 -> 8 channels, K = 64, tc = sc = 2, {T} frames 256x256 -> {T // 2} x 128x128): {us:.1f} us per "
    f"launch (median of 5 x 50 back-to-back); {nbytes / 1e6:.1f} MB read + written -> {nbytes / us / 1e6:.2f} TB/s = "
    f"{100 * nbytes / us / 1e6 / 6.3:.0f} % of the 6.3 TB/s achievable HBM rate ({100 * nbytes / us / 1e6 / 8:.0f} % of the 8 TB/s spec)")
bk0 = pk["blocks"][0]
f8 = torch.randint(0, 256, (1, T, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV)
y0 = torch.empty(1, T, 256, 256, 8, device=DEV)


def down0():
    _lib.check(_lib.lib.oniris_vae_down(f8.data_ptr(), 1, *f8.stride(), 1, T, 256, 256, 3, 1, 1, 1, bk0["wd"].data_ptr(),
                                        bk0["bd"].data_ptr(), 8, y0.data_ptr(), s), "down")


us = per_launch_us(down0)
nbytes = f8.numel() + 4 * y0.numel()
say(f"    down, first block (uint8 frames in, 3 -> 8 channels, {T} frames 256x256): {us:.1f} us per launch; {nbytes / 1e6:.1f} MB read + "
    f"written -> {nbytes / us / 1e6:.2f} TB/s = {100 * nbytes / us / 1e6 / 6.3:.0f} % of 6.3 TB/s")
del x, y, f8, y0

# (a) whole sequence, 1056 frames -> 264 latent frames
T = 1056
frames = torch.randint(0, 256, (1, T, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV)
nat = lambda: vae.frames_to_latents(frames)                   # noqa: E731
ref = lambda: RE.frames_to_latents(sd, vae.kwargs, frames)    # noqa: E731
with torch.no_grad():
    for fn in (nat, ref):
        fn()
    torch.cuda.synchronize()
    tn, tr = [], []
    for _ in range(3):
        dt, mn = timed(nat)
        tn.append(dt)
        del mn
        dt, mr = timed(ref)
        tr.append(dt)
        del mr
    torch.cuda.empty_cache()
    m1 = vae.frames_to_latents(frames[:, :8])
    m2 = RE.frames_to_latents(sd, vae.kwargs, frames[:, :8])
err = ((m1 - m2).norm() / m2.norm()).item()
say(f"(a) whole-sequence frames_to_latents, {T} uint8 frames 256x256 -> {T // 4} latent frames, B = 1: native median "
    f"{1e3 * statistics.median(tn):.1f} ms ({1e3 * statistics.median(tn) / (T // 4):.3f} ms per latent frame), reference formulation (eager "
    f"fp32 PyTorch, same GPU) median {1e3 * statistics.median(tr):.1f} ms; speed-up {statistics.median(tr) / statistics.median(tn):.1f}x "
    f"(3 alternating runs each; native {[round(1e3 * v, 1) for v in tn]}, reference {[round(1e3 * v, 1) for v in tr]}); "
    f"rel L2 native vs reference formulation (first 8 frames) {err:.2e}")
if out:
    out.close()

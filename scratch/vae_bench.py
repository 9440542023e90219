"""VAE decoder timing (gym VAE, channels [3, 8, 8, 8], 64x64 latents, B = 1): prints a text report, and also writes it to the
path given as argv[1] (e.g. profiles/vae_decoder.txt).

  (a) whole-sequence decode of 264 latent frames: the native decoder (csrc/vae.hip) against the reference's formulation in
      eager fp32 PyTorch (tests/vae_cpu_restatement.py run on the GPU), both warmed up, medians of alternating runs;
  (b) streaming latency per latent frame: decode_frames of one frame through the cache, wall time from the call to the
      frames being complete (synchronised), median over 40 frames;
  (c) res A of the last block (the group-causal conv, g = 4, 8 -> 32 channels at 256x256) alone: kernel time (events around
      50 back-to-back launches) against its fp32 roofline (157.3 TFLOP/s).
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
import vae_cpu_restatement as R  # noqa: E402

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


vae = VAE.from_pretrained(os.path.join(ROOT, "tests", "golden", "g14_vae_gym.pt")).to(DEV)
sd = {k: v for k, v in vae.state_dict().items()}
g = torch.Generator().manual_seed(0)
say(f"device: {torch.cuda.get_device_name(0)}; gym VAE {vae.kwargs['channels']}, n_res_blocks {vae.kwargs['n_res_blocks']}")

# (b) streaming, one latent frame per call
lat = torch.randn(1, 48, 8, 64, 64, generator=g).to(DEV)
cache, per = None, []
for i in range(48):
    dt, (f, cache) = timed(lambda: vae.decode_frames(lat[:, i:i + 1], cache=cache))
    if i >= 8:
        per.append(dt)
say(f"(b) streaming decode_frames, 1 latent frame (4 RGB frames 256x256) per call, B = 1: median {1e3 * statistics.median(per):.3f} ms, "
    f"min {1e3 * min(per):.3f}, max {1e3 * max(per):.3f} over {len(per)} frames (wall, call to synchronised frames)")

# (c) res A of the last block alone
C, gs, H = 8, 4, 256
x = torch.randn(1, 4, H, H, C, device=DEV)
u = torch.empty_like(x)
cout = torch.empty(1, gs, H, H, C, device=DEV)
pk = vae._pack(torch.device(DEV))
bk = pk["blocks"][2]
rb = bk["res"][0]
emb = torch.randn(2 * C, device=DEV) * 0.1
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def res_a():
    _lib.check(_lib.lib.oniris_vae_res_a(x.data_ptr(), None, cout.data_ptr(), emb.data_ptr(), rb["wa"].data_ptr(), rb["ba"].data_ptr(),
                                         1, 4, H, H, C, gs, bk["nch"], bk["gpt"], u.data_ptr(), s), "res_a")


for _ in range(5):
    res_a()
ts = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        res_a()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / 50 * 1e3)
us = statistics.median(ts)
flop = 2.0 * H * H * (C * gs) * (2 * gs * 9 * C)
say(f"(c) res A, last block (g = 4, 8 -> 32 channels, K = 576, 256x256 positions, 1 time step): {us:.1f} us per launch "
    f"(median of 5 x 50 back-to-back); {flop / 1e9:.2f} GFLOP -> {flop / us / 1e6:.1f} TFLOP/s = "
    f"{100 * flop / us / 1e6 / 157.3:.1f} % of the 157.3 TFLOP/s fp32 roofline (roofline time {flop / 157.3e12 * 1e6:.1f} us)")

# (a) whole sequence, 264 latent frames
T = 264
z = torch.randn(1, 8, T, 64, 64, generator=g).to(DEV)
t = torch.full((1,), 0.1, device=DEV)
nat = lambda: vae.decode(z, t)[0]                 # noqa: E731
ref = lambda: R.decode(sd, vae.kwargs, z, t)[0]   # noqa: E731
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
m1 = vae.decode(z[:, :, :8], t)[0]
m2 = R.decode(sd, vae.kwargs, z[:, :, :8], t)[0]
err = ((m1 - m2).norm() / m2.norm()).item()
say(f"(a) whole-sequence decode, {T} latent frames -> {4 * T} RGB frames 256x256, B = 1: native median {1e3 * statistics.median(tn):.1f} ms "
    f"({1e3 * statistics.median(tn) / T:.3f} ms per latent frame), reference formulation (eager fp32 PyTorch, same GPU) median "
    f"{1e3 * statistics.median(tr):.1f} ms; speed-up {statistics.median(tr) / statistics.median(tn):.1f}x "
    f"(3 alternating runs each; native {[round(1e3 * v, 1) for v in tn]}, reference {[round(1e3 * v, 1) for v in tr]}); "
    f"rel L2 native vs reference formulation (first 8 frames) {err:.2e}")
if out:
    out.close()

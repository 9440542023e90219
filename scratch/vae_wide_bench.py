"""Wide VAE decoder timing (channels [3, 16, 64, 256, 8], n_res_blocks 3, time compressions [1, 2, 2, 1], spatial compressions
[1, 2, 2, 2], seeded; 32x32 latents -> 256x256 frames, B = 1): prints a text report, and also writes it to the path given as
argv[1] (e.g. profiles/vae_wide.txt).

  (a) whole decode of 32 latent frames: the native decoder (csrc/vae.hip + csrc/vae_wide.hip) against the reference's formulation
      in eager fp32 PyTorch (tests/vae_cpu_restatement.py run on the GPU), same process, both warmed up, medians of alternating
      runs.  This eager time is the yardstick;
  (b) streaming latency per latent frame: decode_frames of one frame through the cache, wall time from the call to the frames
      being complete (synchronised), median over 24 frames;
  (c) conv A of the 256-wide block (g = 2, 64 frames of 64x64) alone: time per launch and TFLOP/s against the 157.3 TFLOP/s fp32
      matrix roofline; the block's other launches, and the same conv in eager PyTorch;
  (d) the narrow blocks that follow it (64 and 16 channels, register-tile kernels): their ResBlock launches against the same
      conv in eager PyTorch -- where the rest of (a)'s time goes.
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
from vae_wide_oracle import seed_params  # noqa: E402

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


def per_launch(fn, reps=5, inner=5):
    """Median over `reps` of the event time around `inner` back-to-back launches, in microseconds per launch."""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(ts)


KW = dict(channels=[3, 16, 64, 256, 8], n_res_blocks=3, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2],
          mean=[0.0] * 8, std=[1.0] * 8)
torch.manual_seed(0)
vae = seed_params(VAE(**KW), 2290).eval().to(DEV)
sd = {k: v for k, v in vae.state_dict().items()}
g = torch.Generator().manual_seed(0)
say(f"device: {torch.cuda.get_device_name(0)}; VAE {KW['channels']}, n_res_blocks {KW['n_res_blocks']}, decoder widths "
    f"{vae.decoder.in_channels} at group sizes {vae.decoder.group_sizes}; 32x32 latents, B = 1")

# (b) streaming, one latent frame per call
lat = torch.randn(1, 32, 8, 32, 32, generator=g).to(DEV)
cache, per = None, []
for i in range(32):
    dt, (f, cache) = timed(lambda: vae.decode_frames(lat[:, i:i + 1], cache=cache))
    if i >= 8:
        per.append(dt)
say(f"(b) streaming decode_frames, 1 latent frame ({f.shape[1]} RGB frames {f.shape[2]}x{f.shape[3]}) per call: median "
    f"{1e3 * statistics.median(per):.3f} ms, min {1e3 * min(per):.3f}, max {1e3 * max(per):.3f} over {len(per)} frames (wall, call "
    f"to synchronised frames)")
del cache

# (c) the launches of one ResBlock of the 256-wide block
pk = vae._pack(torch.device(DEV))
bk = pk["blocks"][1]
rb = bk["res"][0]
C, gs, T, H = bk["C"], bk["g"], 64, 64
assert bk["wide"] and C == 256
x = torch.randn(1, T, H, H, C, device=DEV)
S = torch.empty(1, gs + T, H, H, C, device=DEV)
a, u, y = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
cout = torch.empty(1, gs, H, H, C, device=DEV)
emb = torch.randn(2 * C, device=DEV) * 0.1
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
L = _lib.lib
p = lambda t: t.data_ptr()  # noqa: E731
act1 = lambda: _lib.check(L.oniris_vae_wide_act(p(x), p(emb), None, p(cout), p(S), 1, T, H, H, C, gs, s), "act1")      # noqa: E731
conv_a = lambda: _lib.check(L.oniris_vae_wide_conv_a(p(S), p(rb["wa"]), p(rb["ba"]), p(a), 1, T, H, H, C, gs, s), "conv_a")  # noqa: E731
act2 = lambda: _lib.check(L.oniris_vae_wide_act(p(a), None, None, None, p(u), 1, T, H, H, C, 0, s), "act2")              # noqa: E731
conv_b = lambda: _lib.check(L.oniris_vae_wide_conv_b(p(u), p(x), p(rb["wb"]), p(rb["bb"]), p(y), 1, T, H, H, C, s), "conv_b")  # noqa: E731
act1()
us_a = per_launch(conv_a)
flop = 2.0 * T * H * H * C * (2 * gs * 9 * C)
say(f"(c) conv A of the 256-wide block (g = {gs}, K = {2 * gs * 9 * C}, {T} frames of {H}x{H}): {us_a / 1e3:.2f} ms per launch (median "
    f"of 5 x 5 back-to-back); {flop / 1e12:.2f} TFLOP -> {flop / us_a / 1e6:.1f} TFLOP/s = {100 * flop / us_a / 1e6 / 157.3:.1f} % of "
    f"the 157.3 TFLOP/s fp32 matrix roofline (roofline time {flop / 157.3e12 * 1e3:.2f} ms)")
us_b = per_launch(conv_b)
flop_b = 2.0 * T * H * H * C * 9 * C
say(f"    conv B: {us_b / 1e3:.2f} ms per launch, {flop_b / us_b / 1e6:.1f} TFLOP/s; act1 (sequence form, "
    f"{(2 * T + 2 * gs) * H * H * C * 4 / 1e6:.0f} MB moved): {per_launch(act1):.0f} us; act2: {per_launch(act2):.0f} us")

# the same conv A as the eager formulation runs it: F.conv3d on the padded channels-first sequence (MIOpen)
w3 = vae.decoder.encoder_blocks[1].res_blocks[0].conv3d0.conv3d
seq = torch.randn(1, C, gs + T, H + 2, H + 2, device=DEV)
us_e = per_launch(lambda: torch.nn.functional.conv3d(seq, w3.weight, w3.bias, stride=(gs, 1, 1)))
say(f"    the same conv A in eager PyTorch (F.conv3d, channels-first, stride ({gs}, 1, 1)): {us_e / 1e3:.2f} ms, "
    f"{flop / us_e / 1e6:.1f} TFLOP/s; native / eager = {us_a / us_e:.2f}")
del x, S, a, u, y, seq

# (d) the narrow blocks behind it, on the register-tile kernels of csrc/vae_conv3.h (unchanged here): res A / res B of the
# 64-channel block (g = 4, 128 frames of 128x128) and of the 16-channel block (g = 4, 128 frames of 256x256)
for bi, (Tn, Hn) in ((2, (128, 128)), (3, (128, 256))):
    bn = pk["blocks"][bi]
    rn, Cn, gn = bn["res"][0], bn["C"], bn["g"]
    xn = torch.randn(1, Tn, Hn, Hn, Cn, device=DEV)
    un, yn = torch.empty_like(xn), torch.empty_like(xn)
    cn = torch.empty(1, gn, Hn, Hn, Cn, device=DEV)
    en = torch.randn(2 * Cn, device=DEV) * 0.1
    ra = lambda: _lib.check(L.oniris_vae_res_a(p(xn), None, p(cn), p(en), p(rn["wa"]), p(rn["ba"]), 1, Tn, Hn, Hn, Cn, gn, bn["nch"],  # noqa: E731
                                               bn["gpt"], p(un), s), "res_a")
    rbn = lambda: _lib.check(L.oniris_vae_res_b(p(un), p(xn), p(rn["wb"]), p(rn["bb"]), 1, Tn, Hn, Hn, Cn, bn["nch"], p(yn), s), "res_b")  # noqa: E731
    ua, ub = per_launch(ra, 3, 3), per_launch(rbn, 3, 3)
    fa = 2.0 * Tn * Hn * Hn * Cn * (2 * gn * 9 * Cn)
    wn = vae.decoder.encoder_blocks[bi].res_blocks[0].conv3d0.conv3d
    sq = torch.randn(1, Cn, gn + Tn, Hn + 2, Hn + 2, device=DEV)
    ue = per_launch(lambda: torch.nn.functional.conv3d(sq, wn.weight, wn.bias, stride=(gn, 1, 1)), 3, 3)
    say(f"(d) narrow block {bi} ({Cn} channels, g = {gn}, {Tn} frames of {Hn}x{Hn}), per ResBlock: res A {ua / 1e3:.2f} ms "
        f"({fa / ua / 1e6:.1f} TFLOP/s), res B {ub / 1e3:.2f} ms; its conv A in eager PyTorch {ue / 1e3:.2f} ms "
        f"(native res A / eager conv = {ua / ue:.2f}; res A also holds both activations)")
    del xn, un, yn, cn, sq

# (a) whole decode, 32 latent frames
T = 32
z = torch.randn(1, 8, T, 32, 32, generator=g).to(DEV)
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
    dt, mr = timed(ref)
    tr.append(dt)
err = ((mn - mr).norm() / mr.norm()).item()
del mn, mr
mn_, mr_ = statistics.median(tn), statistics.median(tr)
say(f"(a) whole decode, {T} latent frames -> {4 * T} RGB frames 256x256, B = 1: native median {1e3 * mn_:.1f} ms "
    f"({1e3 * mn_ / T:.2f} ms per latent frame), reference formulation (eager fp32 PyTorch, same GPU) median {1e3 * mr_:.1f} ms; "
    f"native / eager time = {mn_ / mr_:.2f} ({'native is faster' if mn_ < mr_ else 'NATIVE IS SLOWER'}) "
    f"(3 alternating runs each; native {[round(1e3 * v, 1) for v in tn]}, reference {[round(1e3 * v, 1) for v in tr]}); "
    f"rel L2 native vs reference formulation {err:.2e}")
if out:
    out.close()

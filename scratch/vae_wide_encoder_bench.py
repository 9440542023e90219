"""Wide VAE encoder timing (channels [3, 16, 64, 256, 8], n_res_blocks 3, time compressions [1, 2, 2, 1], spatial compressions
[1, 2, 2, 2], seeded; 256x256 uint8 frames -> 32x32 latents, B = 1): prints a text report, and also writes it to the path given as
argv[1] (e.g. profiles/vae_wide_encoder.txt; the compile-time resource figures at its head are kept by hand).

  (a) whole-sequence frames_to_latents of 64 frames: the native encoder (csrc/vae_encoder.hip + csrc/vae_wide.hip) against the
      reference's formulation in eager fp32 PyTorch (tests/vae_encoder_cpu_restatement.py run on the GPU), same process, both
      warmed up, medians of alternating runs.  Nothing on the eager side is a target here;
  (b) streaming latency: encode_frames of 8 frames (2 latent frames, the smallest chunk of this model: block 1 sees T / 2 frames
      in groups of 4) through the cache, wall time from the call to the latents being complete (synchronised), median over 6
      calls, and that per latent frame;
  (c) each oniris_vae_wide_down launch of that model alone (64 -> 256 at K = 512, 256 -> 8 at K = 1024), at the sizes of (a): time
      per launch, the bytes it must move and the FLOPs it must do, and its share of the larger of the HBM (6.3 TB/s achievable)
      and fp32-matrix (157.3 TFLOP/s) roofline times.  The 256 -> 8 launch has 128-element area windows on 8 live channels: its
      time is split between the GEMM and the area loop with a control launch of the same input at Cout = K = 1024, whose
      windows have length 1 and whose GEMM is 32 blocks of 32 channels (the 256 -> 8 launch computes one such block).
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
from autoregressive_diffusion_amd.vae import VAE, _pack_down_wide  # noqa: E402
import vae_encoder_cpu_restatement as RE  # noqa: E402
from vae_wide_oracle import seed_params  # noqa: E402

DEV = "cuda"
HBM, MATRIX = 6.3e12, 157.3e12
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
vae = seed_params(VAE(**KW), 2390).eval().to(DEV)
sd = {k: v for k, v in vae.state_dict().items()}
g = torch.Generator().manual_seed(0)
T, HW = 64, 256
frames = torch.randint(0, 256, (1, T, HW, HW, 3), generator=g, dtype=torch.uint8).to(DEV)
say(f"device: {torch.cuda.get_device_name(0)}; VAE {KW['channels']}, n_res_blocks {KW['n_res_blocks']}, encoder widths "
    f"{vae.encoder.out_channels} at group sizes {vae.encoder.group_sizes}; {HW}x{HW} uint8 frames, B = 1")

# (b) streaming, two latent frames (8 frames) per call
cache, per = None, []
for i in range(0, T, 8):
    dt, (lat, cache) = timed(lambda: vae.encode_frames(frames[:, i:i + 8], cache=cache))
    if i >= 16:
        per.append(dt)
say(f"(b) streaming encode_frames, 8 frames -> 2 latent frames {tuple(lat.shape[2:])} per call: median "
    f"{1e3 * statistics.median(per):.3f} ms ({1e3 * statistics.median(per) / 2:.3f} ms per latent frame), min {1e3 * min(per):.3f}, max "
    f"{1e3 * max(per):.3f} over {len(per)} calls (wall, call to synchronised latents)")
del cache

# (c) the two oniris_vae_wide_down launches at the sizes of the whole-sequence encode
pk = vae._pack_encoder(torch.device(DEV))
assert [bool(bk.get("wide_down")) for bk in pk["blocks"]] == [False, False, True, True]
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
L = _lib.lib
p = lambda t: t.data_ptr()  # noqa: E731


def down_launch(x, To, Ho, Cin, tc, sc, w, b, Cout):
    y = torch.empty(1, To, Ho, Ho, Cout, device=DEV)
    fn = lambda: _lib.check(L.oniris_vae_wide_down(p(x), 0, *x.stride()[:4], 1, 1, To, Ho, Ho, Cin, tc, sc, 0, p(w), p(b), Cout, p(y),  # noqa: E731
                                                   s), "vae_wide_down")
    return per_launch(fn), y


def report(name, us, To, Ho, Cin, tc, sc, Cout):
    K, pix = Cin * tc * sc * sc, To * Ho * Ho
    byts = 4.0 * (pix * K + pix * Cout + K * (-(-Cout // 32) * 32))
    flop = 2.0 * pix * K * Cout
    t_hbm, t_mx = byts / HBM * 1e6, flop / MATRIX * 1e6
    bound = "HBM" if t_hbm >= t_mx else "the fp32 matrix rate"
    say(f"(c) {name}: K = {K}, {To} output frames of {Ho}x{Ho}: {us:.0f} us per launch (median of 5 x 5 back-to-back); must move "
        f"{byts / 1e6:.0f} MB ({t_hbm:.0f} us at 6.3 TB/s) and do {flop / 1e9:.1f} GFLOP ({t_mx:.0f} us at 157.3 TFLOP/s): bound by "
        f"{bound}, roofline time {max(t_hbm, t_mx):.0f} us = {100 * max(t_hbm, t_mx) / us:.1f} % of the launch")


b2, b3 = pk["blocks"][2], pk["blocks"][3]
x2 = torch.randn(1, T // 2, HW // 2, HW // 2, 64, device=DEV)
us2, _ = down_launch(x2, T // 4, HW // 4, 64, 2, 2, b2["wd"], b2["bd"], 256)
report("down 64 -> 256 (tc 2, sc 2, vector staging, NB = 2)", us2, T // 4, HW // 4, 64, 2, 2, 256)
del x2
x3 = torch.randn(1, T // 4, HW // 4, HW // 4, 256, device=DEV)
us3, _ = down_launch(x3, T // 4, HW // 8, 256, 1, 2, b3["wd"], b3["bd"], 8)
report("down 256 -> 8 (tc 1, sc 2, vector staging, NB = 1, 128-element area windows on 8 live channels)", us3, T // 4, HW // 8, 256,
       1, 2, 8)
ctl = torch.nn.Conv3d(1024, 1024, kernel_size=1).to(DEV)
wc, bc = _pack_down_wide(ctl.weight, ctl.bias, 256, 1024, 4, dict(device=DEV, dtype=torch.float32))
usc, _ = down_launch(x3, T // 4, HW // 8, 256, 1, 2, wc, bc, 1024)
say(f"    control, the same input at Cout = 1024 (windows of length 1, 32 blocks of 32 channels as 16 workgroup columns at NB = 2): "
    f"{usc:.0f} us per launch = {usc / 32:.1f} us per 32-channel block; the 256 -> 8 launch computes one such block, so about "
    f"{usc / 32:.0f} us of its {us3:.0f} us are the GEMM and its staging and about {us3 - usc / 32:.0f} us "
    f"({100 * (us3 - usc / 32) / us3:.0f} %) the area loop (the control's blocks share the staged input through L2 and run at NB = 2, "
    f"so this GEMM share is a lower bound)")
del x3

# (a) whole sequence
nat = lambda: vae.frames_to_latents(frames)                  # noqa: E731
ref = lambda: RE.frames_to_latents(sd, vae.kwargs, frames)   # noqa: E731
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
mn_, mr_ = statistics.median(tn), statistics.median(tr)
say(f"(a) whole frames_to_latents, {T} frames {HW}x{HW} -> {T // 4} latent frames, B = 1: native median {1e3 * mn_:.1f} ms "
    f"({1e3 * mn_ / (T // 4):.2f} ms per latent frame), reference formulation (eager fp32 PyTorch, same GPU) median {1e3 * mr_:.1f} ms; "
    f"native / eager time = {mn_ / mr_:.2f} ({'native is faster' if mn_ < mr_ else 'NATIVE IS SLOWER'}) "
    f"(3 alternating runs each; native {[round(1e3 * v, 1) for v in tn]}, reference {[round(1e3 * v, 1) for v in tr]}); "
    f"rel L2 native vs reference formulation {err:.2e}")
if out:
    out.close()

"""VAE512 timing at the full-size Counter-Strike model ([3,32,128,512,8] with five ResBlocks, time compressions [1,2,2,1], spatial
[1,2,2,2], B = 1, 32 frames of 256x256): prints a text report, and also appends it to the path given as argv[1] (e.g.
profiles/vae_512.txt).  Sections (argv --only=a,b,c picks some; each is best run as a process of its own under `timeout -k 10`):

  (a) conv A of the 512-wide block alone (g = 4, 32x32 pixels, B = 1, T = 32) with oniris_vae_wide_set_nb_max at 2 and at 4 in the
      same process, alternating after warm-up: median kernel time, TFLOP/s and the share of the 157.3 TFLOP/s fp32 matrix roofline;
      and its weight gradient: time, the workspace bytes and the number of slabs under the policy of vae_train._nslab, next to
      what the floor of 64 slabs would have allocated (computed, not allocated);
  (b) inference: decode_frames per streamed latent frame and over the whole sequence, and encode, against the reference's
      formulation in eager fp32 PyTorch (tests/vae_cpu_restatement.py, tests/vae_encoder_cpu_restatement.py run on the GPU), same
      process, both warmed up, medians of alternating runs;
  (c) one training forward + backward and its peak memory (torch.cuda.max_memory_allocated), at the largest T of 32, 16, 8 that fits.
The eager fp32 training step of this model is not timed here: on an MI355X one forward + backward of the training restatement wrote
nothing for seven minutes, twice, and was taken out."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import _lib, vae as V, vae_train  # noqa: E402
from autoregressive_diffusion_amd.vae import VAE512  # noqa: E402
import vae_cpu_restatement as R  # noqa: E402
import vae_encoder_cpu_restatement as RE  # noqa: E402
from vae_wide_oracle import seed_params  # noqa: E402

DEV = "cuda"
ROOF = 157.3
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
only = next((a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--only=")), ["a", "b", "c"])
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


def event_us(fn, n=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


KW = dict(channels=[3, 32, 128, 512, 8], n_res_blocks=5, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2],
          mean=[0.0] * 8, std=[1.0] * 8)
B, T, H, W = 1, 32, 256, 256
s, p = V._stream(), V._p
say(f"device: {torch.cuda.get_device_name(0)}; VAE512 {KW['channels']}, n_res_blocks {KW['n_res_blocks']}, B = {B}, {T} frames of {H}x{W}")

if "a" in only:
    C, g, h = 512, 4, 32
    gen = torch.Generator().manual_seed(1)
    wa = torch.randn(2 * g, 3, 3, C, g, C, generator=gen).to(DEV) / (18 * g * C) ** 0.5
    ba = torch.zeros(g, C, device=DEV)
    S = torch.randn(B, g + T, h, h, C, generator=gen).to(DEV)
    pk = dict(wa=wa, ba=ba)
    flops = 2.0 * B * T * h * h * C * C * 2 * g * 9
    run = lambda: V.wide_conv_a(S, pk, g, s)   # noqa: E731
    was = _lib.lib.oniris_vae_wide_set_nb_max(2)
    us = {2: [], 4: []}
    outs = {}
    for nb in (2, 4):                                            # warm-up, and the bits
        _lib.lib.oniris_vae_wide_set_nb_max(nb)
        outs[nb] = run()
        run()
    torch.cuda.synchronize()
    for _ in range(7):
        for nb in (2, 4):
            _lib.lib.oniris_vae_wide_set_nb_max(nb)
            us[nb].append(event_us(run))
    _lib.lib.oniris_vae_wide_set_nb_max(was)
    say(f"(a) conv A at C = {C}, g = {g}, {h}x{h}, B = {B}, T = {T} (K = {2 * g * 9 * C}, {flops / 1e9:.0f} GFLOP), 7 alternating "
        f"medians of 3 launches each; equal bits: {bool(torch.equal(outs[2], outs[4]))}")
    for nb in (2, 4):
        m = statistics.median(us[nb])
        say(f"    NB = {nb} ({32 * nb} output channels per workgroup): {m:.0f} us, {flops / m / 1e6:.1f} TFLOP/s = "
            f"{100 * flops / m / 1e6 / ROOF:.1f} % of the {ROOF} TFLOP/s fp32 matrix roofline   (runs {[round(v) for v in us[nb]]})")
    m2, m4 = statistics.median(us[2]), statistics.median(us[4])
    say(f"    NB = 4 against NB = 2: {100 * (m2 / m4 - 1):+.1f} % (kept as the default only above +5 %)")
    del outs
    D = torch.randn(B, T + g, h, h, C, generator=gen).to(DEV)
    items = B * (T // g) * (h // 16) ** 2
    n = 2 * g * g * 9 * C * C + g * C
    nslab = vae_train._nslab(items, n, C)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    wg = lambda: vae_train._wide_conv3_dw(S, D, B, T, h, h, C, g, True)   # noqa: E731
    wg()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ts = [event_us(wg, 1) for _ in range(5)]
    m = statistics.median(ts)
    say(f"    conv A weight gradient: {items} work items, {nslab} slab(s) of {4 * n / 1e6:.1f} MB = {4 * n * nslab / 1e6:.1f} MB of workspace "
        f"(peak allocation above the operands {peak / 1e6:.1f} MB; the floor of 64 slabs would be {4 * n * vae_train._nslab(items, n) / 1e9:.2f} GB, "
        f"not allocated here); {m:.0f} us, {flops / m / 1e6:.1f} TFLOP/s = {100 * flops / m / 1e6 / ROOF:.1f} % of the roofline")
    del S, D, wa
    torch.cuda.empty_cache()

if "b" in only or "c" in only:
    vae = seed_params(VAE512(**KW), 7).to(DEV)

if "b" in only:
    vae.eval()
    sd = {k: v.detach() for k, v in vae.state_dict().items()}
    gen = torch.Generator().manual_seed(2)
    lat = torch.randn(B, T // 4, 8, H // 8, W // 8, generator=gen).to(DEV)
    z = lat.permute(0, 2, 1, 3, 4).contiguous()
    t = 0.1 * torch.ones(B, device=DEV)
    x = (torch.rand(B, 3, T, H, W, generator=gen) * 2 - 1).to(DEV)

    def stream():
        cache = None
        for i in range(lat.shape[1]):
            _, cache = vae.decode_frames(lat[:, i:i + 1], cache=cache)

    with torch.no_grad():
        cases = (("decode_frames, streamed one latent frame at a time", stream, lambda: R.decode(sd, vae.kwargs, z, t)[0], lat.shape[1]),
                 ("decode_frames, the whole sequence", lambda: vae.decode_frames(lat), lambda: R.decode(sd, vae.kwargs, z, t)[0], 1),
                 ("encode", lambda: vae.encode(x), lambda: RE.encode(sd, vae.kwargs, x)[0], 1))
        say(f"(b) inference, {T} frames = {T // 4} latent frames; eager = the restatement in fp32 PyTorch on the same GPU, whole sequence")
        for name, nat, ref, per in cases:
            nat(), ref()
            tn, te = [], []
            for _ in range(3):
                tn.append(timed(nat))
                te.append(timed(ref))
            mn, me = statistics.median(tn), statistics.median(te)
            say(f"    {name}: native median {1e3 * mn:.1f} ms" + (f" = {1e3 * mn / per:.1f} ms per latent frame" if per > 1 else "") +
                f", eager median {1e3 * me:.1f} ms; eager / native = {me / mn:.2f}x (native {[round(1e3 * v, 1) for v in tn]}, eager "
                f"{[round(1e3 * v, 1) for v in te]})")
        e = ((vae.encode(x)[0] - RE.encode(sd, vae.kwargs, x)[0]).norm() / RE.encode(sd, vae.kwargs, x)[0].norm()).item()
        say(f"    rel L2 of encode against the eager fp32 restatement: {e:.2e}")
    del lat, z, x
    torch.cuda.empty_cache()

if "c" in only:
    vae.train()

    def operands(T_):
        g_ = torch.Generator().manual_seed(0)
        x_ = (torch.rand(B, 3, T_, H, W, generator=g_) * 2 - 1).to(DEV)
        return x_, (torch.rand(B, generator=g_) * 0.1).to(DEV), torch.randn(B, 8, T_ // 4, H // 8, W // 8, generator=g_).to(DEV)

    def loss_of(x_, r_mean, r_logvar):
        return 0.5 * (r_logvar + (x_ - r_mean) ** 2 / torch.exp(r_logvar)).mean()

    def native(x_, ts, noise):
        vae.zero_grad(set_to_none=True)
        r_mean, r_logvar, _, _ = vae(x_, t_sample=ts, noise=noise)
        loss_of(x_, r_mean, r_logvar).backward()

    say("(c) one training forward + backward (VAE512: the training path is on as constructed)")
    for name, step in (("native", native),):
        for T_ in (32, 16, 8):
            try:
                ops_ = operands(T_)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                step(*ops_)
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated()
                ts_ = [timed(lambda: step(*ops_)) for _ in range(3)]
            except torch.OutOfMemoryError:
                say(f"    {name}, {T_} frames: out of memory")
                vae.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                continue
            say(f"    {name}, {T_} frames: median {1e3 * statistics.median(ts_):.1f} ms ({[round(1e3 * v, 1) for v in ts_]}), peak memory "
                f"{peak / 2 ** 30:.2f} GiB (parameters and their gradients included)")
            break
        vae.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
if out:
    out.close()

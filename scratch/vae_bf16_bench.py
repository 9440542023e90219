"""VAE.bf16_inference() against the fp32 path at the full-size Counter-Strike model ([3,32,128,512,8] with five ResBlocks, time
compressions [1,2,2,1], spatial [1,2,2,2], B = 1, 32 frames of 256x256), switch off and on in the same process, alternating, with
the median protocol of scratch/vae_512_bench.py: prints a text report, and also appends it to the path given as argv[1] (e.g.
profiles/vae_bf16.txt).  Sections (argv --only=a,b,c picks some; each is best run as a process of its own under `timeout -k 10`):

  (a) conv A of the 512-wide block alone (g = 4, 32x32 pixels, B = 1, T = 32): the fp32 launch and the bf16 launch, median kernel
      time, TFLOP/s against the 2.5 PFLOP/s bf16 MFMA roofline and against the weight-stream roofline computed there;
  (b) decode_frames streamed one latent frame at a time, decode_frames over the whole sequence, and encode of 32 frames;
  (c) decode_frames over the whole sequence, stage by stage (events around every launch wrapper of vae.py), switch off and on."""
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import vae as V  # noqa: E402
from autoregressive_diffusion_amd.vae import VAE512  # noqa: E402
from vae_wide_oracle import seed_params  # noqa: E402

DEV = "cuda"
ROOF_BF16, ROOF_F32 = 2500.0, 157.3                              # TFLOP/s: v_mfma_f32_32x32x16_bf16, v_mfma_f32_32x32x2_f32
L2_TBS, MALL_TBS = 18.0, 8.6                                      # TB/s: L2-shared rows (17-19), Infinity-Cache gathers
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
s = V._stream()
say(f"device: {torch.cuda.get_device_name(0)}; VAE512 {KW['channels']}, n_res_blocks {KW['n_res_blocks']}, B = {B}, {T} frames of {H}x{W}")

if "a" in only:
    C, g, h = 512, 4, 32
    gen = torch.Generator().manual_seed(1)
    rb = V.ResBlock(C, (2 * g, 3, 3), g).to(DEV)
    with torch.no_grad():
        rb.conv3d0.conv3d.weight.copy_(torch.randn(rb.conv3d0.conv3d.weight.shape, generator=gen) / (18 * g * C) ** 0.5)
    f32 = dict(device=DEV, dtype=torch.float32)
    packs = {"fp32": V._pack_res_wide(rb, C, g, f32), "bf16": V._pack_res_wide(rb, C, g, f32, bf16=True)}
    del rb
    S = torch.randn(B, g + T, h, h, C, generator=gen).to(DEV)
    K = 2 * g * 9 * C
    flops = 2.0 * B * T * h * h * C * C * 2 * g * 9
    run = lambda kind: V.wide_conv_a(S, packs[kind], g, s)   # noqa: E731
    us, outs = {"fp32": [], "bf16": []}, {}
    for kind in us:                                              # warm-up, and the bits
        outs[kind] = run(kind)
        run(kind)
    torch.cuda.synchronize()
    for _ in range(7):
        for kind in us:
            us[kind].append(event_us(lambda: run(kind)))
    rel = ((outs["bf16"] - outs["fp32"]).norm() / outs["fp32"].norm()).item()
    say(f"(a) conv A at C = {C}, g = {g}, {h}x{h}, B = {B}, T = {T} (K = {K}, {flops / 1e9:.0f} GFLOP), 7 alternating medians of 3 "
        f"launches each; rel L2 of bf16 against fp32: {rel:.2e}")
    med = {k: statistics.median(v) for k, v in us.items()}
    for kind, nb, roof in (("fp32", 4, ROOF_F32), ("bf16", 2, ROOF_BF16)):
        m = med[kind]
        say(f"    {kind} ({32 * nb} output channels per workgroup): {m:.0f} us, {flops / m / 1e6:.1f} TFLOP/s = "
            f"{100 * flops / m / 1e6 / roof:.1f} % of the {roof:.0f} TFLOP/s {kind} matrix roofline   (runs {[round(v) for v in us[kind]]})")
    say(f"    bf16 against fp32: {med['fp32'] / med['bf16']:.2f}x (the condition for shipping: above 1.05x)")
    # the operand streams of a workgroup (256 pixels x 64 outputs, all of K): 2 K 64 bytes of bf16 weights and 324 K 4 bytes of fp32
    # halo (18 x 18 pixels) for 2 256 K 64 flops
    tf = flops / med["bf16"] / 1e6
    fb_w, fb_h = 256.0, 2 * 256 * 64 / (324 * 4)
    say(f"    weight stream: {fb_w:.0f} flop per weight byte ({K * C * g * 2 / 1e6:.0f} MB of bf16 weights: above an XCD's 4 MiB L2, inside the 256 MiB "
        f"Infinity Cache) -> a roofline of {fb_w * MALL_TBS:.0f} TFLOP/s at {MALL_TBS} TB/s of Infinity-Cache reads ({fb_w * L2_TBS:.0f} at {L2_TBS} TB/s "
        f"of L2); measured {tf:.0f} TFLOP/s = {100 * tf / (fb_w * MALL_TBS):.1f} % of it, {tf / fb_w:.2f} TB/s of weight reads")
    say(f"    halo stream: {fb_h:.1f} flop per fp32 halo byte -> the launch reads {tf / fb_h:.1f} TB/s of halo, each tile's by the 16 workgroups "
        f"(4 frames in the group x 4 channel blocks) that share it")
    del S, outs, packs
    torch.cuda.empty_cache()

if "b" in only or "c" in only:
    models = {"fp32": seed_params(VAE512(**KW), 7).to(DEV).eval()}
    models["bf16"] = copy.deepcopy(models["fp32"]).bf16_inference()
    gen = torch.Generator().manual_seed(2)
    lat = torch.randn(B, T // 4, 8, H // 8, W // 8, generator=gen).to(DEV)

if "b" in only:
    x = (torch.rand(B, 3, T, H, W, generator=gen) * 2 - 1).to(DEV)

    def stream(vae):
        cache = None
        for i in range(lat.shape[1]):
            _, cache = vae.decode_frames(lat[:, i:i + 1], cache=cache)

    with torch.no_grad():
        cases = (("decode_frames, streamed one latent frame at a time", stream, lat.shape[1]),
                 ("decode_frames, the whole sequence", lambda vae: vae.decode_frames(lat), 1),
                 ("encode", lambda vae: vae.encode(x), 1))
        say(f"(b) inference, {T} frames = {T // 4} latent frames; switch off (fp32) and on (bf16), 3 alternating runs each after a warm-up")
        for name, fn, per in cases:
            ts = {"fp32": [], "bf16": []}
            for k in ts:
                fn(models[k])
            for _ in range(3):
                for k in ts:
                    ts[k].append(timed(lambda: fn(models[k])))
            m = {k: statistics.median(v) for k, v in ts.items()}
            say(f"    {name}: fp32 median {1e3 * m['fp32']:.1f} ms, bf16 median {1e3 * m['bf16']:.1f} ms" +
                (f" = {1e3 * m['bf16'] / per:.1f} ms per latent frame" if per > 1 else "") +
                f"; fp32 / bf16 = {m['fp32'] / m['bf16']:.2f}x (fp32 {[round(1e3 * v, 1) for v in ts['fp32']]}, bf16 {[round(1e3 * v, 1) for v in ts['bf16']]})")
        a, b = models["fp32"].decode_frames(lat)[0].int(), models["bf16"].decode_frames(lat)[0].int()
        say(f"    uint8 frame bytes of bf16 against fp32 (seeded weights, not a checkpoint): {100 * ((a - b).abs() > 1).float().mean().item():.2f} % "
            f"differ by more than one level, at most {int((a - b).abs().max())} levels")
    del x

if "c" in only:
    # events around every launch wrapper; a stage is keyed by its name and the channel width of its input
    spans, names = [], ("up", "res_a", "res_b", "wide_act", "wide_conv_a", "wide_conv_b", "out", "temb")
    orig = {n: getattr(V, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig[n](*a, **k)
            e1.record()
            width = a[0].shape[-1] if torch.is_tensor(a[0]) and n != "up" else (a[3]["C"] if n == "up" else 0)
            spans.append((n, width, e0, e1))
            return r
        return f

    say("(c) decode_frames over the whole sequence, stage by stage: ms per stage and input width, switch off | on (one run each "
        "after a warm-up; events around each launch, so launch gaps are left out)")
    table = {}
    with torch.no_grad():
        for k, vae in models.items():
            vae.decode_frames(lat)
            for n in names:
                setattr(V, n, wrap(n))
            try:
                vae.decode_frames(lat)
                torch.cuda.synchronize()
            finally:
                for n in names:
                    setattr(V, n, orig[n])
            for n, width, e0, e1 in spans:
                table.setdefault((n, width), {"fp32": 0.0, "bf16": 0.0})[k] += e0.elapsed_time(e1)
            spans.clear()
    for (n, width), v in sorted(table.items(), key=lambda kv: -kv[1]["bf16"]):
        say(f"    {n:12s} C = {width:4d}: {v['fp32']:8.2f} | {v['bf16']:8.2f} ms")
    tot = {k: sum(v[k] for v in table.values()) for k in ("fp32", "bf16")}
    top = max(table.items(), key=lambda kv: kv[1]["bf16"])
    say(f"    sum of the stages: {tot['fp32']:.1f} | {tot['bf16']:.1f} ms; the largest with the switch on: {top[0][0]} at C = {top[0][1]} "
        f"({100 * top[1]['bf16'] / tot['bf16']:.0f} %)")
if out:
    out.close()

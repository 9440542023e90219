"""Discriminator3D / MixedDiscriminator timing at the gym VAE training shape (gym_vae_train.py:87-119: B = 4 clips of 32 frames of
256x256, Discriminator3D(3, (64, 64))): appends a text report to the path given last (e.g. profiles/discriminator3d.txt).

  python scratch/disc3d_bench.py d3 native REPORT      the native 3-D half: forward alone, forward + backward with all gradients,
                                                       forward + backward with the parameters frozen; HIP events, one warm-up,
                                                       median of 5; the FLOPs of its conv / data-gradient / weight-gradient
                                                       launches (useful FLOPs: no channel padding counted) and the bytes its
                                                       launches read and write (from the operand sizes, not hardware counters)
  python scratch/disc3d_bench.py d3 torch REPORT       the same module's plain torch code (`forward_torch`) on the same GPU
  python scratch/disc3d_bench.py mixed native REPORT   MixedDiscriminator(3) on the same clip, both halves native
  python scratch/disc3d_bench.py mixed torch REPORT    the native 2-D half with the torch 3-D half

Run each as its own process under its own `timeout -k 10`, with OMP_NUM_THREADS=16."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from autoregressive_diffusion_amd import discriminator as d  # noqa: E402

what, how = sys.argv[1], sys.argv[2]
out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
SHAPE, WIDTHS = (4, 3, 32, 256, 256), (64, 64)
PEAK = 157.3
torch.set_num_threads(16)


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def conv_flops():
    """Useful FLOPs of one forward of Discriminator3D(3, WIDTHS) at SHAPE, per conv: [(name, FLOPs)]."""
    N, cin, T, H, W = SHAPE
    half = lambda n: (n - 1) // 2 + 1
    T, H, W = half(T), half(H), half(W)
    rows = [("conv_in", 2 * N * T * H * W * 27 * cin * WIDTHS[0])]
    c = WIDTHS[0]
    for i, co in enumerate(WIDTHS):
        down = i < len(WIDTHS) - 1
        pos = N * T * H * W
        rows.append((f"blocks.{i}.conv1", 2 * pos * 27 * c * co))
        if down:
            T, H, W = half(T), half(H), half(W)
        pos2 = N * T * H * W
        rows.append((f"blocks.{i}.conv2", 2 * pos2 * 27 * co * co))
        rows.append((f"blocks.{i}.shortcut", 2 * pos2 * c * co))
        c = co
    rows.append(("conv_out", 2 * N * T * H * W * 27 * c * 2))
    return rows


traffic = [0]


def _bytes(v):
    if torch.is_tensor(v):
        return v.numel() * v.element_size()
    if isinstance(v, (tuple, list)):
        return sum(_bytes(e) for e in v)
    return 0


def counted(fn, twice=()):
    def w(*a, **k):
        r = fn(*a, **k)
        traffic[0] += _bytes(a) + _bytes(list(k.values())) + _bytes(r) + sum(_bytes(a[i]) for i in twice)
        return r
    return w


net = (d.Discriminator3D(3, WIDTHS) if what == "d3" else d.MixedDiscriminator(3)).to("cuda").train()
d3 = net if what == "d3" else net.discriminator3d
if how == "torch":
    d3.forward = d3.forward_torch
x = torch.randn(SHAPE, device="cuda", generator=torch.Generator("cuda").manual_seed(0))


def run(mode):
    net.requires_grad_(mode != "frozen")
    xi = x.clone().requires_grad_(mode != "fwd")
    if mode == "fwd":
        with torch.no_grad():
            net(xi)
        return
    net(xi).square().mean().backward()
    net.zero_grad(set_to_none=True)


def ms(mode):
    run(mode)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(mode)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


name = "Discriminator3D(3, (64, 64))" if what == "d3" else "MixedDiscriminator(3)"
side = {"native": "native", "torch": "3-D half on torch ops (the parent commit's)"}[how]
say(f"device: {torch.cuda.get_device_name(0)}; {name}, {side}, input {SHAPE}, fp32")
fl = sum(f for _, f in conv_flops())
mult = {"fwd": 1, "all": 3, "frozen": 2}
label = {"fwd": "forward", "all": "forward + backward, all gradients", "frozen": "forward + backward, parameters frozen"}
for mode in ("fwd", "all", "frozen"):
    med, lo, hi = ms(mode)
    line = f"{label[mode]}: median {med:.2f} ms (five runs {lo:.2f} .. {hi:.2f})"
    if what == "d3":
        tf = mult[mode] * fl / 1e12
        line += f"; conv launches {tf:.3f} TFLOP -> {tf / med * 1e3:.1f} TFLOP/s over the whole pass = {tf / med * 1e3 / PEAK * 100:.1f} % of {PEAK}"
    say(line)
if what == "d3" and how == "native":
    for fname, twice in (("conv3", ()), ("conv", ()), ("blur3", ()), ("blur3_bwd", ()), ("wgrad3", ()), ("wgrad", ()), ("stem_dgrad3", ()),
                         ("gn_bwd", (0, 1))):
        setattr(d, fname, counted(getattr(d, fname), twice))
    for mode in ("fwd", "all", "frozen"):
        traffic[0] = 0
        run(mode)
        torch.cuda.synchronize()
        say(f"{label[mode]}: launches read + write {traffic[0] / 1e9:.2f} GB (operand sizes; gn backward reads da and z twice)")
    say("conv FLOPs of one forward: " + ", ".join(f"{n} {f / 1e9:.1f} G" for n, f in conv_flops()))
say(f"peak memory {torch.cuda.max_memory_allocated() >> 20} MiB")

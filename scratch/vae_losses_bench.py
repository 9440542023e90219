"""The VAE losses at the gym VAE training shape (gym_vae_train.py:87-119: 4 clips of 32 frames of 256x256, 25.2 M elements per tensor;
`frames` as the scripts hand them over, a permuted channels-last view): appends a text report to the path given as the first argument
(e.g. profiles/vae_losses.txt).  In one process on one GPU:

  recon_losses (Gaussian + L1 + MSE) forward and forward + backward, native, against the torch formulation the scripts run today
      (edm2.utils.GaussianLoss + F.l1_loss + F.mse_loss on the same operands);
  worst_k_percent_loss(percent=0.2) forward and forward + backward, native, against the reference's torch.topk formulation;
  every native pass alone (HIP events around the one launch): bytes moved per element and achieved TB/s; the key pass also on
      all-equal inputs (every lane of every wave on one histogram bin) and on contiguous operands.

HIP events, medians of 7 after a warm-up.  Run under its own `timeout -k 10`, with OMP_NUM_THREADS=16."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from autoregressive_diffusion_amd import _lib, vae_losses as V  # noqa: E402
from autoregressive_diffusion_amd.vae import _p, _stream  # noqa: E402

DEV = "cuda"
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
SHAPE = tuple(int(v) for v in os.environ.get("VAE_LOSS_BENCH_SHAPE", "4,3,32,256,256").split(","))
torch.set_num_threads(16)


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def ms(fn, reps=7):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def torch_gaussian(mean, logvar, target):
    return ((logvar + (mean - target) ** 2 * (torch.exp(-logvar))) * .5 + 0.918).mean()


def torch_worst_k(recon, frames, percent):
    flat = F.mse_loss(recon, frames, reduction='none').flatten()
    return torch.topk(flat, max(1, int(flat.numel() * (percent / 100.0))))[0].mean()


g = torch.Generator(device=DEV).manual_seed(1)
B, C, T, H, W = SHAPE
n = B * C * T * H * W
mean = (0.6 * torch.randn(SHAPE, device=DEV, generator=g)).requires_grad_(True)
logvar = (0.7 * torch.randn(SHAPE, device=DEV, generator=g) - 1).requires_grad_(True)
frames = (torch.rand(B, T, H, W, C, device=DEV, generator=g) * 2 - 1).permute(0, 4, 1, 2, 3)       # 'b t h w c -> b c t h w'
frames_c = frames.contiguous()
say(f"device: {torch.cuda.get_device_name(0)}; operands {SHAPE} fp32 = {n / 1e6:.1f} M elements, {4 * n / 1e6:.0f} MB each; frames strides {frames.stride()}")


def step(loss_fn):
    mean.grad = logvar.grad = None
    loss_fn().backward()


def fwd(loss_fn):
    with torch.no_grad():
        loss_fn()


native3 = lambda: sum(V.recon_losses(mean, logvar, frames))
torch3 = lambda: torch_gaussian(mean, logvar, frames) + F.l1_loss(mean, frames) + F.mse_loss(mean, frames)
native2 = lambda: V.GaussianLoss(mean, logvar, frames) + V.l1_loss(mean, frames)
torch2 = lambda: torch_gaussian(mean, logvar, frames) + F.l1_loss(mean, frames)
say("-- Gaussian + L1 + MSE (recon_losses: one forward launch + partial sum, one backward launch)")
a, b = ms(lambda: fwd(native3)), ms(lambda: fwd(torch3))
say(f"forward: native {a:.3f} ms, torch {b:.3f} ms ({b / a:.1f} x)")
a, b = ms(lambda: step(native3)), ms(lambda: step(torch3))
say(f"forward + backward (d mean, d logvar): native {a:.3f} ms, torch {b:.3f} ms ({b / a:.1f} x)")
say("-- GaussianLoss + l1_loss as cs_vae_train.py:106-107 calls them (two single calls each way)")
a, b = ms(lambda: step(native2)), ms(lambda: step(torch2))
say(f"forward + backward: native {a:.3f} ms, torch {b:.3f} ms ({b / a:.1f} x)")
say("-- worst_k_percent_loss(percent=0.2), k = %d" % V.worst_k(n, 0.2))
nativew = lambda: V.worst_k_percent_loss(mean, frames, percent=0.2)
torchw = lambda: torch_worst_k(mean, frames, 0.2)
a, b = ms(lambda: fwd(nativew)), ms(lambda: fwd(torchw))
say(f"forward: native {a:.3f} ms, torch {b:.3f} ms ({b / a:.1f} x)")
a, b = ms(lambda: step(nativew)), ms(lambda: step(torchw))
say(f"forward + backward (d recon): native {a:.3f} ms, torch {b:.3f} ms ({b / a:.1f} x)")
lw, lt = nativew().item(), torchw().item()
say(f"values: native {lw:.8f}, torch {lt:.8f}")

say("-- native passes alone (bytes per element counted from the operands; TB/s = bytes / time)")
lib, s, blocks = _lib.lib, _stream(), ctypes.c_int(0)
md, lvd = mean.detach(), logvar.detach()


def one(label, bytes_per_el, fn):
    t = ms(fn)
    say(f"{label}: {t * 1e3:.1f} us, {bytes_per_el} B / element -> {bytes_per_el * n / t / 1e9:.2f} TB/s")


for tag, tg in (("channels-last frames", frames), ("contiguous frames", frames_c)):
    nd, size, stride = V._layout([md, lvd, tg])
    part = torch.empty(min(V._MAX_BLOCKS, -(-n // 1024)), 3, device=DEV)
    one(f"fused forward, {tag}", 12, lambda: lib.oniris_vae_loss_fwd(_p(md), _p(lvd), _p(tg), 7, nd, size, stride, _p(part), part.shape[0],
                                                                    ctypes.byref(blocks), s))
    dm, dlv = torch.empty_like(md), torch.empty_like(lvd)
    cot = torch.ones(3, device=DEV)
    nd, size, stride = V._layout([md, lvd, tg, dm, dlv, None])
    one(f"fused backward (d mean, d logvar), {tag}", 20,
        lambda: lib.oniris_vae_loss_bwd(_p(md), _p(lvd), _p(tg), 7, nd, size, stride, _p(cot[0:]), _p(cot[1:]), _p(cot[2:]), _p(dm), _p(dlv), None,
                                        V._MAX_BLOCKS, s))
k = V.worst_k(n, 0.2)
e = torch.empty(n, device=DEV)
ws = torch.zeros(4100, dtype=torch.int32, device=DEV)
for tag, r, tg in (("channels-last frames", md, frames), ("contiguous frames", md, frames_c), ("all elements equal", frames_c, frames_c)):
    nd, size, stride = V._layout([r, tg])
    one(f"worst-k keys pass (e written, 11-bit histogram), {tag}", 12,
        lambda: lib.oniris_vae_loss_topk_keys(_p(r), _p(tg), nd, size, stride, _p(e), _p(ws), V._MAX_BLOCKS, s))
nd, size, stride = V._layout([md, frames])
ws.zero_()
lib.oniris_vae_loss_topk_keys(_p(md), _p(frames), nd, size, stride, _p(e), _p(ws), V._MAX_BLOCKS, s)
lib.oniris_vae_loss_topk_select(_p(ws), 0, k, _p(ws[4096:]), None, 0, None, s)
part = torch.empty(min(V._MAX_BLOCKS, -(-n // 1024)), device=DEV)
one("worst-k count pass, digit 2 (reads e)", 4, lambda: lib.oniris_vae_loss_topk_count(_p(e), n, 0, _p(ws[4096:]), _p(ws[2048:]), None, V._MAX_BLOCKS,
                                                                                      ctypes.byref(blocks), s))
ws[2048:3072].zero_()
lib.oniris_vae_loss_topk_count(_p(e), n, 0, _p(ws[4096:]), _p(ws[2048:]), None, V._MAX_BLOCKS, ctypes.byref(blocks), s)
lib.oniris_vae_loss_topk_select(_p(ws[2048:]), 1, k, _p(ws[4096:]), None, 0, None, s)
one("worst-k count pass, digit 3 (reads e, sums e above the prefix)", 4,
    lambda: lib.oniris_vae_loss_topk_count(_p(e), n, 1, _p(ws[4096:]), _p(ws[3072:]), _p(part), V._MAX_BLOCKS, ctypes.byref(blocks), s))
st = torch.zeros(4, dtype=torch.int32, device=DEV)


def select0():
    st.zero_()
    lib.oniris_vae_loss_topk_select(_p(ws), 0, k, _p(st), None, 0, None, s)


t_sel = ms(select0)
say(f"worst-k select (one workgroup, 2048 bins) + a 16-byte memset: {t_sel * 1e3:.1f} us")
_, state = V.worst_k_select(md, frames, k)
gq, dr = torch.ones((), device=DEV), torch.empty_like(md)
nd, size, stride = V._layout([md, frames, dr, None])
one("worst-k backward (d recon), channels-last frames", 12,
    lambda: lib.oniris_vae_loss_topk_bwd(_p(md), _p(frames), nd, size, stride, _p(state), _p(gq), k, _p(dr), None, V._MAX_BLOCKS, s))
say("worst-k forward in all: 12 + 4 + 4 = 20 B / element over three passes, plus three one-workgroup selects and one 16 KB memset")
if out:
    out.close()

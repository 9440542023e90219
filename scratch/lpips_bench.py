"""LPIPS timing: the native path against the module's own torch formula (`forward_torch`, MIOpen convolutions: what users run today) on
the same GPU in the same process, at (128, 3, 256, 256) -- B = 4 clips of 32 frames, the VAE training shape -- and (32, 3, 64, 64).

  python scratch/lpips_bench.py [REPORT]        appends a text report to REPORT (e.g. profiles/lpips.txt)

Forward alone (no_grad) and forward + backward with in0 requiring grad (the training loop: in1 = the frames, data).  HIP events, two
warm-ups, median of 7 with min / max; the two paths alternate inside every repetition.  The per-kernel split brackets every launch
wrapper of autoregressive_diffusion_amd/lpips.py with its own event pair in a separate pass (events around a launch include ~2 us of
kernel boundary each); FLOPs are useful FLOPs from the shapes.  Run under its own `timeout -k 10`, with OMP_NUM_THREADS=16."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from autoregressive_diffusion_amd import lpips as lp  # noqa: E402
import lpips_cpu_restatement as R  # noqa: E402

out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
SHAPES = [(128, 256, 256), (32, 64, 64)]
PEAK = 157.3          # fp32 matrix = fp32 vector TFLOP/s


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def flops(N, H, W):
    """Useful forward FLOPs per stage for 2 N images."""
    s = lp.feature_sizes(H, W)
    rows = []
    for (name, co, ci, k), (h, w) in zip(lp._TRUNK, s):
        rows.append((name, 2 * 2 * N * h * w * co * ci * k * k))
    return rows


def main():
    assert torch.cuda.is_available(), "no GPU: nothing to measure"
    m = lp.LPIPS(net="alex", weights=R.seeded_weights(3)).cuda()
    say(f"# LPIPS native vs forward_torch on {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    for shape in SHAPES:
        N, H, W = shape
        a, b = (t.cuda() for t in R.images(shape, 1))
        fl = flops(N, H, W)
        tot = sum(f for _, f in fl)
        say(f"\n## shape ({N}, 3, {H}, {W}): forward {tot / 1e9:.1f} GFLOP in the five convs, backward (d in0 only) about half of it "
            f"again")

        def fwd(fn):
            with torch.no_grad():
                return fn(a, b)

        def fwdbwd(fn):
            x = a.detach().requires_grad_(True)
            torch.log(fn(x, b) + 1e-8).mean().backward()
            return x.grad
        v0, v1 = fwd(m), fwd(m.forward_torch)
        g0, g1 = fwdbwd(m), fwdbwd(m.forward_torch)
        rel = lambda p, q: ((p - q).double().norm() / q.double().norm()).item()
        say(f"native vs torch formula: value rel L2 {rel(v0, v1):.2e}, d in0 rel L2 {rel(g0, g1):.2e}")
        t = {k: [] for k in ("native fwd", "torch fwd", "native fwd+bwd", "torch fwd+bwd")}
        for rep in range(9):
            r = [timed(lambda: fwd(m)), timed(lambda: fwd(m.forward_torch)), timed(lambda: fwdbwd(m)),
                 timed(lambda: fwdbwd(m.forward_torch))]
            if rep >= 2:
                for k, x in zip(t, r):
                    t[k].append(x)
        for k, v in t.items():
            say(f"{k:16s} {stats(v)}")
        say(f"forward: native / torch = {statistics.median(t['native fwd']) / statistics.median(t['torch fwd']):.2f}; "
            f"forward + backward: native / torch = {statistics.median(t['native fwd+bwd']) / statistics.median(t['torch fwd+bwd']):.2f}")
        say(f"native forward: {tot / statistics.median(t['native fwd']) / 1e9:.1f} TFLOP/s end to end ({PEAK} peak)")

        # per-kernel split: every launch wrapper bracketed by its own events, one extra pass (after a warm one)
        names = ["stem", "conv", "pool", "heads", "head_bwd", "conv_dgrad", "pool_bwd", "stem_dgrad"]
        orig = {n: getattr(lp, n) for n in names}
        log = []

        def wrap(n):
            def f(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = orig[n](*args, **kw)
                e1.record()
                shp = tuple(args[0][0].shape) if isinstance(args[0], (list, tuple)) else tuple(args[0].shape)
                log.append((n, shp, e0, e1))
                return r
            return f
        for n in names:
            setattr(lp, n, wrap(n))
        try:
            for rep in range(3):
                log.clear()
                fwdbwd(m)
                torch.cuda.synchronize()
        finally:
            for n in names:
                setattr(lp, n, orig[n])
        say("per launch wrapper, forward + backward (d in0 only), in launch order:")
        conv_fl = iter(fl[1:])
        total = 0.0
        for n, shp, e0, e1 in log:
            ms = e0.elapsed_time(e1)
            total += ms
            extra = ""
            if n == "stem":
                extra = f"  {fl[0][1] / ms / 1e9:6.1f} TFLOP/s"
            elif n == "conv":
                extra = f"  {next(conv_fl)[1] / ms / 1e9:6.1f} TFLOP/s"
            say(f"  {n:11s} first operand {str(shp):26s} {ms:8.3f} ms{extra}")
        say(f"  sum {total:.3f} ms")


main()
if out:
    out.close()

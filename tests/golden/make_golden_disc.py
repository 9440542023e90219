"""Generate fixtures G18 / G19 (the VAE discriminator) by IMPORTING the reference (read-only) on CPU in the build container.
Run from the repo root:   python tests/golden/make_golden_disc.py

Parameters come from disc_paramgen.py (seeded) and are loaded strict=True into the reference's modules, which pins key names and
shapes; inputs from disc_paramgen.inputs.  Everything is computed in float64 and stored as float32; `ref32_rel/<name>` is the rel L2 of
the reference's own float32 run of the same call against its float64 run.  Cotangent: cos(0.7 i + 0.3) over the flat index.

  g18_disc2d.npz        three Discriminator2D nets (disc_paramgen.G18_NETS), names `<net>/...`: train mode `logits`, `dx`, the
                        running buffers after TWO consecutive forwards `buf2/<key>`, eval mode `eval_logits`, and `keys` / `shapes`
                        (the state dict's key list with shapes, as strings).
  g18_disc2d_grads.npz  `<net>/grad/<parameter>` for every parameter with a gradient (conv_norm_out has none).
  g19_disc_mixed.npz    MixedDiscriminator(3) and (6) on (2, C, 4, 32, 32): `logits` (2, 2, 5, 8, 8), `dx`, `d3_logits` (the 3-D
                        half alone), `frames` / `recon` with `vae_loss` and `discriminator_loss` on them, `gradnorm/<parameter>`
                        for every parameter gradient of the logits' cotangent, and the full gradients `grad/<k>` of four small ones.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refshim  # noqa: E402

edm2 = _refshim.install()
from edm2.vae.discriminator import Discriminator2D, MixedDiscriminator  # noqa: E402
import disc_paramgen as G  # noqa: E402

torch.set_num_threads(8)
PHI = 0.3


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def run2d(cin, widths, params, x, dtype):
    net = Discriminator2D(cin, widths).train()
    net.load_state_dict(params, strict=True)
    net = net.to(dtype)
    xi = x.to(dtype).requires_grad_(True)
    logits = net(xi)
    (logits * G.cot(logits.shape, PHI, dtype)).sum().backward()
    out = {"logits": logits.detach(), "dx": xi.grad}
    for k, v in net.named_parameters():
        if v.grad is not None:
            out["grad/" + k] = v.grad
    with torch.no_grad():
        net(xi)
    for k, v in net.state_dict().items():
        if "running" in k or "num_batches" in k:
            out["buf2/" + k] = v.clone()
    net2 = Discriminator2D(cin, widths).eval()
    net2.load_state_dict(params, strict=True)
    with torch.no_grad():
        out["eval_logits"] = net2.to(dtype)(xi.detach())
    return out, {k: tuple(v.shape) for k, v in net.state_dict().items()}


def run_mixed(cin, params, x, frames, recon, dtype):
    net = MixedDiscriminator(cin).train()
    net.load_state_dict(params, strict=True)
    net = net.to(dtype)
    xi = x.to(dtype).requires_grad_(True)
    logits = net(xi)
    (logits * G.cot(logits.shape, PHI, dtype)).sum().backward()
    out = {"logits": logits.detach(), "dx": xi.grad}
    for k, v in net.named_parameters():
        if v.grad is not None:
            out["gradnorm/" + k] = v.grad.norm()
            if k in G.G19_FULL:
                out["grad/" + k] = v.grad.clone()
    for name in ("vae_loss", "discriminator_loss"):
        m = MixedDiscriminator(cin).train()
        m.load_state_dict(params, strict=True)
        with torch.no_grad():
            out[name] = getattr(m.to(dtype), name)(frames.to(dtype), recon.to(dtype))
    m = MixedDiscriminator(cin).train()
    m.load_state_dict(params, strict=True)
    with torch.no_grad():
        out["d3_logits"] = m.to(dtype).discriminator3d(x.to(dtype))
    return out, {k: tuple(v.shape) for k, v in net.state_dict().items()}


def pack(store, name, o64, o32, shapes):
    for k, v in o64.items():
        store[f"{name}/{k}"] = v.double().numpy().astype(np.float32) if v.is_floating_point() else v.numpy()
        if v.is_floating_point():
            store[f"{name}/ref32_rel/{k}"] = np.float32(rel(o32[k], v))
    store[f"{name}/keys"] = np.array(list(shapes))
    store[f"{name}/shapes"] = np.array([",".join(map(str, s)) for s in shapes.values()])


def main():
    main_z, grads_z = {}, {}
    for name, (cin, widths, shape, seed) in G.G18_NETS.items():
        shapes = G.disc2d_shapes(cin, widths)
        params = G.fill(shapes, seed)
        x = G.inputs(shape, seed)
        o64, sd_shapes = run2d(cin, widths, params, x, torch.float64)
        o32, _ = run2d(cin, widths, params, x, torch.float32)
        assert {k: tuple(s) for k, s in shapes.items()} == sd_shapes
        assert not any(k.startswith("grad/conv_norm_out") for k in o64)
        both = {}
        pack(both, name, o64, o32, sd_shapes)
        for k, v in both.items():
            (grads_z if "/grad/" in k and "ref32_rel" not in k else main_z)[k] = v
        worst = max((float(v), k) for k, v in both.items() if "ref32_rel" in k and "conv1.bias" not in k)   # (those are zero)
        print(f"G18 {name}: worst ref32_rel {worst[0]:.2e} ({worst[1]})")
    for fn, z in (("g18_disc2d.npz", main_z), ("g18_disc2d_grads.npz", grads_z)):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **z)
        print(f"{fn}: {os.path.getsize(path) / 1024:.0f} KiB")
        assert os.path.getsize(path) < 1024 * 1024
    z = {}
    for name, (cin, shape, seed) in G.G19_NETS.items():
        shapes = G.mixed_shapes(cin)
        params = G.fill(shapes, seed)
        x = G.inputs(shape, seed)
        cf = cin // 2
        frames = G.inputs((1, cf, 4, 32, 32), seed + 1)
        recon = frames.repeat(1, 2, 1, 1, 1)[:, :cin - cf] + 0.3 * G.inputs((1, cin - cf, 4, 32, 32), seed + 2)
        o64, sd_shapes = run_mixed(cin, params, x, frames, recon, torch.float64)
        o32, _ = run_mixed(cin, params, x, frames, recon, torch.float32)
        assert {k: tuple(s) for k, s in shapes.items()} == sd_shapes
        assert tuple(o64["logits"].shape) == (2, 2, 5, 8, 8)
        pack(z, name, o64, o32, sd_shapes)
        z[f"{name}/frames"], z[f"{name}/recon"] = frames.numpy(), recon.numpy()
        worst = max((float(v), k) for k, v in z.items() if k.startswith(name + "/ref32_rel") and "conv1.bias" not in k)
        print(f"G19 {name}: worst ref32_rel {worst[0]:.2e} ({worst[1]}); losses {o64['vae_loss'].item():.6f} "
              f"{o64['discriminator_loss'].item():.6f}")
    path = os.path.join(HERE, "g19_disc_mixed.npz")
    np.savez_compressed(path, **z)
    print(f"g19_disc_mixed.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

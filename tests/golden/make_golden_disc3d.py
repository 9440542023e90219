"""Generate fixture G20 (the VAE discriminator's 3-D half alone) by IMPORTING the reference (read-only) on CPU in the build container.
Run from the repo root:   python tests/golden/make_golden_disc3d.py

Parameters come from disc_paramgen.fill(disc3d_shapes(...), seed) and are loaded strict=True into the reference's Discriminator3D,
which pins key names and shapes; inputs from disc_paramgen.inputs; the nets are disc3d_paramgen.G20_NETS.  Everything is computed
in float64 and stored as float32; `ref32_rel/<name>` is the rel L2 of the reference's own float32 run of the same call against its
float64 run.  Cotangent: cos(0.7 i + 0.3) over the flat index.

  g20_disc3d.npz   per net `<net>/...`: `logits`, `dx`, `grad/<parameter>` for every parameter gradient of at most 16384 elements;
                   for the larger ones (all 27-tap weights) `gradnorm/<parameter>`, `gradtaps/<parameter>` (the 27 per-tap
                   Frobenius norms) and `gradhead/<parameter>` (output channels 0..3 in full); `keys` / `shapes` (the state dict's
                   key list with shapes, as strings); `ref32_rel/<each of the above>`.
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
from edm2.vae.discriminator import Discriminator3D  # noqa: E402
import disc_paramgen as G  # noqa: E402
import disc3d_paramgen as G3  # noqa: E402

torch.set_num_threads(8)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def run3d(cin, widths, params, x, dtype):
    net = Discriminator3D(cin, widths).train()
    net.load_state_dict(params, strict=True)
    net = net.to(dtype)
    xi = x.to(dtype).requires_grad_(True)
    logits = net(xi)
    (logits * G.cot(logits.shape, G3.PHI, dtype)).sum().backward()
    out = {"logits": logits.detach(), "dx": xi.grad}
    for k, v in net.named_parameters():
        if v.grad is not None:
            out.update(G3.grad_entries(k, v.grad.detach()))
    return out, {k: tuple(v.shape) for k, v in net.state_dict().items()}


def main():
    z = {}
    for name, (cin, widths, shape, seed) in G3.G20_NETS.items():
        shapes = G.disc3d_shapes(cin, widths)
        params = G.fill(shapes, seed)
        x = G.inputs(shape, seed)
        o64, sd_shapes = run3d(cin, widths, params, x, torch.float64)
        o32, _ = run3d(cin, widths, params, x, torch.float32)
        assert {k: tuple(s) for k, s in shapes.items()} == sd_shapes
        assert tuple(o64["logits"].shape) == G3.G20_LOGITS[name], o64["logits"].shape
        assert not any("conv_norm_out" in k for k in o64)
        for k, v in o64.items():
            z[f"{name}/{k}"] = v.double().numpy().astype(np.float32)
            z[f"{name}/ref32_rel/{k}"] = np.float32(rel(o32[k], v))
        z[f"{name}/keys"] = np.array(list(sd_shapes))
        z[f"{name}/shapes"] = np.array([",".join(map(str, s)) for s in sd_shapes.values()])
        zero = ["grad/" + k for k in G3.G20_ZERO_BIAS[name]]
        for k in zero:
            wk = k.replace("conv1.bias", "conv1.weight")
            scale = o64[wk].norm() if wk in o64 else o64[wk.replace("grad/", "gradnorm/")]
            assert o64[k].abs().max() <= 1e-9 * scale, k
        worst = max((float(v), k) for k, v in z.items() if k.startswith(name + "/ref32_rel") and k.split("ref32_rel/")[1] not in zero)
        print(f"G20 {name}: worst ref32_rel {worst[0]:.2e} ({worst[1]}); {len(o64)} entries")
    path = os.path.join(HERE, "g20_disc3d.npz")
    np.savez_compressed(path, **z)
    print(f"g20_disc3d.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

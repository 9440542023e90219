"""Generate fixture G21 (the VAE's training losses) by IMPORTING the reference (read-only) on CPU in the build container.
Run from the repo root:   python tests/golden/make_golden_vae_losses.py

Inputs come from vae_losses_gen (seeds; nothing of them is stored).  The reference's GaussianLoss (edm2/utils.py), F.l1_loss,
F.mse_loss and worst_k_percent_loss (edm2/vae/utils.py) run in float64 and in float32; `ref32_rel/<name>` is the relative deviation
(rel L2 for gradients) of the float32 run from the float64 run.

  g21_vae_losses.npz
    per fused case `<case>/...`: `gauss`, `l1`, `mse` (float64 losses), `termabs/<loss>` (the float64 mean of |term|, the scale of the
        loss tolerance), and per loss with a unit cotangent `<loss>/dmean`, `<loss>/dlogvar` (gauss only), `<loss>/dtarget`: in full up
        to vae_losses_gen.FULL_GRADS elements, else `<loss>/norm/d...` (the L2 norm)
    per worst-k case `<wk>/...`: `k`, `thr` (the float32 bit pattern of the k-th largest squared error), `count_gt`, `count_eq`
        (numpy, from the float32 squared errors), `loss` (float64), `drecon` in full or `norm/drecon`, `nonzero` (how many elements the
        reference's gradient touches)
For every worst-k case without a tie at the threshold the generator asserts that the float64 reference selects exactly the elements
the float32 keys select."""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refshim  # noqa: E402

edm2 = _refshim.install()
from edm2.utils import GaussianLoss  # noqa: E402
from edm2.vae.utils import worst_k_percent_loss  # noqa: E402
from torch.nn import functional as F  # noqa: E402
import vae_losses_gen as G  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import vae_losses_cpu_restatement as R  # noqa: E402

torch.set_num_threads(8)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def run_fused(case, dtype):
    out = {}
    for name, fn, has_lv in (("gauss", GaussianLoss, True), ("l1", F.l1_loss, False), ("mse", F.mse_loss, False)):
        m, lv, tg = (t.to(dtype).requires_grad_(True) for t in G.inputs(case))
        loss = fn(m, lv, tg) if has_lv else fn(m, tg)
        loss.backward()
        out[name] = loss.detach()
        out[f"{name}/dmean"], out[f"{name}/dtarget"] = m.grad, tg.grad
        if has_lv:
            out[f"{name}/dlogvar"] = lv.grad
    return out


def run_worstk(case, percent, dtype):
    m, _, tg = (t.to(dtype) for t in G.inputs(case))
    m.requires_grad_(True)
    loss = worst_k_percent_loss(m, tg, percent=percent)
    loss.backward()
    return {"loss": loss.detach(), "drecon": m.grad}


def store(z, prefix, o64, o32):
    for k, v in o64.items():
        r = abs(o32[k].double() - v).item() / abs(v).item() if v.dim() == 0 else rel(o32[k], v)
        z[f"{prefix}/ref32_rel/{k}"] = np.float64(r)
        if v.dim() == 0:
            z[f"{prefix}/{k}"] = np.float64(v.item())
        elif v.numel() <= G.FULL_GRADS:
            z[f"{prefix}/{k}"] = v.double().numpy().astype(np.float32)
        else:
            head, _, leaf = k.rpartition("/")
            z[f"{prefix}/{head + '/' if head else ''}norm/{leaf}"] = np.float64(v.double().norm().item())


def main():
    z = {}
    for case in G.CASES:
        o64, o32 = run_fused(case, torch.float64), run_fused(case, torch.float32)
        store(z, case, o64, o32)
        _, termabs, _ = R.fused(*G.inputs(case), (1.0, 0.0, 0.0))
        for name, v in zip(("gauss", "l1", "mse"), termabs):
            z[f"{case}/termabs/{name}"] = np.float64(v)
        worst = max((float(v), k) for k, v in z.items() if k.startswith(case + "/ref32_rel"))
        print(f"G21 {case}: worst ref32_rel {worst[0]:.2e} ({worst[1]})")
    for wk, (case, percent) in G.WORSTK.items():
        m, _, tg = G.inputs(case)
        k = G.worst_k(m.numel(), percent)
        sel = R.select(m, tg, k)
        o64, o32 = run_worstk(case, percent, torch.float64), run_worstk(case, percent, torch.float32)
        store(z, wk, o64, o32)
        z[f"{wk}/k"], z[f"{wk}/thr"] = np.int64(k), np.uint32(sel["thr"])
        z[f"{wk}/count_gt"], z[f"{wk}/count_eq"] = np.int64(sel["count_gt"]), np.int64(sel["count_eq"])
        nz = o64["drecon"].flatten() != 0
        z[f"{wk}/nonzero"] = np.int64(int(nz.sum()))
        if sel["count_eq"] == 1:
            assert np.array_equal(nz.numpy(), sel["key"] >= sel["thr"]), f"{wk}: float64 selects another set than the float32 keys"
        print(f"G21 {wk}: k {k}, thr {int(sel['thr']):#010x}, count_gt {sel['count_gt']}, count_eq {sel['count_eq']}, "
              f"ref32_rel loss {z[wk + '/ref32_rel/loss']:.2e} drecon {z[wk + '/ref32_rel/drecon']:.2e}")
    path = os.path.join(HERE, "g21_vae_losses.npz")
    np.savez_compressed(path, **z)
    print(f"g21_vae_losses.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
